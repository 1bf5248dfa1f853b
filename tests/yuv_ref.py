"""YUV 4:2:0 <-> BGR: the contract of include/simple_pose_hip.h restated in numpy int64, and its float64 definition.

Both directions, both formats (NV12: Y [h, w] and UV [ch, 2 * cw]; I420: Y, U [ch, cw], V [ch, cw]), odd sizes; planes are tight arrays here
and `pitched` / `unpitch` put them into buffers with a pitch and a base offset for the tests that need them."""
import numpy as np

NV12, I420 = 0, 1
BT601, BT709 = 0, 1
LIMITED, FULL = 0, 1
MODES = ((BT601, FULL), (BT601, LIMITED), (BT709, FULL), (BT709, LIMITED))
_NAMES = ("yoff", "ay", "rv", "bu", "gu", "gv", "yr", "yg", "yb", "ur", "ug", "ub", "vr", "vg", "vb")
TABLE = {
    (BT601, FULL): (0, 65536, 91881, 116130, 22554, 46802, 19595, 38470, 7471, -11059, -21709, 32768, 32768, -27439, -5329),
    (BT601, LIMITED): (16, 76309, 104597, 132201, 25675, 53279, 16829, 33039, 6416, -9714, -19071, 28784, 28784, -24103, -4681),
    (BT709, FULL): (0, 65536, 103206, 121609, 12276, 30679, 13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005),
    (BT709, LIMITED): (16, 76309, 117489, 138438, 13975, 34925, 11966, 40254, 4064, -6596, -22189, 28784, 28784, -26145, -2639),
}


def coefs(matrix, rng):
    return dict(zip(_NAMES, TABLE[(matrix, rng)]))


def decode_px(Y, U, V, matrix, rng):
    """Integer arrays Y, U, V (one chroma sample per pixel already) -> (R, G, B) int64."""
    k = coefs(matrix, rng)
    yy, uu, vv = np.asarray(Y, np.int64) - k["yoff"], np.asarray(U, np.int64) - 128, np.asarray(V, np.int64) - 128
    R = np.clip((k["ay"] * yy + k["rv"] * vv + 32768) >> 16, 0, 255)
    G = np.clip((k["ay"] * yy - k["gu"] * uu - k["gv"] * vv + 32768) >> 16, 0, 255)
    B = np.clip((k["ay"] * yy + k["bu"] * uu + 32768) >> 16, 0, 255)
    return R, G, B


def encode_px(R, G, B, matrix, rng):
    """Integer arrays R, G, B -> per-pixel (Yp, Up, Vp) int64, before the chroma average."""
    k = coefs(matrix, rng)
    R, G, B = (np.asarray(a, np.int64) for a in (R, G, B))
    Yp = (k["yr"] * R + k["yg"] * G + k["yb"] * B + (k["yoff"] << 16) + 32768) >> 16
    Up = (k["ur"] * R + k["ug"] * G + k["ub"] * B + (128 << 16) + 32767) >> 16
    Vp = (k["vr"] * R + k["vg"] * G + k["vb"] * B + (128 << 16) + 32767) >> 16
    return Yp, Up, Vp


def _kr_kb(matrix):
    return (0.299, 0.114) if matrix == BT601 else (0.2126, 0.0722)


def decode_px_f64(Y, U, V, matrix, rng):
    """The float64 definition, rounded half up and clamped: (R, G, B)."""
    kr, kb = _kr_kb(matrix)
    kg = 1.0 - kr - kb
    yoff, sy, sc = (0, 1.0, 1.0) if rng == FULL else (16, 255.0 / 219.0, 255.0 / 224.0)
    y, u, v = np.asarray(Y, np.float64) - yoff, np.asarray(U, np.float64) - 128, np.asarray(V, np.float64) - 128
    R = sy * y + 2 * (1 - kr) * sc * v
    G = sy * y - 2 * kb * (1 - kb) / kg * sc * u - 2 * kr * (1 - kr) / kg * sc * v
    B = sy * y + 2 * (1 - kb) * sc * u
    return tuple(np.clip(np.floor(a + 0.5), 0, 255).astype(np.int64) for a in (R, G, B))


def encode_px_f64(R, G, B, matrix, rng):
    """The float64 definition, rounded half up and clamped: per-pixel (Y, U, V)."""
    kr, kb = _kr_kb(matrix)
    kg = 1.0 - kr - kb
    yoff, ey, ec = (0, 1.0, 1.0) if rng == FULL else (16, 219.0 / 255.0, 224.0 / 255.0)
    R, G, B = (np.asarray(a, np.float64) for a in (R, G, B))
    luma = kr * R + kg * G + kb * B
    Y = yoff + ey * luma
    U = 128 + ec * (B - luma) / (2 * (1 - kb))
    V = 128 + ec * (R - luma) / (2 * (1 - kr))
    return tuple(np.clip(np.floor(a + 0.5), 0, 255).astype(np.int64) for a in (Y, U, V))


def split_chroma(planes, fmt):
    """(Y, UV) or (Y, U, V) -> Y, U, V as [h, w], [ch, cw], [ch, cw]."""
    if fmt == NV12:
        y, uv = planes
        return y, uv[:, 0::2], uv[:, 1::2]
    return planes


def join_chroma(y, u, v, fmt):
    if fmt == NV12:
        uv = np.empty((u.shape[0], 2 * u.shape[1]), np.uint8)
        uv[:, 0::2], uv[:, 1::2] = u, v
        return (y, uv)
    return (y, u, v)


def yuv420_to_bgr(planes, h, w, fmt, matrix, rng):
    """Tight planes -> uint8 BGR [h, w, 3]; the pixel (r, c) uses the chroma sample (r >> 1, c >> 1)."""
    y, u, v = split_chroma(planes, fmt)
    assert y.shape == (h, w) and u.shape == v.shape == ((h + 1) // 2, (w + 1) // 2)
    up = lambda p: np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)[:h, :w]
    R, G, B = decode_px(y, up(u), up(v), matrix, rng)
    return np.stack([B, G, R], axis=-1).astype(np.uint8)


def bgr_to_yuv420(bgr, fmt, matrix, rng):
    """uint8 BGR [h, w, 3] -> tight planes; chroma sample (i, j) = (sum + 2) >> 2 over the pixels (min(2i + a, h - 1), min(2j + b, w - 1))."""
    h, w = bgr.shape[:2]
    ch, cw = (h + 1) // 2, (w + 1) // 2
    Yp, Up, Vp = encode_px(bgr[..., 2], bgr[..., 1], bgr[..., 0], matrix, rng)
    rows = np.minimum(np.arange(2 * ch), h - 1)
    cols = np.minimum(np.arange(2 * cw), w - 1)

    def avg(p):
        q = p[rows][:, cols]
        return ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2).astype(np.uint8)

    return join_chroma(Yp.astype(np.uint8), avg(Up), avg(Vp), fmt)


def pitched(plane, pitch, offset, fill=0xA5, guard_rows=0):
    """A tight plane [rows, row_bytes] copied into a flat `fill`ed buffer at `offset` + guard_rows * pitch with `pitch` bytes per row.
    Returns (buffer, first byte of the plane in it)."""
    rows, rb = plane.shape
    assert pitch >= rb
    buf = np.full(offset + (rows + 2 * guard_rows) * pitch, fill, np.uint8)
    start = offset + guard_rows * pitch
    view = np.lib.stride_tricks.as_strided(buf[start:], (rows, rb), (pitch, 1))
    view[...] = plane
    return buf, start


def unpitch(buf, start, rows, row_bytes, pitch):
    """(the tight plane, a copy of the buffer with the plane's bytes set to 0xA5: what must have stayed untouched)."""
    buf = np.asarray(buf)
    view = np.lib.stride_tricks.as_strided(buf[start:], (rows, row_bytes), (pitch, 1))
    plane = view.copy()
    rest = buf.copy()
    np.lib.stride_tricks.as_strided(rest[start:], (rows, row_bytes), (pitch, 1))[...] = 0xA5
    return plane, rest
