"""Cases and references of the crop warp's edge tests (csrc/warp.hip, four launchers): tests/test_warp_edges_host.py holds the C oracle to
them on the CPU, tests/test_gpu_warp_edges.py the kernels on the MI355X.  Three sources of expected values, used together:

1. CLOSED FORMS that restate neither the kernel nor the oracle (`closed_form`): maps whose sample positions fall on pixel centres or exact
   half pixels, so cv.warpAffine's result is a shifted copy, a rounded mean of two or of four pixels, or one pixel everywhere.
2. A FLOAT64 BILINEAR REFERENCE with BORDER_CONSTANT 0 at the exact real sample position (`bilinear_f64`) and a derived bound (`bound`).
3. BIT EQUALITY with pose_oracle.warp_affine_u8c3 on every case (flip cases: the oracle on np.fliplr(src)).

The bound, derived (not measured).  Let p = (px, py) be the exact position M_inv (x, y, 1) and f the bilinear interpolant of the source
extended by zeros (what BORDER_CONSTANT 0 samples).  The fixed-point warp computes, per axis and in units of 1/1024 px,
a = round((M1 y + M2) 1024) and b = round(M0 x 1024): two roundings of at most 0.5 each, so |a + b - 1024 px| <= 1.  It then takes
X = (a + b + 16) >> 5, the position in 1/32 px: |32 X - (a + b)| <= 16.  Together the quantised position q is within 17/1024 px of p on each
axis.  The four weights (32 - fy)(32 - fx) 32, ... are exact products, sum to 2^15, and are the bilinear weights of q exactly - except at
fx = fy = 0, where the table holds (32767, 0, 0, 1): the sum is v0 2^15 + (v3 - v0) and, as |v3 - v0| <= 255 < 2^14, (sum + 2^14) >> 15 is
still v0 = f(q).  So the kernel's value is f(q) rounded half up: |out - f(q)| <= 0.5.  f is piecewise bilinear, along x its slope is a
convex combination of horizontal neighbour differences, so |f(q) - f(p)| <= Gx |qx - px| + Gy |qy - py| with Gx, Gy the largest
absolute differences of horizontally / vertically adjacent pixels of the zero-extended source.  Hence

    |out - f(p)| <= 0.5 + (17/1024) (Gx + Gy)            (+ 1e-6 for the float64 evaluation of p and f themselves).

With the smooth sources below (Gx, Gy <= 8) that is 0.766: under one grey level."""
import math

import numpy as np

from oracle import pose_oracle

SOURCE_SIZES = ((1, 1), (1, 9), (9, 1), (2, 2), (37, 29))          # (h, w)
OUT_SIZES = ((1, 1), (5, 7), (33, 31), (1, 1025))                  # (oh, ow): 105 B slots; 1025 px = a third pass of the grid-stride loop
COUNTS = (31, 32, 33, 65)                                          # crops / samples per call: around WARP_BATCH = 32
MEAN = (0.485, 0.456, 0.406)


def hard_source(h, w, seed=0):
    """Random bytes with 0 and 255 side by side (the 32767 / 1 weight correction has the largest v3 - v0 to work on)."""
    rng = np.random.default_rng(1000 * h + w + seed)
    s = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    s[0, 0] = (255, 0, 255)
    if w > 1:
        s[0, 1] = (0, 255, 0)
    if h > 1:
        s[1, 0] = (0, 255, 255)
    if h > 1 and w > 1:
        s[1, 1] = (255, 0, 0)
        s[h - 1, w - 1] = (255, 255, 1)
    return s


def smooth_source(h, w):
    """A tent over the image: neighbours differ by at most 8 / 7 / 6 per channel, the zero border included (edge pixels are 8 / 7 / 6)."""
    y, x = np.mgrid[0:h, 0:w]
    d = np.minimum(np.minimum(x + 1, w - x), np.minimum(y + 1, h - y))
    return np.stack([np.minimum(d * k, 255) for k in (8, 7, 6)], -1).astype(np.uint8)


def gradients(src):
    """(Gx, Gy): the largest absolute difference between horizontal / vertical neighbours of the zero-extended source."""
    p = np.pad(src.astype(np.int64), ((1, 1), (1, 1), (0, 0)))
    return int(np.abs(np.diff(p, axis=1)).max()), int(np.abs(np.diff(p, axis=0)).max())


def bound(src):
    gx, gy = gradients(src)
    return 0.5 + (17.0 / 1024.0) * (gx + gy) + 1e-6


def invert_affine(fwd):
    """sp_invert_affine / cv::warpAffine's inversion of the forward 2x3 map, statement by statement in IEEE double (Python floats)."""
    m = [float(v) for v in np.asarray(fwd, np.float64).reshape(6)]
    d = m[0] * m[4] - m[1] * m[3]
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m[4] * d, m[0] * d
    m[0], m[1], m[3], m[4] = a11, m[1] * -d, m[3] * -d, a22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return np.array(m, np.float64)


def bilinear_f64(src, fwd, oh, ow):
    """f(p): float64 bilinear interpolation of the zero-extended source at p = M_inv (x, y, 1), [oh, ow, 3]."""
    h, w, _ = src.shape
    m = invert_affine(fwd)
    y, x = np.mgrid[0:oh, 0:ow].astype(np.float64)
    px, py = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    px, py = np.clip(px, -4.0, w + 4.0), np.clip(py, -4.0, h + 4.0)          # far outside is outside: keeps the index arithmetic small
    x0, y0 = np.floor(px), np.floor(py)
    fx, fy = (px - x0)[..., None], (py - y0)[..., None]
    s = np.pad(src.astype(np.float64), ((6, 6), (6, 6), (0, 0)))
    xi, yi = x0.astype(np.int64) + 6, y0.astype(np.int64) + 6
    return ((1 - fy) * ((1 - fx) * s[yi, xi] + fx * s[yi, xi + 1]) + fy * ((1 - fx) * s[yi + 1, xi] + fx * s[yi + 1, xi + 1]))


def _fetch(src, yy, xx):
    """src[yy, xx] with zeros outside, integer index arrays -> int64 [.., 3]."""
    h, w, _ = src.shape
    ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
    return np.where(ok[..., None], src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64), 0)


def closed_form(kind, arg, src, oh, ow):
    """Expected uint8 [oh, ow, 3] of the closed-form maps; `fwd_of` gives their forward matrices."""
    y, x = np.mgrid[0:oh, 0:ow]
    if kind == "shift":                                   # dst = src + (tx, ty), integers: a copy with a zero border
        tx, ty = arg
        return _fetch(src, y - ty, x - tx).astype(np.uint8)
    if kind == "half_x":                                  # sample at x + arg, arg = +0.5 / -0.5: the mean of two, rounded half up
        x0 = x if arg > 0 else x - 1
        return ((_fetch(src, y, x0) + _fetch(src, y, x0 + 1) + 1) >> 1).astype(np.uint8)
    if kind == "half_y":
        y0 = y if arg > 0 else y - 1
        return ((_fetch(src, y0, x) + _fetch(src, y0 + 1, x) + 1) >> 1).astype(np.uint8)
    if kind == "decimate2":                               # sample at (2x + 0.5, 2y + 0.5): the mean of four
        return ((_fetch(src, 2 * y, 2 * x) + _fetch(src, 2 * y, 2 * x + 1) + _fetch(src, 2 * y + 1, 2 * x) +
                 _fetch(src, 2 * y + 1, 2 * x + 1) + 2) >> 2).astype(np.uint8)
    if kind == "degenerate":                              # zero determinant: cv::warpAffine's inverse is the zero map, every pixel samples (0, 0)
        return np.broadcast_to(src[0, 0], (oh, ow, 3)).copy()
    raise KeyError(kind)


def fwd_of(kind, arg):
    """Forward maps whose inversion is exact in binary (unit or power-of-two determinant, dyadic translations)."""
    if kind == "shift":
        return np.array([1, 0, arg[0], 0, 1, arg[1]], np.float64)
    if kind == "half_x":
        return np.array([1, 0, -arg, 0, 1, 0], np.float64)
    if kind == "half_y":
        return np.array([1, 0, 0, 0, 1, -arg], np.float64)
    if kind == "decimate2":
        return np.array([0.5, 0, -0.25, 0, 0.5, -0.25], np.float64)
    if kind == "degenerate":
        return np.array([1, 2, 3, 2, 4, 5], np.float64)
    if kind == "frac":                                    # sample at (x + ax/32, y + ay/32): fx / fy = 0 .. 31 on every pixel
        return np.array([1, 0, -arg[0] / 32.0, 0, 1, -arg[1] / 32.0], np.float64)
    if kind == "general":                                 # rotation by `deg` about the source centre, scale s, centre moved to the output centre
        deg, s, cx, cy, ox, oy = arg
        c, sn = math.cos(math.radians(deg)) * s, math.sin(math.radians(deg)) * s
        return np.array([c, -sn, ox - (c * cx - sn * cy), sn, c, oy - (sn * cx + c * cy)], np.float64)
    raise KeyError(kind)


def base_maps(h, w, oh, ow):
    """[(kind, arg)]: the maps every (source, output) pair is warped by.  Shifts by +1 put the samples of output row / column 0 exactly
    on row / column -1 (no tap counts), the -0.5 halves put them between -1 and 0 (one or two taps inside), the +0.5 halves and
    frac (31, .) do the same at the last row / column; +-100000 px is wholly outside (and saturates the 16-bit pixel index)."""
    cx, cy, ox, oy = (w - 1) / 2.0, (h - 1) / 2.0, (ow - 1) / 2.0, (oh - 1) / 2.0
    return [("shift", (0, 0)), ("shift", (1, 1)), ("shift", (-1, 0)), ("shift", (0, -1)), ("shift", (2, -3)), ("shift", (w, 0)),
            ("shift", (0, -h)), ("shift", (100000, 0)), ("shift", (0, -100000)),
            ("half_x", 0.5), ("half_x", -0.5), ("half_y", 0.5), ("half_y", -0.5), ("decimate2", None), ("degenerate", None),
            ("frac", (31, 0)), ("frac", (0, 31)), ("frac", (31, 31)), ("frac", (-31, -1)), ("frac", (1, 16)),
            ("general", (17.0, 0.7, cx, cy, ox, oy)), ("general", (-33.0, 1.9, cx, cy, ox, oy)), ("general", (90.0, 1.0, cx, cy, ox, oy)),
            ("general", (180.0, 0.31, cx, cy, ox - 0.4, oy + 0.3)), ("general", (5.0, 3.3, cx, cy, ox, oy))]


def cases(h, w, oh, ow, n, seed=0):
    """n cases [(kind, arg, fwd [6])] for one (source, output) pair: the base maps, then seeded general maps up to n."""
    out = [(k, a, fwd_of(k, a)) for k, a in base_maps(h, w, oh, ow)][:n]
    rng = np.random.default_rng(seed + 7919 * (h * 100 + w) + oh * 2000 + ow)
    while len(out) < n:
        a = (float(rng.uniform(-180, 180)), float(np.exp(rng.uniform(-1.2, 1.2))), (w - 1) / 2.0 + float(rng.uniform(-2, 2)),
             (h - 1) / 2.0 + float(rng.uniform(-2, 2)), (ow - 1) / 2.0, (oh - 1) / 2.0)
        out.append(("general", a, fwd_of("general", a)))
    return out


CLOSED = ("shift", "half_x", "half_y", "decimate2", "degenerate")


def expected(src, kind, arg, fwd, flip, oh, ow):
    """The expected crop of one case from all three sources at once: the oracle's bytes, asserted equal to the closed form where there is one
    and inside the derived bound of the float64 reference always.  `flip`: the warp of np.fliplr(src)."""
    s = np.ascontiguousarray(src[:, ::-1]) if flip else src
    got = pose_oracle.warp_affine_u8c3(s, fwd.reshape(2, 3), (ow, oh))
    if kind in CLOSED:
        want = closed_form(kind, arg, s, oh, ow)
        assert np.array_equal(got, want), (kind, arg, src.shape, (oh, ow), flip)
    if kind != "degenerate":                              # (the zero map is not the inverse of anything: no real sample position)
        err = np.abs(got.astype(np.float64) - bilinear_f64(s, fwd, oh, ow)).max()
        assert err <= bound(s), (kind, arg, src.shape, (oh, ow), flip, err, bound(s))
    return got


def normalised(crops_u8):
    """[N, oh, ow, 3] BGR bytes -> [N, 3, oh, ow] fp32 RGB planes, (float)v / 255.0f - mean evaluated in fp32 (numpy float32 arithmetic
    is IEEE single, operation by operation)."""
    v = crops_u8[..., ::-1].astype(np.float32) / np.float32(255.0) - np.array(MEAN, np.float32)
    return np.ascontiguousarray(v.transpose(0, 3, 1, 2))
