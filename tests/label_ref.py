"""The overlay text's rules (include/simple_pose_hip.h above sp_render_labels_u8c3) restated in numpy and Python ints: a CHECKER only, never
imported by the package.  The kernels (simple_pose_amd/csrc/labels.hip) and the CPU program (tests/label_core_main.cpp) are compared with
`render` bit for bit.  Written from the header's comment: text is built as Python strings, a plate as a small bitmap of font pixels that is
enlarged s times and pasted, clipped, at its corner.  The glyphs come through sp_render_font_glyph (a host function)."""
import ctypes
import functools

import numpy as np

F_ID, F_SCORE, F_CONF, F_N, F_IMAGE = 1, 2, 3, 4, 5
LABEL_CHARS, CAPTION_BYTES = 24, 64


class Style:
    """`template`: bytes (printable ASCII and the field bytes), empty for no labels; scales 1..8; opacities in sixteenths; corner one of
    "tl", "tr", "bl", "br"; palette uint8 [P, 3] BGR."""

    def __init__(self, template=b"#\x01 \x02", label_scale=1, label_opacity=16, caption_scale=1, caption_opacity=12, caption_corner="tl",
                 palette=None):
        self.template = bytes(template)
        self.label_scale, self.label_opacity = int(label_scale), int(label_opacity)
        self.caption_scale, self.caption_opacity, self.caption_corner = int(caption_scale), int(caption_opacity), caption_corner
        if palette is None:                                  # dark and light entries: both text colours occur
            palette = [[(37 * i + 11) % 256, (91 * i + 60) % 256, (153 * i + 200) % 256] for i in range(7)]
        self.palette = np.asarray(palette, np.uint8).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def glyphs():
    """uint8 [95, 7]: the rows of the characters 0x20 .. 0x7E, bit 4 the leftmost column."""
    from simple_pose_amd import _lib
    out = np.zeros((95, 7), np.uint8)
    for ch in range(0x20, 0x7F):
        buf = (ctypes.c_uint8 * 7)()
        assert _lib.lib().sp_render_font_glyph(ch, buf) == 0
        out[ch - 0x20] = list(buf)
    return out


def number(v):
    """{score}, {conf}: "?" unless finite and >= 0; else c = rint(min(v, 99.99) * 100), ties to even, printed as c / 100 '.' two digits."""
    v = np.float64(v)
    if not np.isfinite(v) or v < 0:
        return "?"
    c = int(np.rint(min(v, np.float64(99.99)) * np.float64(100.0)))
    return f"{c // 100}.{c % 100:02d}"


def label_text(template, pick, track_id, score, conf):
    out = ""
    for c in template:
        if c == F_ID:
            out += str(int(track_id) if track_id is not None and int(track_id) > 0 else pick + 1)
        elif c == F_SCORE:
            out += number(score)
        elif c == F_CONF:
            out += number(np.float64(np.float32(conf)))
        else:
            assert 0x20 <= c <= 0x7E, c
            out += chr(c)
    return out[:LABEL_CHARS]


def caption_text(row64, n, image):
    out = ""
    for c in bytes(row64)[:CAPTION_BYTES]:
        if c == 0:
            break
        out += str(n) if c == F_N else str(image) if c == F_IMAGE else chr(c) if 0x20 <= c <= 0x7E else "?"
    return out[:CAPTION_BYTES]


def quantise(v):
    v = np.float64(v)
    if not np.isfinite(v) or abs(v) > 32768.0:
        return None
    return int(np.rint(v * np.float64(16.0)))


def plate_bitmap(text, s):
    """bool [9s, (6L + 1)s]: where a glyph bit is set."""
    g = glyphs()
    small = np.zeros((9, 6 * len(text) + 1), bool)
    for i, ch in enumerate(text):
        for row in range(7):
            for col in range(5):
                small[1 + row, 1 + 6 * i + col] = bool((int(g[ord(ch) - 0x20, row]) >> (4 - col)) & 1)
    return np.repeat(np.repeat(small, s, axis=0), s, axis=1)


def paste(img, text, s, x0, y0, plate, ink, opacity):
    """One plate onto img (int64 [h, w, 3]) in place, clipped: out = (in * (256 - a) + c * a + 128) >> 8, a = 16 * opacity."""
    if not text:
        return
    h, w = img.shape[:2]
    bits = plate_bitmap(text, s)
    ph, pw = bits.shape
    xa, ya, xb, yb = max(x0, 0), max(y0, 0), min(x0 + pw, w), min(y0 + ph, h)
    if xa >= xb or ya >= yb:
        return
    on = bits[ya - y0:yb - y0, xa - x0:xb - x0][:, :, None]
    c = np.where(on, np.asarray(ink, np.int64)[None, None, :], np.asarray(plate, np.int64)[None, None, :])
    a = 16 * opacity
    win = img[ya:yb, xa:xb]
    win[...] = (win * (256 - a) + c * a + 128) >> 8


def kept(scene, image, with_ids=True, rows=None, keep_count=None):
    """(box [n, 5], score [n], track_id [n] or None, n): the image's kept rows in pick order, the count clamped as the device clamps it."""
    rows = scene["box"].shape[0] if rows is None else rows
    kc = scene["keep_count"] if keep_count is None else keep_count
    lo, n = int(scene["seg"][image]), 0
    if 0 <= lo <= rows:
        n = min(max(int(kc[image]), 0), rows, rows - lo)
    sel = np.asarray(scene["keep"][lo:lo + n], np.int64)
    assert ((sel >= 0) & (sel < rows)).all()
    return scene["box"][sel], scene["score"][sel], scene["track_id"][sel] if with_ids else None, n


def render(img, style, box, score, track_id, n, image=0, caption=None):
    """The labels of the n kept persons (pick order arrays) and the caption (`caption`: the image's 64 bytes, or None) on a uint8 BGR
    image: a new uint8 array."""
    out = np.asarray(img).astype(np.int64)
    h, w = out.shape[:2]
    P = style.palette.shape[0]
    if style.template:
        s = style.label_scale
        for pick in range(n - 1, -1, -1):                    # slot p holds pick n - 1 - p: the best pose's label last
            qx, qy = quantise(np.float64(box[pick, 0])), quantise(np.float64(box[pick, 1]))
            if qx is None or qy is None:
                continue
            tid = None if track_id is None else int(track_id[pick])
            text = label_text(style.template, pick, tid, score[pick], box[pick, 4])
            colour = style.palette[(tid - 1) % P] if tid is not None and tid > 0 else style.palette[pick % P]
            b, g, r = (int(v) for v in colour)
            ink = (0, 0, 0) if 29 * b + 150 * g + 77 * r >= 32768 else (255, 255, 255)
            bx, by = qx >> 4, qy >> 4                        # Python's >> floors
            width = (6 * len(text) + 1) * s
            y0 = by - 9 * s
            if y0 < 0:
                y0 = by
            x0 = bx
            if x0 + width > w:
                x0 = w - width
            if x0 < 0:
                x0 = 0
            paste(out, text, s, x0, y0, (b, g, r), ink, style.label_opacity)
    if caption is not None:
        s = style.caption_scale
        text = caption_text(caption, n, image)
        width, height = (6 * len(text) + 1) * s, 9 * s
        x0 = w - s - width if style.caption_corner in ("tr", "br") else s
        y0 = h - s - height if style.caption_corner in ("bl", "br") else s
        paste(out, text, s, x0, y0, (0, 0, 0), (255, 255, 255), style.caption_opacity)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)
