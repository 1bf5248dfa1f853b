"""The overlay's text, host side: the three entry points are declared, exported and bound without an ABI bump and refuse bad arguments
before they touch the GPU; the font is what sp_font.h draws; PoseRenderer's text options refuse what they cannot draw, its template parser
gives the bytes written out here and its key tells label options apart but not caption texts; and tests/label_ref.py (the numpy restatement
the kernels and the CPU program are compared with) gives the answers written out here on hand-made cases."""
import ctypes
import os
import re

import numpy as np
import pytest

from simple_pose_amd import _lib, build
from simple_pose_amd.build import LIB_PATH
from tests import label_ref, label_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sp_render_font_glyph", "sp_render_labels_workspace_bytes", "sp_render_labels_u8c3")
ONE = ctypes.c_void_p(4096)         # a non-null, aligned pointer that is never dereferenced: every call below fails its argument check first


def _glyph(ch):
    buf = (ctypes.c_uint8 * 7)()
    assert _lib.lib().sp_render_font_glyph(ch, buf) == 0, ch
    return bytes(buf)


# ---- ABI and build ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_exported_bound_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(sp_\w+)\s*\(", hdr, flags=re.M))
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(handle, name), name
    assert re.search(r"#define SP_ABI_VERSION 36\b", hdr)
    assert _lib.ABI_VERSION == 36 and _lib.lib().sp_abi_version() == 36
    # the header's struct, field by field: 4-byte ints and bytes only, so its size is the sum
    body = re.search(r"typedef struct sp_label_style \{(.*?)\} sp_label_style;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    consts = {k: int(v) for k, v in re.findall(r"#define (SP_\w+) (\d+)\b", hdr)}
    size = 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        kind, names = re.match(r"(int32_t|unsigned char)\s+(.*)", decl, flags=re.S).groups()
        for name in names.split(","):
            dims = [consts[d] if d in consts else int(d) for d in re.findall(r"\[(\w+)\]", name)]
            size += (4 if kind == "int32_t" else 1) * int(np.prod(dims or [1]))
    assert size == 4 + 32 + 6 * 4 + 96 == ctypes.sizeof(_lib.LabelStyle)
    assert [f[0] for f in _lib.LabelStyle._fields_] == re.findall(r"(\w+)(?:\[\w+\])*\s*[,;]", body)
    # sp_render_style keeps its size
    assert ctypes.sizeof(_lib.RenderStyle) == 4 + 512 + 16 + 4 + 8 + 8 + 96
    names = [os.path.basename(s) for s in build.sources()]
    assert "labels.hip" in names and "render.hip" in names
    for f in ("sp_font.h", "sp_label.h"):                        # headers every object depends on: build._stale and build() glob them
        assert os.path.isfile(os.path.join(build.CSRC, f))


# ---- the font ---------------------------------------------------------------------------------------------------------------------------
def test_font_glyphs():
    assert _glyph(ord(" ")) == bytes(7)
    assert _glyph(ord("0")) == bytes([0b01110, 0b10001, 0b10011, 0b10101, 0b11001, 0b10001, 0b01110])
    assert _glyph(ord("1")) == bytes([0b00100, 0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110])
    assert _glyph(ord("#")) == bytes([0b01010, 0b01010, 0b11111, 0b01010, 0b11111, 0b01010, 0b01010])
    assert _glyph(ord("A")) == bytes([0b01110, 0b10001, 0b10001, 0b10001, 0b11111, 0b10001, 0b10001])
    every = [_glyph(c) for c in range(0x20, 0x7F)]
    assert len(every) == 95 == len(set(every))
    assert all(any(g) for g in every[1:])
    assert all(b < 32 for g in every for b in g)
    lib, buf = _lib.lib(), (ctypes.c_uint8 * 7)()
    for ch in (31, 127, -1, 256):
        assert lib.sp_render_font_glyph(ch, buf) == -1 and b"no glyph" in lib.sp_last_error(), ch
    assert lib.sp_render_font_glyph(65, None) == -1 and b"null" in lib.sp_last_error()
    assert (label_ref.glyphs() == np.array([list(g) for g in every], np.uint8)).all()


# ---- argument checks --------------------------------------------------------------------------------------------------------------------
def test_workspace_bytes():
    lib, n = _lib.lib(), ctypes.c_int64(-1)
    assert lib.sp_render_labels_workspace_bytes(32, ctypes.byref(n)) == 0 and n.value == 33 * 116
    assert lib.sp_render_labels_workspace_bytes(0, ctypes.byref(n)) == 0 and n.value == 116
    assert lib.sp_render_labels_workspace_bytes(32, None) == -1 and b"null" in lib.sp_last_error()
    for rows in (-1, 2049):
        assert lib.sp_render_labels_workspace_bytes(rows, ctypes.byref(n)) == -1 and b"rows" in lib.sp_last_error()


def test_bad_arguments_return_einval_without_touching_the_gpu():
    lib = _lib.lib()
    good = label_scenes.style_struct(label_ref.Style())

    def call(img=ONE, h=48, w=64, box=ONE, score=ONE, tid=None, keep=ONE, kc=ONE, seg=ONE, image=0, rows=32, style=good, cap=ONE, ws=ONE):
        return lib.sp_render_labels_u8c3(img, h, w, box, score, tid, keep, kc, seg, image, rows, None if style is None else ctypes.byref(style),
                                         cap, ws, None)

    for kw in ({"img": None}, {"box": None}, {"score": None}, {"keep": None}, {"kc": None}, {"seg": None}, {"style": None}, {"ws": None}):
        assert call(**kw) == -1 and b"null" in lib.sp_last_error(), kw
    for field, values, word in (("label_scale", (0, 9, -1), b"scale"), ("caption_scale", (0, 9), b"scale"), ("label_opacity", (-1, 17), b"opacity"),
                                ("caption_opacity", (-1, 17), b"opacity"), ("caption_corner", (-1, 4), b"caption_corner"),
                                ("palette_n", (0, 33), b"palette_n"), ("template_len", (-1, 33), b"template length")):
        for v in values:
            st = label_scenes.style_struct(label_ref.Style())
            setattr(st, field, v)
            assert call(style=st) == -1 and word in lib.sp_last_error(), (field, v)
    for byte, word in ((0x00, b"neither printable"), (0x06, b"neither printable"), (0x1F, b"neither printable"), (0x7F, b"neither printable"),
                       (0x80, b"neither printable"), (0x04, b"caption field"), (0x05, b"caption field")):
        st = label_scenes.style_struct(label_ref.Style(b"ab\x01"))
        st.label_template[1] = byte
        assert call(style=st) == -1 and word in lib.sp_last_error() and b"byte 1" in lib.sp_last_error(), byte
    for kw in ({"h": 0}, {"w": 0}, {"h": 16385}, {"w": 16385}, {"h": -4}):
        assert call(**kw) == -1 and b"image" in lib.sp_last_error(), kw
    assert call(image=-1) == -1 and b"image index" in lib.sp_last_error()
    for rows in (-1, 2049):
        assert call(rows=rows) == -1 and b"rows" in lib.sp_last_error()
    assert call(ws=ctypes.c_void_p(4098)) == -1 and b"aligned" in lib.sp_last_error()
    # nothing to do, nothing launched: no rows and no caption; no template and no caption
    assert call(rows=0, cap=None, box=None, score=None, keep=None, kc=None, seg=None, ws=None) == 0
    assert call(style=label_scenes.style_struct(label_ref.Style(b"")), cap=None, box=None, score=None, keep=None, kc=None, seg=None, ws=None) == 0


def test_renderer_text_option_refusals():
    from simple_pose_amd.visualize import PoseRenderer
    for kw, name in (({"label": "{who}"}, "label"), ({"label": "{n}"}, "label"), ({"label": "{image}"}, "label"), ({"label": "café"}, "label"),
                     ({"label": "a\tb"}, "label"), ({"label": "x" * 33}, "label"), ({"label": 7}, "label"), ({"label": "{id"}, "label"),
                     ({"label": "id}"}, "label"), ({"label_scale": 0}, "label_scale"), ({"label_scale": 9}, "label_scale"),
                     ({"label_scale": 2.0}, "label_scale"), ({"label_scale": True}, "label_scale"), ({"label_opacity": 1.5}, "label_opacity"),
                     ({"label_opacity": -0.1}, "label_opacity"), ({"caption": "{id}"}, "caption"), ({"caption": "{score}"}, "caption"),
                     ({"caption": "{x}"}, "caption"), ({"caption": "y" * 65}, "caption"), ({"caption": "ü"}, "caption"),
                     ({"caption": []}, "caption"), ({"caption": ["ok", 3]}, "caption"), ({"caption": 3}, "caption"),
                     ({"caption_scale": 0}, "caption_scale"), ({"caption_scale": 9}, "caption_scale"), ({"caption_corner": "top"}, "caption_corner"),
                     ({"caption_opacity": 2}, "caption_opacity")):
        with pytest.raises(ValueError, match=name):
            PoseRenderer(**kw)
    r = PoseRenderer(caption="a")
    with pytest.raises(ValueError, match="caption"):
        r.caption = "{conf}"
    assert r.caption == "a"                                      # a refused assignment changes nothing
    r.caption = ["x", "y {n}"]
    assert r.caption_rows(2).shape == (2, 64) and bytes(r.caption_rows(2)[1, :5]) == b"y \x04\x00\x00"
    for images in (1, 3):
        with pytest.raises(ValueError, match="one per image"):
            r.caption_rows(images)
    r.caption = "z{image}"
    assert bytes(r.caption_rows(3)[2, :3]) == b"z\x05\x00"


# ---- parsing and keys -------------------------------------------------------------------------------------------------------------------
def test_template_parser():
    """Braces CAN be escaped: `{{` and `}}` are literal braces, as in str.format; a lone brace is an error."""
    from simple_pose_amd.visualize import CAPTION_FIELDS, LABEL_FIELDS, PoseRenderer, parse_template
    assert parse_template("#{id} {score}", LABEL_FIELDS, 32, "label") == b"#\x01 \x02"
    assert parse_template("{conf}", LABEL_FIELDS, 32, "label") == b"\x03"
    assert parse_template("cam {image}: {n}", CAPTION_FIELDS, 64, "caption") == b"cam \x05: \x04"
    assert parse_template("{{id}} {{{id}}}", LABEL_FIELDS, 32, "label") == b"{id} {\x01}"
    assert parse_template("", LABEL_FIELDS, 32, "label") == b""
    for bad in ("{name}", "{", "}", "{ id}", "{ID}", "a{b", "{}"):
        with pytest.raises(ValueError, match="label"):
            parse_template(bad, LABEL_FIELDS, 32, "label")
    # a field is one byte: 32 pass, 33 do not
    assert len(parse_template("{score}" + "x" * 31, LABEL_FIELDS, 32, "label")) == 32
    assert PoseRenderer(label="x" * 32).label == b"x" * 32
    with pytest.raises(ValueError, match="33 bytes"):
        parse_template("{score}" + "x" * 32, LABEL_FIELDS, 32, "label")
    r = PoseRenderer(label="#{id} {score}", label_scale=3, label_opacity=0.5, caption="cam {image}", caption_corner="br")
    ls = r._label_style
    assert ls.template_len == 4 and bytes(ls.label_template)[:5] == b"#\x01 \x02\x00"
    assert (ls.label_scale, ls.label_opacity, ls.caption_scale, ls.caption_opacity, ls.caption_corner) == (3, 8, 2, 12, 3)
    assert ls.palette_n == 20 and bytes(ls.palette[1]) == bytes([31, 112, 255])


def test_key_tells_label_options_apart_but_not_caption_texts():
    from simple_pose_amd.visualize import DEFAULT_PALETTE, COCO_SKELETON, PoseRenderer
    base = PoseRenderer()
    today = (tuple(COCO_SKELETON), 48, 16, 8, 16, 0.2, "person", np.asarray(DEFAULT_PALETTE, np.uint8).tobytes())
    assert base.key()[:len(today)] == today
    assert not base.has_text and base.label is None and base.caption is None
    keys = [base.key()] + [PoseRenderer(**kw).key() for kw in ({"label": "{id}"}, {"label": "{score}"}, {"label": "{id}", "label_scale": 3},
                                                                {"label": "{id}", "label_opacity": 0.5}, {"caption": "a"},
                                                                {"caption": "a", "caption_scale": 3}, {"caption": "a", "caption_corner": "br"},
                                                                {"caption": "a", "caption_opacity": 1.0})]
    assert len(set(keys)) == len(keys)
    r = PoseRenderer(caption="a")
    k = r.key()
    r.caption = "another text {n}"
    assert r.key() == k == PoseRenderer(caption=["p", "q"]).key()
    r.caption = None
    assert r.key() == base.key()


# ---- label_ref on hand-made cases -------------------------------------------------------------------------------------------------------
def test_ref_number_format():
    # the double products: 0.995 * 100.0 is 99.5 exactly (the tie goes to the even 100), 12.345 * 100.0 is 1234.5 exactly (to the even 1234)
    want = ((0.0, "0.00"), (-0.0, "0.00"), (0.004999, "0.00"), (0.995, "1.00"), (1.0, "1.00"), (12.345, "12.34"), (1e9, "99.99"), (99.99, "99.99"),
            (99.996, "99.99"), (0.93, "0.93"), (-0.1, "?"), (float("nan"), "?"), (float("inf"), "?"), (-float("inf"), "?"))
    for v, text in want:
        assert label_ref.number(v) == text, v
    # 0.125 * 100 = 12.5 exactly: ties to even
    assert label_ref.number(0.125) == "0.12" and label_ref.number(0.375) == "0.38"


def test_ref_texts_and_truncation():
    T = label_scenes.T_FULL
    assert label_ref.label_text(T, 4, 17, 0.931, 0.5) == "#17 0.93 0.50"
    assert label_ref.label_text(T, 4, 0, 0.931, 0.5) == "#5 0.93 0.50" == label_ref.label_text(T, 4, None, 0.931, 0.5) == label_ref.label_text(T, 4, -5, 0.931, 0.5)
    assert label_ref.label_text(b"\x01", 0, 2147483647, 0, 0) == "2147483647"
    assert label_ref.label_text(b"x" * 30, 0, 1, 0, 0) == "x" * 24
    assert label_ref.caption_text(b"cam \x05: \x04" + bytes(55), 260, 3) == "cam 3: 260"
    assert label_ref.caption_text(b"a\x80b\x01c\x7f" + bytes(58), 0, 0) == "a?b?c?"
    assert label_ref.caption_text(b"\x04" * 64, 260, 0) == ("260" * 22)[:64]
    assert label_ref.caption_text(bytes(range(0x30, 0x70)), 1, 1) == bytes(range(0x30, 0x70)).decode()


def test_ref_one_label_pixel_by_pixel():
    """"1" at scale 2, opacity 16, box corner (10.4, 30.0): a 14 x 18 plate at (10, 12); palette[0] is light, so the text is black."""
    img = np.full((40, 50, 3), 99, np.uint8)
    st = label_ref.Style(b"\x01", label_scale=2, palette=[(200, 220, 240), (10, 20, 30)])
    box = np.array([[10.4, 30.0, 20, 39, 0.5]], np.float32)
    out = label_ref.render(img, st, box, np.array([0.5]), None, 1)
    assert (out[12:30, 10:24] != 99).all() and (out[11] == 99).all() and (out[30] == 99).all() and (out[:, 9] == 99).all() and (out[:, 24] == 99).all()
    ink = (out[12:30, 10:24] == 0).all(axis=2)
    rows = [0b00100, 0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110]
    want = np.zeros((9, 7), bool)
    for r, bits in enumerate(rows):
        for c in range(5):
            want[1 + r, 1 + c] = bool(bits >> (4 - c) & 1)
    assert (ink == np.kron(want, np.ones((2, 2), bool))).all()
    assert out[12, 10].tolist() == [200, 220, 240]
    # id 2 -> palette[1], dark: white text; half opacity blends once
    half = label_ref.render(img, label_ref.Style(b"\x01", label_scale=2, label_opacity=8, palette=st.palette), box, np.array([0.5]), np.array([2]), 1)
    assert half[12, 10].tolist() == [(99 * 128 + c * 128 + 128) >> 8 for c in (10, 20, 30)]
    assert half[12 + 2, 10 + 6].tolist() == [(99 * 128 + 255 * 128 + 128) >> 8] * 3          # font pixel (col 2, row 0) of "2" is set
    # the top edge flips the label inside; the right edge shifts it left; a corner q rejects draws nothing
    top = label_ref.render(img, st, np.array([[10.4, 5.0, 20, 39, 0.5]], np.float32), np.array([0.5]), None, 1)
    assert (top[5:23, 10:24] != 99).all() and (top[:5] == 99).all()
    right = label_ref.render(img, st, np.array([[45.0, 30.0, 60, 39, 0.5]], np.float32), np.array([0.5]), None, 1)
    assert (right[12:30, 36:50] != 99).all() and (right[:, 35] == 99).all()
    for bad in (np.nan, np.inf, 4e4):
        assert (label_ref.render(img, st, np.array([[bad, 30.0, 60, 39, 0.5]], np.float32), np.array([0.5]), None, 1) == 99).all()


def test_ref_caption_corners_and_order():
    img = np.full((40, 60, 3), 99, np.uint8)
    cap = label_scenes.captions([b"\x04"])[0]
    for corner, (y, x) in (("tl", (1, 1)), ("tr", (1, 52)), ("bl", (30, 1)), ("br", (30, 52))):
        out = label_ref.render(img, label_ref.Style(b"", caption_corner=corner, caption_opacity=16), np.zeros((0, 5), np.float32), np.zeros(0), None, 7, 0, cap)
        changed = np.argwhere((out != 99).any(axis=2))
        assert changed.min(axis=0).tolist() == [y, x] and changed.max(axis=0).tolist() == [y + 8, x + 6], corner
        assert out[y, x].tolist() == [0, 0, 0] and out[y + 1, x + 1].tolist() == [255, 255, 255]      # "7" starts with a full row
    # the best pose's label (pick 0) lies on top of pick 1's
    sc = label_scenes.overlap()
    st = label_ref.Style(label_scenes.T_SHORT)
    box, score, tid, n = label_ref.kept(sc, 0)
    both = label_ref.render(sc["img"], st, box, score, tid, n)
    first = label_ref.render(sc["img"], st, box[:1], score[:1], tid[:1], 1)
    assert n == 2 and (both[11:20, 20:23] == first[11:20, 20:23]).all() and (both != first).any()


def test_crowd_scene_crosses_the_scan_chunk():
    sc = label_scenes.crowd(260)
    assert sc["box"].shape[0] == 260 > label_scenes.CHUNK and int(sc["keep_count"][0]) == 260
    names = [c["name"] for c in label_scenes.cases()]
    assert len(names) == len(set(names))
