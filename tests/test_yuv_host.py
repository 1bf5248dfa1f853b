"""YUV 4:2:0 <-> BGR, host side: the integer contract (tests/yuv_ref.py) against its float64 definition over all 2^24 triples, the encode
ranges, grey and the extremes, the sp_yuv_ref mirror, the new symbols without an ABI bump, and everything the entry points and
simple_pose_amd.video refuse before a launch.  No GPU is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib
from simple_pose_amd.build import LIB_PATH
from simple_pose_amd.mixed_batch import check_images
from simple_pose_amd.video import REF_BYTES, YuvBatch, YuvFrame, from_bgr, to_bgr
from tests import yuv_ref
from tests.yuv_ref import BT601, BT709, FULL, I420, LIMITED, MODES, NV12

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sp_yuv420_to_bgr_u8c3", "sp_yuv420_to_bgr_images_u8c3", "sp_bgr_to_yuv420_u8c3", "sp_bgr_to_yuv420_images_u8c3", "sp_yuv420_wide_path")
ONE = ctypes.c_void_p(4096)          # non-null pointers that are never dereferenced: every call below fails its argument check first
TWO, THREE, FOUR = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20)
MODE_IDS = ["bt601-full", "bt601-limited", "bt709-full", "bt709-limited"]


def _all_triples():
    a = np.arange(256, dtype=np.int64)
    return np.meshgrid(a, a, a, indexing="ij", sparse=True)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_integer_contract_is_within_one_level_of_float64_over_all_triples(mode):
    """Both directions, all 2^24 triples: every channel within 1 level of the float64 definition rounded half up, at most 0.5 % of the
    triples differing in a channel (a cap: the contract stays within 0.24 %); and the encode ranges."""
    A, B, C = _all_triples()
    ints = yuv_ref.decode_px(A, B, C, *mode)
    flts = yuv_ref.decode_px_f64(A, B, C, *mode)
    for name, i, f in zip("RGB", ints, flts):
        d = np.abs(i - f)
        print(f"decode {name}: max {int(d.max())}, differing {float((d > 0).mean()):.5f}")
        assert d.max() <= 1 and (d > 0).mean() <= 0.005, name
    ints = yuv_ref.encode_px(A, B, C, *mode)                     # (R, G, B) = the three axes
    flts = yuv_ref.encode_px_f64(A, B, C, *mode)
    for name, i, f in zip("YUV", ints, flts):
        d = np.abs(i - f)
        print(f"encode {name}: max {int(d.max())}, differing {float((d > 0).mean()):.5f}")
        assert d.max() <= 1 and (d > 0).mean() <= 0.005, name
    want = ((0, 255), (0, 255), (0, 255)) if mode[1] == FULL else ((16, 235), (16, 240), (16, 240))
    assert tuple((int(i.min()), int(i.max())) for i in ints) == want


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_grey_and_extremes(mode):
    g = np.arange(256)
    Y, U, V = yuv_ref.encode_px(g, g, g, *mode)
    assert (U == 128).all() and (V == 128).all()                 # grey carries no chroma in any mode
    lo, hi = (0, 255) if mode[1] == FULL else (16, 235)
    assert Y[0] == lo and Y[255] == hi                           # black and white
    R, G, B = yuv_ref.decode_px(Y, U, V, *mode)
    assert np.abs(R - g).max() <= 1 and (R == G).all() and (G == B).all() and R[0] == 0 and R[255] == 255
    # a frame of one colour keeps that chroma through the 2x2 average, odd sizes included
    bgr = np.empty((3, 5, 3), np.uint8)
    bgr[...] = (255, 0, 0)
    y, u, v = yuv_ref.bgr_to_yuv420(bgr, I420, *mode)
    Yp, Up, Vp = yuv_ref.encode_px(0, 0, 255, *mode)
    assert u.shape == (2, 3) and (y == Yp).all() and (u == Up).all() and (v == Vp).all()
    assert Up == (255 if mode[1] == FULL else 240)               # pure blue: the top of the U range


def test_ref_formats_agree_and_average_counts_edge_pixels_twice():
    rng = np.random.default_rng(3)
    bgr = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    y, uv = yuv_ref.bgr_to_yuv420(bgr, NV12, BT709, LIMITED)
    y2, u, v = yuv_ref.bgr_to_yuv420(bgr, I420, BT709, LIMITED)
    assert uv.shape == (3, 8) and (y == y2).all() and (uv[:, 0::2] == u).all() and (uv[:, 1::2] == v).all()
    _, Up, _ = yuv_ref.encode_px(bgr[..., 2], bgr[..., 1], bgr[..., 0], BT709, LIMITED)
    assert u[2, 3] == (4 * Up[4, 6] + 2) >> 2 and u[2, 0] == (2 * Up[4, 0] + 2 * Up[4, 1] + 2) >> 2
    assert (yuv_ref.yuv420_to_bgr((y, uv), 5, 7, NV12, BT709, LIMITED) == yuv_ref.yuv420_to_bgr((y, u, v), 5, 7, I420, BT709, LIMITED)).all()


def test_yuv_ref_mirrors_the_header():
    assert ctypes.sizeof(_lib.YuvRef) == REF_BYTES == 64 and ctypes.alignment(_lib.YuvRef) == 8
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    body = re.search(r"typedef struct sp_yuv_ref \{(.*?)\} sp_yuv_ref;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f for f, _ in _lib.YuvRef._fields_]
    assert [w for w in re.findall(r"[A-Za-z_]\w*", body) if w in fields] == fields          # the same members in the same order
    offsets = {f: getattr(_lib.YuvRef, f).offset for f in fields}
    assert offsets == {"y": 0, "u": 8, "v": 16, "bgr": 24, "h": 32, "w": 36, "pitch_y": 40, "pitch_c": 44, "pitch_bgr": 48, "format": 52,
                       "matrix": 56, "range": 60}
    for name, val in (("SP_YUV_NV12", 0), ("SP_YUV_I420", 1), ("SP_YUV_BT601", 0), ("SP_YUV_BT709", 1), ("SP_YUV_LIMITED", 0), ("SP_YUV_FULL", 1)):
        assert re.search(rf"#define {name} {val}\b", hdr) and getattr(_lib, name) == val == getattr(yuv_ref, name[7:])
    # the header's table is the reference's
    for (matrix, rng), row in yuv_ref.TABLE.items():
        label = f"BT.{'601' if matrix == BT601 else '709'} {'full' if rng == FULL else 'limited'}"
        line = re.search(rf"\* +{re.escape(label)} +(.*)", hdr).group(1)
        assert tuple(int(v) for v in line.split()) == row, label


def test_new_symbols_declared_exported_bound_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(sp_\w+)\s*\(", hdr, flags=re.M))
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(handle, name), name
    assert re.search(r"#define SP_ABI_VERSION 36\b", hdr)
    assert _lib.ABI_VERSION == 36 and _lib.lib().sp_abi_version() == 36


def _dec(lib, y=ONE, u=TWO, v=THREE, h=4, w=6, py=6, pc=6, fmt=NV12, matrix=BT601, rng=LIMITED, bgr=FOUR, pb=18):
    return lib.sp_yuv420_to_bgr_u8c3(y, u, v, h, w, py, pc, fmt, matrix, rng, bgr, pb, None)


def _enc(lib, bgr=FOUR, pb=18, h=4, w=6, fmt=NV12, matrix=BT601, rng=LIMITED, y=ONE, u=TWO, v=THREE, py=6, pc=6):
    return lib.sp_bgr_to_yuv420_u8c3(bgr, pb, h, w, fmt, matrix, rng, y, u, v, py, pc, None)


@pytest.mark.parametrize("call", (_dec, _enc), ids=("to_bgr", "from_bgr"))
def test_single_frame_calls_refuse_bad_arguments_without_touching_the_gpu(call):
    lib = _lib.lib()
    at = lambda a: ctypes.c_void_p(a)
    bad = (dict(h=0), dict(w=0), dict(h=32768), dict(w=32768), dict(h=-1), dict(py=5), dict(pc=5), dict(pb=17), dict(w=5, py=5, pb=15, pc=5),
           dict(fmt=I420, pc=2), dict(fmt=2), dict(fmt=-1), dict(matrix=2), dict(rng=2), dict(rng=-1), dict(y=None), dict(u=None),
           dict(bgr=None), dict(fmt=I420, pc=3, v=None),
           dict(bgr=ONE), dict(bgr=at(4096 + 23)), dict(bgr=at(4096 - 71)), dict(bgr=at((1 << 20) + 11)), dict(bgr=at((1 << 20) - 70)),
           dict(fmt=I420, pc=3, bgr=at((2 << 20) + 5)))
    for kw in bad:
        assert call(lib, **kw) == -1, kw
        msg = lib.sp_last_error().decode()
        assert msg.startswith("sp_yuv420_to_bgr_u8c3: " if call is _dec else "sp_bgr_to_yuv420_u8c3: "), (kw, msg)
    assert call(lib, w=5, py=5, pb=15, pc=5) == -1 and "pitch_c 5 below the chroma row (6 bytes)" in lib.sp_last_error().decode()
    assert call(lib, bgr=at(4096 + 23)) == -1 and "overlaps" in lib.sp_last_error().decode()


def test_encoder_refuses_output_planes_that_overlap_each_other():
    lib, at = _lib.lib(), (lambda a: ctypes.c_void_p(a))
    for kw in (dict(u=at(4096 + 23)), dict(fmt=I420, pc=3, v=at(4096 + 6)), dict(fmt=I420, pc=3, v=at((1 << 20) + 4))):
        assert _enc(lib, **kw) == -1 and "overlap each other" in lib.sp_last_error().decode(), kw


def test_table_calls_refuse_bad_arguments_and_take_an_empty_table():
    lib = _lib.lib()
    for fn in (lib.sp_yuv420_to_bgr_images_u8c3, lib.sp_bgr_to_yuv420_images_u8c3):
        assert fn(None, 0, 0, 0, None) == 0 and fn(ONE, 0, 8, 8, None) == 0                  # count == 0: nothing to do, nothing launched
        for args in ((None, 1, 8, 8), (ONE, -1, 8, 8), (ONE, 65536, 8, 8), (ONE, 1, 0, 8), (ONE, 1, 8, 0), (ONE, 1, 32768, 8), (ONE, 1, 8, 32768)):
            assert fn(*args, None) == -1 and lib.sp_last_error(), args


def test_wide_path_predicate():
    lib = _lib.lib()
    w = lambda y=4096, u=8192, v=0, bgr=16384, py=144, pc=144, pb=400, fmt=NV12: lib.sp_yuv420_wide_path(y, u, v, bgr, py, pc, pb, fmt)
    assert w() == 1 and w(v=7) == 1 and w(fmt=I420, v=12288, pc=80) == 1
    for kw in (dict(y=4097), dict(u=8200), dict(bgr=16392), dict(py=130), dict(pc=136), dict(pb=390), dict(fmt=I420, v=12296), dict(fmt=I420, v=7)):
        assert w(**kw) == 0, kw


def _planes(h, w, fmt=NV12):
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if fmt == NV12:
        return (np.zeros((h, w), np.uint8), np.zeros((ch, 2 * cw), np.uint8))
    return (np.zeros((h, w), np.uint8), np.zeros((ch, cw), np.uint8), np.zeros((ch, cw), np.uint8))


def test_yuv_frame_checks_everything_when_it_is_made():
    f = YuvFrame(_planes(5, 7), 5, 7)
    assert f.shape == (5, 7, 3) and f.is_host and (f.pitch_y, f.pitch_c) == (7, 8) and f.codes == (NV12, BT601, LIMITED)
    f = YuvFrame(_planes(5, 7, I420), 5, 7, "i420", "bt709", True)
    assert (f.pitch_y, f.pitch_c) == (7, 4) and f.codes == (I420, BT709, FULL)
    buf = np.zeros((9, 32), np.uint8)                            # pitched views: stride(0) is the pitch
    f = YuvFrame((buf[:5, :7], buf[5:8, :8]), 5, 7)
    assert (f.pitch_y, f.pitch_c) == (32, 32)
    assert YuvFrame((buf[:5, :7], buf[5:8, :8].reshape(3, 4, 2)), 5, 7).pitch_c == 32         # UV as [ch, cw, 2] pairs
    assert isinstance(f[None], YuvBatch) and f[None].shape == (1, 5, 7, 3)
    y, uv = _planes(5, 7)
    with pytest.raises(ValueError, match="format"):
        YuvFrame((y, uv), 5, 7, "nv21")
    with pytest.raises(ValueError, match="matrix"):
        YuvFrame((y, uv), 5, 7, "nv12", "bt2020")
    with pytest.raises(TypeError, match="full_range"):
        YuvFrame((y, uv), 5, 7, "nv12", "bt601", 1)
    for hw in ((0, 7), (5, 0), (32768, 7), (5.0, 7), (True, 7)):
        with pytest.raises(ValueError, match="height|width"):
            YuvFrame((y, uv), *hw)
    with pytest.raises(ValueError, match=r"\(Y\).*expected \[5, 7\]"):      # wrong plane shape
        YuvFrame((np.zeros((5, 8), np.uint8), uv), 5, 7)
    with pytest.raises(ValueError, match=r"\(UV\).*expected \[3, 8\]"):
        YuvFrame((y, np.zeros((3, 7), np.uint8)), 5, 7)
    with pytest.raises(ValueError, match="has 3 planes"):
        YuvFrame((y, uv), 5, 7, "i420")
    with pytest.raises(TypeError, match="uint8"):                          # wrong dtype
        YuvFrame((y.astype(np.int16), uv), 5, 7)
    with pytest.raises(TypeError, match="uint8"):
        YuvFrame((y, uv.astype(np.float32)), 5, 7)
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):     # a CPU tensor
        YuvFrame((torch.zeros((5, 7), dtype=torch.uint8), torch.zeros((3, 8), dtype=torch.uint8)), 5, 7)
    with pytest.raises(ValueError, match="pitch 4 is below the row"):      # overlapping rows: a pitch below the row
        YuvFrame((np.lib.stride_tricks.as_strided(np.zeros(64, np.uint8), (5, 7), (4, 1)), uv), 5, 7)
    with pytest.raises(ValueError, match="inner stride"):
        YuvFrame((np.zeros((5, 14), np.uint8)[:, ::2], uv), 5, 7)
    with pytest.raises(ValueError, match="share one pitch"):
        YuvFrame((y, np.zeros((3, 4), np.uint8), np.zeros((3, 8), np.uint8)[:, :4]), 5, 7, "i420")
    with pytest.raises(TypeError, match="expected a CUDA uint8 tensor or a numpy"):
        YuvFrame((y, [[0] * 8] * 3), 5, 7)


def test_surface_and_i420_constructors():
    h, w, pitch = 5, 7, 16
    buf = np.arange((h + 3) * pitch, dtype=np.uint8)
    f = YuvFrame.from_surface(buf, h, w, pitch, "bt709")
    assert f.format == "nv12" and (f.pitch_y, f.pitch_c) == (16, 16) and f.planes[0][1, 2] == buf[18] and f.planes[1][2, 7] == buf[7 * 16 + 7]
    short = buf[:(h + 2) * pitch + 8]                            # the last UV row ends with the image
    f = YuvFrame.from_surface(short, h, w, pitch)
    assert f.planes[1].shape == (3, 8) and f.planes[1][2, 7] == buf[7 * 16 + 7]
    assert YuvFrame.from_surface(buf.reshape(h + 3, pitch), h, w).pitch_y == 16
    with pytest.raises(ValueError, match="fewer"):
        YuvFrame.from_surface(short[:-1], h, w, pitch)
    with pytest.raises(ValueError, match="pitch"):
        YuvFrame.from_surface(buf, h, w, 7)
    packed = np.arange(5 * 7 + 2 * 3 * 4, dtype=np.uint8)
    f = YuvFrame.from_i420(packed, 5, 7)
    assert f.format == "i420" and (f.pitch_y, f.pitch_c) == (7, 4) and f.planes[1][0, 0] == 35 and f.planes[2][0, 0] == 47
    with pytest.raises(ValueError, match="expected 59 bytes"):
        YuvFrame.from_i420(packed[:-1], 5, 7)


def test_to_bgr_and_from_bgr_refuse_before_any_launch():
    f = YuvFrame(_planes(4, 6), 4, 6)
    with pytest.raises(TypeError, match="YuvFrame"):
        to_bgr(np.zeros((4, 6, 3), np.uint8))
    with pytest.raises(TypeError, match="frame 1"):
        to_bgr([f, np.zeros((4, 6, 3), np.uint8)])
    with pytest.raises(ValueError, match="out"):
        to_bgr([f, f], out=[None])
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        to_bgr(f, out=torch.zeros((4, 6, 3), dtype=torch.uint8))
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        from_bgr(torch.zeros((4, 6, 3), dtype=torch.uint8))
    with pytest.raises(TypeError, match="expected a CUDA uint8 BGR image"):
        from_bgr(np.zeros((4, 6, 3), np.uint8))
    with pytest.raises(ValueError, match="format"):
        from_bgr(torch.zeros((4, 6, 3), dtype=torch.uint8), "yuyv")
    assert to_bgr([]) == [] and from_bgr([]) == []               # nothing to do, nothing launched


def test_image_checks_take_a_frame_for_the_image_it_stands_for():
    from simple_pose_amd.pipeline import TopDownPoseEstimator
    f, g = YuvFrame(_planes(48, 64), 48, 64), YuvFrame(_planes(47, 81, I420), 47, 81, "i420")
    assert check_images([f, np.zeros((9, 2, 3), np.uint8), g]) == [(48, 64), (9, 2), (47, 81)]
    shape_of = TopDownPoseEstimator._shape_of
    assert shape_of(f, batched=False) is f
    b = shape_of([f, f], batched=True)
    assert isinstance(b, YuvBatch) and b.shape == (2, 48, 64, 3) and shape_of(b, batched=True) is b
    with pytest.raises(ValueError, match="share one size"):
        shape_of([f, g], batched=True)
    with pytest.raises(ValueError, match="one image"):
        shape_of([f], batched=False)
    with pytest.raises(TypeError):
        shape_of(b, batched=False)
    with pytest.raises(TypeError):
        shape_of(f, batched=True)
