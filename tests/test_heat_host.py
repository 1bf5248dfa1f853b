"""The heat overlay, host side: the two entry points are declared, exported and bound without an ABI bump and refuse bad arguments before
they touch the GPU; HeatOverlay's and the estimator's constructors refuse what they cannot do; and tests/heat_ref.py (the numpy
restatement the kernels and the CPU program are compared with) has the properties an overlay must have, on hand-made cases and on the
scenes the GPU tests use."""
import ctypes
import os
import re

import numpy as np
import pytest

from simple_pose_amd import _lib
from simple_pose_amd.build import LIB_PATH
from tests import heat_ref, heat_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sp_heat_overlay_workspace_bytes", "sp_heat_overlay_u8c3")
ONE = ctypes.c_void_p(4096)         # a non-null, aligned pointer that is never dereferenced: every call below fails its argument check first
S = heat_ref.Style


def test_new_symbols_declared_exported_bound_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(sp_\w+)\s*\(", hdr, flags=re.M))
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(handle, name), name
    assert re.search(r"#define SP_ABI_VERSION 36\b", hdr)
    assert _lib.ABI_VERSION == 36 and _lib.lib().sp_abi_version() == 36
    for f in ("heat.hip", "sp_heat.h"):
        assert os.path.isfile(os.path.join(ROOT, "simple_pose_amd", "csrc", f))
    assert "sp_heat_style" in hdr and ctypes.sizeof(_lib.HeatStyle) == 24
    H = _lib.HeatStyle
    assert (H.joint_mask.offset, H.scale.offset, H.threshold.offset, H.opacity16.offset, H.alpha.offset) == (0, 8, 12, 16, 20)
    assert (_lib.SP_HEAT_ALPHA_CONSTANT, _lib.SP_HEAT_ALPHA_VALUE) == (0, 1)
    assert re.search(r"#define SP_HEAT_ALPHA_CONSTANT 0\b", hdr) and re.search(r"#define SP_HEAT_ALPHA_VALUE 1\b", hdr)
    # the rules are stated once: the header calls the overlay's count clamp and the warps' inversion instead of restating them
    rules = open(os.path.join(ROOT, "simple_pose_amd", "csrc", "sp_heat.h")).read()
    assert "sp_invert_affine(" in rules and "sp_render_live(" in rules and "1. / D" not in rules and "keep_count[" not in rules
    assert "#pragma clang fp contract(off)" in rules
    assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "simple_pose_amd", "csrc", "heat.hip")).read()
    common = open(os.path.join(ROOT, "simple_pose_amd", "csrc", "sp_common.h")).read()
    assert '#include "sp_affine.h"' in common                   # sp_common.h still provides the inversion, from the one statement of it


def test_workspace_bytes():
    lib, n = _lib.lib(), ctypes.c_int64(-1)
    assert lib.sp_heat_overlay_workspace_bytes(32, 64, 48, ctypes.byref(n)) == 0 and n.value == 32 * (64 + 64 * 48)
    assert lib.sp_heat_overlay_workspace_bytes(0, 64, 48, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.sp_heat_overlay_workspace_bytes(2048, 256, 256, ctypes.byref(n)) == 0 and n.value == 2048 * (64 + 65536)
    assert lib.sp_heat_overlay_workspace_bytes(32, 64, 48, None) == -1 and b"null" in lib.sp_last_error()
    for rows in (2049, -1):
        assert lib.sp_heat_overlay_workspace_bytes(rows, 64, 48, ctypes.byref(n)) == -1 and b"rows" in lib.sp_last_error()
    for mh, mw in ((0, 48), (64, 0), (257, 48), (64, 257), (-1, 4)):
        assert lib.sp_heat_overlay_workspace_bytes(4, mh, mw, ctypes.byref(n)) == -1 and b"heat map" in lib.sp_last_error()


def test_bad_arguments_return_einval_without_touching_the_gpu():
    lib = _lib.lib()
    good = heat_scenes.style_struct(S())

    def call(src=ONE, dst=ONE, h=48, w=64, hm=ONE, joints=17, mh=64, mw=48, ti=ONE, keep=ONE, kc=ONE, seg=ONE, image=0, rows=32, style=good,
             lut=ONE, ws=ONE):
        return lib.sp_heat_overlay_u8c3(src, dst, h, w, hm, joints, mh, mw, ti, keep, kc, seg, image, rows,
                                        None if style is None else ctypes.byref(style), lut, ws, None)

    for kw in ({"src": None}, {"dst": None}, {"hm": None}, {"ti": None}, {"keep": None}, {"kc": None}, {"seg": None}, {"style": None},
               {"lut": None}, {"ws": None}):
        assert call(**kw) == -1 and b"null" in lib.sp_last_error(), kw
    for kw in ({"h": 0}, {"w": 0}, {"h": 16385}, {"w": 16385}, {"h": -4}):
        assert call(**kw) == -1 and b"image" in lib.sp_last_error(), kw
    for joints in (0, 65, -1):
        assert call(joints=joints) == -1 and b"joints" in lib.sp_last_error()
    for kw in ({"mh": 0}, {"mw": 0}, {"mh": 257}, {"mw": 257}, {"mw": -2}):
        assert call(**kw) == -1 and b"heat map" in lib.sp_last_error(), kw
    for rows in (-1, 2049):
        assert call(rows=rows) == -1 and b"rows" in lib.sp_last_error()
    assert call(image=-1) == -1 and b"image index" in lib.sp_last_error()
    for field, values, word in (("threshold", (0, 256, -1), b"threshold"), ("opacity16", (-1, 17), b"opacity16"), ("alpha", (-1, 2), b"alpha"),
                                ("scale", (float("nan"), float("inf"), -1.0, float("-inf")), b"scale")):
        for v in values:
            st = heat_scenes.style_struct(S())
            setattr(st, field, v)
            assert call(style=st) == -1 and word in lib.sp_last_error(), (field, v)
    for delta in (1, 48 * 64 * 3 - 1, -30):                                      # dst inside src's bytes, or src inside dst's
        assert call(dst=ctypes.c_void_p(4096 + delta)) == -1 and b"overlap" in lib.sp_last_error(), delta
    assert call(ws=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.sp_last_error()
    assert call(hm=ctypes.c_void_p(4098)) == -1 and b"aligned" in lib.sp_last_error()
    assert call(ti=ctypes.c_void_p(4097)) == -1 and b"aligned" in lib.sp_last_error()
    # in place, no rows: nothing to do, nothing launched, nothing but the image and the style looked at
    assert call(rows=0, hm=None, ti=None, keep=None, kc=None, seg=None, lut=None, ws=None) == 0
    st = heat_scenes.style_struct(S(scale=0.0, opacity16=0, threshold=255, alpha="constant"))
    assert call(rows=0, style=st) == 0                                           # the ends of every range are accepted


class _Model:
    training = False

    def hip_program(self, x):
        raise AssertionError("the constructor does not lower anything")


def test_heat_overlay_constructor_refusals_quantisation_and_colour_tables():
    import torch
    from simple_pose_amd.pipeline import TopDownPoseEstimator
    from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
    from simple_pose_amd.visualize import HeatOverlay, PoseRenderer, Redactor
    for kw, name in (({"colormap": "viridis"}, "colormap"), ({"colormap": np.zeros((256, 3), np.int32)}, "colormap"),
                     ({"colormap": np.zeros((255, 3), np.uint8)}, "colormap"), ({"colormap": 3}, "colormap"), ({"opacity": 1.1}, "opacity"),
                     ({"opacity": -0.1}, "opacity"), ({"opacity": "1"}, "opacity"), ({"opacity": True}, "opacity"), ({"alpha": "linear"}, "alpha"),
                     ({"alpha": 1}, "alpha"), ({"threshold": 1.5}, "threshold"), ({"threshold": -0.2}, "threshold"),
                     ({"threshold": float("nan")}, "threshold"), ({"gain": -1.0}, "gain"), ({"gain": float("inf")}, "gain"),
                     ({"gain": float("nan")}, "gain"), ({"gain": 1e38}, "gain"), ({"gain": "2"}, "gain"), ({"joints": []}, "joints"),
                     ({"joints": [0, 64]}, "joints"), ({"joints": [-1]}, "joints"), ({"joints": [1.5]}, "joints"), ({"joints": 3}, "joints"),
                     ({"joints": [True]}, "joints")):
        with pytest.raises(ValueError, match=name):
            HeatOverlay(**kw)
    h = HeatOverlay()
    assert (h.opacity16, h.alpha, h.threshold, float(h.scale), h.joint_mask, h.joints) == (10, "value", 25, 255.0, (1 << 64) - 1, None)
    s = h._style
    assert (s.joint_mask, s.scale, s.threshold, s.opacity16, s.alpha) == ((1 << 64) - 1, 255.0, 25, 10, 1)
    h2 = HeatOverlay(colormap="gray", opacity=1.0, alpha="constant", threshold=0.0, gain=0.1, joints=[9, 0, 9, 63])
    assert (h2.opacity16, h2.threshold, h2.scale, h2.joint_mask, h2.joints) == (16, 1, np.float32(255.0 * 0.1), (1 << 63) | (1 << 9) | 1, (0, 9, 63))
    assert HeatOverlay(threshold=1.0).threshold == 255 and HeatOverlay(threshold=0.5).threshold == 127 and HeatOverlay(gain=0).scale == 0
    assert h.key() == HeatOverlay().key() != h2.key()
    for kw in ({"colormap": "hot"}, {"opacity": 0.5}, {"alpha": "constant"}, {"threshold": 0.2}, {"gain": 2.0}, {"joints": [0]}):
        assert HeatOverlay(**kw).key() != h.key(), kw                            # everything the launch depends on is in the key
    # the tables: gray is the reference's GRAY2BGR; hot and jet are the written-down integer formulas, BGR
    assert (h2.lut == np.arange(256, dtype=np.uint8)[:, None]).all()
    hot, jet = HeatOverlay(colormap="hot").lut, h.lut
    assert hot.dtype == jet.dtype == np.uint8 and hot.shape == jet.shape == (256, 3)
    assert hot[0].tolist() == [0, 0, 0] and hot[85].tolist() == [0, 0, 255] and hot[170].tolist() == [0, 255, 255] and hot[255].tolist() == [255] * 3
    assert (np.diff(hot.astype(int), axis=0) >= 0).all()
    assert jet[0].tolist() == [127, 0, 0] and jet[64].tolist() == [255, 128, 0] and jet[255].tolist() == [0, 0, 127]
    assert jet[128].tolist() == [125, 255, 129] and jet[191].tolist() == [0, 128, 255]
    for v in (0, 1, 31, 32, 63, 64, 96, 127, 128, 160, 191, 192, 223, 224, 255):
        t = v / 255.0
        want = [255.0 * min(1.0, max(0.0, 1.5 - abs(4 * t - k))) for k in (1, 2, 3)]        # B, G, R of the classic definition
        assert np.abs(jet[v] - np.array(want)).max() <= 0.5 + 1e-9, v
    custom = heat_scenes.random_lut()
    hc = HeatOverlay(colormap=custom)
    custom[0, 0] ^= 1
    assert (hc.lut != custom).any() and hc.colormap is None                      # the overlay keeps its own copy
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        h.overlay(torch.zeros((48, 64, 3), dtype=torch.uint8), torch.zeros((1, 17, 64, 48)), torch.zeros((1, 2, 3)))
    with pytest.raises(TypeError, match="uint8"):
        h.overlay(np.zeros((48, 64, 3), np.float32), None, None)
    # the estimator takes a heat overlay or nothing, next to the others or alone
    det = object.__new__(YOLOv5Detector)
    det.device, det.conf_thresh, det.iou_thresh = "cuda:0", 0.25, 0.45
    for bad in (object(), PoseRenderer(), Redactor(), "jet"):
        with pytest.raises(TypeError, match="heat_overlay"):
            TopDownPoseEstimator(det, _Model(), heat_overlay=bad)
    est = TopDownPoseEstimator(det, _Model(), heat_overlay=h, redactor=Redactor(), renderer=PoseRenderer())
    bare = TopDownPoseEstimator(det, _Model())
    assert est.heat_overlay is h and bare.heat_overlay is None
    assert est._params(None, None)[-1] == (h.key(), id(h))
    # without an overlay the key is the key of before, entry for entry (the decoder's identity aside): nothing is appended
    none = TopDownPoseEstimator(det, _Model(), heat_overlay=None)._params(None, None)
    assert len(bare._params(None, None)) == len(none) == len(est._params(None, None)) - 1 and none[-1] is None
    other = TopDownPoseEstimator(det, _Model(), heat_overlay=HeatOverlay())      # equal parameters, another table in device memory
    assert other._params(None, None) != TopDownPoseEstimator(det, _Model(), heat_overlay=h)._params(None, None)


# ---- heat_ref: the properties of the overlay --------------------------------------------------------------------------------------------------
def _identity(n=1):
    return np.tile(np.array([[1, 0, 0], [0, 1, 0]], np.float32), (n, 1, 1))


def test_ref_identity_gray_is_the_references_draw_heat_map():
    """commons/transforms.py:56-61 with a mask of ones: max over the joints, * 255, astype(uint8), GRAY2BGR - on maps in [0, 1]."""
    rng = np.random.default_rng(0)
    hm = rng.uniform(0, 1, (1, 17, 64, 48)).astype(np.float32)
    hm[0, :, 5, 7] = np.float32(37) / np.float32(255)
    img = rng.integers(0, 256, (64, 48, 3), dtype=np.uint8)
    out = heat_ref.overlay(img, S(threshold=1, opacity16=16, alpha="constant"), hm, _identity(), [0], heat_ref.gray_lut())
    merge = hm[0].max(axis=0)
    want = (merge * 255).astype(np.uint8)                                        # float32 throughout, as numpy computes the reference's line
    assert merge.dtype == np.float32 and want.min() >= 1
    assert (out == want[..., None]).all()
    # the stand-in for the visibility mask: masked joints do not take part
    only = heat_ref.overlay(img, S(joint_mask=0b101, threshold=1, opacity16=16, alpha="constant"), hm, _identity(), [0], heat_ref.gray_lut())
    assert (only == (np.maximum(hm[0, 0], hm[0, 2]) * 255).astype(np.uint8)[..., None]).all()


def test_ref_quantisation_edges():
    q = lambda v, s=255.0: int(heat_ref.q8(np.array([v], np.float32), s)[0])
    assert [q(v) for v in (np.nan, np.inf, -np.inf, -0.5, 0.0, -0.0, 1.0, 1.7, 0.5, 1 / 255, 0.0039)] == [0, 255, 0, 0, 0, 0, 255, 255, 127, 1, 0]
    assert q(np.inf, 0.0) == 0 and q(5.0, 0.0) == 0 and q(254.999, 1.0) == 254 and q(255.0, 1.0) == 255
    for k in range(256):                                                         # k / 255 * 255 in float32: k, or the float just below it
        v = np.float32(k) / np.float32(255)
        assert q(v) in (k, k - 1) and q(v) == int(np.float32(v * np.float32(255)))
    nan_loses = heat_ref.plane(np.array([[[np.nan]], [[0.25]], [[np.nan]]], np.float32), 0b111, 255.0)
    assert nan_loses.tolist() == [[63]] and heat_ref.plane(np.full((2, 1, 1), np.nan, np.float32), 0b11, 255.0).tolist() == [[0]]
    assert heat_ref.plane(np.ones((17, 2, 2), np.float32), 1 << 17, 255.0) is None      # no bit below J


def test_ref_scale_by_four_puts_the_peak_at_the_mapped_pixel():
    hm = np.zeros((1, 3, 8, 8), np.float32)
    hm[0, 1, 2, 5] = 1.0
    ti = np.array([[[4, 0, 3], [0, 4, 1]]], np.float32)                          # heat (5, 2) -> image (23, 9)
    assert heat_ref.forward(ti[0]) == [16384, 0, -49152, 0, 16384, -16384]
    vm = heat_ref.vmax(40, 40, S(), hm, ti, [0])
    assert vm.max() == 255 and np.argwhere(vm == 255).tolist() == [[9, 23]]
    assert vm[9, 24] == 191 and vm[9, 22] == 191 and vm[10, 24] == (192 * 192 * 255 + 32768) >> 16 and vm[9, 27] == 0 and vm[9, 19] == 0
    assert (vm[:5] == 0).all() and (vm[:, :19] == 0).all()
    # a tap outside the map reads 0: a peak in the corner cell fades out over the same distance outside the map
    hm[:] = 0
    hm[0, 0, 0, 0] = 1.0
    vm = heat_ref.vmax(40, 40, S(), hm, ti, [0])
    assert vm[1, 3] == 255 and vm[1, 2] == 191 and vm[0, 3] == 191 and vm[1, 0] == 64      # (0, 1) is heat (-0.75, 0)
    assert vm[0, 0] == (64 * 192 * 255 + 32768) >> 16 == 48                      # (0, 0) is heat (-0.75, -0.25): the tap (0, 0) alone


def test_ref_threshold_order_and_singular_maps():
    rng = np.random.default_rng(2)
    scene = heat_scenes.make("street")
    img, hm, ti, lut = scene["img"], scene["hm"], scene["trans_inv"], scene["lut"]
    rows = heat_ref.live_rows(scene["keep"], scene["keep_count"], scene["seg"], 0, hm.shape[0])
    assert len(rows) == 5
    st = S(threshold=90)
    vm = heat_ref.vmax(97, 131, st, hm, ti, rows)
    out = heat_ref.overlay(img, st, hm, ti, rows, lut)
    assert ((vm > 0) & (vm < 90)).any() and (vm >= 90).any()
    assert (out[vm < 90] == img[vm < 90]).all() and (out[vm >= 90] != img[vm >= 90]).any()        # below the threshold: the source bytes
    # the order of the persons does not matter, and a person listed twice is a person listed once
    assert (heat_ref.overlay(img, st, hm, ti, rows[::-1], lut) == out).all()
    assert (heat_ref.overlay(img, st, hm, ti, list(rng.permutation(rows)) + rows, lut) == out).all()
    # the overlap of a and b is the maximum, not a sum or the later one
    a, b = (heat_ref.vmax(97, 131, st, hm, ti, [r]) for r in rows[:2])
    both = heat_ref.vmax(97, 131, st, hm, ti, rows[:2])
    assert ((a > 0) & (b > 0)).any() and (both == np.maximum(a, b)).all() and (a > b).any() and (b > a).any()
    # opacity 0 draws nothing; constant alpha at opacity 1 is the table's colour
    assert (heat_ref.overlay(img, S(opacity16=0), hm, ti, rows, lut) == img).all()
    full = heat_ref.overlay(img, S(opacity16=16, alpha="constant", threshold=90), hm, ti, rows, lut)
    assert (full[vm >= 90] == lut[vm[vm >= 90]]).all()
    # singular and refused maps draw nothing
    for bad in ([[0, 0, 0], [0, 0, 0]], [[1, 2, 3], [2, 4, 5]], [[np.nan, 0, 0], [0, 1, 0]], [[np.inf, 0, 0], [0, 1, 0]], [[1e-4, 0, 0], [0, 1, 0]],
                [[1, 0, -1048577.0], [0, 1, 0]]):
        assert heat_ref.forward(np.array(bad, np.float32)) is None, bad
        assert (heat_ref.overlay(img, S(threshold=1), hm, np.tile(np.array(bad, np.float32), (7, 1, 1)), rows, lut) == img).all()
    assert heat_ref.forward(np.array([[1, 0, -1048576.0], [0, 1, 0]], np.float32)) is not None
    assert heat_ref.forward(np.array([[1 / 1024, 0, 0], [0, 1, 0]], np.float32))[0] == 1024 * 65536


def test_scenes_hold_what_the_gpu_tests_rely_on():
    street = heat_scenes.make("street")
    rows = heat_ref.live_rows(street["keep"], street["keep_count"], street["seg"], 0, 7)
    per = [heat_ref.vmax(97, 131, S(), street["hm"], street["trans_inv"], [r]) for r in rows]
    assert ((per[0] > 0) & (per[1] > 0)).any()                                   # a and b overlap
    assert (per[2][:, -1] > 0).any() and (per[2] > 0).any()                       # c reaches the right edge: half outside
    assert not (per[3] > 0).any()                                                # d: wholly outside
    e = per[4] > 0                                                               # e: rotated - its pixels do not fill their bounding box
    ys, xs = np.nonzero(e)
    assert e.any() and e[ys.min():ys.max() + 1, xs.min():xs.max() + 1].mean() < 0.9
    ext = heat_scenes.make("extremes", seed=2)
    rows = heat_ref.live_rows(ext["keep"], ext["keep_count"], ext["seg"], 0, 7)
    c = [heat_ref.forward(ext["trans_inv"][r]) for r in rows]
    assert c[0][0] == 65536 // 80 + 0 or abs(c[0][0] - 65536 / 80) <= 1           # a cell covers 80 px: more than a tile
    assert c[1][0] > 48 * 65536 and c[2] is None and c[3][0] == 1024 * 65536 and c[4] is None
    one = heat_ref.vmax(97, 131, S(threshold=1), ext["hm"], ext["trans_inv"], [rows[3]])
    assert 1 <= (one > 0).sum() <= 4                                             # |F| == 1024: the whole map within a pixel or two
    lim = heat_scenes.make("limits", seed=4)
    rows = heat_ref.live_rows(lim["keep"], lim["keep_count"], lim["seg"], 0, 7)
    assert [heat_ref.forward(lim["trans_inv"][r]) is None for r in rows] == [False, True, True, True, False]
    for name, scene, style, image in heat_scenes.cases():
        assert scene["hm"].dtype == np.float32 and scene["trans_inv"].dtype == np.float32 and scene["lut"].shape == (256, 3), name
    specials = street["hm"]
    assert np.isnan(specials).any() and np.isposinf(specials).any() and np.isneginf(specials).any() and (specials > 1).any() and (specials < 0).any()
