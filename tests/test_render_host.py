"""The overlay, host side: the two entry points are declared, exported and bound without an ABI bump and refuse bad arguments before they
touch the GPU; PoseRenderer's constructor refuses what it cannot draw; and tests/render_ref.py (the numpy restatement the kernels and the
CPU program are compared with) gives the answers written out here on hand-made cases."""
import ctypes
import os
import re

import numpy as np
import pytest

from simple_pose_amd import _lib
from simple_pose_amd.build import LIB_PATH
from tests import render_ref, render_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sp_render_workspace_bytes", "sp_render_poses_u8c3")
ONE = ctypes.c_void_p(4096)         # a non-null, aligned pointer that is never dereferenced: every call below fails its argument check first


def test_new_symbols_declared_exported_bound_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(sp_\w+)\s*\(", hdr, flags=re.M))
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(handle, name), name
    assert re.search(r"#define SP_ABI_VERSION 36\b", hdr)
    assert _lib.ABI_VERSION == 36 and _lib.lib().sp_abi_version() == 36
    for f in ("render.hip", "sp_render.h"):
        assert os.path.isfile(os.path.join(ROOT, "simple_pose_amd", "csrc", f))
    assert "sp_render_style" in hdr and ctypes.sizeof(_lib.RenderStyle) == 4 + 512 + 16 + 4 + 8 + 8 + 96       # (4 bytes pad before the double)


def test_workspace_bytes():
    lib, n = _lib.lib(), ctypes.c_int64(-1)
    assert lib.sp_render_workspace_bytes(32, 17, 19, ctypes.byref(n)) == 0 and n.value == 32 * (4 + 19 + 17) * 40
    assert lib.sp_render_workspace_bytes(0, 17, 19, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.sp_render_workspace_bytes(32, 17, 19, None) == -1 and b"null" in lib.sp_last_error()
    assert lib.sp_render_workspace_bytes(2049, 17, 19, ctypes.byref(n)) == -1 and b"rows" in lib.sp_last_error()
    assert lib.sp_render_workspace_bytes(32, 65, 19, ctypes.byref(n)) == -1 and b"joints" in lib.sp_last_error()
    assert lib.sp_render_workspace_bytes(32, 17, 65, ctypes.byref(n)) == -1 and b"edges" in lib.sp_last_error()


def test_bad_arguments_return_einval_without_touching_the_gpu():
    lib = _lib.lib()
    good = render_scenes.style_struct(render_ref.Style())

    def call(src=ONE, dst=ONE, h=48, w=64, kps=ONE, box=ONE, tid=None, keep=ONE, kc=ONE, seg=ONE, image=0, rows=32, joints=17, style=good, ws=ONE):
        return lib.sp_render_poses_u8c3(src, dst, h, w, kps, box, tid, keep, kc, seg, image, rows, joints,
                                        None if style is None else ctypes.byref(style), ws, None)

    for kw in ({"src": None}, {"dst": None}, {"kps": None}, {"box": None}, {"keep": None}, {"kc": None}, {"seg": None}, {"style": None}, {"ws": None}):
        assert call(**kw) == -1 and b"null" in lib.sp_last_error(), kw
    for joints in (0, 65, -1):
        assert call(joints=joints) == -1 and b"joints" in lib.sp_last_error()
    assert call(joints=16) == -1 and b"edge[" in lib.sp_last_error()             # COCO's skeleton names joint 16
    for field, values, word in (("joint_r", (-1, 1025), b"radius"), ("limb_r", (-1, 1025), b"radius"), ("box_r", (-1, 1025), b"radius"),
                                ("opacity", (-1, 17), b"opacity"), ("edges", (-1, 65), b"edges"), ("palette_n", (0, 33), b"palette_n"),
                                ("colour_by", (2,), b"colour_by")):
        for v in values:
            st = render_scenes.style_struct(render_ref.Style())
            setattr(st, field, v)
            assert call(style=st) == -1 and word in lib.sp_last_error(), (field, v)
    st = render_scenes.style_struct(render_ref.Style())
    st.edge[3][1] = -2
    assert call(style=st) == -1 and b"edge[3][1]" in lib.sp_last_error()
    for kw in ({"h": 0}, {"w": 0}, {"h": 16385}, {"w": 16385}, {"h": -4}):
        assert call(**kw) == -1 and b"image" in lib.sp_last_error(), kw
    assert call(image=-1) == -1 and b"image index" in lib.sp_last_error()
    assert call(rows=-1) == -1 and b"rows" in lib.sp_last_error()
    assert call(rows=2049) == -1 and b"rows" in lib.sp_last_error()
    for delta in (1, 48 * 64 * 3 - 1, -30):                                      # dst inside src's bytes, or src inside dst's
        assert call(dst=ctypes.c_void_p(4096 + delta)) == -1 and b"overlap" in lib.sp_last_error(), delta
    assert call(ws=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.sp_last_error()
    assert call(rows=0, kps=None, box=None, keep=None, kc=None, seg=None, ws=None) == 0      # in place, no rows: nothing to do, nothing launched


class _Model:
    training = False

    def hip_program(self, x):
        raise AssertionError("the constructor does not lower anything")


def test_renderer_constructor_refusals_and_quantisation():
    import torch
    from simple_pose_amd.pipeline import PoseResult, TopDownPoseEstimator
    from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
    from simple_pose_amd.visualize import COCO_SKELETON, PoseRenderer
    assert len(COCO_SKELETON) == 19 and COCO_SKELETON == render_ref.COCO_SKELETON
    assert {v for e in COCO_SKELETON for v in e} == set(range(17)) and len(set(map(frozenset, COCO_SKELETON))) == 19
    for kw, name in (({"skeleton": [(0, 64)]}, "skeleton"), ({"skeleton": [(0, -1)]}, "skeleton"), ({"skeleton": [(0, 1.5)]}, "skeleton"),
                     ({"skeleton": [(0, 1)] * 65}, "skeleton"), ({"skeleton": 7}, "skeleton"), ({"skeleton": [(0, 1, 2)]}, "skeleton"),
                     ({"joint_radius": -1.0}, "joint_radius"), ({"joint_radius": 64.5}, "joint_radius"), ({"joint_radius": "3"}, "joint_radius"),
                     ({"joint_radius": True}, "joint_radius"), ({"limb_width": -0.5}, "limb_width"), ({"limb_width": 129.0}, "limb_width"),
                     ({"box_width": -1}, "box_width"), ({"box_width": float("nan")}, "box_width"), ({"opacity": 1.5}, "opacity"),
                     ({"opacity": -0.1}, "opacity"), ({"in_vis_thre": "x"}, "in_vis_thre"), ({"in_vis_thre": float("nan")}, "in_vis_thre"),
                     ({"colour_by": "limb"}, "colour_by"), ({"palette": []}, "palette"), ({"palette": [(0, 0, 256)]}, "palette"),
                     ({"palette": [(0, 0)]}, "palette"), ({"palette": [(1, 2, 3)] * 33}, "palette"), ({"palette": [(0.5, 0, 0)]}, "palette")):
        with pytest.raises(ValueError, match=name):
            PoseRenderer(**kw)
    r = PoseRenderer()
    assert (r.joint_r, r.limb_r, r.box_r, r.opacity16, r.in_vis_thre, r.colour_by) == (48, 16, 8, 16, 0.2, "person")
    r2 = PoseRenderer(joint_radius=2.53, limb_width=3.1, box_width=0, opacity=0.7, colour_by="part", palette=[(1, 2, 3), (4, 5, 6)])
    assert (r2.joint_r, r2.limb_r, r2.box_r, r2.opacity16) == (40, 25, 0, 11) and r2._style.palette_n == 2 and r2._style.palette[1][2] == 6
    assert r.key() == PoseRenderer().key() != r2.key()
    assert r._style.edges == 19 and (r._style.edge[0][0], r._style.edge[0][1]) == (15, 13)
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        r.render(torch.zeros((48, 64, 3), dtype=torch.uint8), PoseResult(np.zeros((0, 17, 3)), np.zeros(0), np.zeros((0, 5), np.float32)))
    with pytest.raises(TypeError, match="uint8"):
        r.render(np.zeros((48, 64, 3), np.float32), None)
    # the estimator takes a renderer or nothing
    det = object.__new__(YOLOv5Detector)
    det.device = "cuda:0"
    with pytest.raises(TypeError, match="renderer"):
        TopDownPoseEstimator(det, _Model(), renderer=object())
    est = TopDownPoseEstimator(det, _Model(), renderer=r)
    assert est.renderer is r and TopDownPoseEstimator(det, _Model()).renderer is None
    res = PoseResult(np.zeros((1, 17, 3)), np.zeros(1), np.zeros((1, 5), np.float32))
    assert res.image is None and res.track_id is None


# ---- render_ref on hand-made cases ----------------------------------------------------------------------------------------------------------
def test_ref_horizontal_limb_covers_its_row_and_nothing_two_rows_away():
    """y = 5.5 is the centre line of pixel row 5; r = 16 (1 px) reaches every sample of the row (|dy| <= 6/16 px) between the end points."""
    prim = render_ref.capsule(3.0, 5.5, 20.0, 5.5, 16, (1, 2, 3))
    assert prim[:5] == (48, 88, 320, 88, 16)
    y0, x0, k = render_ref.coverage(prim, 12, 30)
    row = lambda y: k[y - y0] if y0 <= y < y0 + k.shape[0] else np.zeros(k.shape[1], np.int64)
    assert (row(5)[3 - x0:20 - x0] == 16).all()
    assert (row(7) == 0).all() and (row(3) == 0).all()
    assert 0 < row(4)[10 - x0] < 16 and row(4)[10 - x0] == row(6)[10 - x0]          # the neighbours are partly covered, alike
    assert k[:, 25 - x0:].sum() == 0                                                  # and nothing far past the end


def test_ref_disc_is_symmetric_under_xy_swap():
    for cx, cy, r in ((10.3, 7.9, 48), (6.5, 6.5, 33), (9.0625, 12.4375, 80)):
        a = render_ref.coverage(render_ref.capsule(cx, cy, cx, cy, r, (0, 0, 0)), 40, 40)
        b = render_ref.coverage(render_ref.capsule(cy, cx, cy, cx, r, (0, 0, 0)), 40, 40)
        full_a, full_b = np.zeros((40, 40), np.int64), np.zeros((40, 40), np.int64)
        full_a[a[0]:a[0] + a[2].shape[0], a[1]:a[1] + a[2].shape[1]] = a[2]
        full_b[b[0]:b[0] + b[2].shape[0], b[1]:b[1] + b[2].shape[1]] = b[2]
        assert full_a.sum() > 0 and (full_a == full_b.T).all()


def test_ref_full_opacity_on_a_full_pixel_is_the_colour_and_zero_opacity_changes_nothing():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (20, 24, 3), dtype=np.uint8)
    kps = np.zeros((1, 17, 3))
    kps[0, :, :2], kps[0, :, 2] = (12.5, 9.5), 1.0
    box = np.array([[2, 2, 20, 18, 1]], np.float32)
    st = render_ref.Style(skeleton=(), joint_r=64, box_r=0, opacity=16, palette=[(9, 200, 77)])
    out = render_ref.render(img, st, kps, box)
    assert out[9, 12].tolist() == [9, 200, 77] and out[8, 11].tolist() == [9, 200, 77]        # k = 16: the colour exactly
    assert (out[0] == img[0]).all() and (out != img).any()
    st0 = render_ref.Style(opacity=0)
    assert (render_ref.render(img, st0, kps, box) == img).all()
    half = render_ref.render(img, render_ref.Style(skeleton=(), joint_r=64, box_r=0, opacity=8, palette=[(9, 200, 77)]), kps[:, :1], box)     # ONE disc, blended once
    assert half[9, 12].tolist() == [(int(v) * 128 + c * 128 + 128) >> 8 for v, c in zip(img[9, 12], (9, 200, 77))]


def test_ref_quantisation_visibility_order_and_colours():
    assert render_ref.quantise(1.03125) == 16 and render_ref.quantise(1.09375) == 18 and render_ref.quantise(-0.03125) == 0     # ties to even
    assert render_ref.quantise(32768.0) == 524288 and render_ref.quantise(32768.01) is None
    assert render_ref.quantise(np.nan) is None and render_ref.quantise(-np.inf) is None
    st = render_ref.Style(palette=[(1, 1, 1), (2, 2, 2), (3, 3, 3)])
    kps = np.ones((2, 17, 3))
    kps[0, 5, 2], kps[1, 6, 2] = 0.2, np.nan                                           # c == thre and NaN: not visible
    box = np.array([[0, 0, 4, 4, 1], [1, 1, 5, 5, 1]], np.float32)
    prims = render_ref.primitives(st, kps, box, None)
    per = 4 + 19 + 17
    assert len(prims) == 2 * per
    assert prims[0][5] == (2, 2, 2) and prims[per][5] == (1, 1, 1)                     # pick 1 is painted first, pick 0 last (on top)
    assert prims[per + 4 + 19 + 5] is None and prims[4 + 19 + 6] is None and prims[per + 4 + 19 + 6] is not None
    limbs5 = [e for e, ab in enumerate(render_ref.COCO_SKELETON) if 5 in ab]
    assert limbs5 and all(prims[per + 4 + e] is None for e in limbs5)
    prims = render_ref.primitives(st, kps, box, np.array([5, 0], np.int32))
    assert prims[per][5] == (2, 2, 2) and prims[0][5] == (2, 2, 2)                     # id 5 -> palette[4 % 3]; id 0 -> pick position 1
    part = render_ref.primitives(render_ref.Style(colour_by="part", palette=[(1, 1, 1), (2, 2, 2), (3, 3, 3)]), kps, box, None)
    assert part[4 + 4][5] == (2, 2, 2) and part[4 + 19 + 2][5] == (3, 3, 3) and part[1][5] == (2, 2, 2)
    assert render_ref.primitives(render_ref.Style(box_r=0), kps, box)[:4] == [None] * 4


def test_crowd_scene_crosses_the_scan_chunk_and_the_list_limit():
    """The scene the GPU test relies on: more than two scan chunks, and one tile whose list must be applied before the scan ends."""
    sc = render_scenes.crowd(24)
    kps, box, tid = render_ref.kept(sc["kps"], sc["box"], sc["track_id"], sc["keep"], sc["keep_count"], sc["seg"], 0)
    prims = render_ref.primitives(render_scenes.styles()["part"], kps, box, tid)
    assert len(prims) == 24 * 40 > 2 * render_scenes.CHUNK
    assert render_ref.tile_hits(prims, 40, 132).max() > render_scenes.LIST
