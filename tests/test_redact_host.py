"""Redaction, host side: the two entry points are declared, exported and bound without an ABI bump and refuse bad arguments before they
touch the GPU; Redactor's constructor refuses what it cannot do; and tests/redact_ref.py (the numpy restatement the kernels and the CPU
program are compared with) has the properties a redaction must have, on hand-made cases and on the scenes the GPU tests use."""
import ctypes
import os
import re

import numpy as np
import pytest

from simple_pose_amd import _lib
from simple_pose_amd.build import LIB_PATH
from tests import redact_ref, redact_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sp_redact_workspace_bytes", "sp_redact_u8c3")
ONE = ctypes.c_void_p(4096)         # a non-null, aligned pointer that is never dereferenced: every call below fails its argument check first


def test_new_symbols_declared_exported_bound_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(sp_\w+)\s*\(", hdr, flags=re.M))
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(handle, name), name
    assert re.search(r"#define SP_ABI_VERSION 36\b", hdr)
    assert _lib.ABI_VERSION == 36 and _lib.lib().sp_abi_version() == 36
    for f in ("redact.hip", "sp_redact.h"):
        assert os.path.isfile(os.path.join(ROOT, "simple_pose_amd", "csrc", f))
    assert "sp_redact_style" in hdr and ctypes.sizeof(_lib.RedactStyle) == 6 * 4 + 8 * 4 + 2 * 4 + 8 + 8       # (fill[3] padded to 8)
    assert _lib.RedactStyle.in_vis_thre.offset == 64 and _lib.RedactStyle.fill.offset == 72
    # the rules are stated once: the header reuses the overlay's quantisation and clamp instead of restating them
    rules = open(os.path.join(ROOT, "simple_pose_amd", "csrc", "sp_redact.h")).read()
    assert "sp_render_q(" in rules and "sp_render_live(" in rules and "rint" not in rules


def test_workspace_bytes():
    lib, n = _lib.lib(), ctypes.c_int64(-1)
    assert lib.sp_redact_workspace_bytes(32, ctypes.byref(n)) == 0 and n.value == 32 * 36
    assert lib.sp_redact_workspace_bytes(0, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.sp_redact_workspace_bytes(2048, ctypes.byref(n)) == 0 and n.value == 2048 * 36
    assert lib.sp_redact_workspace_bytes(32, None) == -1 and b"null" in lib.sp_last_error()
    assert lib.sp_redact_workspace_bytes(2049, ctypes.byref(n)) == -1 and b"rows" in lib.sp_last_error()
    assert lib.sp_redact_workspace_bytes(-1, ctypes.byref(n)) == -1 and b"rows" in lib.sp_last_error()


def test_bad_arguments_return_einval_without_touching_the_gpu():
    lib = _lib.lib()
    good = redact_scenes.style_struct(redact_ref.Style())

    def call(src=ONE, dst=ONE, h=48, w=64, kps=ONE, box=ONE, keep=ONE, kc=ONE, seg=ONE, image=0, rows=32, joints=17, style=good, ws=ONE):
        return lib.sp_redact_u8c3(src, dst, h, w, kps, box, keep, kc, seg, image, rows, joints, None if style is None else ctypes.byref(style), ws,
                                  None)

    for kw in ({"src": None}, {"dst": None}, {"kps": None}, {"box": None}, {"keep": None}, {"kc": None}, {"seg": None}, {"style": None}, {"ws": None}):
        assert call(**kw) == -1 and b"null" in lib.sp_last_error(), kw
    for joints in (0, 65, -1):
        assert call(joints=joints) == -1 and b"joints" in lib.sp_last_error()
    assert call(joints=4) == -1 and b"head_joint[4]" in lib.sp_last_error()      # the default head joints name joint 4
    for field, values, word in (("region", (-1, 2), b"region"), ("mode", (-1, 2), b"mode"), ("cell", (0, 2, 12, 128, -16), b"cell"),
                                ("expand", (15, 65, -1), b"expand"), ("head_min", (-1, 257), b"head_min"), ("top_frac", (-1, 257), b"top_frac"),
                                ("fallback", (-1, 3), b"fallback"), ("head_joints", (0, 9, -1), b"head_joints")):
        for v in values:
            st = redact_scenes.style_struct(redact_ref.Style())
            setattr(st, field, v)
            assert call(style=st) == -1 and word in lib.sp_last_error(), (field, v)
    st = redact_scenes.style_struct(redact_ref.Style())
    st.head_joint[2] = -2
    assert call(style=st) == -1 and b"head_joint[2]" in lib.sp_last_error()
    st.region = _lib.SP_REDACT_REGIONS["person"]                                 # a person region does not read the head joints:
    assert call(style=st, rows=0) == 0                                           # nothing refused, and in place without rows nothing to do
    for kw in ({"h": 0}, {"w": 0}, {"h": 16385}, {"w": 16385}, {"h": -4}):
        assert call(**kw) == -1 and b"image" in lib.sp_last_error(), kw
    assert call(image=-1) == -1 and b"image index" in lib.sp_last_error()
    assert call(rows=-1) == -1 and b"rows" in lib.sp_last_error()
    assert call(rows=2049) == -1 and b"rows" in lib.sp_last_error()
    for delta in (1, 48 * 64 * 3 - 1, -30):                                      # dst inside src's bytes, or src inside dst's
        assert call(dst=ctypes.c_void_p(4096 + delta)) == -1 and b"overlap" in lib.sp_last_error(), delta
    assert call(ws=ctypes.c_void_p(4098)) == -1 and b"aligned" in lib.sp_last_error()
    assert call(kps=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.sp_last_error()
    assert call(rows=0, kps=None, box=None, keep=None, kc=None, seg=None, ws=None) == 0      # in place, no rows: nothing to do, nothing launched


class _Model:
    training = False

    def hip_program(self, x):
        raise AssertionError("the constructor does not lower anything")


def test_redactor_constructor_refusals_and_quantisation():
    import torch
    from simple_pose_amd.pipeline import PoseResult, TopDownPoseEstimator
    from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
    from simple_pose_amd.visualize import PoseRenderer, Redactor
    for kw, name in (({"region": "face"}, "region"), ({"region": 0}, "region"), ({"mode": "blur"}, "mode"), ({"cell": 12}, "cell"),
                     ({"cell": 16.0}, "cell"), ({"cell": True}, "cell"), ({"cell": 128}, "cell"), ({"expand": 0.9}, "expand"),
                     ({"expand": 4.5}, "expand"), ({"expand": "2"}, "expand"), ({"expand": float("nan")}, "expand"), ({"head_min": -0.1}, "head_min"),
                     ({"head_min": 1.5}, "head_min"), ({"top_frac": 1.01}, "top_frac"), ({"top_frac": True}, "top_frac"),
                     ({"head_joints": ()}, "head_joints"), ({"head_joints": tuple(range(9))}, "head_joints"), ({"head_joints": (0, 64)}, "head_joints"),
                     ({"head_joints": (0, -1)}, "head_joints"), ({"head_joints": (0, 1.5)}, "head_joints"), ({"head_joints": 3}, "head_joints"),
                     ({"fallback": "top"}, "fallback"), ({"fallback": None}, "fallback"), ({"in_vis_thre": "x"}, "in_vis_thre"),
                     ({"in_vis_thre": float("nan")}, "in_vis_thre"), ({"fill": (0, 0)}, "fill"), ({"fill": (0, 0, 256)}, "fill"),
                     ({"fill": (0.5, 0, 0)}, "fill"), ({"fill": 7}, "fill"), ({"fill": (-1, 0, 0)}, "fill")):
        with pytest.raises(ValueError, match=name):
            Redactor(**kw)
    r = Redactor()
    assert (r.region, r.mode, r.cell, r.expand16, r.head_min256, r.head_joints, r.fallback, r.top_frac256, r.in_vis_thre, r.fill) == \
        ("head", "mosaic", 16, 24, 20, (0, 1, 2, 3, 4), "box_top", 64, 0.2, (0, 0, 0))
    s = r._style
    assert (s.region, s.mode, s.cell, s.expand, s.head_min, s.head_joints, s.fallback, s.top_frac, s.in_vis_thre) == (0, 0, 16, 24, 20, 5, 0, 64, 0.2)
    assert list(s.head_joint)[:5] == [0, 1, 2, 3, 4] and list(s.fill) == [0, 0, 0]
    r2 = Redactor(region="person", mode="fill", cell=64, expand=2.53, head_min=0.1, head_joints=[0], fallback="none", top_frac=1 / 3, fill=(1, 2, 3))
    assert (r2.expand16, r2.head_min256, r2.top_frac256, r2.fill) == (40, 26, 85, (1, 2, 3))
    s2 = r2._style
    assert (s2.region, s2.mode, s2.cell, s2.fallback, s2.head_joints, list(s2.fill)) == (1, 1, 64, 2, 1, [1, 2, 3])
    assert r.key() == Redactor().key() != r2.key()
    for kw in ({"cell": 8}, {"fill": (0, 0, 1)}, {"expand": 2.0}, {"head_min": 0.2}, {"top_frac": 0.5}, {"fallback": "box"}, {"mode": "fill"},
               {"region": "person"}, {"head_joints": (0,)}, {"in_vis_thre": 0.3}):
        assert Redactor(**kw).key() != r.key(), kw                               # everything the launch depends on is in the key
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        r.redact(torch.zeros((48, 64, 3), dtype=torch.uint8), PoseResult(np.zeros((0, 17, 3)), np.zeros(0), np.zeros((0, 5), np.float32)))
    with pytest.raises(TypeError, match="uint8"):
        r.redact(np.zeros((48, 64, 3), np.float32), None)
    # the estimator takes a redactor or nothing, next to a renderer or alone
    det = object.__new__(YOLOv5Detector)
    det.device, det.conf_thresh, det.iou_thresh = "cuda:0", 0.25, 0.45
    with pytest.raises(TypeError, match="redactor"):
        TopDownPoseEstimator(det, _Model(), redactor=object())
    with pytest.raises(TypeError, match="redactor"):
        TopDownPoseEstimator(det, _Model(), redactor=PoseRenderer())
    est = TopDownPoseEstimator(det, _Model(), redactor=r, renderer=PoseRenderer())
    assert est.redactor is r and TopDownPoseEstimator(det, _Model()).redactor is None
    assert est._params(None, None)[-1] == r.key() and TopDownPoseEstimator(det, _Model())._params(None, None)[-1] is None


# ---- redact_ref: the properties of a redaction ----------------------------------------------------------------------------------------------
def _one(head_xy, box, c=0.9):
    kps = np.zeros((1, 17, 3))
    kps[0, :, :2], kps[0, :, 2] = head_xy, c
    return kps, np.array([list(box) + [1.0]], np.float32)


def test_ref_regions_by_hand():
    S = redact_ref.Style
    kps, box = _one((40.0, 30.0), (10.0, 10.0, 74.0, 138.0))
    kps[0, 1, :2], kps[0, 2, :2] = (44.0, 31.0), (36.5, 29.0)
    # bounding box of the head joints: x 584 .. 704, y 464 .. 496 (1/16 px); e = 120; s = 128 px = 2048; r0 = max(60, 2048 * 20 >> 8 = 160)
    assert redact_ref.region(S(), kps[0], box[0]) == ("disc", 644, 480, 240)
    assert redact_ref.region(S(head_min=0), kps[0], box[0]) == ("disc", 644, 480, 90)
    assert redact_ref.region(S(head_min=0, expand=16), kps[0], box[0]) == ("disc", 644, 480, 60)
    assert redact_ref.region(S(head_min=256, expand=64), kps[0], box[0]) == ("disc", 644, 480, 8192)
    assert redact_ref.region(S(region="person"), kps[0], box[0]) == ("rect", 160, 160, 1184, 2208)
    assert redact_ref.region(S(region="person"), kps[0], box[0, [2, 3, 0, 1]]) == ("rect", 160, 160, 1184, 2208)        # corners by min / max
    assert redact_ref.region(S(head_joints=(2,)), kps[0], box[0]) == ("disc", 584, 464, 240)
    # the radius is capped
    far = kps.copy()
    far[0, 0, :2], far[0, 1, :2] = (-32768.0, 0.0), (32768.0, 0.0)
    assert redact_ref.region(S(expand=64), far[0], box[0]) == ("disc", 0, 240, 1 << 20)
    # a negative centre: the arithmetic shift rounds down
    neg, nbox = _one((-3.03125, -1.0), (-8.0, -4.0, 2.0, 9.0))
    neg[0, 1, :2] = (-3.0, -1.0)
    assert redact_ref.region(S(head_min=0), neg[0], nbox[0])[:3] == ("disc", (-48 - 48) >> 1, -16)


def test_ref_fallback_rules_and_rejected_coordinates():
    S = redact_ref.Style
    kps, box = _one((40.0, 30.0), (10.0, 10.0, 74.0, 138.0), c=0.2)              # c == thre: no head joint is visible
    assert redact_ref.region(S(), kps[0], box[0]) == ("rect", 160, 160, 1184, 160 + ((2048 * 64) >> 8))
    assert redact_ref.region(S(top_frac=0), kps[0], box[0]) == ("rect", 160, 160, 1184, 160)
    assert redact_ref.region(S(top_frac=256), kps[0], box[0]) == redact_ref.region(S(fallback="box"), kps[0], box[0]) == ("rect", 160, 160, 1184, 2208)
    assert redact_ref.region(S(fallback="none"), kps[0], box[0]) is None
    assert redact_ref.region(S(), kps[0], box[0, [0, 3, 2, 1]]) == ("rect", 160, 160, 1184, 672)      # the top is the smaller y, whatever the order
    nan_c = kps.copy()
    nan_c[0, :, 2] = np.nan
    assert redact_ref.region(S(fallback="none"), nan_c[0], box[0]) is None                            # a NaN confidence is not visible
    # a rejected coordinate hides the joint; a rejected box gives s = 0 or an empty region
    vis, _ = _one((40.0, 30.0), (10.0, 10.0, 74.0, 138.0))
    for bad in (np.nan, np.inf, -np.inf, 32768.5, -1e9):
        k = vis.copy()
        k[0, :5, 0] = bad
        assert redact_ref.region(S(fallback="none"), k[0], box[0]) is None, bad
        k[0, 3, 0] = 12.0
        assert redact_ref.region(S(fallback="none", head_min=0), k[0], box[0]) == ("disc", 192, 480, 0), bad
        b = box.copy()
        b[0, 2] = bad
        assert redact_ref.region(S(region="person"), vis[0], b[0]) is None, bad
        assert redact_ref.region(S(), kps[0], b[0]) is None and redact_ref.region(S(fallback="box"), kps[0], b[0]) is None, bad
        assert redact_ref.region(S(), vis[0], b[0]) == ("disc", 640, 480, 0), bad                     # s = 0 and e = 0: a point


def test_ref_a_point_redacts_exactly_its_cell_and_a_disc_its_neighbours():
    S = redact_ref.Style
    img = np.random.default_rng(0).integers(0, 256, (40, 52, 3), dtype=np.uint8)
    kps, box = _one((21.0, 9.5), (np.nan, 0, 0, 0))                              # r == 0 at pixel (21, 9)
    for cell in redact_ref.CELLS:
        hit = redact_ref.hit_cells(redact_ref.regions(S(cell=cell), kps, box), 40, 52, cell)
        assert hit.sum() == 1 and hit[9 // cell, 21 // cell], cell
    # on a cell corner (16.0, 16.0) the point lies in the pixel square [16, 16 + 15/16] only: one cell, not four
    kps, box = _one((16.0, 16.0), (np.nan, 0, 0, 0))
    hit = redact_ref.hit_cells(redact_ref.regions(S(cell=16), kps, box), 40, 52, 16)
    assert hit.sum() == 1 and hit[1, 1]
    # a disc of radius 1/16 px round it reaches the three neighbours: the closed squares end at 15 + 15/16
    kps, box = _one((16.0, 16.0), (0.0, 0.0, 0.0, 0.0625))                        # s = 1/16 px; r0 = 1 * 256 >> 8 = 1; r = 1 * 24 >> 4 = 1
    reg = redact_ref.regions(S(cell=16, head_min=256), kps, box)
    assert reg == [("disc", 256, 256, 1)]
    hit = redact_ref.hit_cells(reg, 40, 52, 16)
    assert hit.sum() == 3 and hit[1, 1] and hit[0, 1] and hit[1, 0] and not hit[0, 0]       # the corner cell is sqrt(2) / 16 px away
    # the disc test is exact at the rim: r * r == dx * dx + dy * dy hits, one less misses
    assert redact_ref.meets(("disc", 0, 0, 5), 3 // 16, 0, 0, 0) and redact_ref.meets(("disc", -3, -4, 5), 0, 0, 0, 0)
    assert not redact_ref.meets(("disc", -3, -4, 4), 0, 0, 0, 0) and redact_ref.meets(("rect", -9, -9, 0, 0), 0, 0, 0, 0)
    assert not redact_ref.meets(("rect", -9, -9, -1, 5), 0, 0, 0, 0) and not redact_ref.meets(None, 0, 0, 9, 9)


@pytest.mark.parametrize("name", ["head_mosaic", "head_fill", "person_mosaic", "person_fill"])
def test_ref_properties_on_the_street_scene(name):
    style = redact_scenes.styles()[name]
    scene = redact_scenes.street()
    img, cell = scene["img"], style.cell
    h, w = img.shape[:2]
    kps, box = redact_scenes.kept_rows(scene)
    hit = redact_ref.hit_cells(redact_ref.regions(style, kps, box), h, w, cell)
    assert 0 < hit.sum() < hit.size
    out = redact_ref.redact(img, style, kps, box)
    pixel_hit = np.repeat(np.repeat(hit, cell, 0), cell, 1)[:h, :w]
    # pixels outside hit cells are unchanged; every hit cell is one colour
    assert (out[~pixel_hit] == img[~pixel_hit]).all()
    for cy, cx in zip(*np.nonzero(hit)):
        block = out[cy * cell:cy * cell + cell, cx * cell:cx * cell + cell].reshape(-1, 3)
        assert (block == block[0]).all()
        if style.mode == "fill":
            assert tuple(block[0]) == style.fill
    # redacting the output again changes nothing (a mean of equal values is the value)
    assert (redact_ref.redact(out, style, kps, box) == out).all()
    # the order of the persons does not matter, and a person listed twice is a person listed once
    perm = np.random.default_rng(3).permutation(len(kps))
    assert (redact_ref.redact(img, style, kps[perm], box[perm]) == out).all()
    assert (redact_ref.redact(img, style, np.concatenate([kps, kps]), np.concatenate([box, box])) == out).all()
    # nothing but the cell sums gets through: permuting the source pixels inside every hit cell leaves the output unchanged
    rng = np.random.default_rng(4)
    mixed = img.copy()
    for cy, cx in zip(*np.nonzero(hit)):
        ys, xs = slice(cy * cell, min(cy * cell + cell, h)), slice(cx * cell, min(cx * cell + cell, w))
        block = mixed[ys, xs]
        mixed[ys, xs] = rng.permutation(block.reshape(-1, 3)).reshape(block.shape)
    assert (mixed != img).any() and (redact_ref.redact(mixed, style, kps, box) == out).all()
    if style.mode == "mosaic":                                                   # and the mean is the rounded mean of the clipped cell
        cy, cx = [int(v[-1]) for v in np.nonzero(hit)]
        block = img[cy * cell:cy * cell + cell, cx * cell:cx * cell + cell].reshape(-1, 3).astype(np.int64)
        n = block.shape[0]
        assert (out[cy * cell, cx * cell] == (block.sum(0) + n // 2) // n).all()
        assert np.abs(out[cy * cell, cx * cell] - block.mean(0)).max() <= 0.5


def test_scenes_hold_what_the_gpu_tests_rely_on():
    S = redact_ref.Style
    street = redact_scenes.street()
    kps, box = redact_scenes.kept_rows(street)
    regs = {fb: redact_ref.regions(S(fallback=fb), kps, box) for fb in ("box_top", "box", "none")}
    kinds = [None if r is None else r[0] for r in regs["box_top"]]
    assert kinds == ["disc", "rect", "disc", "disc", "disc", None, "disc"]
    assert regs["box"][1][0] == "rect" and regs["box"][1] != regs["box_top"][1] and regs["none"][1] is None
    assert regs["box_top"][6][3] == 0                                            # g: a point
    d = regs["box_top"][3]
    assert d[1] < 0 and d[1] + d[3] >= 0                                         # d: centred outside, reaching in
    e = regs["box_top"][4]
    assert e[1] - e[3] > 16 * 131 and e[2] - e[3] > 16 * 97                      # e: wholly outside
    only_d = redact_ref.hit_cells([d], 97, 131, 8)
    assert only_d[:, 0].any() and not only_d[:, 2:].any()
    assert not redact_ref.hit_cells([e, regs["box_top"][5]], 97, 131, 4).any()
    for cell in redact_ref.CELLS:                                                # some tiles are hit and some are not, at every cell size
        tiles = redact_ref.tile_hits(redact_ref.regions(S(cell=cell), kps, box), 97, 131, cell)
        assert (tiles > 0).any() and ((tiles == 0).any() or cell == 64), cell
    wide = redact_scenes.street(96, 128)
    tiles = redact_ref.tile_hits(redact_ref.regions(S(cell=8), *redact_scenes.kept_rows(wide)), 96, 128, 8)
    assert (tiles > 0).any() and (tiles == 0).any()
    # the crowd: more records than one scan chunk, and the cells of the lower right corner are hit by records of the second chunk only
    crowd = redact_scenes.crowd()
    kps, box = redact_scenes.kept_rows(crowd)
    assert len(kps) == 300 > redact_scenes.CHUNK
    first = redact_ref.hit_cells(redact_ref.regions(S(cell=4), kps[:256], box[:256]), 64, 64, 4)
    every = redact_ref.hit_cells(redact_ref.regions(S(cell=4), kps, box), 64, 64, 4)
    assert not first[10:, 10:].any() and every[10:, 10:].any() and not every.all()
