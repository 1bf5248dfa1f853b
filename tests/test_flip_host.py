"""Flip test, host side: the two entry points are declared, exported and bound without an ABI bump and refuse bad arguments before they
touch the GPU; pairs_to_perm, the estimator's constructor and the CPU-tensor refusals of metrics.flip."""
import ctypes
import os
import re

import pytest

from simple_pose_amd import _lib
from simple_pose_amd.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sp_mirror_w", "sp_heat_map_flip_merge")
# non-null pointers that are never dereferenced (every call below fails its argument check first), 1 MiB apart
ONE, TWO, THREE = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20)


def test_new_symbols_declared_exported_bound_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(sp_\w+)\s*\(", hdr, flags=re.M))
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(handle, name), name
    assert re.search(r"#define SP_ABI_VERSION 36\b", hdr)
    assert _lib.ABI_VERSION == 36 and _lib.lib().sp_abi_version() == 36


def test_mirror_w_refuses_bad_arguments_without_touching_the_gpu():
    lib = _lib.lib()
    mirror = lambda src=ONE, dst=TWO, rows=8, w=48, eb=4: lib.sp_mirror_w(src, dst, rows, w, eb, None)
    assert mirror(src=None) == -1 and b"null" in lib.sp_last_error()
    assert mirror(dst=None) == -1 and b"null" in lib.sp_last_error()
    assert mirror(eb=2) == -1 and b"elem_bytes" in lib.sp_last_error()
    assert mirror(w=0) == -1 and b"w 0" in lib.sp_last_error()
    assert mirror(rows=-1) == -1 and b"rows" in lib.sp_last_error()
    assert mirror(dst=ONE) == -1 and b"overlap" in lib.sp_last_error()                       # in place
    for eb in (3, 4):                                                                         # dst one byte short of / past the end of src
        n = 8 * 48 * eb
        assert mirror(dst=ctypes.c_void_p(ONE.value + n - 1), eb=eb) == -1 and b"overlap" in lib.sp_last_error()
        assert mirror(dst=ctypes.c_void_p(ONE.value - n + 1), eb=eb) == -1 and b"overlap" in lib.sp_last_error()
    assert mirror(rows=0) == 0                                                                # a no-op: nothing is launched


def test_flip_merge_refuses_bad_arguments_without_touching_the_gpu():
    lib = _lib.lib()
    ident = lambda n: (ctypes.c_int32 * n)(*range(n))

    def merge(hm=ONE, fl=TWO, perm=None, batch=2, joints=17, h=64, w=48, out=THREE, null_perm=False):
        perm = None if null_perm else (ident(max(joints, 1)) if perm is None else perm)
        return lib.sp_heat_map_flip_merge(hm, fl, perm, batch, joints, h, w, 0, out, None)

    for kw in ({"hm": None}, {"fl": None}, {"out": None}, {"null_perm": True}):
        assert merge(**kw) == -1 and b"null" in lib.sp_last_error(), kw
    assert merge(joints=65, perm=ident(65)) == -1 and b"joints 65" in lib.sp_last_error()
    assert merge(joints=0) == -1 and b"joints 0" in lib.sp_last_error()
    assert merge(w=0) == -1 and b"shape" in lib.sp_last_error()
    assert merge(batch=-1) == -1 and b"shape" in lib.sp_last_error()
    repeat = ident(17)
    repeat[3] = 4
    assert merge(perm=repeat) == -1 and b"not a permutation" in lib.sp_last_error()
    for bad in (17, -1):
        outside = ident(17)
        outside[16] = bad
        assert merge(perm=outside) == -1 and b"out of range" in lib.sp_last_error()
    n = 2 * 17 * 64 * 48 * 4
    assert merge(out=TWO) == -1 and b"hm_flipped" in lib.sp_last_error()
    assert merge(out=ctypes.c_void_p(TWO.value + n - 4)) == -1 and b"hm_flipped" in lib.sp_last_error()
    assert merge(out=ctypes.c_void_p(TWO.value - n + 4)) == -1 and b"hm_flipped" in lib.sp_last_error()
    assert merge(out=ctypes.c_void_p(ONE.value + 16)) == -1 and b"without being hm" in lib.sp_last_error()
    assert merge(batch=0) == 0                                                                # a no-op: nothing is launched


def test_pairs_to_perm():
    from simple_pose_amd.metrics import COCO_JOINT_PAIRS, pairs_to_perm
    assert len(COCO_JOINT_PAIRS) == 8
    assert pairs_to_perm(COCO_JOINT_PAIRS, 17) == [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]
    assert pairs_to_perm((), 3) == [0, 1, 2] and pairs_to_perm([[0, 2]], 3) == [2, 1, 0]
    for bad in (((1, 2), (2, 3)), ((1, 2), (3, 1)), ((4, 4),)):                               # overlapping pairs
        with pytest.raises(ValueError, match="disjoint"):
            pairs_to_perm(bad, 17)
    for bad in (((1, 17),), ((-1, 2),), ((16, 15), (0, 99))):
        with pytest.raises(ValueError, match="out of range"):
            pairs_to_perm(bad, 17)
    for bad in (((1, 2.0),), ((1, "2"),), ((True, 2),), ((1, 2, 3),), (5,), 7):
        with pytest.raises(ValueError, match="joint_pairs"):
            pairs_to_perm(bad, 17)
    with pytest.raises(ValueError, match="num_joints"):
        pairs_to_perm(COCO_JOINT_PAIRS, 65)


class _Model:
    training = False

    def hip_program(self, x):
        raise AssertionError("the constructor does not lower anything")


def test_estimator_constructor_accepts_flip_test_and_refuses_bad_pairs():
    from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
    from simple_pose_amd.metrics import COCO_JOINT_PAIRS
    from simple_pose_amd.pipeline import TopDownPoseEstimator
    det = object.__new__(YOLOv5Detector)            # (a real one needs the GPU; the constructor only checks the type)
    det.device = "cuda:0"
    est = TopDownPoseEstimator(det, _Model(), flip_test=True)
    assert est.flip_test and not est.shift_heatmap and est.joint_pairs == tuple(COCO_JOINT_PAIRS) and est._pose_batch() == 64
    est = TopDownPoseEstimator(det, _Model(), flip_test=True, joint_pairs=[[0, 1]], shift_heatmap=True, capacity=5)
    assert est.joint_pairs == ((0, 1),) and est.shift_heatmap and est._pose_batch() == 10
    plain = TopDownPoseEstimator(det, _Model())
    assert not plain.flip_test and not plain.shift_heatmap and plain._pose_batch() == 32
    for bad in (((1, 2), (2, 3)), ((1, 2.5),), ((1,),), 3):
        with pytest.raises(ValueError, match="joint_pairs"):
            TopDownPoseEstimator(det, _Model(), flip_test=True, joint_pairs=bad)


def test_cpu_tensors_are_refused():
    import torch
    from simple_pose_amd.metrics import merge_flipped, mirror_input
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        mirror_input(torch.zeros((1, 4, 4, 3), dtype=torch.uint8))
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        mirror_input(torch.zeros((1, 3, 4, 4)))
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        merge_flipped(torch.zeros((1, 17, 4, 4)), torch.zeros((1, 17, 4, 4)))
