"""Top-down estimator, host side: the three new entry points are declared, exported and bound without an ABI bump, refuse bad arguments
before they touch the GPU, and the estimator's constructor refuses what it cannot run."""
import ctypes
import os
import re

import pytest

from simple_pose_amd import _lib
from simple_pose_amd.build import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sp_yolo_nms_device", "sp_topdown_plan", "sp_warp_affine_plan_u8c3")
ONE = ctypes.c_void_p(256)          # a non-null pointer that is never dereferenced: every call below fails its argument check first


def test_new_symbols_declared_exported_bound_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(sp_\w+)\s*\(", hdr, flags=re.M))
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(handle, name), name
    assert re.search(r"#define SP_ABI_VERSION 36\b", hdr)
    assert _lib.ABI_VERSION == 36 and _lib.lib().sp_abi_version() == 36


def _plan(lib, det=ONE, counts=ONE, batch=1, max_det=300, capacity=32, out=ONE):
    return lib.sp_topdown_plan(det, counts, batch, max_det, 0, 0.0, capacity, 192, 256, 48, 64, out, out, out, out, out, out, out, out, out, out, None)


def test_bad_arguments_return_einval_without_touching_the_gpu():
    lib = _lib.lib()
    assert _plan(lib, det=None) == -1 and b"null" in lib.sp_last_error()
    assert _plan(lib, out=None) == -1 and b"null" in lib.sp_last_error()
    assert _plan(lib, capacity=0) == -1 and b"capacity" in lib.sp_last_error()
    assert _plan(lib, capacity=2049) == -1 and b"capacity" in lib.sp_last_error()
    assert _plan(lib, batch=0) == -1 and b"batch" in lib.sp_last_error()
    warp = lambda src=ONE, batch=1, capacity=32, seg=ONE: lib.sp_warp_affine_plan_u8c3(src, batch, 480, 640, ONE, ONE, seg, capacity, ONE, 256, 192, None)
    assert warp(src=None) == -1 and b"null" in lib.sp_last_error()
    assert warp(seg=None) == -1 and b"null" in lib.sp_last_error()
    assert warp(capacity=0) == -1 and b"capacity" in lib.sp_last_error()
    assert warp(capacity=2049) == -1 and b"capacity" in lib.sp_last_error()
    assert warp(batch=0) == -1 and b"batch" in lib.sp_last_error()
    nms = lambda pred=ONE, batch=1, status=ONE, ws_bytes=1 << 30, max_det=300: lib.sp_yolo_nms_device(
        pred, batch, 100, 6, 0.1, 0.5, 1, 1, 0, max_det, ONE, ws_bytes, ONE, ONE, status, None)
    assert nms(pred=None) == -1 and b"null" in lib.sp_last_error()
    assert nms(status=None) == -1 and b"null" in lib.sp_last_error()
    assert nms(batch=0) == -1 and b"batch" in lib.sp_last_error()
    assert nms(max_det=_lib.SP_YOLO_NMS_MAX_DET + 1) == -1
    assert nms(ws_bytes=16) == -1 and b"workspace" in lib.sp_last_error()


class _Model:
    training = False

    def hip_program(self, x):
        raise AssertionError("the constructor does not lower anything")


def test_constructor_refusals():
    from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
    from simple_pose_amd.pipeline import TopDownPoseEstimator
    det = object.__new__(YOLOv5Detector)            # (a real one needs the GPU; the constructor only checks the type)
    det.device = "cuda:0"
    for cap in (0, 2049, -1, 2.5, True):
        with pytest.raises(ValueError, match="capacity"):
            TopDownPoseEstimator(det, _Model(), capacity=cap)
    with pytest.raises(TypeError, match="detector"):
        TopDownPoseEstimator(object(), _Model())
    with pytest.raises(TypeError, match="hip_program"):
        TopDownPoseEstimator(det, object())
    with pytest.raises(TypeError, match="decoder"):
        TopDownPoseEstimator(det, _Model(), decoder=lambda hm, t: None)
    training = _Model()
    training.training = True
    with pytest.raises(ValueError, match="eval"):
        TopDownPoseEstimator(det, training)
    with pytest.raises(ValueError, match="person_cls"):
        TopDownPoseEstimator(det, _Model(), person_cls=-2)
    with pytest.raises(ValueError, match="input_shape"):
        TopDownPoseEstimator(det, _Model(), input_shape=(192, 256), output_shape=(64, 48))
    est = TopDownPoseEstimator(det, _Model(), capacity=2048)
    assert est.capacity == 2048 and est.use_graph and type(est.decoder).__name__ == "GaussTaylorKeyPointDecoder"


def test_cpu_images_and_mixed_sizes_are_refused():
    import numpy as np
    import torch
    from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
    from simple_pose_amd.pipeline import TopDownPoseEstimator
    det = object.__new__(YOLOv5Detector)
    det.device = "cuda:0"
    est = TopDownPoseEstimator(det, _Model())
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        est.estimate(torch.zeros((48, 64, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="one size"):
        est.estimate_batch([np.zeros((48, 64, 3), np.uint8), np.zeros((48, 80, 3), np.uint8)])
    with pytest.raises(ValueError):
        est.estimate(np.zeros((2, 48, 64, 3), np.uint8))


def test_pose_result_coco_dicts():
    import numpy as np
    from simple_pose_amd.pipeline import PoseResult
    k = np.arange(2 * 17 * 3, dtype=np.float64).reshape(2, 17, 3)
    r = PoseResult(k, np.array([0.5, 0.25]), np.zeros((2, 5), np.float32), dropped=3)
    out = r.coco(7)
    assert len(r) == 2 and r.dropped == 3
    assert out[1] == {"image_id": 7, "score": 0.25, "category_id": 1, "keypoints": k[1].reshape(-1).tolist()}
