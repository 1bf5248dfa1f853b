"""The host side of batches of differently sized images (simple_pose_amd/mixed_batch.py): grouping by net shape, the sp_image_ref table and
the checks that run before anything is launched.  No GPU is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib
from simple_pose_amd.detector.yolov5_detector import ScalePadding
from simple_pose_amd.mixed_batch import MAX_SIDE, REF_BYTES, check_det_counts, check_images, pack_image_refs, plan_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(432, 640), (864, 1280), (432, 426), (216, 320), (324, 640), (640, 427), (432, 640), (1, 1), (7, 3000)]


def _transform():
    return ScalePadding(target_size=(640, 640), minimum_rectangle=True, padding_val=(114, 114, 114))      # YOLOv5Detector's


def test_image_ref_mirrors_the_header():
    assert ctypes.sizeof(_lib.ImageRef) == REF_BYTES == 40 and ctypes.alignment(_lib.ImageRef) == 8
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    body = re.search(r"typedef struct sp_image_ref \{(.*?)\} sp_image_ref;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f for f, _ in _lib.ImageRef._fields_]
    assert [w for w in re.findall(r"[A-Za-z_]\w*", body) if w in fields] == fields          # the same members in the same order
    offsets = {f: getattr(_lib.ImageRef, f).offset for f, _ in _lib.ImageRef._fields_}
    assert offsets == {"data": 0, "h": 8, "w": 12, "new_h": 16, "new_w": 20, "top": 24, "left": 28, "ratio": 32, "dst_index": 36}


def test_groups_follow_the_net_shape_in_first_appearance_order():
    t = _transform()
    geoms, groups = plan_groups(SHAPES, t)
    assert len(geoms) == len(SHAPES)
    for (h, w), g in zip(SHAPES, geoms):
        assert g == t.geometry(h, w)                                             # what single_predict letterboxes the image with
    seen = []
    for (oh, ow), members in groups:
        assert members == sorted(members) and members
        for i in members:
            assert (geoms[i]["out_h"], geoms[i]["out_w"]) == (oh, ow)
        seen += members
    assert sorted(seen) == list(range(len(SHAPES)))                              # every image in exactly one group
    assert [members[0] for _, members in groups] == sorted(members[0] for _, members in groups)
    by_shape = dict(groups)
    assert by_shape[(448, 640)] == [0, 1, 3, 6] and by_shape[(640, 640)] == [2, 7] and by_shape[(384, 640)] == [4]
    assert len(groups) >= 4 and len(groups) == len({(g["out_h"], g["out_w"]) for g in geoms})


def test_table_holds_caller_order_then_groups():
    t = _transform()
    geoms, groups = plan_groups(SHAPES, t)
    B = len(SHAPES)
    ptrs = [0x10000 + 0x1000 * i for i in range(B)]
    refs, starts = pack_image_refs(ptrs, SHAPES, geoms, groups)
    assert len(refs) == 2 * B and len(starts) == len(groups) and starts[0] == B

    def same(r, i):
        g = t.geometry(*SHAPES[i])
        assert (r.data, r.h, r.w, r.dst_index) == (ptrs[i], SHAPES[i][0], SHAPES[i][1], i)
        assert (r.new_h, r.new_w, r.top, r.left) == (g["new_h"], g["new_w"], g["top"], g["left"])
        assert r.ratio == np.float32(g["ratio"])                                 # the float sp_yolo_boxes_to_source gets from single_predict

    for i in range(B):
        same(refs[i], i)
    k = B
    for (_, members), lo in zip(groups, starts):
        assert lo == k
        for i in members:
            same(refs[k], i)
            k += 1
    assert k == 2 * B


def test_a_placement_outside_the_canvas_is_refused():
    geoms, groups = plan_groups([(432, 640)], _transform())
    geoms[0] = dict(geoms[0], top=geoms[0]["out_h"])
    with pytest.raises(ValueError, match="does not fit"):
        pack_image_refs([256], [(432, 640)], geoms, groups)


def test_bad_image_lists_raise_before_any_launch():
    ok = np.zeros((4, 5, 3), np.uint8)
    assert check_images([ok, np.zeros((9, 2, 3), np.uint8)]) == [(4, 5), (9, 2)]
    with pytest.raises(ValueError, match="empty"):
        check_images([])
    with pytest.raises(TypeError, match="uint8"):
        check_images([ok, np.zeros((4, 5, 3), np.float32)])
    with pytest.raises(TypeError, match="uint8"):
        check_images([ok, [[1, 2, 3]]])
    for shape in ((0, 5, 3), (4, 0, 3), (4, 5), (4, 5, 4)):
        with pytest.raises(ValueError, match="image 1"):
            check_images([ok, np.zeros(shape, np.uint8)])
    with pytest.raises(ValueError, match="above"):
        check_images([np.zeros((1, MAX_SIDE + 1, 3), np.uint8)])
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        check_images([ok, torch.zeros((4, 5, 3), dtype=torch.uint8)])
    with pytest.raises(TypeError):
        check_images(ok)


def test_detections_must_match_the_number_of_images():
    det = np.zeros((3, 7, 6), np.float32)
    assert check_det_counts(3, det, None) == 7 and check_det_counts(3, torch.from_numpy(det), [7, 0, 2]) == 7
    assert check_det_counts(3, det, torch.tensor([1, 2, 3])) == 7
    for bad in (det[:2], det[:, :, :5], det[0], det[:, :0]):
        with pytest.raises(ValueError, match="det"):
            check_det_counts(3, bad, None)
    for bad in ([7, 7], np.zeros(4, np.int32), torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="counts"):
            check_det_counts(3, det, bad)


def test_table_launches_reject_bad_arguments_without_touching_the_gpu():
    OH, OW = 64, 96
    lib, one = _lib.lib(), ctypes.c_void_p(256)
    for rc in (lib.sp_yolo_letterbox_images(None, 1, OH, OW, _lib.SP_LETTERBOX_U8, one, None),
               lib.sp_yolo_letterbox_images(one, 0, OH, OW, _lib.SP_LETTERBOX_U8, one, None),
               lib.sp_yolo_letterbox_images(one, 1, OH + 1, OW, _lib.SP_LETTERBOX_U8, one, None),
               lib.sp_yolo_letterbox_images(one, 1, OH, OW + 1, _lib.SP_LETTERBOX_FOCUS, one, None),
               lib.sp_yolo_boxes_to_source_images(one, one, one, None, 1, 8, 64.0, 64.0, one, one, one, None),
               lib.sp_yolo_boxes_to_source_images(one, one, one, one, 0, 8, 64.0, 64.0, one, one, one, None),
               lib.sp_warp_affine_plan_images_u8c3(None, 1, one, one, one, 4, one, 256, 192, None),
               lib.sp_warp_affine_plan_images_u8c3(one, 0, one, one, one, 4, one, 256, 192, None)):
        assert rc == -1 and lib.sp_last_error()


def test_estimator_refuses_a_bad_mixed_list_before_any_launch():
    from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
    from simple_pose_amd.pipeline import TopDownPoseEstimator

    class Model:
        training = False

        def hip_program(self, x):
            raise AssertionError("nothing is lowered before the checks")

    det = object.__new__(YOLOv5Detector)             # (a real one needs the GPU; the constructor only checks the type)
    det.device = "cuda:0"
    est = TopDownPoseEstimator(det, Model())
    a, b = np.zeros((48, 64, 3), np.uint8), np.zeros((48, 80, 3), np.uint8)
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        est.estimate_batch([a, torch.zeros((48, 80, 3), dtype=torch.uint8)])
    with pytest.raises(TypeError, match="uint8"):
        est.estimate_batch([a, b.astype(np.float32)])
    with pytest.raises(ValueError, match="empty"):
        est.estimate_batch([])
    with pytest.raises(ValueError, match="det"):
        est.estimate_boxes([a, b], np.zeros((3, 4, 6), np.float32))
    with pytest.raises(ValueError, match="counts"):
        est.estimate_boxes([a, b], np.zeros((2, 4, 6), np.float32), [4])
    with pytest.raises(ValueError, match="detector.transform"):       # a detector without a letterbox cannot group the images by net shape
        est.estimate_batch([a, b])
