"""Merge-NMS can leave candidates but no box: its redundancy filter keeps a box only when a second candidate overlaps it.  Such an image
comes back from non_max_suppression as an empty [0, 6] view (not None), and boxes_to_source / the detector's finishing step have to pass
it through instead of handing a null pointer to the launch."""
import numpy as np
import pytest
import torch

from simple_pose_amd.detector.yolov5_detector import boxes_to_source, non_max_suppression

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lonely_candidates():
    pred = torch.zeros((2, 8, 6), device=DEV)
    for i in range(4):                                  # image 0: four candidates far apart - nothing overlaps anything
        pred[0, i] = torch.tensor([50.0 + 150 * i, 60.0, 40.0, 80.0, 0.9, 0.9])
    pred[1, 0] = torch.tensor([100.0, 100.0, 40.0, 80.0, 0.9, 0.9])      # image 1: an overlapping pair survives the filter
    pred[1, 1] = torch.tensor([102.0, 101.0, 40.0, 80.0, 0.8, 0.9])
    return pred


def test_merge_nms_with_candidates_but_no_box_passes_through():
    out = non_max_suppression(_lonely_candidates(), 0.1, 0.5, merge=True)
    assert out[0] is not None and tuple(out[0].shape) == (0, 6)          # candidates, but the redundancy filter left none
    assert out[1] is not None and out[1].shape[0] == 1
    got = boxes_to_source(out[0], (448, 640), 0.0, 8.0, 1.0)
    assert tuple(got.shape) == (0, 6)
    want = out[1].cpu().numpy().copy()
    want[:, [1, 3]] -= np.float32(8.0)
    np.testing.assert_array_equal(boxes_to_source(out[1], (448, 640), 0.0, 8.0, 1.0).cpu().numpy(), want)


def test_without_merge_the_same_candidates_are_kept():
    out = non_max_suppression(_lonely_candidates(), 0.1, 0.5, merge=False)
    assert out[0].shape[0] == 4 and out[1].shape[0] == 1
