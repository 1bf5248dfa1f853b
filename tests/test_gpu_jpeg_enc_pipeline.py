"""The JPEG encoder inside TopDownPoseEstimator / PoseTracker: `PoseResult.jpeg` is the file of the frame's canvas (of the source without
a renderer), and an estimator without an encoder computes what it computed before."""
import numpy as np
import pytest
import torch

from simple_pose_amd import synth
from simple_pose_amd.datasets.jpeg import JpegDecoder, JpegEncoder
from simple_pose_amd.detector.nets.yolov5 import YOLOv5
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
from simple_pose_amd.pipeline import TopDownPoseEstimator
from simple_pose_amd.tracking import PoseTracker
from simple_pose_amd.visualize import PoseRenderer
from tests.detector_ref import detector_state_dict

pytestmark = pytest.mark.gpu
G = "g14_detector.npz"
DEV = "cuda:0"


@pytest.fixture(scope="module")
def detector(golden):
    m = YOLOv5(scale_name="s", num_cls=80)
    d = YOLOv5Detector(num_cls=80, scale_name="s", device=DEV, slice_idx=0, state_dict=detector_state_dict(m, 14))
    conf, iou, _ = golden(G)["sp_a_thresh"]
    d.conf_thresh, d.iou_thresh = float(conf), float(iou)
    return d


@pytest.fixture(scope="module")
def dconv():
    from oracle import nets_oracle
    from simple_pose_amd.nets import pose_resnet_dconv
    m = pose_resnet_dconv.resnet50(pretrained=False, num_classes=17)
    sd = synth.conditioned_state_dict(nets_oracle.state_dict_shapes_resnet50("dconv"), 0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    m.compute_dtype, m.autotune = "fp32", False
    return m


def _same(a, b):
    np.testing.assert_array_equal(a.keypoints, b.keypoints)
    np.testing.assert_array_equal(a.score, b.score)
    np.testing.assert_array_equal(a.box, b.box)
    assert a.dropped == b.dropped


def test_result_carries_the_file_of_its_canvas(golden, detector, dconv):
    a = golden(G)["sp_a_image"]
    enc, dec = JpegEncoder(DEV, quality=85, subsampling="4:2:0", restart_interval=0), JpegDecoder(DEV)
    est = TopDownPoseEstimator(detector, dconv, capacity=32, renderer=PoseRenderer(), encoder=enc)
    drawn = TopDownPoseEstimator(detector, dconv, capacity=32, renderer=PoseRenderer())
    bare = TopDownPoseEstimator(detector, dconv, capacity=32, encoder=None)
    plain = TopDownPoseEstimator(detector, dconv, capacity=32)
    for graph in (False, True):
        est.use_graph = drawn.use_graph = bare.use_graph = plain.use_graph = graph
        for _ in range(2 if graph else 1):                                   # the capture, then a replay
            res, ref = est.estimate(a), drawn.estimate(a)
        assert isinstance(res.jpeg, bytes) and res.jpeg[:2] == b"\xff\xd8" and res.jpeg[-2:] == b"\xff\xd9" and ref.jpeg is None
        _same(res, ref)
        image = res.image.clone()
        assert torch.equal(image, ref.image) and (image.cpu().numpy() != a).any()
        again = JpegEncoder(DEV, quality=85, subsampling="4:2:0").encode([image])[0]
        assert res.jpeg == again
        assert torch.equal(dec.decode([res.jpeg])[0], dec.decode([again])[0]) and dec.status.cpu().tolist() == [0]
        assert tuple(dec.decode([res.jpeg])[0].shape) == a.shape
        # encoder=None is the estimator without the argument
        x, y = bare.estimate(a), plain.estimate(a)
        assert x.jpeg is None and y.jpeg is None and x.image is None
        _same(x, y)
        _same(x, res)
    # without a renderer the source is encoded; a batch gives one file per image
    src = TopDownPoseEstimator(detector, dconv, capacity=32, encoder=enc)
    b = np.ascontiguousarray(a[:, ::-1])
    out = src.estimate_batch([a, b])
    want = JpegEncoder(DEV, quality=85, subsampling="4:2:0").encode(torch.from_numpy(np.stack([a, b])).to(DEV))
    assert [r.jpeg for r in out] == want and out[0].image is None
    # the tracker's frames carry their file as well
    trk = PoseTracker(est, detect_every=2)
    for img in (a, b, a):
        r = trk.update(img)
        assert r.jpeg == JpegEncoder(DEV, quality=85, subsampling="4:2:0").encode([r.image.clone()])[0]
