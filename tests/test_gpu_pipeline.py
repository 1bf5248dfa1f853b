"""Top-down estimator on the MI355X.  The yardstick everywhere is the staged composition of the functions that existed before the
estimator (single_predict -> crop_boxes -> forward_crops -> decoder -> filter_poses, non_max_suppression, the host matrix helpers), each
already pinned to the reference; both sides run the same pixel, network and NMS kernels on the same bits, so every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib, synth
from simple_pose_amd.commons.joint_utils import box_to_center_scale, get_affine_transform
from simple_pose_amd.datasets.naive_data import crop_boxes, filter_poses
from simple_pose_amd.detector.nets.yolov5 import YOLOv5
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector, _workspace, non_max_suppression
from simple_pose_amd.metrics import GaussTaylorKeyPointDecoder
from simple_pose_amd.pipeline import TopDownPoseEstimator
from tests.detector_ref import detector_state_dict

pytestmark = pytest.mark.gpu
G = "g14_detector.npz"
DEV = "cuda:0"
P = _lib.ptr


def _stream():
    return _lib.current_stream(torch.device(DEV))


# ---- 1. sp_yolo_nms_device ------------------------------------------------------------------------------------------------------------
def _nms_device(pred, conf, iou, merge, max_det=300):
    max_det = int(max_det)
    pred = pred.contiguous()
    B, N, no = pred.shape
    out = torch.zeros((B, max_det, 6), device=DEV)
    counts = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    status = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ws = _workspace(B, pred.device)
    _lib.check(_lib.lib().sp_yolo_nms_device(P(pred), B, N, no, float(conf), float(iou), int(bool(merge)), 1, 0, int(max_det), P(ws), ws.numel(),
                                             P(out), P(counts), P(status), _stream()), "sp_yolo_nms_device")
    return out.cpu().numpy(), counts.cpu().numpy(), status.cpu().numpy()


def _assert_same_as_host_nms(pred, conf, iou, merge, max_det=300):
    want = non_max_suppression(pred, conf, iou, merge=bool(merge), max_det=int(max_det))
    got, counts, status = _nms_device(pred, conf, iou, merge, max_det)
    for b, w in enumerate(want):
        n = 0 if w is None else w.shape[0]
        assert counts[b] == n and status[b] == 0
        if n:
            np.testing.assert_array_equal(got[b, :n].view(np.uint32), w.cpu().numpy().view(np.uint32))
    return counts


@pytest.mark.parametrize("case", ["merge_a", "plain_a", "merge_b", "plain_b", "many"])
def test_nms_device_equals_nms_bitwise(golden, case):
    z = golden(G)
    conf, iou, merge, max_det = z[f"nms_{case}_args"]
    counts = _assert_same_as_host_nms(torch.from_numpy(z[f"nms_{case}_pred"]).to(DEV), conf, iou, merge, max_det)
    assert counts[0] == z[f"nms_{case}_out"].shape[0] > 0


def test_nms_device_batch_with_an_empty_image(golden):
    z = golden(G)
    for case in ("merge_a", "plain_b"):
        conf, iou, merge, max_det = z[f"nms_{case}_args"]
        p = torch.from_numpy(z[f"nms_{case}_pred"]).to(DEV)
        batch = torch.cat([p, torch.zeros_like(p), p.flip(1)])
        counts = _assert_same_as_host_nms(batch, conf, iou, merge, max_det)
        assert counts[0] > 0 and counts[1] == 0 and counts[2] > 0


def test_nms_device_overflow_sets_status_and_spares_the_neighbours(golden):
    z = golden(G)
    conf, iou, merge, max_det = z["nms_plain_a_args"]
    small = torch.from_numpy(z["nms_plain_a_pred"]).to(DEV)                     # [1, 216, 8]
    N, no = _lib.SP_YOLO_NMS_MAX_CANDIDATES + 1, small.shape[2]
    batch = torch.zeros((3, N, no), device=DEV)
    batch[0, :small.shape[1]] = small[0]
    batch[1, :, 2:4] = 10.0                                                     # more candidates than the cap: every row, one class
    batch[1, :, 4:6] = 0.9
    batch[2, N - small.shape[1]:] = small[0]
    want = non_max_suppression(batch[[0, 2]].contiguous(), conf, iou, merge=bool(merge), max_det=int(max_det))
    got, counts, status = _nms_device(batch, conf, iou, merge, max_det)
    assert status.tolist() == [0, 1, 0] and counts[1] == 0
    for b, w in ((0, want[0]), (2, want[1])):
        assert counts[b] == w.shape[0] > 0
        np.testing.assert_array_equal(got[b, :counts[b]].view(np.uint32), w.cpu().numpy().view(np.uint32))


# ---- 2. sp_topdown_plan -----------------------------------------------------------------------------------------------------------------
def _plan(det, counts, capacity, keep_cls=-1, min_score=0.0):
    det = torch.from_numpy(np.ascontiguousarray(det, np.float32)).to(DEV)
    B, M, _ = det.shape
    cnt = torch.tensor(list(counts), dtype=torch.int32, device=DEV)
    nan32, nan64 = float("nan"), float("nan")
    o = dict(seg=torch.full((B + 1,), -7, dtype=torch.int32, device=DEV), src_index=torch.full((capacity,), -7, dtype=torch.int32, device=DEV),
             m_inv=torch.full((capacity, 6), nan64, dtype=torch.float64, device=DEV), trans_inv=torch.full((capacity, 2, 3), nan32, device=DEV),
             center=torch.full((capacity, 2), nan32, device=DEV), scale=torch.full((capacity, 2), nan32, device=DEV),
             area=torch.full((capacity,), nan64, dtype=torch.float64, device=DEV), box_score=torch.full((capacity,), nan64, dtype=torch.float64, device=DEV),
             box=torch.full((capacity, 5), nan32, device=DEV), dropped=torch.full((B,), -7, dtype=torch.int32, device=DEV))
    _lib.check(_lib.lib().sp_topdown_plan(P(det), P(cnt), B, M, int(keep_cls), float(min_score), capacity, 192, 256, 48, 64, P(o["seg"]),
                                          P(o["src_index"]), P(o["m_inv"]), P(o["trans_inv"]), P(o["center"]), P(o["scale"]), P(o["area"]),
                                          P(o["box_score"]), P(o["box"]), P(o["dropped"]), _stream()), "sp_topdown_plan")
    return {k: v.cpu().numpy() for k, v in o.items()}, o


def _invert_affine_host(fwd):
    """invert_affine of csrc/warp.hip (cv::warpAffine's inversion) in numpy float64 scalars: one rounding per operation, no contraction."""
    M = [np.float64(v) for v in np.asarray(fwd, np.float64).reshape(6)]
    D = M[0] * M[4] - M[1] * M[3]
    D = np.float64(1.0) / D if D != 0 else np.float64(0.0)
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11; M[1] = M[1] * (-D); M[3] = M[3] * (-D); M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return np.array(M, np.float64)


def _host_geometry(boxes):
    """What crop_boxes computes per float32 box, plus the inverted input map sp_warp_affine_u8c3 derives from m_fwd on the host."""
    n = boxes.shape[0]
    m_inv, tinv = np.empty((n, 6), np.float64), np.empty((n, 2, 3), np.float32)
    centers, scales = np.empty((n, 2), np.float32), np.empty((n, 2), np.float32)
    for i, (x1, y1, x2, y2) in enumerate(boxes):
        center, scale = box_to_center_scale(x1, y1, x2 - x1, y2 - y1, 192 / 256)
        m_inv[i] = _invert_affine_host(get_affine_transform(center, scale, 0, (192, 256))[0])
        tinv[i] = get_affine_transform(center, scale, 0, (48, 64))[1]
        centers[i], scales[i] = center, scale
    return m_inv, tinv, centers, scales, (scales[:, 0] * scales[:, 1]).astype(np.float64)


def _seeded_boxes():
    rng = np.random.default_rng(20)
    f = np.float32
    groups = []
    h = (rng.integers(1, 400, 150) * 4).astype(f)                                # w exactly 0.75 h: neither fix-up branch
    x1, y1 = rng.integers(0, 3000, 150).astype(f), rng.integers(0, 3000, 150).astype(f)
    groups.append(np.stack([x1, y1, x1 + f(0.75) * h, y1 + h], 1))
    for wide in (True, False):                                                   # w above / below 0.75 h
        hh = rng.uniform(8, 600, 250).astype(f)
        ww = (hh * rng.uniform(0.8, 4.0, 250) if wide else hh * rng.uniform(0.05, 0.7, 250)).astype(f)
        x1, y1 = rng.uniform(0, 3300, 250).astype(f), rng.uniform(0, 3300, 250).astype(f)
        groups.append(np.stack([x1, y1, x1 + ww, y1 + hh], 1))
    x1, y1 = rng.uniform(-300, 50, 150).astype(f), rng.uniform(-300, 50, 150).astype(f)     # partly outside the image
    groups.append(np.stack([x1, y1, x1 + rng.uniform(100, 700, 150).astype(f), y1 + rng.uniform(100, 700, 150).astype(f)], 1))
    x1, y1 = rng.uniform(0, 640, 150).astype(f), rng.uniform(0, 480, 150).astype(f)         # sub-pixel boxes
    groups.append(np.stack([x1, y1, x1 + rng.uniform(0.01, 0.9, 150).astype(f), y1 + rng.uniform(0.01, 0.9, 150).astype(f)], 1))
    x1, y1 = rng.uniform(3500, 3990, 150).astype(f), rng.uniform(3500, 3990, 150).astype(f)  # coordinates up to 4,000
    groups.append(np.stack([x1, y1, np.minimum(x1 + rng.uniform(1, 500, 150).astype(f), f(4000)), np.minimum(y1 + rng.uniform(1, 500, 150).astype(f), f(4000))], 1))
    boxes = np.concatenate(groups).astype(f)
    assert boxes.shape[0] >= 1000 and (boxes[:, 2] > boxes[:, 0]).all() and (boxes[:, 3] > boxes[:, 1]).all()
    w, hh = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    assert (w[:150] == f(0.75) * hh[:150]).all() and (w > f(0.75) * hh).sum() > 200 and (w < f(0.75) * hh).sum() > 200
    return boxes


def test_plan_geometry_equals_host_bitwise():
    boxes = _seeded_boxes()
    n = boxes.shape[0]
    rng = np.random.default_rng(21)
    det = np.concatenate([boxes, rng.uniform(0.05, 1.0, (n, 1)).astype(np.float32), np.zeros((n, 1), np.float32)], 1)[None]
    got, _ = _plan(det, [n], 2048)
    m_inv, tinv, centers, scales, area = _host_geometry(boxes)
    assert got["seg"].tolist() == [0, n] and got["dropped"].tolist() == [0]
    for name, want, view in (("m_inv", m_inv, np.uint64), ("trans_inv", tinv, np.uint32), ("center", centers, np.uint32), ("scale", scales, np.uint32),
                             ("area", area, np.uint64), ("box_score", det[0, :, 4].astype(np.float64), np.uint64),
                             ("box", det[0, :, :5], np.uint32)):
        np.testing.assert_array_equal(got[name][:n].view(view), np.ascontiguousarray(want).view(view), err_msg=name)
    assert (got["src_index"][:n] == 0).all() and (got["src_index"][n:] == -1).all()
    for name in ("m_inv", "trans_inv", "center", "scale", "area", "box_score", "box"):
        assert (got[name][n:] == 0).all(), name                                  # dead slots: defined values


def _select(det, counts, keep_cls, min_score):
    return [(b, r) for b in range(det.shape[0]) for r in range(counts[b])
            if (keep_cls < 0 or det[b, r, 5] == keep_cls) and det[b, r, 4] >= np.float32(min_score)]


@pytest.mark.parametrize("keep_cls,min_score,capacity", [(0, 0.0, 64), (-1, 0.0, 64), (0, 0.3, 64), (-1, 0.3, 7), (0, 0.0, 6), (-1, 0.0, 1)])
def test_plan_selection_order_and_capacity(keep_cls, min_score, capacity):
    rng = np.random.default_rng(22)
    B, M = 5, 16
    counts = [5, 0, 16, 0, 3]                                                    # empty images in the middle of the batch
    x1, y1 = rng.uniform(0, 500, (B, M)), rng.uniform(0, 300, (B, M))
    det = np.stack([x1, y1, x1 + rng.uniform(20, 120, (B, M)), y1 + rng.uniform(40, 170, (B, M)), rng.uniform(0.05, 1.0, (B, M)),
                    rng.integers(0, 3, (B, M)).astype(np.float64)], -1).astype(np.float32)
    got, _ = _plan(det, counts, capacity, keep_cls, min_score)
    sel = _select(det, counts, keep_cls, min_score)
    kept = sel[:capacity]                                                        # dropped from the END of the (image, row) order
    assert len(sel) > capacity or capacity == 64
    seg = [sum(1 for b, _ in kept if b < i) for i in range(B + 1)]
    assert got["seg"].tolist() == seg
    assert got["dropped"].tolist() == [sum(1 for b, _ in sel[capacity:] if b == i) for i in range(B)]
    assert got["src_index"].tolist() == [b for b, _ in kept] + [-1] * (capacity - len(kept))
    rows = np.stack([det[b, r, :5] for b, r in kept])
    np.testing.assert_array_equal(got["box"][:len(kept)].view(np.uint32), rows.view(np.uint32))
    _, tinv, _, _, _ = _host_geometry(rows[:, :4])
    np.testing.assert_array_equal(got["trans_inv"][:len(kept)].view(np.uint32), tinv.view(np.uint32))
    assert (got["trans_inv"][len(kept):] == 0).all()


# ---- 3. sp_warp_affine_plan_u8c3 --------------------------------------------------------------------------------------------------------
def test_plan_warp_equals_crop_boxes_bitwise():
    rng = np.random.default_rng(23)
    B, M, cap = 2, 8, 12
    imgs = torch.from_numpy(rng.integers(0, 256, (B, 480, 640, 3), dtype=np.uint8)).to(DEV)
    counts = [3, 5]
    x1, y1 = rng.uniform(-40, 500, (B, M)), rng.uniform(-40, 300, (B, M))
    det = np.stack([x1, y1, x1 + rng.uniform(20, 220, (B, M)), y1 + rng.uniform(40, 300, (B, M)), rng.uniform(0.05, 1.0, (B, M)),
                    np.zeros((B, M))], -1).astype(np.float32)
    got, dev = _plan(det, counts, cap)
    crops = torch.full((cap, 256, 192, 3), 255, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().sp_warp_affine_plan_u8c3(P(imgs), B, 480, 640, P(dev["m_inv"]), P(dev["src_index"]), P(dev["seg"]), cap, P(crops), 256, 192,
                                                   _stream()), "sp_warp_affine_plan_u8c3")
    assert got["seg"].tolist() == [0, 3, 8]
    for b in range(B):
        want = crop_boxes(imgs[b], det[b, :counts[b], :4])[0]
        assert want.float().std().item() > 1.0                                   # real pixels, not an all-border crop
        assert torch.equal(crops[got["seg"][b]:got["seg"][b + 1]], want)
    assert (crops[8:] == 0).all()                                                # dead slots are written, as zeros


# ---- 4 - 7. the estimator ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector(golden):
    m = YOLOv5(scale_name="s", num_cls=80)
    d = YOLOv5Detector(num_cls=80, scale_name="s", device=DEV, slice_idx=0, state_dict=detector_state_dict(m, 14))
    conf, iou, _ = golden(G)["sp_a_thresh"]                                      # g14's single_predict thresholds: their margins keep the
    d.conf_thresh, d.iou_thresh = float(conf), float(iou)                        # detector's own decisions stable
    return d


def _pose_model(tag):
    from oracle import nets_oracle
    from simple_pose_amd.nets import pose_resnet_dconv, pose_resnet_duc
    if tag.startswith("hrnet"):
        from simple_pose_amd.nets.pose_hrnet import get_pose_net, hrnet_state_dict_shapes
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        m = get_pose_net(os.path.join(root, "simple_pose_amd", "nets", "hrnet_w32.yaml"), pretrained=None, joint_num=17)
        sd = synth.conditioned_state_dict(hrnet_state_dict_shapes(m.cfg, 17), 0)
    else:
        head = "dconv" if tag.startswith("dconv") else "duc"
        m = (pose_resnet_dconv if head == "dconv" else pose_resnet_duc).resnet50(pretrained=False, num_classes=17)
        sd = synth.conditioned_state_dict(nets_oracle.state_dict_shapes_resnet50(head), 0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    m.compute_dtype = "bf16" if tag.endswith("bf16") else "fp32"
    m.autotune = False               # tile timing moves speed only (same bits); both sides of every comparison share the model's program
    return m


@pytest.fixture(scope="module")
def dconv():
    return _pose_model("dconv_fp32")


def _staged(detector, model, img, capacity, image_id=7, person_cls=0, in_vis_thre=0.2, oks_thre=0.9, boxes=None):
    """The chain as a user assembles it from the public pieces; returns (dicts, selected detections, persons that reached the pose net)."""
    dev_img = torch.from_numpy(img).to(DEV)
    if boxes is None:
        boxes = detector.single_predict(img)
        if isinstance(boxes, list):
            return [], 0, 0
        boxes = boxes[boxes[:, 5] == person_cls]
    take = boxes[:capacity]
    if take.shape[0] == 0:
        return [], int(boxes.shape[0]), 0
    crops, tinv, _, _, area = crop_boxes(dev_img, take[:, :4].cpu().numpy())
    with torch.no_grad():
        hm = model.forward_crops(crops)
        kps, mv = GaussTaylorKeyPointDecoder()(hm, tinv)
    res = filter_poses(torch.cat([kps, mv], -1), take[:, 4].double().cpu().numpy(), area, [image_id] * take.shape[0], in_vis_thre, oks_thre)
    return res, int(boxes.shape[0]), int(take.shape[0])


@pytest.mark.parametrize("tag", ["dconv_fp32", "duc_bf16", "hrnet_w32_bf16"])
def test_estimate_equals_staged_chain(golden, detector, tag):
    img = golden(G)["sp_a_image"]
    model = _pose_model(tag)
    want, n_sel, n_pose = _staged(detector, model, img, 32)
    assert n_pose >= 8 and len(want) >= 1                                        # cannot pass on nothing
    est = TopDownPoseEstimator(detector, model, capacity=32)
    for graph in (False, True):
        est.use_graph = graph
        res = est.estimate(img)
        assert res.coco(7) == want
        assert res.dropped == n_sel - n_pose
        assert res.keypoints.shape == (len(want), 17, 3) and res.box.shape == (len(want), 5) and res.box.dtype == np.float32


def test_oks_nms_really_suppresses(detector, dconv):
    rng = np.random.default_rng(24)
    img = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    six = np.array([[50, 60, 200, 400, 0.9, 0], [300, 20, 500, 460, 0.8, 0], [10, 10, 120, 200, 0.7, 0], [400, 200, 630, 470, 0.6, 0],
                    [220, 100, 330, 330, 0.5, 0], [120, 250, 260, 470, 0.4, 0]], np.float32)
    twice = np.repeat(six, 2, axis=0)                                            # identical crops -> identical poses -> OKS 1
    boxes = torch.from_numpy(twice).to(DEV)
    for oks_thre in (0.9, 1.0):
        est = TopDownPoseEstimator(detector, dconv, capacity=16, oks_thre=oks_thre)
        res = est.estimate_boxes(img, twice)[0]
        want, _, n_pose = _staged(detector, dconv, img, 16, oks_thre=oks_thre, boxes=boxes)
        assert n_pose == 12 and res.coco(7) == want and res.dropped == 0
        assert (len(res) == 12) if oks_thre == 1.0 else (1 <= len(res) <= 6)


def test_graph_equals_eager_and_replays_are_not_stale(golden, detector, dconv):
    a = golden(G)["sp_a_image"]
    rng = np.random.default_rng(25)
    b = rng.integers(0, 256, a.shape, dtype=np.uint8)
    est = TopDownPoseEstimator(detector, dconv, capacity=32)
    est.use_graph = False
    eager_a, eager_b = est.estimate(a), est.estimate(b)
    assert len(eager_a) >= 1
    est.use_graph = True
    first, second = est.estimate(a), est.estimate(a)                             # capture + replay, then a second replay
    other, back = est.estimate(b), est.estimate(torch.from_numpy(a).to(DEV))     # a different image through the same graph, and back
    assert len(est._frames) == 1 and next(iter(est._frames.values())).graph is not None
    for got, want in ((first, eager_a), (second, eager_a), (other, eager_b), (back, eager_a)):
        assert got.coco(1) == want.coco(1) and got.dropped == want.dropped
        np.testing.assert_array_equal(got.box, want.box)
    assert eager_b.coco(1) == _staged(detector, dconv, b, 32, image_id=1)[0]


def test_image_without_detections_through_the_same_graph(golden, detector, dconv):
    """conf_thresh 0.36 separates the two inputs with room: the flat black image's best candidate scores 0.3506, a has 37 candidates above
    0.36 (margins ~1e-2, the network's fp32 repeatability is ~1e-5).  Both facts are checked on the staged detector first."""
    a = golden(G)["sp_a_image"]
    black = np.zeros_like(a)
    keep = detector.conf_thresh
    detector.conf_thresh = 0.36
    try:
        assert isinstance(detector.single_predict(black), list) and not isinstance(detector.single_predict(a), list)
        est = TopDownPoseEstimator(detector, dconv, capacity=32)
        want = _staged(detector, dconv, a, 32, image_id=1)[0]
        first = est.estimate(a)
        graph = next(iter(est._frames.values())).graph
        assert graph is not None and len(want) >= 1 and first.coco(1) == want
        empty = est.estimate(black)
        assert len(empty) == 0 and empty.coco(1) == [] and empty.dropped == 0
        assert empty.keypoints.shape == (0, 17, 3) and empty.box.shape == (0, 5) and empty.score.shape == (0,)
        assert est.estimate(a).coco(1) == want                                   # and nothing of the empty frame lingers
        assert len(est._frames) == 1 and next(iter(est._frames.values())).graph is graph
    finally:
        detector.conf_thresh = keep


def test_estimate_batch_equals_two_estimates(golden, detector, dconv):
    a = golden(G)["sp_a_image"]
    b = np.random.default_rng(26).integers(0, 256, a.shape, dtype=np.uint8)
    est = TopDownPoseEstimator(detector, dconv, capacity=640)                    # 2 x max_det fit: the images do not compete for slots
    one = [est.estimate(a), est.estimate(b)]
    both = est.estimate_batch(np.stack([a, b]))
    assert len(both) == 2 and len(one[0]) >= 1
    for got, want in zip(both, one):
        assert got.coco(3) == want.coco(3) and got.dropped == want.dropped == 0
        np.testing.assert_array_equal(got.box, want.box)


def test_nms_overflow_raises_after_the_transfer(detector, dconv):
    """The overflow path is covered in two halves, not end to end: the kernel's flag by test_nms_device_overflow_sets_status_and_spares_the_
    neighbours, the estimator's reaction here by setting the status word of a frame by hand (a real image with more than 32,768 candidates
    would need a detector built for the purpose)."""
    est = TopDownPoseEstimator(detector, dconv, capacity=4)
    img = np.zeros((64, 64, 3), np.uint8)
    fr = est._frame(1, 64, 64, est.MAX_DET, 17)
    fr.status.fill_(1)
    with pytest.raises(_lib.HipLibraryError, match="candidates"):
        est._results(fr)
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        est.estimate(torch.from_numpy(img))
