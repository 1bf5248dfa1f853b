"""Batches of differently sized images on the MI355X: the three table-driven launches against their dense counterparts run per image, and
the detector / estimator on a mixed list against the same calls per image.  Both sides of every comparison run the same device functions
on the same bits, so everything is compared bit for bit: there is no tolerance in this file."""
import ctypes

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib, synth
from simple_pose_amd.datasets.jpeg import JpegDecoder, JpegEncoder
from simple_pose_amd.detector.nets.yolov5 import YOLOv5
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
from simple_pose_amd.pipeline import TopDownPoseEstimator
from simple_pose_amd.visualize import PoseRenderer
from tests.detector_ref import detector_state_dict

pytestmark = pytest.mark.gpu
G = "g14_detector.npz"
DEV = "cuda:0"
P = _lib.ptr


def _stream():
    return _lib.current_stream(torch.device(DEV))


def _table(entries):
    """[(device tensor [h, w, 3], new_h, new_w, top, left, ratio, dst_index)] -> the table of sp_image_ref on the device."""
    refs = (_lib.ImageRef * len(entries))()
    for r, (t, nh, nw, top, left, ratio, dst) in zip(refs, entries):
        r.data, r.h, r.w = t.data_ptr(), t.shape[0], t.shape[1]
        r.new_h, r.new_w, r.top, r.left, r.ratio, r.dst_index = nh, nw, top, left, ratio, dst
    raw = np.frombuffer(bytes(refs), np.uint8).reshape(len(entries), ctypes.sizeof(_lib.ImageRef))
    return torch.from_numpy(raw.copy()).to(DEV)


# ---- 1. sp_yolo_letterbox_images ----------------------------------------------------------------------------------------------------------
OH, OW = 64, 96
#            source     new       (top, left)
LB_CASES = [((1, 1), (5, 7), (3, 4)),
            ((1, 7), (4, 20), (0, 0)),
            ((7, 1), (30, 3), (10, 50)),
            ((33, 17), (50, 26), (14, 70)),          # touches the canvas' bottom right corner
            ((40, 60), (20, 30), (22, 33)),          # an exact 2x downscale: INTER_AREA's 2x2 mean
            ((64, 96), (64, 96), (0, 0))]            # new == src: the copy, filling the canvas


def _letterbox_each(srcs, cases, mode):
    out = []
    for s, ((sh, sw), (nh, nw), (top, left)) in zip(srcs, cases):
        o = torch.full((OH, OW, 3), 7, dtype=torch.uint8, device=DEV) if mode == _lib.SP_LETTERBOX_U8 else \
            torch.full((OH // 2, OW // 2, 12), -7.0, device=DEV)
        _lib.check(_lib.lib().sp_yolo_letterbox(P(s), 1, sh, sw, nh, nw, top, left, OH, OW, mode, P(o), _stream()), "sp_yolo_letterbox")
        out.append(o)
    return torch.stack(out)


def _letterbox_images(srcs, cases, mode):
    table = _table([(s, nh, nw, top, left, 1.0, i) for i, (s, (_, (nh, nw), (top, left))) in enumerate(zip(srcs, cases))])
    n = len(cases)
    o = torch.full((n, OH, OW, 3), 9, dtype=torch.uint8, device=DEV) if mode == _lib.SP_LETTERBOX_U8 else \
        torch.full((n, OH // 2, OW // 2, 12), -9.0, device=DEV)
    _lib.check(_lib.lib().sp_yolo_letterbox_images(P(table), n, OH, OW, mode, P(o), _stream()), "sp_yolo_letterbox_images")
    return o


def test_letterbox_images_equals_letterbox_per_image_bitwise():
    rng = np.random.default_rng(40)
    srcs = [torch.from_numpy(rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)).to(DEV) for (sh, sw), _, _ in LB_CASES]
    want = _letterbox_each(srcs, LB_CASES, _lib.SP_LETTERBOX_U8)
    got = _letterbox_images(srcs, LB_CASES, _lib.SP_LETTERBOX_U8)
    for i in range(len(LB_CASES)):
        assert torch.equal(got[i], want[i]), LB_CASES[i]
    assert (want[0] == 114).any() and (want[3] != 114).any() and want[3].float().std().item() > 1.0     # padding and pixels both occur
    two = [3, 4]                                                                 # the bilinear and the 2x image again, through Focus
    cases, pick = [LB_CASES[i] for i in two], [srcs[i] for i in two]
    want = _letterbox_each(pick, cases, _lib.SP_LETTERBOX_FOCUS)
    got = _letterbox_images(pick, cases, _lib.SP_LETTERBOX_FOCUS)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert want.std().item() > 0.01


# ---- 2. sp_yolo_boxes_to_source_images ------------------------------------------------------------------------------------------------------
def test_boxes_to_source_images_scatters_two_groups_bitwise():
    rng = np.random.default_rng(41)
    M, total = 8, 5
    dummy = torch.zeros((1, 1, 3), dtype=torch.uint8, device=DEV)
    # (caller indices, canvas (h, w), counts, per image (left, top, ratio)): the two groups interleave in the caller's order
    groups = [([0, 2, 4], (448.0, 640.0), [0, 3, M], [(0, 8, 1.0), (4, 0, 0.5), (13, 2, 1.4814814814814814)]),
              ([1, 3], (384.0, 640.0), [M, 3], [(0, 30, 2.0), (7, 0, 0.7123)])]
    det_all = torch.full((total, M, 6), float("nan"), device=DEV)
    counts_all = torch.full((total,), -7, dtype=torch.int32, device=DEV)
    status_all = torch.full((total,), -7, dtype=torch.int32, device=DEV)
    want_det, want_counts, want_status = [None] * total, [None] * total, [None] * total
    for members, (ih, iw), counts, geo in groups:
        n = len(members)
        det = rng.uniform(-60, 700, (n, M, 6)).astype(np.float32)                # below 0 and beyond the canvas: the clip acts
        det[..., 4:] = rng.uniform(0, 1, (n, M, 2))
        status = rng.integers(0, 2, n).astype(np.int32)
        d_dev, c_dev, s_dev = torch.from_numpy(det).to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV), torch.from_numpy(status).to(DEV)
        table = _table([(dummy, 1, 1, top, left, ratio, dst) for dst, (left, top, ratio) in zip(members, geo)])
        _lib.check(_lib.lib().sp_yolo_boxes_to_source_images(P(d_dev), P(c_dev), P(s_dev), P(table), n, M, ih, iw, P(det_all), P(counts_all),
                                                             P(status_all), _stream()), "sp_yolo_boxes_to_source_images")
        assert np.array_equal(d_dev.cpu().numpy().view(np.uint32), det.view(np.uint32))          # out of place: the group's rows stay
        for b, dst in enumerate(members):
            one = torch.from_numpy(det[b]).to(DEV)
            left, top, ratio = geo[b]
            _lib.check(_lib.lib().sp_yolo_boxes_to_source(P(one), M, ih, iw, float(left), float(top), float(ratio), _stream()), "sp_yolo_boxes_to_source")
            want_det[dst], want_counts[dst], want_status[dst] = one.cpu().numpy(), counts[b], int(status[b])
    got = det_all.cpu().numpy()
    assert counts_all.tolist() == want_counts == [0, M, 3, 3, M] and status_all.tolist() == want_status
    for i in range(total):
        c = want_counts[i]
        np.testing.assert_array_equal(got[i, :c].view(np.uint32), want_det[i][:c].view(np.uint32), err_msg=f"image {i}")
        assert (got[i, c:] == 0).all()                                           # rows past the count are written, as zeros


# ---- 3. sp_warp_affine_plan_images_u8c3 -----------------------------------------------------------------------------------------------------
def _plan(det, counts, capacity):
    det = torch.from_numpy(np.ascontiguousarray(det, np.float32)).to(DEV)
    B, M, _ = det.shape
    cnt = torch.tensor(list(counts), dtype=torch.int32, device=DEV)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
    o = dict(seg=z((B + 1,), torch.int32), src_index=z((capacity,), torch.int32), m_inv=z((capacity, 6), torch.float64),
             trans_inv=z((capacity, 2, 3), torch.float32), center=z((capacity, 2), torch.float32), scale=z((capacity, 2), torch.float32),
             area=z((capacity,), torch.float64), box_score=z((capacity,), torch.float64), box=z((capacity, 5), torch.float32),
             dropped=z((B,), torch.int32))
    _lib.check(_lib.lib().sp_topdown_plan(P(det), P(cnt), B, M, -1, 0.0, capacity, 192, 256, 48, 64, P(o["seg"]), P(o["src_index"]), P(o["m_inv"]),
                                          P(o["trans_inv"]), P(o["center"]), P(o["scale"]), P(o["area"]), P(o["box_score"]), P(o["box"]),
                                          P(o["dropped"]), _stream()), "sp_topdown_plan")
    return o


def test_plan_warp_images_equals_plan_warp_per_image_bitwise():
    rng = np.random.default_rng(42)
    sizes, counts, M, cap = [(480, 640), (97, 131), (300, 211)], [3, 2, 4], 4, 12
    srcs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(DEV) for h, w in sizes]
    det = np.zeros((3, M, 6), np.float32)
    for b, (h, w) in enumerate(sizes):                                           # boxes inside and partly outside each image
        x1, y1 = rng.uniform(-0.1 * w, 0.6 * w, M), rng.uniform(-0.1 * h, 0.5 * h, M)
        det[b] = np.stack([x1, y1, x1 + rng.uniform(0.2 * w, 0.5 * w, M), y1 + rng.uniform(0.3 * h, 0.6 * h, M), rng.uniform(0.1, 1, M), np.zeros(M)], 1)
    o = _plan(det, counts, cap)
    seg = o["seg"].tolist()
    assert seg == [0, 3, 5, 9] and seg[-1] < cap
    table = _table([(s, 1, 1, 0, 0, 1.0, 99) for s in srcs])                     # dst_index is not read by this launch
    crops = torch.full((cap, 256, 192, 3), 255, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().sp_warp_affine_plan_images_u8c3(P(table), 3, P(o["m_inv"]), P(o["src_index"]), P(o["seg"]), cap, P(crops), 256, 192,
                                                          _stream()), "sp_warp_affine_plan_images_u8c3")
    for b, (h, w) in enumerate(sizes):
        n = seg[b + 1] - seg[b]
        m_inv = o["m_inv"][seg[b]:seg[b + 1]].contiguous()
        index = torch.zeros((n,), dtype=torch.int32, device=DEV)
        seg_b = torch.tensor([0, n], dtype=torch.int32, device=DEV)
        want = torch.full((n, 256, 192, 3), 255, dtype=torch.uint8, device=DEV)
        _lib.check(_lib.lib().sp_warp_affine_plan_u8c3(P(srcs[b]), 1, h, w, P(m_inv), P(index), P(seg_b), n, P(want), 256, 192, _stream()),
                   "sp_warp_affine_plan_u8c3")
        assert want.float().std().item() > 1.0                                   # real pixels, not all-border crops
        assert torch.equal(crops[seg[b]:seg[b + 1]], want), f"image {b}"
    assert (crops[seg[-1]:] == 0).all()                                          # dead slots are written, as zeros


# ---- 4 - 9. detector and estimator ------------------------------------------------------------------------------------------------------------
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
    m.compute_dtype = "fp32"
    m.autotune = False
    return m


@pytest.fixture(scope="module")
def mixed(golden):
    """a; a repeated 2x in both axes (same net shape, the exact-2x path); a[::2, ::2] (same net shape, an upscale); a crop of a with
    another net shape."""
    a = np.ascontiguousarray(golden(G)["sp_a_image"])
    return [a, np.ascontiguousarray(np.repeat(np.repeat(a, 2, 0), 2, 1)), np.ascontiguousarray(a[::2, ::2]), np.ascontiguousarray(a[:, :426])]


def _same_result(got, want, image_id=5):
    assert got.coco(image_id) == want.coco(image_id) and got.dropped == want.dropped
    np.testing.assert_array_equal(got.box.view(np.uint32), want.box.view(np.uint32))
    np.testing.assert_array_equal(got.keypoints.view(np.uint64), want.keypoints.view(np.uint64))


def test_predict_on_a_mixed_list_equals_single_predict(detector, mixed):
    net = [(g["out_h"], g["out_w"]) for g in (detector.transform.geometry(*i.shape[:2]) for i in mixed)]
    assert net[3] != net[0] and net[0] == net[1] == net[2]                       # two net shapes; three source sizes within one of them
    assert len({i.shape for i in mixed[:3]}) == 3
    want = [detector.single_predict(i) for i in mixed]
    for w in want:
        assert not isinstance(w, list) and w.shape[0] >= 1                       # every image has a box at this conf_thresh
    for imgs in (mixed, [torch.from_numpy(i).to(DEV) if k % 2 else i for k, i in enumerate(mixed)]):       # numpy, and numpy / CUDA mixed
        got = detector.predict(imgs)
        assert len(got) == len(mixed)
        for g, w in zip(got, want):
            assert g.shape == w.shape
            assert torch.equal(g.view(torch.int32), w.view(torch.int32))
    again = detector.single_predict(mixed[0])                                    # the program goes back to its dense source form
    assert torch.equal(again.view(torch.int32), want[0].view(torch.int32))


@pytest.mark.parametrize("pick", [(0, 1, 2, 3), (0, 3)])
def test_estimate_batch_on_a_mixed_list_equals_estimate_per_image(detector, dconv, mixed, pick):
    """Every image of the list yields MAX_DET = 300 person rows at g14's thresholds, so 300 slots per image are what keeps the images from
    competing - where the pose network can run that many crops: the fp32 implicit GEMM refuses an operand of 2 GiB or more, and layer1's
    [capacity, 64, 48, 256] fp32 activation reaches that at 683 crops.  So the pair of images (two net shapes) runs at 300 x 2 = 600 with
    every detection, and the whole list of four at 640 (test_estimate_batch_equals_two_estimates' capacity) with min_box_score = 0.35,
    which leaves each image between about 40 and 90 of its detections (their scores run from 0.38 down; rank 40 lies near 0.35 - 0.36 and
    rank 80 near 0.34 - 0.35 in every image).  `dropped == 0` on both sides, asserted, is what shows that nothing competed."""
    imgs = [mixed[i] for i in pick]
    est = TopDownPoseEstimator(detector, dconv, capacity=min(300 * len(imgs), 640), min_box_score=0.0 if len(imgs) == 2 else 0.35)
    est.use_graph = False
    one = [est.estimate(i) for i in imgs]
    assert sum(1 for r in one if len(r) >= 1) >= 2 and len({i.shape for r, i in zip(one, imgs) if len(r) >= 1}) >= 2
    got = est.estimate_batch(imgs)
    assert len(got) == len(imgs)
    for g, w in zip(got, one):
        _same_result(g, w)
        assert g.dropped == 0 and w.dropped == 0
    back = est.estimate_batch([torch.from_numpy(i).to(DEV) for i in reversed(imgs)])        # CUDA inputs, another order
    for g, w in zip(back, reversed(one)):
        _same_result(g, w)


def test_mixed_path_keeps_order_and_capacity_semantics(golden, detector, dconv):
    a = golden(G)["sp_a_image"]
    b = np.random.default_rng(26).integers(0, 256, a.shape, dtype=np.uint8)
    est = TopDownPoseEstimator(detector, dconv, capacity=5)
    want = est.estimate_batch(np.stack([a, b, a]))
    assert any(r.dropped > 0 for r in want) and len(want[0]) >= 1
    est._force_mixed = True                                                      # the same-sized list down the mixed path
    got = est.estimate_batch([a, b, a])
    assert [k for k in est._frames if k[1] == 0] and len(got) == 3               # it did take the mixed path: a frame without a source shape
    for g, w in zip(got, want):
        _same_result(g, w)


@pytest.mark.parametrize("flip_test", [False, True])
def test_estimate_boxes_on_three_sizes_equals_per_image(detector, dconv, flip_test):
    rng = np.random.default_rng(43)
    six = np.array([[50, 60, 200, 400, 0.9, 0], [300, 20, 500, 460, 0.8, 0], [10, 10, 120, 200, 0.7, 0], [400, 200, 630, 470, 0.6, 0],
                    [220, 100, 330, 330, 0.5, 0], [120, 250, 260, 470, 0.4, 0]], np.float32)
    sizes = [(480, 640), (240, 320), (360, 333)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    det = np.stack([np.repeat(six * np.array([w / 640, h / 480, w / 640, h / 480, 1, 1], np.float32), 2, axis=0) for h, w in sizes])
    counts = [12, 7, 12]
    est = TopDownPoseEstimator(detector, dconv, capacity=40, flip_test=flip_test)
    one = [est.estimate_boxes(i, d, [c])[0] for i, d, c in zip(imgs, det, counts)]
    assert all(len(r) >= 1 for r in one) and len(one[0]) < 12                    # OKS-NMS suppressed the duplicates
    got = est.estimate_boxes(imgs, det, counts)
    for g, w in zip(got, one):
        _same_result(g, w)
    with pytest.raises(ValueError, match="det"):
        est.estimate_boxes(imgs, det[:2], counts)
    with pytest.raises(ValueError, match="counts"):
        est.estimate_boxes(imgs, det, counts[:2])


def test_renderer_and_encoder_on_a_mixed_list(detector, dconv, mixed):
    imgs = [mixed[0], mixed[2], mixed[3]]
    est = TopDownPoseEstimator(detector, dconv, capacity=600, min_box_score=0.35, renderer=PoseRenderer(), encoder=JpegEncoder(device=DEV))
    est.use_graph = False
    one = []
    for i in imgs:
        r = est.estimate(i)
        one.append((r, r.image.clone(), r.jpeg))
    assert len(one[0][0]) >= 1 and not torch.equal(one[0][1].cpu(), torch.from_numpy(imgs[0]))      # something was drawn
    got = est.estimate_batch(imgs)
    for g, (w, image, jpeg), src in zip(got, one, imgs):
        _same_result(g, w)
        assert g.dropped == 0 and w.dropped == 0                                 # (min_box_score: see the estimate_batch test above)
        assert tuple(g.image.shape) == src.shape and torch.equal(g.image, image)
        assert isinstance(g.jpeg, bytes) and g.jpeg == jpeg and len(jpeg) > 100
    plain = TopDownPoseEstimator(detector, dconv, capacity=600, min_box_score=0.35, encoder=JpegEncoder(device=DEV))    # no renderer: the sources
    plain.use_graph = False
    for g, src in zip(plain.estimate_batch(imgs), imgs):
        assert g.image is None and g.jpeg == plain.estimate(src).jpeg


def test_estimate_files_equals_estimate_batch_on_the_decoded_files(detector, dconv, mixed, tmp_path):
    files = JpegEncoder(device=DEV, quality=90).encode([torch.from_numpy(mixed[0]).to(DEV), torch.from_numpy(mixed[3]).to(DEV)])
    est = TopDownPoseEstimator(detector, dconv, capacity=600)
    decoded = [t.clone() for t in JpegDecoder(device=DEV).decode(files)]
    assert [tuple(t.shape) for t in decoded] == [mixed[0].shape, mixed[3].shape]
    want = est.estimate_batch(decoded)
    assert len(want[0]) >= 1
    path = tmp_path / "b.jpg"
    path.write_bytes(files[1])
    for got in (est.estimate_files(files), est.estimate_files([files[0], str(path)], decoder=JpegDecoder(device=DEV))):
        for g, w in zip(got, want):
            _same_result(g, w)
