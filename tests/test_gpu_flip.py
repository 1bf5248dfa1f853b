"""Flip test on the MI355X.  The two kernels against the numpy statement of their arithmetic (tests/flip_ref.py), forward_crops and the
estimator against the staged composition of the public pieces.  Both sides of every comparison perform the same single-rounded float32
operations (one add, one multiply by 0.5) on the same network output, so every comparison is bitwise."""
import ctypes

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib
from simple_pose_amd.datasets.naive_data import crop_boxes, filter_poses
from simple_pose_amd.detector.nets.yolov5 import YOLOv5
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
from simple_pose_amd.metrics import COCO_JOINT_PAIRS, GaussTaylorKeyPointDecoder, merge_flipped, mirror_input
from simple_pose_amd.pipeline import TopDownPoseEstimator
from tests import flip_ref
from tests.detector_ref import detector_state_dict
from tests.test_gpu_pipeline import _pose_model

pytestmark = pytest.mark.gpu
G = "g14_detector.npz"
DEV = "cuda:0"
P = _lib.ptr
GUARD = 0xA5


def _stream():
    return _lib.current_stream(torch.device(DEV))


# ---- 1. sp_mirror_w -------------------------------------------------------------------------------------------------------------------------
def _halves(n_bytes, offset):
    """One allocation [guard | src | dst | guard] of bytes, src starting `offset` bytes past a 256-byte aligned base."""
    buf = torch.full((offset + 2 * n_bytes + 64,), GUARD, dtype=torch.uint8, device=DEV)
    return buf, buf[offset:offset + n_bytes], buf[offset + n_bytes:offset + 2 * n_bytes]


def _assert_rest_untouched(buf, offset, src_bytes):
    n = src_bytes.size
    b = buf.cpu().numpy()
    assert (b[:offset] == GUARD).all() and (b[offset + 2 * n:] == GUARD).all()
    np.testing.assert_array_equal(b[offset:offset + n], src_bytes)               # the source is only read


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", [(1, 1, 1, 3), (2, 3, 5, 3), (3, 2, 192, 3)])
def test_mirror_w_u8c3_into_the_second_half(shape, offset):
    """(3, 2, 192, 3) from the aligned base takes the 12-byte path; one byte further on the same shape takes the byte path."""
    x = np.random.default_rng(30).integers(0, 256, shape, dtype=np.uint8)
    buf, src, dst = _halves(x.size, offset)
    src.copy_(torch.from_numpy(x.reshape(-1)))
    got = mirror_input(src.view(shape), out=dst.view(shape))
    assert got.data_ptr() == dst.data_ptr() and got.data_ptr() % 4 == (offset + x.size) % 4
    np.testing.assert_array_equal(got.cpu().numpy(), x[:, :, ::-1, :])
    np.testing.assert_array_equal(got.cpu().numpy(), flip_ref.mirror_w(x))
    _assert_rest_untouched(buf, offset, x.reshape(-1))


@pytest.mark.parametrize("rows,w", [(1, 1), (3, 2), (5, 7), (4, 48), (2, 192)])
def test_mirror_w_f32_into_the_second_half(rows, w):
    """4 x 48 and 2 x 192 take the 16-byte path, the others one element per lane; compared as bit patterns (NaN payloads included)."""
    rng = np.random.default_rng(31)
    x = rng.integers(0, 2 ** 32, (rows, w), dtype=np.uint64).astype(np.uint32)   # every bit pattern is a legal fp32 to MOVE
    buf, src, dst = _halves(x.size * 4, 0)
    src.copy_(torch.from_numpy(x.view(np.uint8).reshape(-1)))
    _lib.check(_lib.lib().sp_mirror_w(P(src), P(dst), rows, w, 4, _stream()), "sp_mirror_w")
    np.testing.assert_array_equal(dst.cpu().numpy().view(np.uint32).reshape(rows, w), x[:, ::-1])
    _assert_rest_untouched(buf, 0, x.view(np.uint8).reshape(-1))


def test_mirror_input_f32_nchw_and_empty_batches():
    x = torch.from_numpy(np.random.default_rng(32).standard_normal((2, 3, 5, 48)).astype(np.float32)).to(DEV)
    both = torch.empty((4, 3, 5, 48), device=DEV)
    both[:2].copy_(x)
    got = mirror_input(both[:2], out=both[2:])
    assert got.data_ptr() == both[2:].data_ptr()
    np.testing.assert_array_equal(both[2:].cpu().numpy().view(np.uint32), x.cpu().numpy()[..., ::-1].view(np.uint32))
    np.testing.assert_array_equal(mirror_input(x).cpu().numpy().view(np.uint32), x.cpu().numpy()[..., ::-1].view(np.uint32))
    assert mirror_input(torch.empty((0, 8, 8, 3), dtype=torch.uint8, device=DEV)).shape == (0, 8, 8, 3)
    assert mirror_input(torch.empty((0, 3, 8, 8), device=DEV)).shape == (0, 3, 8, 8)
    e = torch.empty((0, 17, 8, 8), device=DEV)
    assert merge_flipped(e, e).shape == (0, 17, 8, 8)
    with pytest.raises(_lib.HipLibraryError, match="overlap"):
        mirror_input(x, out=x)


# ---- 2. sp_heat_map_flip_merge ----------------------------------------------------------------------------------------------------------------
def _heat(shape, seed):
    """Seeded normal fp32 (negatives included) with one value in sixteen replaced by a denormal of either sign."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape).astype(np.float32)
    flat = a.reshape(-1)
    k = max(1, flat.size // 16)
    idx = rng.choice(flat.size, k, replace=False)
    flat[idx] = (rng.integers(1, 1 << 23, k).astype(np.uint32) | (rng.integers(0, 2, k).astype(np.uint32) << 31)).view(np.float32)
    assert (np.abs(flat[idx]) < np.finfo(np.float32).tiny).all() and (flat[idx] != 0).all()
    return a


MERGE_CASES = [((1, 1, 1, 1), ()), ((2, 3, 4, 5), ((0, 2),)), ((2, 17, 3, 7), COCO_JOINT_PAIRS), ((3, 17, 64, 48), COCO_JOINT_PAIRS)]


@pytest.fixture(scope="module")
def merge_inputs():
    """Per case: hm, hm_flipped (numpy) and the expected output for shift off / on - computed once, never modified."""
    out = {}
    for shape, pairs in MERGE_CASES:
        hm, fl = _heat(shape, 33), _heat(shape, 34)
        want = {s: flip_ref.merge_flipped(hm, fl, pairs, shift=bool(s)) for s in (0, 1)}
        for a in (hm, fl, want[0], want[1]):
            a.setflags(write=False)
        out[shape] = (hm, fl, want)
    return out


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("shape,pairs", MERGE_CASES)
def test_flip_merge_equals_numpy_bitwise(merge_inputs, shape, pairs, shift, in_place, offset):
    """(3, 17, 64, 48) takes the 16-byte path from aligned tensors; `offset` 1 runs every shape from views one element past an aligned
    base (element-per-lane path, also at w = 48)."""
    hm_np, fl_np, want = merge_inputs[shape]
    n = hm_np.size
    view = lambda a: torch.cat([torch.zeros(offset), torch.from_numpy(a.reshape(-1).copy())]).to(DEV)[offset:].view(shape)
    hm, fl = view(hm_np), view(fl_np)
    assert hm.data_ptr() % 16 == 4 * offset and hm.is_contiguous()
    out = hm if in_place else torch.full((offset + n,), float("nan"), device=DEV)[offset:].view(shape)
    got = merge_flipped(hm, fl, pairs, shift=bool(shift), out=out)
    assert got.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want[shift].view(np.uint32))
    np.testing.assert_array_equal(fl.cpu().numpy().view(np.uint32), fl_np.view(np.uint32))                  # read only
    if not in_place:
        np.testing.assert_array_equal(hm.cpu().numpy().view(np.uint32), hm_np.view(np.uint32))
        fresh = merge_flipped(hm, fl, pairs, shift=bool(shift))                                             # out=None: a new tensor
        assert fresh.data_ptr() not in (hm.data_ptr(), fl.data_ptr())
        np.testing.assert_array_equal(fresh.cpu().numpy().view(np.uint32), want[shift].view(np.uint32))


@pytest.mark.parametrize("shape,pairs", MERGE_CASES)
def test_flip_merge_of_an_exact_twin_returns_the_map(merge_inputs, shape, pairs):
    """hm_flipped = mirror + pair swap of hm, shift off: (a + a) * 0.5 == a for every finite fp32, denormals included."""
    hm_np = merge_inputs[shape][0]
    hm, twin = torch.from_numpy(hm_np.copy()).to(DEV), torch.from_numpy(flip_ref.flipped_twin(hm_np, pairs)).to(DEV)
    np.testing.assert_array_equal(merge_flipped(hm, twin, pairs).cpu().numpy().view(np.uint32), hm_np.view(np.uint32))
    if hm_np.shape[3] > 1:                                                                                   # and the shift is not ignored
        assert not np.array_equal(merge_flipped(hm, twin, pairs, shift=True).cpu().numpy().view(np.uint32), hm_np.view(np.uint32))


def test_flip_merge_refusals_on_device_tensors():
    hm = torch.zeros((2, 17, 4, 8), device=DEV)
    with pytest.raises(_lib.HipLibraryError, match="hm_flipped"):
        merge_flipped(hm, hm, out=hm)
    with pytest.raises(ValueError, match="out of range"):
        merge_flipped(hm[:, :3].contiguous(), hm[:, :3].contiguous())                # COCO pairs on 3 joints
    with pytest.raises(ValueError, match="one shape"):
        merge_flipped(hm, hm[:1])
    perm = (ctypes.c_int32 * 17)(*range(17))
    both = torch.zeros((4, 17, 4, 8), device=DEV)
    rc = _lib.lib().sp_heat_map_flip_merge(P(both), P(both[2:]), perm, 2, 17, 4, 8, 0, P(both[1:]), _stream())
    assert rc == -1 and b"hm_flipped" in _lib.lib().sp_last_error()


# ---- 3. forward_crops(flip_test=True) -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dconv():
    return _pose_model("dconv_fp32")


@pytest.fixture(scope="module")
def duc():
    return _pose_model("duc_bf16")


@pytest.mark.parametrize("tag", ["dconv_fp32", "duc_bf16"])
def test_forward_crops_flip_test_equals_the_staged_statement(dconv, duc, tag):
    model = dconv if tag == "dconv_fp32" else duc
    crops = torch.from_numpy(np.random.default_rng(35).integers(0, 256, (3, 256, 192, 3), dtype=np.uint8)).to(DEV)
    mirrored = crops[:, :, torch.arange(191, -1, -1, device=DEV)].contiguous()       # torch indexing: the TEST side only
    with torch.no_grad():
        plain = model.forward_crops(crops)
        a, b = plain.cpu().numpy(), model.forward_crops(mirrored).cpu().numpy()
        for shift in (False, True):
            got = model.forward_crops(crops, flip_test=True, shift_heatmap=shift)
            assert got.shape == (3, 17, 64, 48) and got.dtype == torch.float32
            want = flip_ref.merge_flipped(a, b, COCO_JOINT_PAIRS, shift=shift)
            np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
            assert (got.cpu().numpy() != a).any()                                     # cannot pass on nothing
        off = model.forward_crops(crops, flip_test=False)
        np.testing.assert_array_equal(off.cpu().numpy().view(np.uint32), a.view(np.uint32))
        assert model.forward_crops(crops[:0], flip_test=True).shape == (0, 17, 64, 48)
        with pytest.raises(ValueError, match="joint_pairs"):
            model.forward_crops(crops, flip_test=True, joint_pairs=((1, 2), (2, 3)))


# ---- 4. the estimator ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector(golden):
    m = YOLOv5(scale_name="s", num_cls=80)
    d = YOLOv5Detector(num_cls=80, scale_name="s", device=DEV, slice_idx=0, state_dict=detector_state_dict(m, 14))
    conf, iou, _ = golden(G)["sp_a_thresh"]                                      # g14's single_predict thresholds: their margins keep the
    d.conf_thresh, d.iou_thresh = float(conf), float(iou)                        # detector's own decisions stable
    return d


def _staged(detector, model, img, capacity, image_id=7, shift=False, flip_test=True, boxes=None):
    """single_predict -> crop_boxes -> forward_crops(flip_test=True) -> GaussTaylor -> filter_poses, as a user assembles it; returns
    (dicts, selected detections, persons that reached the pose net)."""
    dev_img = torch.from_numpy(img).to(DEV)
    if boxes is None:
        boxes = detector.single_predict(img)
        if isinstance(boxes, list):
            return [], 0, 0
        boxes = boxes[boxes[:, 5] == 0]
    take = boxes[:capacity]
    if take.shape[0] == 0:
        return [], int(boxes.shape[0]), 0
    crops, tinv, _, _, area = crop_boxes(dev_img, take[:, :4].cpu().numpy())
    with torch.no_grad():
        hm = model.forward_crops(crops, flip_test=flip_test, shift_heatmap=shift)
        kps, mv = GaussTaylorKeyPointDecoder()(hm, tinv)
    res = filter_poses(torch.cat([kps, mv], -1), take[:, 4].double().cpu().numpy(), area, [image_id] * take.shape[0], 0.2, 0.9)
    return res, int(boxes.shape[0]), int(take.shape[0])


def test_estimate_with_flip_test_equals_staged_chain_eager_and_graphed(golden, detector, dconv):
    a = golden(G)["sp_a_image"]
    b = np.random.default_rng(36).integers(0, 256, a.shape, dtype=np.uint8)
    want, n_sel, n_pose = _staged(detector, dconv, a, 32)
    assert n_pose >= 8 and len(want) >= 1                                        # cannot pass on nothing
    est = TopDownPoseEstimator(detector, dconv, capacity=32, flip_test=True)
    est.use_graph = False
    eager_a, eager_b = est.estimate(a), est.estimate(b)
    assert eager_a.coco(7) == want and eager_a.dropped == n_sel - n_pose
    assert eager_b.coco(7) == _staged(detector, dconv, b, 32)[0]
    est.use_graph = True
    first, second = est.estimate(a), est.estimate(a)                             # capture + replay, then a second replay
    other, back = est.estimate(b), est.estimate(torch.from_numpy(a).to(DEV))     # a different image through the same graph, and back
    frame = next(iter(est._frames.values()))
    assert len(est._frames) == 1 and frame.graph is not None and frame.crops.shape[0] == 64
    for got, ref in ((first, eager_a), (second, eager_a), (other, eager_b), (back, eager_a)):
        assert got.coco(7) == ref.coco(7) and got.dropped == ref.dropped
        np.testing.assert_array_equal(got.box, ref.box)
    assert first.keypoints.shape == (len(want), 17, 3)
    plain = TopDownPoseEstimator(detector, dconv, capacity=32)
    plain.use_graph = False
    no_flip = plain.estimate(a)
    assert next(iter(plain._frames.values())).crops.shape[0] == 32
    assert no_flip.coco(7) == _staged(detector, dconv, a, 32, flip_test=False)[0]
    assert no_flip.keypoints.shape != first.keypoints.shape or (no_flip.keypoints != first.keypoints).any()   # the flip test did something


def test_black_image_through_the_flip_test_graph(golden, detector, dconv):
    """conf_thresh 0.36 separates the two inputs with room (test_gpu_pipeline.py documents the margin: the black image's best candidate
    scores 0.3506, image a has 37 candidates above 0.36)."""
    a = golden(G)["sp_a_image"]
    black = np.zeros_like(a)
    keep = detector.conf_thresh
    detector.conf_thresh = 0.36
    try:
        est = TopDownPoseEstimator(detector, dconv, capacity=32, flip_test=True)
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


def test_estimate_boxes_with_shift_heatmap_equals_staged_chain(detector, dconv):
    img = np.random.default_rng(37).integers(0, 256, (480, 640, 3), dtype=np.uint8)
    six = np.array([[50, 60, 200, 400, 0.9, 0], [300, 20, 500, 460, 0.8, 0], [10, 10, 120, 200, 0.7, 0], [400, 200, 630, 470, 0.6, 0],
                    [220, 100, 330, 330, 0.5, 0], [120, 250, 260, 470, 0.4, 0]], np.float32)
    boxes = torch.from_numpy(six).to(DEV)
    got = {}
    for shift in (True, False):
        est = TopDownPoseEstimator(detector, dconv, capacity=8, flip_test=True, shift_heatmap=shift)
        got[shift] = est.estimate_boxes(img, six)[0]
        want, _, n_pose = _staged(detector, dconv, img, 8, shift=shift, boxes=boxes)
        assert n_pose == 6 and len(want) >= 1 and got[shift].coco(7) == want and got[shift].dropped == 0
    assert len(got[True]) != len(got[False]) or (got[True].keypoints != got[False].keypoints).any()           # the shift is not ignored
    with pytest.raises(ValueError, match="out of range"):                        # the range check, once the program's joint count is known
        TopDownPoseEstimator(detector, dconv, capacity=8, flip_test=True, joint_pairs=((1, 17),)).estimate_boxes(img, six)


def test_estimate_batch_with_flip_test_and_reassigned_joint_pairs(golden, detector, dconv):
    """A batch of two images sharing the slots (one of them without detections, conf_thresh 0.36 as above) equals the single-image calls;
    and pairs reassigned after construction reach both the eager launches and a re-captured graph."""
    a = golden(G)["sp_a_image"]
    black = np.zeros_like(a)
    keep = detector.conf_thresh
    detector.conf_thresh = 0.36
    try:
        est = TopDownPoseEstimator(detector, dconv, capacity=32, flip_test=True)
        est.use_graph = False
        one = est.estimate(a)
        assert len(one) >= 1 and one.coco(1) == _staged(detector, dconv, a, 32, image_id=1)[0]
        for imgs, at in ((np.stack([a, black]), 0), (np.stack([black, a]), 1)):
            both = est.estimate_batch(imgs)
            assert len(both) == 2 and len(both[1 - at]) == 0
            assert both[at].coco(1) == one.coco(1) and both[at].dropped == one.dropped
            np.testing.assert_array_equal(both[at].box, one.box)
        est.use_graph = True
        assert est.estimate(a).coco(1) == one.coco(1)
        est.joint_pairs = ((1, 2),)                                              # reassigned: one pair instead of COCO's eight
        fresh = TopDownPoseEstimator(detector, dconv, capacity=32, flip_test=True, joint_pairs=((1, 2),))
        fresh.use_graph = False
        want = fresh.estimate(a)
        assert want.coco(1) != one.coco(1)                                       # the pairs matter
        assert est.estimate(a).coco(1) == want.coco(1)                           # re-captured with the new permutation
        est.use_graph = False
        assert est.estimate(a).coco(1) == want.coco(1)
    finally:
        detector.conf_thresh = keep


# ---- 5. the solver's val.flip_test -----------------------------------------------------------------------------------------------------------------
def test_solver_val_with_flip_test_equals_two_plain_forwards_merged(tmp_path):
    import yaml
    from simple_pose_amd.processors.ddp_pose_resnet_solver import AverageLogger, DDPProcessor
    cfg = {"model_name": "flip", "gpus": "0",
           "data": {"synthetic": 8, "batch_size": 4, "num_workers": 0, "debug": False},
           "model": {"type": "pose_resnet_dconv", "name": "resnet50", "num_joints": 17, "pretrained": False},
           "optim": {"lr": 1e-3, "amp": False, "sync_bn": False, "milestones": [1], "epochs": 1, "gamma": 0.1},
           "val": {"interval": 1, "weight_path": str(tmp_path / "w")}}
    path = tmp_path / "flip.yaml"
    path.write_text(yaml.safe_dump(cfg))
    proc = DDPProcessor(str(path))
    from oracle import nets_oracle
    from simple_pose_amd import synth
    sd = synth.conditioned_state_dict(nets_oracle.state_dict_shapes_resnet50("dconv"), 0)    # heat maps of order one, not the init's zeros
    proc.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    plain = proc.val(0)                                                          # no val.flip_test key: as before
    got = {}
    for shift in (False, True):
        proc.val_cfg.update(flip_test=True, shift_heatmap=shift)
        got[shift] = proc.val(0)
    proc.val_cfg.update(flip_test=True, shift_heatmap=False, joint_pairs=[[1, 2]])
    one_pair = proc.val(0)
    proc.model.eval()
    want = {}
    for key, pairs, shift in ((False, COCO_JOINT_PAIRS, False), (True, COCO_JOINT_PAIRS, True), ("one", ((1, 2),), False)):
        loss_log, acc_log = AverageLogger(), AverageLogger()
        ws = torch.empty(4096, dtype=torch.uint8, device=DEV)
        with torch.no_grad():
            for x, targets, mask, _, _ in proc.vloader:
                a = proc.model(x).cpu().numpy()
                b = proc.model(x[..., torch.arange(x.shape[3] - 1, -1, -1, device=x.device)].contiguous()).cpu().numpy()
                hm = torch.from_numpy(flip_ref.merge_flipped(a, b, pairs, shift=shift)).to(DEV)
                loss = torch.zeros(1, device=DEV)
                B, J, H, W = hm.shape
                _lib.check(_lib.lib().sp_masked_mse(P(hm), P(targets.contiguous()), P(mask.contiguous()), B, J, H * W, P(loss), None, P(ws), _stream()),
                           "sp_masked_mse")
                loss_log.update(loss[0]); acc_log.update(proc.acc_func(hm, targets, mask))
        want[key] = (loss_log.avg(), acc_log.avg())
    proc.model.train()
    assert (got[False]["loss"], got[False]["acc"]) == want[False] and (got[True]["loss"], got[True]["acc"]) == want[True]
    assert (one_pair["loss"], one_pair["acc"]) == want["one"]
    assert len({plain["loss"], got[False]["loss"], got[True]["loss"], one_pair["loss"]}) == 4      # every setting reaches the heat maps
    assert got[False]["results"] == plain["results"] == 4
