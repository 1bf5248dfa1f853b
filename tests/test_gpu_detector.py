"""YOLOv5 detector on the MI355X: every new kernel against its restatement, the conv epilogue bits, the full s forward, NMS and
single_predict against the reference (g14), graph replay against eager, and the detector -> pose chain."""
import ctypes

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib, engine
from simple_pose_amd._lib import ConvDesc
from simple_pose_amd.detector.nets.yolov5 import YOLOv5
from simple_pose_amd.detector.yolov5_detector import ScalePadding, YOLOv5Detector, non_max_suppression
from tests.desc_interp import conv_desc_cpu
from tests.detector_ref import detector_state_dict, focus_np, letterbox_np

pytestmark = pytest.mark.gpu
G = "g14_detector.npz"
DEV = "cuda:0"
P = _lib.ptr


def _stream():
    return _lib.current_stream(torch.device(DEV))


def test_letterbox_u8_and_focus_match_restatement():
    rng = np.random.default_rng(0)
    for h, w in ((300, 301), (480, 640), (1280, 1280), (375, 500), (200, 900)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        t = ScalePadding(target_size=(640, 640), minimum_rectangle=True)
        g = t.geometry(h, w)
        want = letterbox_np(img, g)
        got, _, _ = t.make_border(img)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        f = torch.empty((g["out_h"] // 2, g["out_w"] // 2, 12), device=DEV)
        _lib.check(_lib.lib().sp_yolo_letterbox(P(torch.from_numpy(img).to(DEV)), 1, h, w, g["new_h"], g["new_w"], g["top"], g["left"], g["out_h"],
                                                g["out_w"], _lib.SP_LETTERBOX_FOCUS, P(f), _stream()))
        np.testing.assert_array_equal(f.cpu().numpy(), focus_np(want))


def test_spp_and_upsample_slices_bit_exact():
    torch.manual_seed(0)
    B, h, w, c = 2, 13, 11, 8
    buf = torch.randn(B, h, w, 4 * c + 4, device=DEV)
    x = buf[..., :c].clone()
    _lib.check(_lib.lib().sp_yolo_spp_nhwc(P(buf), B, h, w, c, 4 * c + 4, _stream()))
    xc = x.permute(0, 3, 1, 2)
    for i, k in enumerate((5, 9, 13)):
        ref = torch.nn.functional.max_pool2d(xc, k, 1, k // 2).permute(0, 2, 3, 1)
        assert torch.equal(buf[..., (i + 1) * c:(i + 2) * c], ref)
    src = torch.randn(B, h, w, 20, device=DEV)
    dst = torch.full((B, 2 * h, 2 * w, 16), float("nan"), device=DEV)
    _lib.check(_lib.lib().sp_upsample2_slice_nhwc(P(src) + 4 * 8, 20, P(dst) + 4 * 4, 16, B, h, w, 8, _stream()))
    ref = src[..., 8:16].repeat_interleave(2, 1).repeat_interleave(2, 2)
    assert torch.equal(dst[..., 4:12], ref) and torch.isnan(dst[..., :4]).all() and torch.isnan(dst[..., 12:]).all()


def _desc(h, w, cin, cout, out_c, flags):
    d = ConvDesc()
    d.batch, d.in_h, d.in_w, d.c_in = 1, h, w, cin
    d.grid_h, d.grid_w, d.c_out, d.n_pad = h, w, cout, 64 if cout <= 64 else 128
    d.taps_h, d.taps_w, d.k_pad, d.stride = 1, 1, cin, 1
    d.dy_step = d.dx_step = 1
    d.out_h, d.out_w, d.out_c = h, w, out_c
    d.oy_mul = d.ox_mul = 1
    d.phases_y = d.phases_x = 1
    d.flags = flags
    return d


def test_hardswish_slice_conv_against_interpreter():
    from simple_pose_amd.engine import HipPacker
    torch.manual_seed(1)
    B, h, w, cin, cout = 2, 10, 12, 64, 40
    wt = torch.randn(cout, cin, 1, 1, device=DEV) * 0.2
    packed = HipPacker().conv(wt)[0]
    scale, shift = torch.rand(cout, device=DEV) + 0.5, torch.randn(cout, device=DEV)
    x = torch.randn(B, h, w, cin, device=DEV)
    # hardswish + residual (added after the activation)
    d = _desc(h, w, cin, cout, cout, _lib.SP_CONV_HARDSWISH)
    d.n_pad = packed.shape[0]
    d.batch = B
    res = torch.randn(B, h, w, cout, device=DEV)
    y = torch.empty(B, h, w, cout, device=DEV)
    _lib.check(_lib.lib().sp_conv2d_fwd(d, P(x), P(packed), P(scale), P(shift), P(res), P(y), _stream()))
    t = torch.empty(B, h, w, cout)
    dd = _desc(h, w, cin, cout, cout, 0)
    dd.n_pad, dd.batch = packed.shape[0], B
    conv_desc_cpu(dd, x.cpu(), packed.cpu(), scale.cpu(), shift.cpu(), None, t, B)
    ref = torch.nn.functional.hardswish(t) + res.cpu()
    assert (y.cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()
    # channel slice [8, 48) of a 56-channel tensor, the rest untouched
    ys = torch.full((B, h, w, 56), float("nan"), device=DEV)
    ds = _desc(h, w, cin, cout, 56, _lib.SP_CONV_HARDSWISH | _lib.SP_CONV_OUT_SLICE)
    ds.n_pad, ds.batch = packed.shape[0], B
    _lib.check(_lib.lib().sp_conv2d_fwd(ds, P(x), P(packed), P(scale), P(shift), None, P(ys) + 4 * 8, _stream()))
    hs = torch.nn.functional.hardswish(t)
    assert (ys[..., 8:48].cpu() - hs).abs().max().item() <= 1e-4 * hs.abs().max().item()
    assert torch.isnan(ys[..., :8]).all() and torch.isnan(ys[..., 48:]).all()
    # a residual with the slice is refused
    assert _lib.lib().sp_conv2d_fwd(ds, P(x), P(packed), P(scale), P(shift), P(res), P(ys) + 4 * 8, _stream()) == -1


def test_existing_descriptors_unchanged_and_new_bits_refused():
    lib = _lib.lib()
    # fp32 1x1 that the streaming pw kernel accepts today
    d = _desc(16, 16, 64, 256, 256, 0)
    d.n_pad = 256
    assert lib.sp_conv2d_pw_ok(d) == 1
    for bit in (_lib.SP_CONV_HARDSWISH, _lib.SP_CONV_OUT_SLICE):
        d.flags = bit
        assert lib.sp_conv2d_pw_ok(d) == 0
    # bf16 3x3 32-channel layer: direct / block predicates accept it without, refuse it with the new bits
    b = _desc(16, 16, 32, 32, 32, _lib.SP_CONV_BF16 | _lib.SP_CONV_RELU)
    b.taps_h = b.taps_w = 3
    b.k_pad, b.dy0, b.dx0, b.n_pad = 320, -1, -1, 32
    base = (lib.sp_conv3x3_direct_ok(b), lib.sp_basic_block_c32_ok(b))
    assert base == (1, 1)
    for bit in (_lib.SP_CONV_HARDSWISH, _lib.SP_CONV_OUT_SLICE):
        b.flags = _lib.SP_CONV_BF16 | _lib.SP_CONV_RELU | bit
        assert (lib.sp_conv3x3_direct_ok(b), lib.sp_basic_block_c32_ok(b)) == (0, 0)
        b.tile_m, b.tile_n, b.kernel = 128, 128, _lib.SP_CONV_KERNEL_RING
        assert lib.sp_conv2d_ring_ok(b) == 0
        b.tile_m = b.tile_n = b.kernel = 0
    # bf16 launches refuse the fp32-only bits
    b.flags = _lib.SP_CONV_BF16 | _lib.SP_CONV_HARDSWISH
    buf = torch.zeros(1 << 16, device=DEV)
    assert lib.sp_conv2d_fwd(b, P(buf), P(buf), None, None, None, P(buf), _stream()) == -1


@pytest.fixture(scope="module")
def s_model(golden):
    m = YOLOv5(scale_name="s", num_cls=80)
    m.load_state_dict(detector_state_dict(m, 14))
    return m.to(DEV).eval()


def test_full_s_forward_against_reference(golden, s_model, measured):
    z = golden(G)
    img = z["sp_a_image"]
    g = ScalePadding(target_size=(640, 640), minimum_rectangle=True).geometry(*img.shape[:2])
    canvas = letterbox_np(img, g)
    x = torch.from_numpy(np.ascontiguousarray(canvas[:, :, ::-1].transpose(2, 0, 1))).float().div(255.0)[None].to(DEV)
    full = s_model(x)[0].cpu().numpy()
    want85 = z["pred85"]
    got85 = full[z["pred85_rows"]]
    worst = 0.0
    for lo, hi in ((0, 2), (2, 4), (4, 5), (5, 85)):
        worst = max(worst, np.abs(got85[:, lo:hi] - want85[:, lo:hi]).max() / np.abs(want85[:, lo:hi]).max())
    prog = s_model.hip_program(448, 640, torch.device(DEV), slice_idx=0, source="nchw")
    sl = prog.run(x)[0].cpu().numpy()
    want = z["pred_sliced"]
    for lo, hi in ((0, 2), (2, 4), (4, 5), (5, 6)):
        worst = max(worst, np.abs(sl[:, lo:hi] - want[:, lo:hi]).max() / np.abs(want[:, lo:hi]).max())
    measured("col_group_rel_err", worst, 1e-4)
    assert worst <= 1e-4


@pytest.mark.parametrize("case", ["merge_a", "plain_a", "merge_b", "plain_b", "many"])
def test_gpu_nms_against_reference(golden, case):
    z = golden(G)
    conf, iou, merge, max_det = z[f"nms_{case}_args"]
    pred = torch.from_numpy(z[f"nms_{case}_pred"]).to(DEV)
    got = non_max_suppression(pred, conf, iou, merge=bool(merge), max_det=int(max_det))[0]
    want = z[f"nms_{case}_out"]
    got = np.zeros((0, 6), np.float32) if got is None else got.cpu().numpy()
    assert got.shape == want.shape
    np.testing.assert_array_equal(got[:, 4:], want[:, 4:])      # same boxes kept, same order (score, class)
    np.testing.assert_allclose(got[:, :4], want[:, :4], rtol=1e-5, atol=1e-5 * np.abs(want[:, :4]).max())


def test_nms_above_cap_raises():
    pred = torch.zeros((1, _lib.SP_YOLO_NMS_MAX_CANDIDATES + 1, 6), device=DEV)
    pred[..., 2:4] = 10.0
    pred[..., 4:6] = 0.9
    with pytest.raises(_lib.HipLibraryError, match="cap"):
        non_max_suppression(pred, 0.1, 0.5)


@pytest.fixture(scope="module")
def detector(golden):
    m = YOLOv5(scale_name="s", num_cls=80)
    return YOLOv5Detector(num_cls=80, scale_name="s", device=DEV, slice_idx=0, state_dict=detector_state_dict(m, 14))


def _order_ties(got, want, tie):
    """Rows whose reference scores chain within `tie` of each other (the generator asserts that such candidates never overlap, so only their
    order is open at fp32 network precision) are put in box order in both results; every other row keeps its place."""
    got, want = got.copy(), want.copy()
    i = 0
    while i < len(want):
        j = i + 1
        while j < len(want) and want[j - 1, 4] - want[j, 4] < tie:
            j += 1
        for a in (got, want):
            g = a[i:j]
            a[i:j] = g[np.lexsort((g[:, 1], g[:, 0]))]
        i = j
    return got, want


@pytest.mark.parametrize("case", ["a", "b"])
def test_single_predict_against_reference(golden, detector, case):
    """a: 432x640, r = 1, top = 8, > 3000 candidates (no merge); b: 50x800 resized to 40x640, r = 0.8, top = 12, < 3000 candidates (merge and
    the redundancy filter), boxes clipped at the image border."""
    z = golden(G)
    conf, iou, tie = z[f"sp_{case}_thresh"]
    detector.conf_thresh, detector.iou_thresh = float(conf), float(iou)
    want = z[f"sp_{case}_dets"]
    assert want.shape[0] > 0
    for graph in (False, True):
        detector.use_graph = graph
        got = detector.single_predict(z[f"sp_{case}_image"])
        assert not isinstance(got, list)
        got = got.cpu().numpy()
        assert got.shape == want.shape
        got, want = _order_ties(got, want, tie)
        np.testing.assert_array_equal(got[:, 5], want[:, 5])
        np.testing.assert_allclose(got[:, 4], want[:, 4], rtol=1e-4)            # scores: the network's fp32 parity, same order
        assert np.abs(got[:, :4] - want[:, :4]).max() <= 1e-3


@pytest.mark.parametrize("case", ["a", "b"])
def test_letterboxed_program_against_reference(golden, detector, case, measured):
    """The source="u8" program single_predict runs (letterbox launch + network + decode) against the reference's sliced head output."""
    z = golden(G)
    img = z[f"sp_{case}_image"]
    want = z["pred_sliced"] if case == "a" else z["sp_b_pred"]
    g = detector.transform.geometry(*img.shape[:2])
    got = detector._forward(torch.from_numpy(img).to(DEV)[None], g, False)[0].cpu().numpy()
    assert got.shape == want.shape
    worst = max(np.abs(got[:, lo:hi] - want[:, lo:hi]).max() / np.abs(want[:, lo:hi]).max() for lo, hi in ((0, 2), (2, 4), (4, 5), (5, 6)))
    measured(f"u8_program_rel_err_{case}", worst, 1e-4)
    assert worst <= 1e-4


def test_boxes_to_source_against_restatement():
    from simple_pose_amd.detector.yolov5_detector import boxes_to_source
    rng = np.random.default_rng(9)
    det = rng.uniform(-40, 700, (37, 6)).astype(np.float32)
    h, w, left, top, r = 448, 576, 16, 24, 0.7
    f = np.float32
    want = det.copy()
    want[:, [0, 2]] = (np.clip(want[:, [0, 2]], f(0), f(w)) - f(left)) / f(r)
    want[:, [1, 3]] = (np.clip(want[:, [1, 3]], f(0), f(h)) - f(top)) / f(r)
    got = boxes_to_source(torch.from_numpy(det).to(DEV), (h, w), left, top, r).cpu().numpy()
    np.testing.assert_array_equal(got, want)


def test_graph_replay_equals_eager(detector):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (375, 500, 3), dtype=np.uint8)
    g = detector.transform.geometry(375, 500)
    src = torch.from_numpy(img).to(DEV)[None]
    eager = detector._forward(src, g, False).clone()
    graphed = detector._forward(src, g, True).clone()
    again = detector._forward(src, g, True).clone()
    assert torch.equal(eager, graphed) and torch.equal(graphed, again)
    batch = detector.predict(torch.stack([src[0], src[0]]))
    one = detector.single_predict(img)
    for b in batch:
        assert (isinstance(b, list) and isinstance(one, list)) or torch.equal(b, one)


def test_detector_to_pose_chain(detector):
    from simple_pose_amd.datasets.naive_data import crop_boxes, filter_poses
    from simple_pose_amd.datasets.coco import normalize_crops
    from simple_pose_amd.metrics import GaussTaylorKeyPointDecoder
    from simple_pose_amd.nets import pose_resnet_dconv
    from simple_pose_amd import synth
    from oracle import nets_oracle
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    detector.conf_thresh = 0.05
    boxes = detector.single_predict(img)
    if isinstance(boxes, list) or boxes.shape[0] == 0:           # random weights: fall back to two fixed boxes for the pose half
        boxes = torch.tensor([[50., 60., 200., 400., 0.9, 0.], [300., 20., 500., 460., 0.8, 0.]], device=DEV)
    boxes = boxes[:8]
    crops, tinv, _, _, area = crop_boxes(torch.from_numpy(img).to(DEV), boxes[:, :4].cpu().numpy())
    shapes = nets_oracle.state_dict_shapes_resnet50("dconv")
    sd = {k: torch.from_numpy(v) for k, v in synth.conditioned_state_dict(shapes, seed=0).items()}
    model = pose_resnet_dconv.resnet50(pretrained=False, num_classes=17)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    with torch.no_grad():
        hm = model(normalize_crops(crops))
        kps, mv = GaussTaylorKeyPointDecoder()(hm, tinv)
    kps3 = torch.cat([kps, mv], -1)
    res = filter_poses(kps3, boxes[:, 4].double().cpu().numpy(), area, [7] * boxes.shape[0])
    assert isinstance(res, list) and len(res) >= 1
    for r in res:
        assert r["image_id"] == 7 and len(r["keypoints"]) == 51 and np.isfinite(r["score"])
