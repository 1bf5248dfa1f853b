"""The heat overlay inside TopDownPoseEstimator / PoseTracker / MultiStreamTracker on the MI355X: every canvas is compared, bit for bit,
with tests/heat_ref.py applied to the source (or to the redacted source) with the frame's own heat maps, trans_inv and keep list, and
with tests/render_ref.py on top where a renderer draws.  The detector and the pose net carry the tests' synthetic weights; `gain` is
worked out from the maps they give, so that the overlay is visible."""
import numpy as np
import pytest
import torch

from simple_pose_amd import _lib, synth
from simple_pose_amd.datasets.jpeg import JpegDecoder, JpegEncoder
from simple_pose_amd.detector.nets.yolov5 import YOLOv5
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
from simple_pose_amd.pipeline import TopDownPoseEstimator
from simple_pose_amd.tracking import MultiStreamTracker, PoseTracker
from simple_pose_amd.visualize import HeatOverlay, PoseRenderer, Redactor
from tests import heat_ref, redact_ref, render_ref
from tests.detector_ref import detector_state_dict

pytestmark = pytest.mark.gpu
G = "g14_detector.npz"
DEV = "cuda:0"
CAP = 32


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _differs(got, want, name):
    bad = np.argwhere((got != want).any(axis=2))
    print(f"MEASURED {name}: {bad.shape[0]} of {got.shape[0] * got.shape[1]} pixels differ" + (f", first at (y, x) = {bad[0].tolist()}" if bad.size else ""))
    return bad.shape[0]


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


def _frame_of(est):
    return list(est._frames.values())[-1]            # the most recently used frame


def _frame_arrays(est):
    """The last frame's heat maps, trans_inv and, per image, the rows its keep list names (what the overlay drew)."""
    fr = _frame_of(est)
    hm, ti = fr.hm.cpu().numpy(), fr.trans_inv.cpu().numpy()
    keep, kc, seg = fr.keep.cpu().numpy(), fr.keep_count.cpu().numpy(), fr.seg.cpu().numpy()
    assert hm.shape[0] == est.capacity and hm.dtype == np.float32
    return hm, ti, [heat_ref.live_rows(keep, kc, seg, b, est.capacity) for b in range(fr.B)]


def _style(h):
    return heat_ref.Style(h.joint_mask, h.scale, h.threshold, h.opacity16, h.alpha)


def _heated(est, bases, h=None):
    """heat_ref on `bases` (one image per image of the last frame) with the frame's own buffers."""
    h = est.heat_overlay if h is None else h
    hm, ti, rows = _frame_arrays(est)
    assert len(rows) == len(bases)
    return [heat_ref.overlay(img, _style(h), hm, ti, r, h.lut) for img, r in zip(bases, rows)]


def _redact_style(r):
    return redact_ref.Style(r.region, r.mode, r.cell, r.expand16, r.head_min256, r.head_joints, r.fallback, r.top_frac256, r.in_vis_thre, r.fill)


def _render_style(r):
    return render_ref.Style(r.skeleton, r.joint_r, r.limb_r, r.box_r, r.opacity16, r.in_vis_thre, r.colour_by, r.palette)


def _same_numbers(res, ref, what):
    np.testing.assert_array_equal(res.keypoints, ref.keypoints, err_msg=what)
    np.testing.assert_array_equal(res.score, ref.score, err_msg=what)
    np.testing.assert_array_equal(res.box, ref.box, err_msg=what)
    if ref.track_id is None:
        assert res.track_id is None, what
    else:
        np.testing.assert_array_equal(res.track_id, ref.track_id, err_msg=what)


@pytest.fixture(scope="module")
def gain(golden, detector, dconv):
    """The synthetic pose net's maps are what they are: the gain that puts the largest value of the kept persons' maps at 200 of 255."""
    est = TopDownPoseEstimator(detector, dconv, capacity=CAP, heat_overlay=HeatOverlay())
    est.use_graph = False
    res = est.estimate(golden(G)["sp_a_image"])
    hm, _, rows = _frame_arrays(est)
    top = float(np.nanmax(hm[rows[0]]))
    print(f"MEASURED the kept persons' largest heat value: {top!r} over {len(res)} persons")
    assert len(res) >= 1 and np.isfinite(top) and top > 0
    return 200.0 / 255.0 / top


@pytest.fixture(scope="module")
def heat(gain):
    return HeatOverlay(colormap="jet", opacity=0.75, alpha="value", threshold=0.1, gain=gain)


@pytest.fixture(scope="module")
def redactor():
    return Redactor(mode="fill", fill=(255, 0, 255), cell=8, in_vis_thre=-1.0)          # as tests/test_gpu_redact.py: discs on every head


@pytest.fixture(scope="module")
def renderer():
    return PoseRenderer()


@pytest.fixture(scope="module")
def est(detector, dconv, heat):
    return TopDownPoseEstimator(detector, dconv, capacity=CAP, heat_overlay=heat)


@pytest.fixture(scope="module")
def plain(detector, dconv):
    return TopDownPoseEstimator(detector, dconv, capacity=CAP)


def test_estimate_alone_is_the_reference_eager_and_graphed_and_reassigning_recaptures(golden, est, plain, heat, gain):
    a = golden(G)["sp_a_image"]
    bare = plain.estimate(a)
    assert bare.image is None and len(bare) >= 1
    keep = est.use_graph
    pictures = {}
    try:
        for graph in (False, True):
            est.use_graph = graph
            for _ in range(2 if graph else 1):                                   # the capture, then a replay
                res = est.estimate(a)
            _same_numbers(res, bare, f"heat overlay, use_graph={graph}")
            assert res.image.is_cuda and res.image.dtype == torch.uint8 and tuple(res.image.shape) == a.shape
            want = _heated(est, [a])[0]
            assert (want != a).any()                                             # the overlay is visible
            assert _differs(res.image.cpu().numpy(), want, f"estimate, use_graph={graph}") == 0
            pictures[graph] = res.image.cpu().numpy()
        assert (pictures[False] == pictures[True]).all()                         # replay and eager: the same bytes
        # another overlay on the same estimator: the frame is captured again and shows it
        graph_before = _frame_of(est).graph
        other = HeatOverlay(colormap="gray", opacity=1.0, alpha="constant", threshold=0.3, gain=gain, joints=[0, 5, 6])
        est.heat_overlay = other
        res = est.estimate(a)
        assert _frame_of(est).graph is not graph_before
        want = _heated(est, [a], other)[0]
        assert (want != pictures[True]).any() and (want != a).any()
        assert _differs(res.image.cpu().numpy(), want, "reassigned overlay") == 0
    finally:
        est.use_graph, est.heat_overlay = keep, heat


def test_stand_alone_overlay_of_the_kept_rows_is_the_frames_canvas(golden, est, heat):
    a = golden(G)["sp_a_image"]
    res = est.estimate(a)
    canvas = res.image.clone()
    fr = _frame_of(est)
    _, _, rows = _frame_arrays(est)
    idx = torch.tensor(rows[0], dtype=torch.long, device=DEV)
    assert torch.equal(heat.overlay(a, fr.hm[idx], fr.trans_inv[idx]), canvas)


def test_order_redaction_heat_capsules_and_the_encoder(golden, detector, dconv, plain, heat, redactor, renderer):
    a = golden(G)["sp_a_image"]
    enc, dec = JpegEncoder(DEV, quality=85, subsampling="4:2:0"), JpegDecoder(DEV)
    full = TopDownPoseEstimator(detector, dconv, capacity=CAP, heat_overlay=heat, redactor=redactor, renderer=renderer, encoder=enc)
    bare = plain.estimate(a)
    for graph in (False, True):
        full.use_graph = graph
        for _ in range(2 if graph else 1):
            res = full.estimate(a)
        _same_numbers(res, bare, f"all stages, use_graph={graph}")
        red = redact_ref.redact(a, _redact_style(redactor), res.keypoints, res.box)
        hot = _heated(full, [red])[0]
        want = render_ref.render(hot, _render_style(renderer), res.keypoints, res.box)
        assert (red != a).any() and (hot != red).any() and (want != hot).any()
        assert _differs(res.image.cpu().numpy(), want, f"redaction, heat, capsules, use_graph={graph}") == 0
        again = JpegEncoder(DEV, quality=85, subsampling="4:2:0").encode([_up(want)])[0]
        assert isinstance(res.jpeg, bytes) and res.jpeg == again                 # the file is the file of the canvas
        assert torch.equal(dec.decode([res.jpeg])[0], dec.decode([again])[0])
    # heat alone under an encoder: the canvas, not the source, is encoded
    only = TopDownPoseEstimator(detector, dconv, capacity=CAP, heat_overlay=heat, encoder=enc)
    res = only.estimate(a)
    want = _heated(only, [a])[0]
    assert _differs(res.image.cpu().numpy(), want, "heat + encoder") == 0
    assert res.jpeg == JpegEncoder(DEV, quality=85, subsampling="4:2:0").encode([_up(want)])[0]
    # heat and a renderer without a redactor: out of place from the source, then the capsules in place
    two = TopDownPoseEstimator(detector, dconv, capacity=CAP, heat_overlay=heat, renderer=renderer)
    res = two.estimate(a)
    want = render_ref.render(_heated(two, [a])[0], _render_style(renderer), res.keypoints, res.box)
    assert _differs(res.image.cpu().numpy(), want, "heat + renderer") == 0


def test_flip_test_draws_the_merged_maps(golden, detector, dconv, heat):
    a = golden(G)["sp_a_image"]
    flipped = TopDownPoseEstimator(detector, dconv, capacity=CAP, heat_overlay=heat, flip_test=True)
    ref = TopDownPoseEstimator(detector, dconv, capacity=CAP, flip_test=True)
    single = TopDownPoseEstimator(detector, dconv, capacity=CAP, heat_overlay=heat)
    for graph in (False, True):
        flipped.use_graph = graph
        res = flipped.estimate(a)
        _same_numbers(res, ref.estimate(a), f"flip test, use_graph={graph}")
        fr = _frame_of(flipped)
        assert fr.hm.shape[0] == CAP and fr.crops.shape[0] == 2 * CAP            # the merged first half, not the mirrored second
        want = _heated(flipped, [a])[0]
        assert (want != a).any() and _differs(res.image.cpu().numpy(), want, f"flip test, use_graph={graph}") == 0
    single.estimate(a)
    assert (_frame_arrays(single)[0] != _frame_arrays(flipped)[0]).any()         # the merged maps are other maps


def test_batches_mixed_sizes_and_caller_boxes(golden, est, plain):
    a = golden(G)["sp_a_image"]
    b = np.ascontiguousarray(a[:, ::-1])
    got, ref = est.estimate_batch([a, b]), plain.estimate_batch([a, b])
    wants = _heated(est, [a, b])
    for i, (r, rr, img, want) in enumerate(zip(got, ref, (a, b), wants)):
        _same_numbers(r, rr, "dense batch")
        assert (want != img).any() == (len(r) > 0) and _differs(r.image.cpu().numpy(), want, f"dense batch image {i}") == 0
    assert len(got[0]) > 0
    # the same list down the mixed path, and a list of two sizes
    est._force_mixed = True
    try:
        got = est.estimate_batch([a, b])
        for i, (r, rr, want) in enumerate(zip(got, ref, _heated(est, [a, b]))):
            _same_numbers(r, rr, "forced mixed batch")
            assert _differs(r.image.cpu().numpy(), want, f"forced mixed batch image {i}") == 0
    finally:
        est._force_mixed = False
    c = np.ascontiguousarray(a[: a.shape[0] - 37, : a.shape[1] - 50])
    got, ref = est.estimate_batch([a, c]), plain.estimate_batch([a, c])
    for r, rr, img, want in zip(got, ref, (a, c), _heated(est, [a, c])):
        _same_numbers(r, rr, "mixed batch")
        assert tuple(r.image.shape) == img.shape
        assert _differs(r.image.cpu().numpy(), want, f"mixed batch {img.shape}") == 0
    assert sum(len(r) for r in got) >= 1
    det = np.array([[20, 30, 200, 300, 0.9, 0], [150, 40, 320, 330, 0.8, 0]], np.float32)
    rb = est.estimate_boxes(a, det)[0]
    want = _heated(est, [a])[0]
    assert len(rb) >= 1 and (want != a).any() and _differs(rb.image.cpu().numpy(), want, "estimate_boxes") == 0
    files = JpegEncoder(DEV, quality=90, subsampling="4:4:4").encode([_up(a), _up(c)])
    decoded = [t.cpu().numpy() for t in JpegDecoder(DEV).decode(files)]
    got = est.estimate_files(files)
    for r, img, want in zip(got, decoded, _heated(est, decoded)):
        assert _differs(r.image.cpu().numpy(), want, f"estimate_files {img.shape}") == 0


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphed"])
def test_tracked_frames_detector_and_propagated(golden, detector, dconv, plain, heat, renderer, graph):
    a = golden(G)["sp_a_image"]
    b = np.ascontiguousarray(a[::-1, ::-1])
    drawn = TopDownPoseEstimator(detector, dconv, capacity=CAP, heat_overlay=heat, renderer=renderer)
    keep = plain.use_graph
    try:
        drawn.use_graph = plain.use_graph = graph
        trk, bare = PoseTracker(drawn, detect_every=2), PoseTracker(plain, detect_every=2)
        kinds, visible = [], 0
        for f, img in enumerate((a, b, a, a)):
            res, ref = trk.update(img), bare.update(img)
            kinds.append(trk.last_frame_kind)
            _same_numbers(res, ref, f"frame {f}")
            hot = _heated(drawn, [img])[0]
            visible += int((hot != img).any())
            want = render_ref.render(hot, _render_style(renderer), res.keypoints, res.box, res.track_id)
            assert _differs(res.image.cpu().numpy(), want, f"tracked frame {f} ({kinds[-1]})") == 0
        assert visible >= 2 and {"detector", "propagated"} <= set(kinds)
    finally:
        plain.use_graph = keep


def test_two_streams(golden, est, plain):
    a = golden(G)["sp_a_image"]
    b = a ^ np.uint8(1)
    multi, bare = MultiStreamTracker(est, streams=2, detect_every=2), MultiStreamTracker(plain, streams=2, detect_every=2)
    kinds = []
    for c, frames in enumerate(([a, b], [b, a], [a, a])):
        got, ref = multi.update(frames), bare.update(frames)
        kinds.append(multi.last_frame_kind)
        for s, want in enumerate(_heated(est, frames)):
            _same_numbers(got[s], ref[s], f"call {c} stream {s}")
            assert _differs(got[s].image.cpu().numpy(), want, f"call {c} stream {s} ({kinds[-1]})") == 0
    assert {"detector", "propagated"} <= set(kinds)


def test_without_an_overlay_everything_is_what_it_was(golden, detector, dconv, redactor, renderer):
    """heat_overlay=None: key points, scores, boxes and the canvas of an estimator with a renderer and a redactor are bit for bit those
    of the same estimator built without the argument - and nothing of the overlay is allocated."""
    a = golden(G)["sp_a_image"]
    without = TopDownPoseEstimator(detector, dconv, capacity=CAP, redactor=redactor, renderer=renderer)
    with_none = TopDownPoseEstimator(detector, dconv, capacity=CAP, redactor=redactor, renderer=renderer, heat_overlay=None)
    for graph in (False, True):
        without.use_graph = with_none.use_graph = graph
        r0, r1 = without.estimate(a), with_none.estimate(a)
        _same_numbers(r1, r0, f"heat_overlay=None, use_graph={graph}")
        assert torch.equal(r0.image, r1.image)
        want = render_ref.render(redact_ref.redact(a, _redact_style(redactor), r0.keypoints, r0.box), _render_style(renderer), r0.keypoints, r0.box)
        assert _differs(r1.image.cpu().numpy(), want, f"heat_overlay=None, use_graph={graph}") == 0
        fr = _frame_of(with_none)
        assert fr.heat_ws is None and fr.hm is None
