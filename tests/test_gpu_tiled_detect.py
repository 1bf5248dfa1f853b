"""Tiled detection on the MI355X: the three launches behind sp_tile_ref against their dense counterparts and the numpy restatement
(tests/tiled_ref.py), then the detector, the estimator and the trackers with a `Tiling` against the same result assembled from public
calls.  Both sides of every comparison run the same device functions (or the same float32 operations in the same order), so everything
is compared bit for bit: there is no tolerance in this file."""
import ctypes

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib, synth
from simple_pose_amd.detector.nets.yolov5 import YOLOv5
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector, _workspace
from simple_pose_amd.pipeline import TopDownPoseEstimator
from simple_pose_amd.tiling import Tiling
from simple_pose_amd.tracking import MultiStreamTracker, PoseTracker
from tests import tiled_ref
from tests.detector_ref import detector_state_dict

pytestmark = pytest.mark.gpu
G = "g14_detector.npz"
DEV = "cuda:0"
P = _lib.ptr
F = np.float32


def _stream():
    return _lib.current_stream(torch.device(DEV))


def _table(entries):
    """[dict(data, h, w, pitch, new_h, new_w, top, left, ratio, x0, y0, image, slot)] (missing fields 0) -> sp_tile_ref on the device."""
    refs = (_lib.TileRef * len(entries))()
    for r, e in zip(refs, entries):
        for k, v in e.items():
            setattr(r, k, v)
    raw = np.frombuffer(bytes(refs), np.uint8).reshape(len(entries), ctypes.sizeof(_lib.TileRef))
    return torch.from_numpy(raw.copy()).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- 1. sp_yolo_letterbox_tiles -------------------------------------------------------------------------------------------------------------
FH, FW = 37, 53                      # two frames with an odd pitch
OH, OW = 32, 48
#            frame (y0, x0)   (h, w)    new       (top, left)
LB_CASES = [(0, (3, 5), (20, 30), (20, 30), (4, 6)),             # new == tile: the copy
            (1, (5, 5), (32, 48), (16, 24), (8, 12)),            # an exact 2x reduction; the tile ends in the frame's bottom right corner
            (0, (20, 32), (17, 21), (27, 33), (2, 7)),           # bilinear, enlarging; ends in the bottom right corner too
            (1, (0, 0), (31, 41), (13, 19), (0, 0)),             # bilinear, reducing, from the frame's first pixel
            (1, (36, 52), (1, 1), (5, 7), (27, 41))]             # the last pixel alone, up to the canvas' bottom right corner


@pytest.mark.parametrize("mode", [_lib.SP_LETTERBOX_U8, _lib.SP_LETTERBOX_FOCUS])
def test_letterbox_tiles_equals_letterbox_on_contiguous_copies_bitwise(mode):
    rng = np.random.default_rng(50)
    frames = torch.from_numpy(rng.integers(0, 256, (2, FH, FW, 3), dtype=np.uint8)).to(DEV)
    u8 = mode == _lib.SP_LETTERBOX_U8
    n = len(LB_CASES)
    want = []
    for f, (y0, x0), (h, w), (nh, nw), (top, left) in LB_CASES:
        assert y0 + h <= FH and x0 + w <= FW and top + nh <= OH and left + nw <= OW
        tile = frames[f, y0:y0 + h, x0:x0 + w].contiguous()
        o = torch.full((OH, OW, 3), 7, dtype=torch.uint8, device=DEV) if u8 else torch.full((OH // 2, OW // 2, 12), -7.0, device=DEV)
        _lib.check(_lib.lib().sp_yolo_letterbox(P(tile), 1, h, w, nh, nw, top, left, OH, OW, mode, P(o), _stream()), "sp_yolo_letterbox")
        want.append(o)
    want = torch.stack(want)
    table = _table([dict(data=frames.data_ptr() + ((f * FH + y0) * FW + x0) * 3, h=h, w=w, pitch=FW, new_h=nh, new_w=nw, top=top, left=left,
                         ratio=1.0, x0=x0, y0=y0, image=f, slot=i) for i, (f, (y0, x0), (h, w), (nh, nw), (top, left)) in enumerate(LB_CASES)])
    got = torch.full((n, OH, OW, 3), 9, dtype=torch.uint8, device=DEV) if u8 else torch.full((n, OH // 2, OW // 2, 12), -9.0, device=DEV)
    _lib.check(_lib.lib().sp_yolo_letterbox_tiles(P(table), n, OH, OW, mode, P(got), _stream()), "sp_yolo_letterbox_tiles")
    for i in range(n):
        assert torch.equal(got[i].view(torch.uint8), want[i].view(torch.uint8)), LB_CASES[i]
    if u8:                                                                       # padding and pixels both occur, and the copy is the tile
        assert (want[0] == 114).any() and want[2].float().std().item() > 1.0
        assert torch.equal(got[0, 4:24, 6:36], frames[0, 3:23, 5:35])
    else:
        assert want.std().item() > 0.01


# ---- 2. sp_yolo_boxes_to_frame_tiles --------------------------------------------------------------------------------------------------------
def test_boxes_to_frame_tiles_scatters_two_groups_bitwise():
    rng = np.random.default_rng(51)
    M, frames, passes = 8, 2, 3
    # per group: canvas (h, w), then per pass (image, slot, count, status, left, top, ratio, x0, y0)
    groups = [((448.0, 640.0), [(0, 0, 0, 0, 0, 8, 1.0, 0, 0), (1, 0, M, 0, 4, 0, 0.5, 0, 0)]),
              ((512.0, 640.0), [(0, 1, 3, 0, 0, 0, 2.0, 240, 0), (0, 2, M, 0, 13, 2, 1.4814814814814814, 320, 176),
                                (1, 1, 0, 0, 0, 30, 2.0, 0, 176), (1, 2, 5, 1, 7, 0, 0.7123, 3200, 1520)])]
    cand = torch.full((frames, passes, M, 6), float("nan"), device=DEV)
    cand_counts = torch.full((frames, passes), -7, dtype=torch.int32, device=DEV)
    status_frames = torch.zeros((frames,), dtype=torch.int32, device=DEV)
    want = None
    for (ih, iw), rows in groups:
        n = len(rows)
        det = rng.uniform(-60, 700, (n, M, 6)).astype(F)                         # below 0 and beyond the canvas: the clip acts
        det[..., 4:] = rng.uniform(0, 1, (n, M, 2))
        counts = np.array([r[2] for r in rows], np.int32)
        status = np.array([r[3] for r in rows], np.int32)
        refs = [dict(image=r[0], slot=r[1], left=r[4], top=r[5], ratio=float(F(r[6])), x0=r[7], y0=r[8]) for r in rows]
        d_dev, c_dev, s_dev = torch.from_numpy(det).to(DEV), torch.from_numpy(counts).to(DEV), torch.from_numpy(status).to(DEV)
        _lib.check(_lib.lib().sp_yolo_boxes_to_frame_tiles(P(d_dev), P(c_dev), P(s_dev), P(_table(refs)), n, passes, M, ih, iw, P(cand),
                                                           P(cand_counts), P(status_frames), _stream()), "sp_yolo_boxes_to_frame_tiles")
        assert np.array_equal(_bits(d_dev.cpu().numpy()), _bits(det))           # out of place: the group's rows stay
        want = tiled_ref.scatter_np(det, counts, status, refs, frames, passes, M, ih, iw, *(want or ()))
    got = cand.cpu().numpy()
    assert not np.isnan(got).any()                                               # every row of every block is written
    np.testing.assert_array_equal(_bits(got), _bits(want[0]))
    assert cand_counts.cpu().numpy().tolist() == want[1].tolist() == [[0, 3, M], [M, 0, 5]]
    assert status_frames.tolist() == want[2].tolist() == [0, 1]
    assert (got[0, 1, 3:] == 0).all() and (got[0, 0] == 0).all() and got[1, 2, :5, 1].min() >= 1520     # zeros past the counts; the origin is added


# ---- 3. sp_yolo_merge_passes ----------------------------------------------------------------------------------------------------------------
def _merge(cand, counts, metric="ios", thresh=0.5, agnostic=False, max_det=300):
    """cand [frames, passes, M, 6], counts [frames, passes] (numpy) through the C ABI -> (det, counts), checked against the reference."""
    cand, counts = np.ascontiguousarray(cand, F), np.ascontiguousarray(counts, np.int32)
    frames, passes, M, _ = cand.shape
    assert M == max_det
    ws = _workspace(frames, torch.device(DEV))
    det = torch.full((frames, max_det, 6), float("nan"), device=DEV)
    cnt = torch.full((frames,), -7, dtype=torch.int32, device=DEV)
    c_dev, n_dev = torch.from_numpy(cand).to(DEV), torch.from_numpy(counts).to(DEV)
    code = _lib.SP_TILE_IOS if metric == "ios" else _lib.SP_TILE_IOU
    _lib.check(_lib.lib().sp_yolo_merge_passes(P(c_dev), P(n_dev), frames, passes, max_det, code, thresh, int(agnostic), P(ws), ws.numel(), P(det),
                                               P(cnt), _stream()), "sp_yolo_merge_passes")
    det, cnt = det.cpu().numpy(), cnt.cpu().numpy()
    w_det, w_cnt = tiled_ref.merge_np(cand, counts, metric, thresh, agnostic, max_det)
    assert cnt.tolist() == w_cnt.tolist()
    np.testing.assert_array_equal(_bits(det), _bits(w_det))                      # rows past the count are zeros on both sides
    return det, cnt


def _blocks(frames_passes, M):
    """[[rows of pass 0, rows of pass 1, ...] per frame] -> (cand, counts), the rows past a count filled with a decoy that must not be read."""
    B, Pn = len(frames_passes), max(len(f) for f in frames_passes)
    cand = np.tile(np.array([0, 0, 4000, 4000, 0.99, 0], F), (B, Pn, M, 1))
    counts = np.zeros((B, Pn), np.int32)
    for b, fr in enumerate(frames_passes):
        for p, rows in enumerate(fr):
            rows = np.asarray(rows, F).reshape(-1, 6)
            cand[b, p, :len(rows)] = rows
            counts[b, p] = len(rows)
    return cand, counts


BIG = [10.25, 10.5, 110.25, 210.5, 0.875, 0]
INSIDE = [20.25, 20.25, 60.25, 100.25, 0.75, 0]          # inside BIG: IoU 0.16, IoS 1
FAR = [300.5, 300.5, 340.75, 380.25, 0.5, 0]
EMPTY = [50.25, 50.0, 50.25, 120.0, 0.625, 0]            # zero area, inside BIG: inter 0, IoS 0 / 0


def test_merge_hand_made_cases():
    M = 4
    # the same box from two passes: one survives; an empty frame between two non-empty ones
    cand, counts = _blocks([[[BIG, FAR], [BIG]], [[], []], [[], [FAR]]], M)
    for metric in ("iou", "ios"):
        det, cnt = _merge(cand, counts, metric, 0.5, False, M)
        assert cnt.tolist() == [2, 0, 1] and det[0, 0].tolist() == BIG and det[0, 1].tolist() == FAR and det[2, 0].tolist() == FAR
    # a box contained in a larger one survives IoU at 0.5 and is suppressed under IoS
    cand, counts = _blocks([[[BIG], [INSIDE]]], M)
    assert _merge(cand, counts, "iou", 0.5, False, M)[1].tolist() == [2]
    assert _merge(cand, counts, "ios", 0.5, False, M)[1].tolist() == [1]
    # two classes suppress each other only with `agnostic`
    other = BIG[:4] + [0.5, 1]
    cand, counts = _blocks([[[BIG], [other]]], M)
    for metric in ("iou", "ios"):
        assert _merge(cand, counts, metric, 0.5, False, M)[1].tolist() == [2]
        det, cnt = _merge(cand, counts, metric, 0.5, True, M)
        assert cnt.tolist() == [1] and det[0, 0].tolist() == BIG
    # equal scores across passes: the lower candidate index wins, whichever of the two boxes it is
    a, b = [10, 10, 110, 210, 0.5, 0], [12.5, 10, 112.5, 210, 0.5, 0]
    for first, second in ((a, b), (b, a)):
        cand, counts = _blocks([[[FAR[:4] + [0.25, 0]], [first], [second]]], M)
        det, cnt = _merge(cand, counts, "iou", 0.5, False, M)
        assert cnt.tolist() == [2] and det[0, 0].tolist() == first and det[0, 1, 4] == 0.25
    # a zero-area box: its metric with the box around it is NaN under IoS (0 / 0) and 0 under IoU; neither suppresses, either way round
    for rows in ([[BIG], [EMPTY]], [[EMPTY[:4] + [0.9375, 0]], [BIG]], [[EMPTY], [EMPTY]]):
        cand, counts = _blocks([rows], M)
        for metric in ("iou", "ios"):
            assert _merge(cand, counts, metric, 0.5, False, M)[1].tolist() == [2]


def test_merge_truncates_at_max_det():
    M = 5
    rows = [[40.0 * i, 8.25, 40.0 * i + 30.5, 60.75, 0.25 + i / 64, 0] for i in range(12)]           # 12 disjoint boxes
    cand, counts = _blocks([[rows[:5], rows[5:8], rows[8:]]], M)
    det, cnt = _merge(cand, counts, "ios", 0.5, False, M)
    assert cnt.tolist() == [M] and det[0, :, 4].tolist() == [0.25 + i / 64 for i in (11, 10, 9, 8, 7)]


def test_merge_one_random_frame_at_the_cap():
    """65 passes x 300 rows: every candidate slot the limits allow; quarter-pixel boxes, scores on a 1/4096 grid (ties occur), 3 classes."""
    rng = np.random.default_rng(52)
    Pn, M = _lib.SP_TILE_MAX_PASSES, 300
    assert Pn * M <= _lib.SP_YOLO_NMS_MAX_CANDIDATES
    counts = np.full((1, Pn), M, np.int32)
    # a wide field: the scan reaches max_det early; a narrow one: fewer survivors than max_det, the scan visits all 19500 candidates
    for side, metric, agnostic, full in ((1800, "ios", False, True), (1800, "iou", True, True), (300, "ios", True, False)):
        xy = rng.integers(0, 4 * side, (1, Pn, M, 2)).astype(F) / 4
        wh = rng.integers(4 * 20, 4 * 200, (1, Pn, M, 2)).astype(F) / 4
        sc = rng.integers(1, 4096, (1, Pn, M, 1)).astype(F) / 4096
        cls = rng.integers(0, 3, (1, Pn, M, 1)).astype(F)
        cand = np.concatenate([xy, xy + wh, sc, cls], -1)
        det, cnt = _merge(cand, counts, metric, 0.5, agnostic, M)
        assert ((cnt[0] == M) if full else (5 <= cnt[0] < M)) and (np.diff(det[0, :cnt[0], 4]) <= 0).all()


# ---- 4. the detector, the estimator and the trackers ----------------------------------------------------------------------------------------
TILING = dict(tile=(320, 256), overlap=0.25)                                     # 432x640 -> the frame and six 256x320 tiles


@pytest.fixture(scope="module")
def detector(golden):
    m = YOLOv5(scale_name="s", num_cls=80)
    d = YOLOv5Detector(num_cls=80, scale_name="s", device=DEV, slice_idx=0, state_dict=detector_state_dict(m, 14))
    conf, iou, _ = golden(G)["sp_a_thresh"]                                      # g14's single_predict thresholds
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
def images(golden):
    a = golden(G)["sp_a_image"]
    assert a.shape == (432, 640, 3)
    return a, np.ascontiguousarray(a[::-1, ::-1])                                # b: a turned by 180 degrees


def _staged_tiled(detector, img, tiling, max_det=300):
    """predict_tiled assembled from public calls: single_predict on the frame, predict on contiguous copies of the tiles, the shift by
    the tiles' origins (one float32 add) and the reference merge.  -> (rows [n, 6], candidates per pass)."""
    passes = tiling.plan(img.shape[0], img.shape[1])
    assert passes[0] == (0, 0) + img.shape[:2] and len(passes) == 7
    whole = detector.single_predict(img)
    tiles = detector.predict([np.ascontiguousarray(img[y:y + h, x:x + w]) for y, x, h, w in passes[1:]])
    rows = []
    for (y0, x0, _, _), r in zip(passes, [whole] + tiles):
        r = np.zeros((0, 6), F) if isinstance(r, list) else r.cpu().numpy()
        r[:, 0] += F(x0); r[:, 2] += F(x0); r[:, 1] += F(y0); r[:, 3] += F(y0)
        rows.append(r)
    cat = np.concatenate(rows, 0)
    keep = tiled_ref.merge_rows_np(cat, tiling.metric, tiling.thresh, tiling.agnostic, max_det)
    src = np.repeat(np.arange(len(rows)), [len(r) for r in rows])
    return cat[keep], [len(r) for r in rows], np.bincount(src[keep], minlength=len(rows))


def test_predict_tiled_equals_the_staged_passes(detector, images):
    """At g14's single_predict thresholds (conf 0.02): run_yolo_program_cpu on the seven letterboxed passes with nms_np gives 300 rows for
    every pass (2100 candidates) and 300 merged rows, 111 of them from the frame and 12 to 49 from each tile: every tile contributes and
    the merge both suppresses and truncates."""
    a, b = images
    t = Tiling(**TILING)
    want, per_pass, kept = _staged_tiled(detector, a, t)
    assert sum(n > 0 for n in per_pass[1:]) >= 2 and 0 < len(want) < sum(per_pass)           # cannot pass on nothing
    assert kept[0] > 0 and sum(n > 0 for n in kept[1:]) >= 2                                 # the frame and the tiles both survive the merge
    got = detector.predict_tiled(a, t)
    assert got.is_cuda and got.dtype == torch.float32
    np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(want))
    # no bit depends on the chunking of the forward, nor on the batch the frame comes in
    keep = detector.TILE_CHUNK
    try:
        detector.TILE_CHUNK = 4
        again = detector.predict_tiled(torch.from_numpy(np.stack([b, a])).to(DEV), t)
    finally:
        detector.TILE_CHUNK = keep
    assert len(again) == 2 and torch.equal(again[1], got)
    np.testing.assert_array_equal(_bits(again[0].cpu().numpy()), _bits(_staged_tiled(detector, b, t)[0]))
    # IoU fuses differently from IoS on the same passes
    iou = Tiling(metric="iou", **TILING)
    np.testing.assert_array_equal(_bits(detector.predict_tiled(a, iou).cpu().numpy()), _bits(_staged_tiled(detector, a, iou)[0]))
    with pytest.raises(TypeError):
        detector.predict_tiled(a, TILING)
    with pytest.raises(ValueError):
        detector.predict_tiled([a, a[:400]], t)


def _want(est_plain, detector, img, tiling):
    return est_plain.estimate_boxes(img, detector.predict_tiled(img, tiling))[0]


def _same(got, want):
    assert got.coco(7) == want.coco(7) and got.dropped == want.dropped and len(want) >= 1
    np.testing.assert_array_equal(got.box, want.box)


def test_estimate_with_tiling_equals_estimate_boxes_on_predict_tiled(detector, dconv, images):
    a, b = images
    t = Tiling(**TILING)
    plain = TopDownPoseEstimator(detector, dconv, capacity=32)
    want_a, want_b = _want(plain, detector, a, t), _want(plain, detector, b, t)
    assert want_a.coco(7) != want_b.coco(7) and want_a.coco(7) != plain.estimate(a).coco(7)          # the images and the tiling both matter
    est = TopDownPoseEstimator(detector, dconv, capacity=32, tiling=t)
    for graph in (False, True):
        est.use_graph = graph
        _same(est.estimate(a), want_a)
        _same(est.estimate(b), want_b)                                           # graphed: a replay on another image - nothing is stale
        _same(est.estimate(a), want_a)
    assert next(iter(est._frames.values())).graph is not None


def test_estimate_batch_with_tiling_equals_two_estimates(detector, dconv, images):
    a, b = images
    est = TopDownPoseEstimator(detector, dconv, capacity=640, tiling=Tiling(**TILING))           # 2 x max_det fit: no competition for slots
    est.use_graph = False
    one = [est.estimate(a), est.estimate(b)]
    two = est.estimate_batch(np.stack([a, b]))
    assert len(two) == 2
    for got, want in zip(two, one):
        _same(got, want)
        np.testing.assert_array_equal(got.keypoints, want.keypoints)


def test_mixed_sizes_with_tiling_are_refused_before_any_launch(detector, dconv, images):
    a, _ = images
    est = TopDownPoseEstimator(detector, dconv, capacity=32, tiling=Tiling(**TILING))
    with pytest.raises(ValueError, match="tiling"):
        est.estimate_batch([a, np.ascontiguousarray(a[:400])])
    assert est._frames == {} and est._stage == {}                                # no frame, no staging buffer: nothing was uploaded or launched
    with pytest.raises(TypeError):
        TopDownPoseEstimator(detector, dconv, tiling=TILING)
    with pytest.raises(ValueError, match="tiles"):                               # the plan's limits, before any launch too
        TopDownPoseEstimator(detector, dconv, tiling=Tiling(tile=(32, 32), overlap=0.0)).estimate(a)


def _same_tracked(got, want):
    np.testing.assert_array_equal(got.keypoints, want.keypoints)
    np.testing.assert_array_equal(got.score, want.score)
    np.testing.assert_array_equal(got.box, want.box)


@pytest.mark.parametrize("graph", [False, True])
def test_trackers_detect_through_the_tiled_path(detector, dconv, images, graph):
    a, b = images
    t = Tiling(**TILING)
    # the streams of a call share the capacity: a score bar between two detections leaves at most 8 persons per image, so that both fit
    sa, sb = (np.sort(detector.predict_tiled(i, t)[:, 4].cpu().numpy().astype(np.float64))[::-1] for i in (a, b))
    bar = max((sa[7] + sa[8]) / 2, (sb[7] + sb[8]) / 2)
    assert 1 <= (sa >= bar).sum() <= 8 and 1 <= (sb >= bar).sum() <= 8
    ests = [TopDownPoseEstimator(detector, dconv, capacity=32, tiling=t, min_box_score=float(bar)) for _ in range(3)]
    for e in ests:
        e.use_graph = graph
    want = ests[0].estimate(a)
    assert 1 <= len(want) <= 8 and want.dropped == 0
    singles = [PoseTracker(ests[0], detect_every=2), PoseTracker(ests[1], detect_every=2)]
    first = singles[0].update(a)
    assert singles[0].last_frame_kind == "detector"
    _same_tracked(first, want)                                                   # a detector frame returns estimate's persons
    assert first.track_id.tolist() == list(range(1, len(want) + 1))
    second = singles[0].update(a)
    assert singles[0].last_frame_kind == "propagated" and len(second) >= 1
    # two streams in one call against a tracker each, every one on a tiled estimator of its own
    other = [singles[1].update(b), singles[1].update(b)]
    multi = MultiStreamTracker(ests[2], streams=2, detect_every=2)
    for f, (wa, wb) in enumerate(zip((first, second), other)):
        got = multi.update(np.stack([a, b]))
        assert multi.last_frame_kind == ("detector", "propagated")[f]
        for g, w in zip(got, (wa, wb)):
            _same_tracked(g, w)
            np.testing.assert_array_equal(g.track_id, w.track_id)
