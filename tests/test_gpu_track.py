"""The tracker on the MI355X: sp_track_associate and sp_track_boxes through the C ABI against tests/track_ref.py, and PoseTracker end to
end against the staged chain (estimate / estimate_boxes of the same estimator, with track_ref applied to their PoseResults).  Integer state
and every copied value are compared exactly; the similarity matrix bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib, synth
from simple_pose_amd.commons.joint_utils import box_to_center_scale
from simple_pose_amd.detector.nets.yolov5 import YOLOv5
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
from simple_pose_amd.pipeline import TopDownPoseEstimator
from simple_pose_amd.tracking import OneEuro, PoseTracker
from tests import track_ref
from tests.detector_ref import detector_state_dict

pytestmark = pytest.mark.gpu
G = "g14_detector.npz"
DEV = "cuda:0"
P = _lib.ptr
MAX_AGE = 2
FRAMES = 12


def _stream():
    return _lib.current_stream(torch.device(DEV))


# ---- 1. the kernels through the C ABI -------------------------------------------------------------------------------------------------------
class DeviceTracks:
    """The track state as PoseTracker keeps it, and one call of each entry point."""

    def __init__(self, slots, J, sigmas=None):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
        self.slots, self.J = slots, J
        self.t = {"id": z((slots,), torch.int32), "age": z((slots,), torch.int32), "miss": z((slots,), torch.int32),
                  "kps": z((slots, J, 3), torch.float64), "area": z((slots,), torch.float64), "conf": z((slots,), torch.float32),
                  "next_id": torch.ones((1,), dtype=torch.int32, device=DEV)}
        self.sim = torch.full((slots, slots), 7.0, dtype=torch.float64, device=DEV)
        self.sig = None if sigmas is None else (ctypes.c_double * J)(*sigmas)

    def load(self, st):
        for k in ("id", "age", "miss", "kps", "area", "conf"):
            self.t[k].copy_(torch.from_numpy(getattr(st, k)))
        self.t["next_id"].fill_(int(st.next_id))

    def host(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}

    def associate(self, kps, area, box, keep, keep_count, seg, match_thre, max_age):
        rows = kps.shape[0]
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        kps, area, box, keep = d(kps), d(area), d(box), d(keep.astype(np.int32))
        kc, sg = d(np.array([keep_count], np.int32)), d(np.array(seg, np.int32))
        out = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
        t = self.t
        _lib.check(_lib.lib().sp_track_associate(P(kps), P(area), P(box), P(keep), P(kc), P(sg), rows, self.J, self.sig, match_thre, max_age,
                                                 self.slots, P(t["id"]), P(t["age"]), P(t["miss"]), P(t["kps"]), P(t["area"]), P(t["conf"]),
                                                 P(t["next_id"]), P(self.sim), P(out), _stream()), "sp_track_associate")
        return out.cpu().numpy(), self.sim.cpu().numpy()

    def boxes(self, vis, expand, W, H, max_det, cls=0.0):
        det = torch.full((1, max_det, 6), -7.0, device=DEV)
        counts = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        t = self.t
        _lib.check(_lib.lib().sp_track_boxes(P(t["id"]), P(t["miss"]), P(t["kps"]), P(t["conf"]), self.slots, self.J, vis, expand, cls, W, H, max_det,
                                             P(det), P(counts), _stream()), "sp_track_boxes")
        return det.cpu().numpy()[0], int(counts.item())


def _sequence(slots, J, seed):
    """12 frames of (poses [n, J, 3], area [n], conf [n]) in pick order, n <= slots, from 2 * slots + 2 walking persons: births, a frame with
    n = slots, empty frames, a return inside MAX_AGE and one after it, exact duplicates, more new persons than free slots, and two
    persons who cross (swap positions between two frames) while the list is shuffled."""
    rng = np.random.default_rng(seed)
    people = 2 * slots + 2
    base = rng.uniform(100, 1900, (people, 1, 2))
    shape = rng.uniform(-60, 60, (people, J, 2))
    areas = rng.uniform(8000, 40000, people)
    half = max(1, (slots + 1) // 2)
    first, everyone, late = list(range(half)), list(range(slots)), list(range(slots, 2 * slots))
    dup = ([0, 0] + list(range(1, half)))[:slots]
    plan = [first, first, everyone, [], first, [], [], [], first, first, dup, late]
    assert len(plan) == FRAMES
    frames = []
    for f, who in enumerate(plan):
        pos = base + rng.normal(0, 2.0, (people, 1, 2)) * (f > 0)
        if f == 9 and slots >= 2:
            pos[[0, 1]] = pos[[1, 0]]                                            # the two have crossed: each stands where the other was
            who = [int(w) for w in rng.permutation(who)]
        k = np.concatenate([pos + shape, rng.uniform(0.05, 1.0, (people, J, 1))], 2)
        frames.append((k[who].reshape(len(who), J, 3), areas[who].reshape(len(who)), rng.uniform(0.1, 1.0, len(who)).astype(np.float32)))
    return frames


CASES = {"slots1_j17": (1, 17, None), "slots4_j17": (4, 17, None), "slots40_j17": (40, 17, None),
         "slots4_j5": (4, 5, [0.05, 0.03, 0.08, 0.1, 0.06]), "slots40_j5": (40, 5, [0.05, 0.03, 0.08, 0.1, 0.06])}
_RUNS = {}


def _run(case):
    """One sequence through the kernels and through track_ref, frame by frame; computed once per case and shared by the tests below."""
    if case in _RUNS:
        return _RUNS[case]
    slots, J, sigmas = CASES[case]
    rng = np.random.default_rng(100 + slots + J)
    dev, ref = DeviceTracks(slots, J, sigmas), track_ref.TrackState(slots, J)
    rows, lo = slots + 5, (0 if J == 17 else 2)                                  # the image's rows start at seg[0]; rows it did not keep lie between
    log = []
    for kps, area, conf in _sequence(slots, J, 7 * slots + J):
        n = kps.shape[0]
        where = lo + rng.permutation(rows - lo)[:n]                              # the kept rows, scattered; keep lists them in pick order
        all_kps, all_area = rng.uniform(0, 2000, (rows, J, 3)), rng.uniform(8000, 40000, rows)
        box = rng.uniform(0, 1, (rows, 5)).astype(np.float32)
        all_kps[where], all_area[where], box[where, 4] = kps, area, conf
        keep = np.full(rows, -1, np.int32)
        keep[lo:lo + n] = where
        before = ref.copy()
        want_ids, want_S = track_ref.associate(ref, kps, area, conf, 0.5, MAX_AGE, sigmas)
        want_rows = np.zeros(rows, np.int32)
        want_rows[where] = want_ids
        got_rows, got_S = dev.associate(all_kps, all_area, box, keep, n, [lo, rows], 0.5, MAX_AGE)
        log.append({"n": n, "kps": kps, "area": area, "before": before, "want": ref.copy(), "got": dev.host(), "want_rows": want_rows,
                    "got_rows": got_rows, "want_S": want_S, "got_S": got_S})
    _RUNS[case] = log
    return log


@pytest.mark.parametrize("case", list(CASES))
def test_associate_sequence_equals_the_reference(case):
    slots = CASES[case][0]
    log = _run(case)
    seen = {"birth": 0, "death": 0, "evict": 0, "match": 0, "empty": 0, "full": 0}
    for f, r in enumerate(log):
        want, got, before = r["want"], r["got"], r["before"]
        np.testing.assert_array_equal(got["id"], want.id, err_msg=f"frame {f}")
        np.testing.assert_array_equal(got["age"], want.age, err_msg=f"frame {f}")
        np.testing.assert_array_equal(got["miss"], want.miss, err_msg=f"frame {f}")
        assert int(got["next_id"][0]) == want.next_id, f
        np.testing.assert_array_equal(r["got_rows"], r["want_rows"], err_msg=f"frame {f}")
        np.testing.assert_array_equal(got["kps"].view(np.uint64), want.kps.view(np.uint64), err_msg=f"frame {f}")
        np.testing.assert_array_equal(got["area"].view(np.uint64), want.area.view(np.uint64), err_msg=f"frame {f}")
        np.testing.assert_array_equal(got["conf"].view(np.uint32), want.conf.view(np.uint32), err_msg=f"frame {f}")
        seen["birth"] += want.next_id - before.next_id
        seen["death"] += int(((before.id != 0) & (want.id == 0)).sum())
        seen["evict"] += int(((before.id != 0) & (want.id != 0) & (want.id != before.id)).sum())
        seen["match"] += int(((before.id != 0) & (want.id == before.id) & (want.miss == 0)).sum())
        seen["empty"] += r["n"] == 0
        seen["full"] += r["n"] == slots
    assert all(seen.values()), seen                                              # the sequence really went through every kind of event


@pytest.mark.parametrize("case", list(CASES))
def test_similarity_workspace_is_bitwise_the_reference(case):
    """S [slots, slots] after every frame, bit for bit: the same operations in the same order as track_ref.oks_pair (numpy's), -1 where
    there is no live track or no pose.  That includes exp: no float64 exp is correctly rounded, numpy's differs from the device math
    library's in the last place (and between machines), so track_ref.exp_f64 states the device library's algorithm with exact fused
    multiply-adds, and tests/test_track_host.py holds that statement within 1 ulp of the true exp."""
    worst, wrong, total = 0, 0, 0
    for r in _run(case):
        a, b = r["got_S"].view(np.int64), r["want_S"].view(np.int64)
        wrong += int((a != b).sum())
        total += a.size
        worst = max(worst, int(np.abs(a - b).max()))
    print(f"MEASURED similarity {case}: {wrong} of {total} entries differ, worst {worst} ulp")
    assert wrong == 0


def test_similarity_of_a_pose_with_itself():
    for case in ("slots4_j17", "slots4_j5"):
        slots, J, sigmas = CASES[case]
        dev = DeviceTracks(slots, J, sigmas)
        rng = np.random.default_rng(3)
        kps, area = rng.uniform(0, 500, (slots, J, 3)), rng.uniform(100, 9000, slots)
        box = np.zeros((slots, 5), np.float32)
        for _ in range(2):                                                       # the same poses twice: every track meets itself
            ids, S = dev.associate(kps, area, box, np.arange(slots), slots, [0, slots], 1.0, 5)
        want = np.float64(J) / np.float64(np.float32(J) + np.float32(1e-12))     # J / (J + 1e-12) as float32 arithmetic gives the denominator
        assert (np.diag(S).view(np.int64) == want.view(np.int64)).all() and want == 1.0
        assert ids.tolist() == list(range(1, slots + 1))                         # S == match_thre matches
        assert dev.host()["age"].tolist() == [2] * slots


def _box_state(slots, J, seed, W, H):
    rng = np.random.default_rng(seed)
    st = track_ref.TrackState(slots, J)
    st.id[:] = rng.integers(0, 3, slots) * rng.integers(1, 900, slots)
    st.miss[:] = rng.integers(0, 2, slots) * rng.integers(1, 4, slots)
    st.conf[:] = rng.uniform(0.05, 1, slots)
    st.kps[:, :, 0], st.kps[:, :, 1] = rng.uniform(0, W, (slots, J)), rng.uniform(0, H, (slots, J))
    st.kps[:, :, 2] = rng.uniform(0, 1, (slots, J))
    special = min(slots, 7)
    st.id[:special], st.miss[:special] = np.arange(1, special + 1), 0
    for t in range(special):
        k = st.kps[t]
        if t == 0:
            k[:, 2] = 0.1                                                        # nothing visible: every joint counts
        elif t == 1:
            k[:, 2] = 0.1
            k[3, 2] = 0.9                                                        # one visible joint: still every joint
        elif t == 2:
            k[:, :2] = k[:, :2] * 3 - (W, H)                                     # far outside the image on every side
        elif t == 3:
            k[:, :2] = (W / 3, H / 7)                                            # every joint on one point
        elif t == 4:
            k[:, :2] = (W + 50.0, -9.0)                                          # one point outside the image
        elif t == 5:
            k[1, 0] = np.nan                                                     # a NaN coordinate is skipped
        else:
            k[:, 0] = np.nan                                                     # no x at all: the edges become 0
    return st


@pytest.mark.parametrize("slots,J,W,H", [(40, 17, 640, 432), (4, 5, 800, 50), (1, 17, 33, 47)])
def test_boxes_equal_the_reference_bitwise(slots, J, W, H):
    dev = DeviceTracks(slots, J)
    for seed in (1, 2):
        st = _box_state(slots, J, seed + slots, W, H)
        dev.load(st)
        want = track_ref.boxes(st, 0.2, 1.25, W, H, cls=0.0)
        det, count = dev.boxes(0.2, 1.25, W, H, max_det=slots + 3)
        assert count == want.shape[0] >= 1
        np.testing.assert_array_equal(det[:count].view(np.uint32), want.view(np.uint32))
        assert (det[count:slots] == 0).all() and (det[slots:] == -7).all()      # zeroed up to `slots`, untouched beyond
    st.miss[:] = 1                                                               # nobody was seen in the last frame
    dev.load(st)
    det, count = dev.boxes(0.2, 1.25, W, H, max_det=slots)
    assert count == 0 and (det == 0).all()


# ---- 2. PoseTracker against the staged chain -------------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def est(detector, dconv):
    return TopDownPoseEstimator(detector, dconv, capacity=32)


def _areas(box):
    """The areas sp_topdown_plan hands to OKS-NMS: the float32 product of box_to_center_scale's scale, widened."""
    out = np.empty(box.shape[0], np.float64)
    for i, (x1, y1, x2, y2) in enumerate(box[:, :4]):
        _, scale = box_to_center_scale(x1, y1, x2 - x1, y2 - y1, 192 / 256)
        scale = np.asarray(scale, np.float32)
        out[i] = np.float64(scale[0] * scale[1])
    return out


class Staged:
    """The tracked frame as a user assembles it from the public pieces: estimate on detector frames, track_ref's boxes and estimate_boxes
    on propagated frames, and track_ref's association of the PoseResult either way."""

    def __init__(self, est, detect_every=1, match_thre=0.5, max_age=30, box_expand=1.25):
        self.est, self.detect_every, self.match_thre, self.max_age, self.box_expand = est, detect_every, match_thre, max_age, box_expand
        self.state = track_ref.TrackState(est.capacity, 17)
        self.since, self.prev_n = 0, 0

    def update(self, img):
        detect = self.prev_n == 0 or self.since >= self.detect_every
        if detect:
            res = self.est.estimate(img)
        else:
            det = track_ref.boxes(self.state, self.est.in_vis_thre, self.box_expand, img.shape[1], img.shape[0], cls=0.0)
            assert det.shape[0] >= 1
            res = self.est.estimate_boxes(img, det)[0]
        ids, _ = track_ref.associate(self.state, res.keypoints, _areas(res.box), res.box[:, 4], self.match_thre, self.max_age)
        self.since, self.prev_n = (1 if detect else self.since + 1), len(res)
        return res, ids, "detector" if detect else "propagated"


def _same(got, want, ids, f=0):
    np.testing.assert_array_equal(got.track_id, ids, err_msg=f"frame {f}")
    assert got.track_id.dtype == np.int32 and got.track_id.shape == (len(got),)
    np.testing.assert_array_equal(got.keypoints, want.keypoints, err_msg=f"frame {f}")
    np.testing.assert_array_equal(got.box, want.box, err_msg=f"frame {f}")
    np.testing.assert_array_equal(got.score, want.score, err_msg=f"frame {f}")
    assert got.dropped == want.dropped


def _state_equal(trk, ref):
    h = {k: v.cpu().numpy() for k, v in trk.state.items()}
    for k in ("id", "age", "miss"):
        np.testing.assert_array_equal(h[k], getattr(ref, k), err_msg=k)
    assert int(h["next_id"][0]) == ref.next_id
    live = ref.id != 0
    np.testing.assert_array_equal(h["kps"][live], ref.kps[live])
    np.testing.assert_array_equal(h["area"][live], ref.area[live])
    np.testing.assert_array_equal(h["conf"][live], ref.conf[live])


@pytest.mark.parametrize("detect_every", [1, 3])
def test_sequence_of_two_golden_images_equals_the_staged_chain(golden, est, detect_every):
    a, b = golden(G)["sp_a_image"], golden(G)["sp_b_image"]
    trk, ref = PoseTracker(est, detect_every=detect_every), Staged(est, detect_every)
    kinds, total = [], 0
    for f, img in enumerate((a, b, a, b, a, b)):
        want, ids, kind = ref.update(img)
        got = trk.update(img)
        assert trk.last_frame_kind == kind, f
        _same(got, want, ids, f)
        kinds.append(kind)
        total += len(got)
    _state_equal(trk, ref.state)
    assert total >= 6 and kinds[0] == "detector"
    assert ("propagated" in kinds) == (detect_every > 1)
    print("MEASURED frame kinds", detect_every, kinds)


def test_a_frame_without_persons_is_followed_by_a_detector_frame(golden, est, detector):
    """conf_thresh 0.36 separates the golden image from a flat black one with room (tests/test_gpu_pipeline.py measured the margins)."""
    a = golden(G)["sp_a_image"]
    black = np.zeros_like(a)
    keep = detector.conf_thresh
    detector.conf_thresh = 0.36
    try:
        trk, ref = PoseTracker(est, detect_every=2), Staged(est, 2)
        kinds = []
        for f, img in enumerate((a, a, black, a, a)):
            want, ids, kind = ref.update(img)
            got = trk.update(img)
            _same(got, want, ids, f)
            kinds.append(trk.last_frame_kind)
            if f == 2:
                assert len(got) == 0 and got.track_id.shape == (0,)
        assert kinds == ["detector", "propagated", "detector", "detector", "propagated"]
        _state_equal(trk, ref.state)
    finally:
        detector.conf_thresh = keep


def test_same_image_twice_keeps_the_ids_and_reset_restarts_them(golden, est):
    a = golden(G)["sp_a_image"]
    before = est.estimate(a)
    assert before.track_id is None and len(before) >= 1
    trk = PoseTracker(est)
    first, second = trk.update(a), trk.update(a)
    n = len(first)
    assert n == len(before) and first.track_id.tolist() == list(range(1, n + 1)) == second.track_id.tolist()
    np.testing.assert_array_equal(first.keypoints, second.keypoints)
    t = trk.tracks()
    assert sorted(t["id"].tolist()) == list(range(1, n + 1)) and t["age"].tolist() == [2] * n and t["miss"].tolist() == [0] * n
    trk.reset()
    assert trk.tracks()["id"].size == 0
    again = trk.update(a)
    assert again.track_id.tolist() == list(range(1, n + 1)) and trk.last_frame_kind == "detector"
    # and the plain estimator is what it was: same result, no ids
    after = est.estimate(a)
    assert after.track_id is None and after.coco(1) == before.coco(1)
    np.testing.assert_array_equal(after.box, before.box)
    np.testing.assert_array_equal(first.keypoints, before.keypoints)


def test_graph_replays_equal_eager_frames(golden, est):
    a, b = golden(G)["sp_a_image"], golden(G)["sp_b_image"]
    seq = (a, b, a, a, b, a, torch.from_numpy(a).to(DEV))
    keep = est.use_graph
    try:
        est.use_graph = False
        eager_trk = PoseTracker(est, detect_every=2)
        eager = [(eager_trk.update(i), eager_trk.last_frame_kind) for i in seq]
        est.use_graph = True
        trk = PoseTracker(est, detect_every=2)
        graphed = [(trk.update(i), trk.last_frame_kind) for i in seq]
    finally:
        est.use_graph = keep
    assert {k for _, k in eager} == {"detector", "propagated"}
    for f, ((got, gk), (want, wk)) in enumerate(zip(graphed, eager)):
        assert gk == wk
        _same(got, want, want.track_id, f)
    assert 2 <= len(trk._graphs) <= 4 and not eager_trk._graphs                  # one graph per (source shape, frame kind), replayed
    for k in ("id", "age", "miss", "next_id", "kps"):
        assert torch.equal(trk.state[k], eager_trk.state[k]), k


def test_state_and_smooth_state_are_unbatched_views_of_the_live_memory(golden, est):
    """PoseTracker shows its tracks and its smoother's state without the stream axis, and what it shows is the memory the kernels use."""
    a = golden(G)["sp_a_image"]
    n, J = 256, 17
    trk = PoseTracker(est, slots=n, smooth=OneEuro())
    assert trk.state == {} and trk.smooth_state == {}                            # nothing before the first frame
    first, _ = trk.update(a), trk.update(a)
    assert len(first) >= 1
    shapes = lambda d: {k: (tuple(v.shape), v.dtype) for k, v in d.items()}
    i32, f32, f64 = torch.int32, torch.float32, torch.float64
    assert shapes(trk.state) == {"id": ((n,), i32), "age": ((n,), i32), "miss": ((n,), i32), "kps": ((n, J, 3), f64), "area": ((n,), f64),
                                 "conf": ((n,), f32), "next_id": ((1,), i32)}
    assert shapes(trk.smooth_state) == {"id": ((n,), i32), "x": ((n, J, 2), f64), "dx": ((n, J, 2), f64), "t": ((n, J), f64),
                                        "n": ((n, J), i32), "now": ((1,), f64)}
    assert int(trk.state["next_id"][0]) == len(first) + 1 and int((trk.state["id"] != 0).sum()) == len(first)
    assert float(trk.smooth_state["now"].item()) == 1 / 30.0                     # the second frame's default time: index 1 / fps
    trk.reset()
    for name, d in (("state", trk.state), ("smooth_state", trk.smooth_state)):
        for k, v in d.items():
            want = 1 if k == "next_id" else 0
            assert bool((v == want).all()), (name, k)
    third = trk.update(a)
    assert sorted(trk.state["id"][trk.state["id"] != 0].tolist()) == third.track_id.tolist() == list(range(1, len(first) + 1))
    assert int(trk.state["next_id"][0]) == len(first) + 1
