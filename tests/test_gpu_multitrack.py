"""Several video streams in one call on the MI355X: sp_track_associate_images, sp_track_boxes_images and sp_track_smooth_images through the
C ABI against one tests/track_ref.py / tests/smooth_ref.py state PER STREAM, and MultiStreamTracker end to end against independent
PoseTrackers (and, with propagated frames, against the staged chain of public pieces).  Every comparison is exact: integer state and copied
values with assert_array_equal, doubles bit for bit."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib, synth
from simple_pose_amd.commons.joint_utils import box_to_center_scale
from simple_pose_amd.datasets.jpeg import JpegEncoder
from simple_pose_amd.detector.nets.yolov5 import YOLOv5
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
from simple_pose_amd.pipeline import TopDownPoseEstimator
from simple_pose_amd.tracking import MultiStreamTracker, OneEuro, PoseTracker
from simple_pose_amd.visualize import PoseRenderer
from tests import multitrack_ref, smooth_ref, smooth_scenes, track_ref
from tests.detector_ref import detector_state_dict

pytestmark = pytest.mark.gpu
G = "g14_detector.npz"
DEV = "cuda:0"
P = _lib.ptr
MAX_AGE = 2
FRAMES = 12


def _stream():
    return _lib.current_stream(torch.device(DEV))


def _d(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(DEV)


# ---- 1. the kernels through the C ABI -------------------------------------------------------------------------------------------------------
class DeviceStreams:
    """The stream-major track state as MultiStreamTracker keeps it, and one call of each entry point."""

    def __init__(self, S, slots, J, sigmas=None):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
        self.S, self.slots, self.J = S, slots, J
        self.t = {"id": z((S, slots), torch.int32), "age": z((S, slots), torch.int32), "miss": z((S, slots), torch.int32),
                  "kps": z((S, slots, J, 3), torch.float64), "area": z((S, slots), torch.float64), "conf": z((S, slots), torch.float32),
                  "next_id": torch.ones((S,), dtype=torch.int32, device=DEV)}
        self.sim = torch.full((S, slots, slots), 7.0, dtype=torch.float64, device=DEV)
        self.sig = None if sigmas is None else (ctypes.c_double * J)(*sigmas)

    def load(self, states):
        for k in ("id", "age", "miss", "kps", "area", "conf"):
            self.t[k].copy_(torch.from_numpy(np.stack([getattr(st, k) for st in states])))
        self.t["next_id"].copy_(torch.tensor([int(st.next_id) for st in states], dtype=torch.int32))

    def host(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}

    def associate(self, kps, area, box, keep, keep_count, seg, match_thre, max_age, single=False):
        rows = kps.shape[0]
        kps, area, box, keep = _d(kps), _d(area), _d(box), _d(keep, np.int32)
        kc, sg = _d(keep_count, np.int32), _d(seg, np.int32)
        out = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
        t = self.t
        tail = (P(t["id"]), P(t["age"]), P(t["miss"]), P(t["kps"]), P(t["area"]), P(t["conf"]), P(t["next_id"]), P(self.sim), P(out), _stream())
        if single:
            _lib.check(_lib.lib().sp_track_associate(P(kps), P(area), P(box), P(keep), P(kc), P(sg), rows, self.J, self.sig, match_thre, max_age,
                                                     self.slots, *tail), "sp_track_associate")
        else:
            _lib.check(_lib.lib().sp_track_associate_images(P(kps), P(area), P(box), P(keep), P(kc), P(sg), self.S, rows, self.J, self.sig,
                                                            match_thre, max_age, self.slots, *tail), "sp_track_associate_images")
        return out.cpu().numpy(), self.sim.cpu().numpy()

    def boxes(self, vis, expand, W, H, max_det, cls=0.0):
        """-> det [S + 1, max_det, 6] and counts [S + 1], both prefilled with -7: block S is the neighbour the call must not touch."""
        det = torch.full((self.S + 1, max_det, 6), -7.0, device=DEV)
        counts = torch.full((self.S + 1,), -7, dtype=torch.int32, device=DEV)
        t = self.t
        _lib.check(_lib.lib().sp_track_boxes_images(P(t["id"]), P(t["miss"]), P(t["kps"]), P(t["conf"]), self.S, self.slots, self.J, vis, expand, cls,
                                                    W, H, max_det, P(det), P(counts), _stream()), "sp_track_boxes_images")
        return det.cpu().numpy(), counts.cpu().numpy()


def _sequence(slots, J, seed, rotate=0):
    """tests/test_gpu_track.py's 12-frame plan of (poses [n, J, 3], area [n], conf [n]) in pick order, n <= slots, from 2 * slots + 2
    walking persons - births, a frame with n = slots, empty frames, a return inside MAX_AGE and one after it, exact duplicates, more new
    persons than free slots, two persons who cross - with a seed per stream, and started `rotate` frames into the plan."""
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
    return frames[rotate:] + frames[:rotate]


def _pack(per_stream, slots, J, rng, over=None):
    """One call's shared buffers from every stream's (kps, area, conf): the images' rows back to back behind seg, the kept rows scattered
    among rows the image did not keep.  A stream without poses gets an EMPTY segment when its index is odd (the last one then starts at
    `rows`).  `over`: the stream whose keep_count exceeds `slots` when it is full - two more kept rows follow its first `slots`, which the
    entry must ignore (track_id 0).  -> buffers, and per stream the global rows of the poses the tracker sees."""
    S = len(per_stream)
    sizes = [0 if (kps.shape[0] == 0 and s % 2 == 1) else slots + 5 for s, (kps, _, _) in enumerate(per_stream)]
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rows = max(int(seg[-1]), 1)
    all_kps, all_area = rng.uniform(0, 2000, (rows, J, 3)), rng.uniform(8000, 40000, rows)
    box = rng.uniform(0, 1, (rows, 5)).astype(np.float32)
    keep, keep_count, where = np.full(rows, -1, np.int32), np.zeros(S, np.int32), []
    for s, (kps, area, conf) in enumerate(per_stream):
        n, lo = kps.shape[0], int(seg[s])
        extra = 2 if (s == over and n == slots) else 0
        w = lo + rng.permutation(sizes[s])[:n + extra]
        all_kps[w[:n]], all_area[w[:n]], box[w[:n], 4] = kps, area, conf
        keep[lo:lo + n + extra] = w
        keep_count[s] = n + extra
        where.append(w[:n])
    return {"kps": all_kps, "area": all_area, "box": box, "keep": keep, "keep_count": keep_count, "seg": seg, "rows": rows}, where


CASES = {"s3_slots4_j17": (3, 4, 17, None), "s2_slots1_j5": (2, 1, 5, [0.05, 0.03, 0.08, 0.1, 0.06]), "s5_slots40_j17": (5, 40, 17, None)}
_RUNS = {}


def _run(case):
    """FRAMES calls through the kernels and through one track_ref.TrackState per stream; computed once per case."""
    if case in _RUNS:
        return _RUNS[case]
    S, slots, J, sigmas = CASES[case]
    rng = np.random.default_rng(1000 + 10 * slots + S)
    dev, refs = DeviceStreams(S, slots, J, sigmas), [track_ref.TrackState(slots, J) for _ in range(S)]
    seqs = [_sequence(slots, J, 7 * slots + J + 101 * s, rotate=s) for s in range(S)]
    log = []
    for f in range(FRAMES):
        per_stream = [seqs[s][f] for s in range(S)]
        buf, where = _pack(per_stream, slots, J, rng, over=S - 1)
        want_rows = np.zeros(buf["rows"], np.int32)
        want_S, before = [], [r.copy() for r in refs]
        for s, (kps, area, conf) in enumerate(per_stream):
            ids, Sm = track_ref.associate(refs[s], kps, area, conf, 0.5, MAX_AGE, sigmas)
            want_rows[where[s]] = ids
            want_S.append(Sm)
        got_rows, got_S = dev.associate(buf["kps"], buf["area"], buf["box"], buf["keep"], buf["keep_count"], buf["seg"], 0.5, MAX_AGE)
        log.append({"n": [p[0].shape[0] for p in per_stream], "before": before, "want": [r.copy() for r in refs], "got": dev.host(),
                    "want_rows": want_rows, "got_rows": got_rows, "want_S": np.stack(want_S), "got_S": got_S, "buf": buf})
    _RUNS[case] = log
    return log


def _states_equal(got, want, what):
    """The device's stream-major state against one reference per stream."""
    for s, w in enumerate(want):
        for k in ("id", "age", "miss"):
            np.testing.assert_array_equal(got[k][s], getattr(w, k), err_msg=f"{what} stream {s} {k}")
        assert int(got["next_id"][s]) == w.next_id, (what, s)
        live = w.id != 0
        np.testing.assert_array_equal(got["kps"][s][live].view(np.uint64), w.kps[live].view(np.uint64), err_msg=f"{what} stream {s} kps")
        np.testing.assert_array_equal(got["area"][s][live].view(np.uint64), w.area[live].view(np.uint64), err_msg=f"{what} stream {s} area")
        np.testing.assert_array_equal(got["conf"][s][live].view(np.uint32), w.conf[live].view(np.uint32), err_msg=f"{what} stream {s} conf")


@pytest.mark.parametrize("case", list(CASES))
def test_associate_images_every_stream_equals_its_own_reference(case):
    S, slots = CASES[case][0], CASES[case][1]
    seen = {"birth": 0, "death": 0, "evict": 0, "match": 0, "empty": 0, "full": 0, "empty_segment": 0, "over": 0}
    for f, r in enumerate(_run(case)):
        _states_equal(r["got"], r["want"], f"{case} call {f}")
        np.testing.assert_array_equal(r["got_rows"], r["want_rows"], err_msg=f"call {f}")                # unkept rows 0, nothing left at -7
        np.testing.assert_array_equal(r["got_S"].view(np.uint64), r["want_S"].view(np.uint64), err_msg=f"call {f} similarity")
        seg, kc = r["buf"]["seg"], r["buf"]["keep_count"]
        seen["empty_segment"] += int((np.diff(seg) == 0).any())
        seen["over"] += int((kc > slots).any())
        for s in range(S):
            want, before = r["want"][s], r["before"][s]
            seen["birth"] += want.next_id - before.next_id
            seen["death"] += int(((before.id != 0) & (want.id == 0)).sum())
            seen["evict"] += int(((before.id != 0) & (want.id != 0) & (want.id != before.id)).sum())
            seen["match"] += int(((before.id != 0) & (want.id == before.id) & (want.miss == 0)).sum())
            seen["empty"] += r["n"][s] == 0
            seen["full"] += r["n"][s] == slots
    assert all(seen.values()), seen                                              # the calls really went through every kind of event


def test_a_stream_fed_its_neighbours_poses_one_call_later_keeps_its_own_ids():
    """The cross-talk trap: stream 1 sees exactly stream 0's poses, one call later.  Were any state shared (next_id, the similarity block,
    a track), stream 1's ids would continue stream 0's; both sequences start at 1 and equal their own references."""
    slots, J = 4, 17
    seq = _sequence(slots, J, 77)
    empty = (np.zeros((0, J, 3)), np.zeros(0), np.zeros(0, np.float32))
    rng = np.random.default_rng(5)
    dev, refs = DeviceStreams(2, slots, J), [track_ref.TrackState(slots, J) for _ in range(2)]
    ids_of = [[], []]
    for f in range(FRAMES):
        per_stream = [seq[f], seq[f - 1] if f else empty]
        buf, where = _pack(per_stream, slots, J, rng)
        want_rows = np.zeros(buf["rows"], np.int32)
        for s, (kps, area, conf) in enumerate(per_stream):
            ids, _ = track_ref.associate(refs[s], kps, area, conf, 0.5, MAX_AGE)
            want_rows[where[s]] = ids
            ids_of[s].append(ids.tolist())
        got_rows, _ = dev.associate(buf["kps"], buf["area"], buf["box"], buf["keep"], buf["keep_count"], buf["seg"], 0.5, MAX_AGE)
        np.testing.assert_array_equal(got_rows, want_rows, err_msg=f"call {f}")
        _states_equal(dev.host(), refs, f"call {f}")
        for s in range(2):
            assert got_rows[where[s]].tolist() == ids_of[s][-1]
    assert ids_of[1][1:] == ids_of[0][:-1] and ids_of[1][0] == [] and ids_of[0][0][0] == 1 == ids_of[1][1][0]


def test_one_image_equals_the_single_image_entry():
    """images = 1 against sp_track_associate on the same inputs: the state and the similarity workspace, bit for bit."""
    slots, J = 40, 17
    rng_a, rng_b = np.random.default_rng(9), np.random.default_rng(9)
    a, b = DeviceStreams(1, slots, J), DeviceStreams(1, slots, J)
    for f, fr in enumerate(_sequence(slots, J, 11)):
        buf, _ = _pack([fr], slots, J, rng_a)
        rows_a, S_a = a.associate(buf["kps"], buf["area"], buf["box"], buf["keep"], buf["keep_count"], buf["seg"], 0.5, MAX_AGE)
        buf, _ = _pack([fr], slots, J, rng_b)
        rows_b, S_b = b.associate(buf["kps"], buf["area"], buf["box"], buf["keep"], buf["keep_count"], buf["seg"], 0.5, MAX_AGE, single=True)
        np.testing.assert_array_equal(rows_a, rows_b, err_msg=f"call {f}")
        np.testing.assert_array_equal(S_a.view(np.uint64), S_b.view(np.uint64), err_msg=f"call {f}")
        ha, hb = a.host(), b.host()
        for k in ha:
            np.testing.assert_array_equal(ha[k].view(np.uint8), hb[k].view(np.uint8), err_msg=f"call {f} {k}")
    assert int(a.host()["next_id"][0]) > slots


def _box_state(slots, J, seed, W, H):
    """tests/test_gpu_track.py's box states: random tracks, and up to seven special ones (nothing visible, one visible joint, far outside,
    one point, one point outside, a NaN coordinate, no x at all)."""
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
            k[:, 2] = 0.1
        elif t == 1:
            k[:, 2] = 0.1
            k[3, 2] = 0.9
        elif t == 2:
            k[:, :2] = k[:, :2] * 3 - (W, H)
        elif t == 3:
            k[:, :2] = (W / 3, H / 7)
        elif t == 4:
            k[:, :2] = (W + 50.0, -9.0)
        elif t == 5:
            k[1, 0] = np.nan
        else:
            k[:, 0] = np.nan
    return st


@pytest.mark.parametrize("S,slots,J,W,H", [(3, 40, 17, 640, 432), (2, 1, 17, 33, 47)])
def test_boxes_images_equal_the_reference_per_stream(S, slots, J, W, H):
    dev = DeviceStreams(S, slots, J)
    states = [_box_state(slots, J, 50 + 13 * s + slots, W, H) for s in range(S)]
    states[1].miss[:] = 1                                                        # stream 1: nobody was seen in the last frame
    dev.load(states)
    max_det = slots + 3
    det, counts = dev.boxes(0.2, 1.25, W, H, max_det)
    for s, st in enumerate(states):
        want = track_ref.boxes(st, 0.2, 1.25, W, H, cls=0.0)
        assert int(counts[s]) == want.shape[0], s
        assert (want.shape[0] == 0) == (s == 1)
        np.testing.assert_array_equal(det[s, :want.shape[0]].view(np.uint32), want.view(np.uint32), err_msg=f"stream {s}")
        assert (det[s, want.shape[0]:slots] == 0).all() and (det[s, slots:] == -7).all()     # zeroed up to `slots`, untouched beyond
    assert (det[S] == -7).all() and int(counts[S]) == -7                         # the neighbour's block


SMOOTH_CASE = "slots4_j17"
SMOOTH_S = 3
STILL, JUMP = 4, 6                        # the call at which stream 1's time stands still, and the one at which stream 2's jumps past max_gap


def _smooth_times():
    t = np.zeros((SMOOTH_S, smooth_scenes.FRAMES))
    t[0] = 0.04 * np.arange(smooth_scenes.FRAMES)
    t[1] = 10.0 + 0.033 * np.arange(smooth_scenes.FRAMES)
    t[1, STILL] = t[1, STILL - 1]
    t[2] = 5.0 + 0.04 * np.arange(smooth_scenes.FRAMES)
    t[2, JUMP:] += 0.7
    return t


def test_smooth_images_equal_the_reference_per_stream():
    """Stream s runs smooth_scenes' sequence started s frames in, with a clock of its own.  At call STILL stream 1's time does not advance,
    at call JUMP stream 2's jumps by more than max_gap: those streams' filters start again at those calls, and nobody else's."""
    slots, J = smooth_scenes.CASES[SMOOTH_CASE]
    p = smooth_scenes.PARAMS
    frames = smooth_scenes.sequence(SMOOTH_CASE)
    times = _smooth_times()
    S = SMOOTH_S
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
    st = {"id": z((S, slots), torch.int32), "x": z((S, slots, J, 2), torch.float64), "dx": z((S, slots, J, 2), torch.float64),
          "t": z((S, slots, J), torch.float64), "n": z((S, slots, J), torch.int32)}
    now = z((S,), torch.float64)
    refs = [smooth_ref.SmoothState(slots, J) for _ in range(S)]
    filtered = 0
    for f in range(smooth_scenes.FRAMES):
        frs = [frames[(f + s) % smooth_scenes.FRAMES] for s in range(S)]
        base = np.concatenate([[0], np.cumsum([fr["kps"].shape[0] for fr in frs])]).astype(np.int32)
        kps, box = np.concatenate([fr["kps"] for fr in frs]), np.concatenate([fr["box"] for fr in frs])
        tid = np.concatenate([fr["track_id"] for fr in frs])
        keep = np.concatenate([np.where(fr["keep"] >= 0, fr["keep"] + b, -1) for fr, b in zip(frs, base)]).astype(np.int32)
        seg = np.array([b + fr["seg"][0] for fr, b in zip(frs, base)] + [base[-1]], np.int32)
        kc = np.array([fr["keep_count"] for fr in frs], np.int32)
        t_id = np.stack([fr["t_id"] for fr in frs])
        rows = kps.shape[0]
        out = torch.full((rows, J, 3), -7.0, dtype=torch.float64, device=DEV)
        now.copy_(torch.from_numpy(times[:, f].copy()))
        d_kps, d_box, d_tid, d_keep, d_kc, d_seg, d_t = _d(kps), _d(box), _d(tid), _d(keep), _d(kc), _d(seg), _d(t_id)
        _lib.check(_lib.lib().sp_track_smooth_images(P(d_kps), P(d_box), P(d_tid), P(d_keep), P(d_kc), P(d_seg), S, rows, J, P(d_t), slots, P(now),
                                                     p["min_cutoff"], p["beta"], p["d_cutoff"], p["max_gap"], p["in_vis_thre"], P(st["id"]),
                                                     P(st["x"]), P(st["dx"]), P(st["t"]), P(st["n"]), P(out), _stream()), "sp_track_smooth_images")
        got, got_st = out.cpu().numpy(), {k: v.cpu().numpy() for k, v in st.items()}
        for s, fr in enumerate(frs):
            ev0 = dict(refs[s].events)
            want = smooth_ref.smooth(refs[s], fr["kps"], fr["box"], fr["track_id"], fr["keep"], fr["keep_count"], fr["seg"], fr["t_id"],
                                     times[s, f], p)
            smooth_scenes.bits_equal(got[base[s]:base[s + 1]], want, f"call {f} stream {s} kps_smooth")
            for k in ("id", "x", "dx", "t", "n"):
                smooth_scenes.bits_equal(got_st[k][s], getattr(refs[s], k), f"call {f} stream {s} s_{k}")
            filtered += int(((want != fr["kps"]) & ~np.isnan(fr["kps"])).any())
            by_time = refs[s].events["restart_time"] - ev0["restart_time"]
            by_gap = refs[s].events["restart_gap"] - ev0["restart_gap"]
            assert (by_time > 0) == (f == STILL and s == 1), (f, s, by_time)
            assert (by_gap > 0) == (f == JUMP and s == 2), (f, s, by_gap)
    assert filtered >= 6 and all(r.events["update"] > 0 and r.events["takeover"] > 0 for r in refs)


# ---- 2. MultiStreamTracker against independent PoseTrackers and the staged chain ---------------------------------------------------------------
S3 = 3
CAP = 128                                 # >= 3 x 37: at conf_thresh 0.36 image `a` has at most 37 candidates (tests/test_gpu_pipeline.py counts
#                                           them; tests/test_multitrack_host.py counts the golden rows), so the streams never compete for slots
#        s0 s1 s2     a: the golden image, b: flat black - no candidate at 0.36
PLAN = ["aba", "aaa", "baa", "aaa", "aba", "aaa"]


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
def renderer():
    return PoseRenderer()


@pytest.fixture
def at_036(detector):
    """conf_thresh 0.36 while the test runs: it separates the golden image from a flat black one with room
    (tests/test_gpu_pipeline.py::test_image_without_detections_through_the_same_graph records both margins)."""
    keep = detector.conf_thresh
    detector.conf_thresh = 0.36
    try:
        yield detector
    finally:
        detector.conf_thresh = keep


@pytest.fixture(scope="module")
def est(detector, dconv):
    return TopDownPoseEstimator(detector, dconv, capacity=CAP)


@pytest.fixture(scope="module")
def images(golden):
    a = golden(G)["sp_a_image"]
    return {"a": a, "b": np.zeros_like(a), "c": a ^ np.uint8(1)}                  # c: `a` with every byte's lowest bit flipped


def _calls(images, plan=PLAN):
    return [[images[c] for c in row] for row in plan]


def _same(got, want, what, ids=None):
    np.testing.assert_array_equal(got.track_id, want.track_id if ids is None else ids, err_msg=what)
    assert got.track_id.dtype == np.int32 and got.track_id.shape == (len(got),)
    np.testing.assert_array_equal(got.keypoints, want.keypoints, err_msg=what)
    np.testing.assert_array_equal(got.score, want.score, err_msg=what)
    np.testing.assert_array_equal(got.box, want.box, err_msg=what)
    assert got.dropped == 0 and want.dropped == 0, what                          # the condition CAP is sized for


def _states_match(multi, singles):
    """Stream s's block of the device state against the PoseTracker that saw the same frames."""
    for s, one in enumerate(singles):
        for k in ("id", "age", "miss", "kps", "area", "conf"):
            assert torch.equal(multi.state[k][s], one.state[k]), (s, k)
        assert int(multi.state["next_id"][s]) == int(one.state["next_id"][0]), s


def test_every_detector_frame_equals_three_independent_trackers(at_036, est, images):
    multi, singles = MultiStreamTracker(est, streams=S3), [PoseTracker(est) for _ in range(S3)]
    persons = 0
    for c, frames in enumerate(_calls(images)):
        got = multi.update(frames if c % 2 else np.stack(frames))                # a list and an array alike
        assert multi.last_frame_kind == "detector" and len(got) == S3
        for s in range(S3):
            want = singles[s].update(frames[s])
            _same(got[s], want, f"call {c} stream {s}")
            assert (len(got[s]) == 0) == (PLAN[c][s] == "b"), (c, s)
            persons += len(got[s])
        _states_match(multi, singles)
    assert persons >= 15
    for s in range(S3):
        t, w = multi.tracks(s), singles[s].tracks()
        assert set(t) == set(w)
        for k in t:
            np.testing.assert_array_equal(t[k], w[k])


def _areas(box):
    """The areas sp_topdown_plan hands to OKS-NMS: the float32 product of box_to_center_scale's scale, widened."""
    out = np.empty(box.shape[0], np.float64)
    for i, (x1, y1, x2, y2) in enumerate(box[:, :4]):
        _, scale = box_to_center_scale(x1, y1, x2 - x1, y2 - y1, 192 / 256)
        scale = np.asarray(scale, np.float32)
        out[i] = np.float64(scale[0] * scale[1])
    return out


class Staged:
    """One stream of the tracked call as a user assembles it from the public pieces: estimate on detector calls, track_ref's boxes and
    estimate_boxes on propagated calls (nothing at all when no track was seen in the last call), track_ref's association either way.  The
    call's kind comes from outside: multitrack_ref.FrameKinds over all streams."""

    def __init__(self, est, match_thre=0.5, max_age=30, box_expand=1.25):
        self.est, self.match_thre, self.max_age, self.box_expand = est, match_thre, max_age, box_expand
        self.state = track_ref.TrackState(est.capacity, 17)

    def update(self, img, detect):
        if detect:
            res = self.est.estimate(img)
        else:
            det = track_ref.boxes(self.state, self.est.in_vis_thre, self.box_expand, img.shape[1], img.shape[0], cls=0.0)
            res = self.est.estimate_boxes(img, det)[0] if det.shape[0] else None
        if res is None:
            kps, box = np.zeros((0, 17, 3)), np.zeros((0, 5), np.float32)
        else:
            kps, box = res.keypoints, res.box
        ids, _ = track_ref.associate(self.state, kps, _areas(box), box[:, 4], self.match_thre, self.max_age)
        return res, ids


def _drive(multi, refs, kinds, frames, what):
    """One call through the tracker and through the staged chain of every stream -> (results, the streams that had no track to follow on
    a propagated call)."""
    detect = kinds.next()
    had_tracks = [bool(((r.state.id != 0) & (r.state.miss == 0)).any()) for r in refs]
    want = [r.update(f, detect) for r, f in zip(refs, frames)]
    got = multi.update(frames)
    assert multi.last_frame_kind == kinds.name(detect), what
    silent = []
    for s, (res, ids) in enumerate(want):
        if res is None:
            assert not detect and not had_tracks[s], (what, s)
            assert len(got[s]) == 0 and got[s].track_id.shape == (0,) and got[s].keypoints.shape == (0, 17, 3) and got[s].dropped == 0, (what, s)
            silent.append(s)
        else:
            _same(got[s], res, f"{what} stream {s}", ids)
    kinds.done(detect, [len(g) for g in got])
    return got, silent


def _states_match_refs(multi, refs):
    h = {k: v.cpu().numpy() for k, v in multi.state.items()}
    for s, r in enumerate(refs):
        for k in ("id", "age", "miss"):
            np.testing.assert_array_equal(h[k][s], getattr(r.state, k), err_msg=f"stream {s} {k}")
        assert int(h["next_id"][s]) == r.state.next_id, s
        live = r.state.id != 0
        np.testing.assert_array_equal(h["kps"][s][live], r.state.kps[live])
        np.testing.assert_array_equal(h["area"][s][live], r.state.area[live])
        np.testing.assert_array_equal(h["conf"][s][live], r.state.conf[live])


def test_detect_every_3_equals_the_staged_chain_per_stream(at_036, est, images):
    multi, refs, kinds = MultiStreamTracker(est, streams=S3, detect_every=3), [Staged(est) for _ in range(S3)], multitrack_ref.FrameKinds(S3, 3)
    seen, silent = [], []
    for c, frames in enumerate(_calls(images)):
        silent.append(_drive(multi, refs, kinds, frames, f"call {c}")[1])
        seen.append(multi.last_frame_kind)
    assert seen == ["detector", "propagated", "propagated", "detector", "propagated", "propagated"]
    assert silent[1] == [1] and silent[2] == [1]        # stream 1 saw black at the first detector call: no persons until the next one
    assert silent[0] == silent[3] == silent[4] == silent[5] == []
    _states_match_refs(multi, refs)


def test_a_call_without_persons_in_any_stream_is_followed_by_a_detector_call(at_036, est, images):
    multi = MultiStreamTracker(est, streams=S3, detect_every=2)
    kinds = []
    for row in ("aaa", "aab", "bbb", "aaa", "aaa"):
        got = multi.update([images[c] for c in row])
        kinds.append(multi.last_frame_kind)
        if row == "bbb":
            assert [len(g) for g in got] == [0, 0, 0]
    # the third is due (detect_every); the fourth would be propagated had the third seen anybody
    assert kinds == ["detector", "propagated", "detector", "detector", "propagated"]
    assert all(len(g) >= 1 for g in got)


def test_one_stream_equals_the_single_tracker(at_036, est, images):
    """PoseTracker is the one-stream MultiStreamTracker, so the two sides are one implementation: each of them is also held, frame by
    frame, to the staged chain under multitrack_ref's rule, which shares no code with either."""
    multi, one = MultiStreamTracker(est, streams=1, detect_every=2), PoseTracker(est, detect_every=2)
    ref, rule = Staged(est), multitrack_ref.FrameKinds(1, 2)
    kinds = []
    for f, c in enumerate("aabaa"):
        detect = rule.next()
        res, ids = ref.update(images[c], detect)
        got, want = multi.update(images[c][None])[0], one.update(images[c])
        assert multi.last_frame_kind == one.last_frame_kind == rule.name(detect), f
        kinds.append(multi.last_frame_kind)
        _same(got, want, f"frame {f}")
        assert res is not None, f                                                # (every propagated frame here follows a frame with persons)
        _same(got, res, f"frame {f} against the staged chain", ids)
        _same(want, res, f"frame {f}, PoseTracker against the staged chain", ids)
        rule.done(detect, [len(res)])
    assert kinds == ["detector", "propagated", "detector", "detector", "propagated"]
    _states_match(multi, [one])
    _states_match_refs(multi, [ref])


def test_reset_of_one_stream_restarts_its_ids_and_forces_a_detector_call(at_036, est, images):
    multi, refs, kinds = MultiStreamTracker(est, streams=S3, detect_every=4), [Staged(est) for _ in range(S3)], multitrack_ref.FrameKinds(S3, 4)
    a3 = [images["a"]] * S3
    first, _ = _drive(multi, refs, kinds, a3, "call 0")
    _drive(multi, refs, kinds, a3, "call 1")
    n = len(first[0])
    assert n >= 1 and multi.last_frame_kind == "propagated"
    assert all(r.track_id.tolist() == list(range(1, n + 1)) for r in first)
    before = [int(v) for v in multi.state["next_id"].cpu()]
    live0 = multi.tracks(0)["id"].tolist()
    multi.reset(stream=1)
    refs[1] = Staged(est)
    kinds.reset(1)
    assert multi.tracks(1)["id"].size == 0 and multi.tracks(0)["id"].tolist() == live0 and live0
    again, _ = _drive(multi, refs, kinds, a3, "call 2")                          # equals the staged chains: streams 0 and 2 went on, 1 began again
    assert multi.last_frame_kind == "detector"                                   # two calls after a detector call, detect_every = 4: the reset did it
    assert again[1].track_id.tolist() == list(range(1, n + 1))
    after = [int(v) for v in multi.state["next_id"].cpu()]
    assert after[1] == n + 1 and after[0] >= before[0] > n and after[2] >= before[2] > n     # ids of the others are never handed out again
    _states_match_refs(multi, refs)
    multi.reset()
    assert all(multi.tracks(s)["id"].size == 0 for s in range(S3))
    assert [r.track_id.tolist() for r in multi.update(a3)] == [list(range(1, n + 1))] * S3 and multi.last_frame_kind == "detector"


def test_graphed_calls_equal_eager_calls(at_036, est, images):
    calls = _calls(images) + _calls(images, ["aab", "aaa"])
    keep = est.use_graph
    try:
        est.use_graph = False
        eager_trk = MultiStreamTracker(est, streams=S3, detect_every=2)
        eager = [(eager_trk.update(f), eager_trk.last_frame_kind) for f in calls]
        est.use_graph = True
        trk = MultiStreamTracker(est, streams=S3, detect_every=2)
        graphed = [(trk.update(f), trk.last_frame_kind) for f in calls]
    finally:
        est.use_graph = keep
    assert {k for _, k in eager} == {"detector", "propagated"}
    for c, ((got, gk), (want, wk)) in enumerate(zip(graphed, eager)):
        assert gk == wk
        for s in range(S3):
            _same(got[s], want[s], f"call {c} stream {s}")
    # one graph per frame kind, replayed with other frame sets (which streams are black changes from call to call) and back: nothing stale
    assert len(trk._graphs) == 2 and not eager_trk._graphs
    counts = [[len(r) for r in g] for g, _ in graphed]
    assert counts[0] != counts[2] and counts[0] == counts[4] and counts[0][1] == 0 and counts[2][0] == 0
    for k in ("id", "age", "miss", "next_id", "kps", "area", "conf"):
        assert torch.equal(trk.state[k], eager_trk.state[k]), k


TIMES3 = [[0.0, 0.03, 0.08, 0.07, 0.13, 0.16], [5.0, 5.04, 5.08, 5.12, 5.95, 5.99], [9.0, 9.02, 9.02, 9.1, 9.15, 9.2]]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphed"])
def test_smoothing_with_a_clock_per_stream_equals_independent_smoothing_trackers(at_036, detector, dconv, renderer, images, graph):
    """Stream 0's time steps backwards once, stream 1's jumps past max_gap, stream 2's stands still for a call.  slots above the capacity,
    as tests/test_gpu_smooth.py explains.  The detector calls alternate between the golden image and the same image with every byte's
    lowest bit flipped: its persons are found again a fraction of a pixel away, so the filters have something to filter (the same image
    twice is a pose at rest, which comes out exactly unchanged)."""
    est_r = TopDownPoseEstimator(detector, dconv, capacity=CAP, renderer=renderer)
    est_r.use_graph = graph
    one_euro = OneEuro(min_cutoff=1.0, beta=0.5, d_cutoff=1.0, max_gap=0.5)
    multi = MultiStreamTracker(est_r, streams=S3, slots=256, detect_every=2, smooth=one_euro)
    bare = MultiStreamTracker(est_r, streams=S3, slots=256, detect_every=2)
    singles = [PoseTracker(est_r, slots=256, detect_every=2, smooth=one_euro) for _ in range(S3)]
    moved = 0
    for c, frames in enumerate(_calls(images, ["aaa", "aaa", "ccc", "ccc", "aaa", "aaa"])):
        times = [TIMES3[s][c] for s in range(S3)]
        got, raw = multi.update(frames, timestamps=times), bare.update(frames)
        for s in range(S3):
            want = singles[s].update(frames[s], timestamp=times[s])
            assert singles[s].last_frame_kind == multi.last_frame_kind == bare.last_frame_kind
            what = f"call {c} stream {s}"
            _same(got[s], want, what)
            _same(got[s], raw[s], what)                                          # keypoints, score, box, ids: unchanged by smoothing
            assert raw[s].keypoints_smooth is None
            smooth_scenes.bits_equal(got[s].keypoints_smooth, want.keypoints_smooth, what + " keypoints_smooth")
            for k in ("id", "x", "dx", "t", "n"):
                smooth_scenes.bits_equal(multi.smooth_state[k][s].cpu().numpy(), singles[s].smooth_state[k].cpu().numpy(), what + " s_" + k)
            assert float(multi.smooth_state["now"][s].item()) == times[s]
            assert torch.equal(got[s].image, want.image), what                   # drawn from the smoothed poses, per stream
            moved += int((got[s].keypoints_smooth != got[s].keypoints).any())
    print("MEASURED results with filtered key points", "graphed" if graph else "eager", moved, "of", 6 * S3)
    assert moved >= 3 and int(multi.smooth_state["n"].max()) >= 2 and (len(multi._graphs) == 2) == graph


def test_renderer_and_encoder_give_an_image_and_a_file_per_stream(at_036, detector, dconv, renderer, images):
    est_r = TopDownPoseEstimator(detector, dconv, capacity=CAP, renderer=renderer, encoder=JpegEncoder(DEV))
    multi, singles = MultiStreamTracker(est_r, streams=S3), [PoseTracker(est_r) for _ in range(S3)]
    for c, frames in enumerate(_calls(images, ["aba", "aab"])):
        got = multi.update(frames)
        for s in range(S3):
            want = singles[s].update(frames[s])
            _same(got[s], want, f"call {c} stream {s}")
            assert torch.equal(got[s].image, want.image), (c, s)
            assert torch.equal(got[s].image, renderer.render(frames[s], got[s])), (c, s)
            assert isinstance(got[s].jpeg, bytes) and got[s].jpeg[:2] == b"\xff\xd8" and got[s].jpeg[-2:] == b"\xff\xd9", (c, s)
