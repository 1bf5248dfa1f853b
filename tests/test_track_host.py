"""Tracker, host side: the two entry points are declared, exported and bound without an ABI bump and refuse bad arguments before they
touch the GPU; PoseTracker's constructor refuses what it cannot run; and tests/track_ref.py (the CPU restatement the GPU tests compare
the kernels with) gives the answers written out here on hand-made cases."""
import ctypes
import os
import re

import numpy as np
import pytest

from simple_pose_amd import _lib
from simple_pose_amd.build import LIB_PATH
from tests import track_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sp_track_associate", "sp_track_boxes")
ONE = ctypes.c_void_p(256)          # a non-null pointer that is never dereferenced: every call below fails its argument check first


def test_new_symbols_declared_exported_bound_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(sp_\w+)\s*\(", hdr, flags=re.M))
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(handle, name), name
    assert re.search(r"#define SP_ABI_VERSION 36\b", hdr)
    assert _lib.ABI_VERSION == 36 and _lib.lib().sp_abi_version() == 36
    assert os.path.isfile(os.path.join(ROOT, "simple_pose_amd", "csrc", "track.hip"))


def test_bad_arguments_return_einval_without_touching_the_gpu():
    lib = _lib.lib()
    sig5 = (ctypes.c_double * 5)(*([0.05] * 5))

    def assoc(kps=ONE, keep=ONE, t_id=ONE, sim=ONE, out=ONE, rows=32, joints=17, sigmas=None, max_age=30, slots=32):
        return lib.sp_track_associate(kps, ONE, ONE, keep, ONE, ONE, rows, joints, sigmas, 0.5, max_age, slots, t_id, ONE, ONE, ONE, ONE, ONE, ONE,
                                      sim, out, None)

    for kw in ({"kps": None}, {"keep": None}, {"t_id": None}, {"sim": None}, {"out": None}):
        assert assoc(**kw) == -1 and b"null" in lib.sp_last_error(), kw
    for slots in (0, 257, -1):
        assert assoc(slots=slots) == -1 and b"slots" in lib.sp_last_error()
    for joints in (0, 65):
        assert assoc(joints=joints, sigmas=sig5) == -1 and b"joints" in lib.sp_last_error()
    assert assoc(joints=5) == -1 and b"sigmas" in lib.sp_last_error()
    assert assoc(rows=0) == -1 and b"rows" in lib.sp_last_error()
    assert assoc(max_age=-1) == -1 and b"max_age" in lib.sp_last_error()

    def boxes(t_id=ONE, det=ONE, counts=ONE, slots=32, joints=17, max_det=300, expand=1.25, w=640, h=480):
        return lib.sp_track_boxes(t_id, ONE, ONE, ONE, slots, joints, 0.2, expand, 0.0, w, h, max_det, det, counts, None)

    for kw in ({"t_id": None}, {"det": None}, {"counts": None}):
        assert boxes(**kw) == -1 and b"null" in lib.sp_last_error(), kw
    for slots in (0, 257):
        assert boxes(slots=slots) == -1 and b"slots" in lib.sp_last_error()
    for joints in (0, 65):
        assert boxes(joints=joints) == -1 and b"joints" in lib.sp_last_error()
    assert boxes(slots=32, max_det=31) == -1 and b"max_det" in lib.sp_last_error()
    assert boxes(w=0) == -1 and b"image" in lib.sp_last_error()
    assert boxes(expand=0.0) == -1 and b"box_expand" in lib.sp_last_error()


class _Model:
    training = False

    def hip_program(self, x):
        raise AssertionError("the constructor does not lower anything")


def _estimator(capacity=32):
    from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
    from simple_pose_amd.pipeline import TopDownPoseEstimator
    det = object.__new__(YOLOv5Detector)            # (a real one needs the GPU; the constructors only check the type)
    det.device = "cuda:0"
    return TopDownPoseEstimator(det, _Model(), capacity=capacity)


def test_tracker_constructor_refusals():
    import torch
    from simple_pose_amd.tracking import PoseTracker
    est = _estimator()
    with pytest.raises(TypeError, match="estimator"):
        PoseTracker(object())
    with pytest.raises(ValueError, match="256"):
        PoseTracker(est, slots=257)
    with pytest.raises(ValueError, match="256"):
        PoseTracker(_estimator(capacity=300))       # the default is the estimator's capacity
    for slots in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="slots"):
            PoseTracker(est, slots=slots)
    with pytest.raises(ValueError, match="capacity"):
        PoseTracker(est, slots=16)
    for kw, name in (({"match_thre": 0.0}, "match_thre"), ({"match_thre": 1.5}, "match_thre"), ({"match_thre": "x"}, "match_thre"),
                     ({"max_age": -1}, "max_age"), ({"max_age": 1.5}, "max_age"), ({"detect_every": 0}, "detect_every"),
                     ({"detect_every": 2.0}, "detect_every"), ({"box_expand": 0.0}, "box_expand"), ({"box_expand": float("inf")}, "box_expand"),
                     ({"sigmas": [0.1, -0.1]}, "sigmas"), ({"sigmas": []}, "sigmas")):
        with pytest.raises(ValueError, match=name):
            PoseTracker(est, **kw)
    trk = PoseTracker(est, detect_every=4)
    assert trk.slots == 32 and trk.match_thre == 0.5 and trk.max_age == 30 and trk.box_expand == 1.25 and trk.detect_every == 4
    trk.reset()                                     # before the first frame: nothing to forget, nothing touches the GPU
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        trk.update(torch.zeros((48, 64, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        trk.update(np.zeros((2, 48, 64, 3), np.uint8))


def test_pose_result_track_id_is_a_trailing_optional_field():
    from simple_pose_amd.pipeline import PoseResult
    k = np.zeros((2, 17, 3))
    r = PoseResult(k, np.array([0.5, 0.25]), np.zeros((2, 5), np.float32), 3)
    assert r.track_id is None and r.dropped == 3
    r = PoseResult(k, np.array([0.5, 0.25]), np.zeros((2, 5), np.float32), 0, np.array([4, 9], np.int32))
    assert r.track_id.tolist() == [4, 9] and "track_id" not in r.coco(1)[0]


# ---- track_ref on hand-made cases ---------------------------------------------------------------------------------------------------------
_SKELETON = np.array([[0, -60], [-5, -65], [5, -65], [-10, -60], [10, -60], [-25, -35], [25, -35], [-35, 0], [35, 0], [-40, 30], [40, 30],
                      [-15, 40], [15, 40], [-17, 90], [17, 90], [-18, 140], [18, 140]], np.float64)
AREA = 150.0 * 260.0


def pose(cx, cy):
    return np.concatenate([_SKELETON + (cx, cy), np.ones((17, 1))], 1)


def frame(state, poses, **kw):
    poses = np.stack(poses) if len(poses) else np.zeros((0, 17, 3))
    n = poses.shape[0]
    ids, S = track_ref.associate(state, poses, np.full(n, AREA), np.linspace(0.9, 0.5, n).astype(np.float32), **kw)
    return ids.tolist(), S


def test_ref_two_persons_swapping_places_in_the_list():
    st = track_ref.TrackState(4, 17)
    assert frame(st, [pose(100, 200), pose(400, 200)])[0] == [1, 2]
    assert st.id.tolist() == [1, 2, 0, 0] and st.age.tolist() == [1, 1, 0, 0] and st.next_id == 3
    ids, S = frame(st, [pose(398, 203), pose(103, 199)])                       # the same two, a few pixels on, listed the other way round
    assert ids == [2, 1] and S[0, 1] > 0.95 > 0.05 > S[0, 0] and S[1, 0] > 0.95 > 0.05 > S[1, 1]    # ~3.6 px on a 150 x 260 person: 0.98; 300 px: ~0
    assert st.id.tolist() == [1, 2, 0, 0] and st.age.tolist() == [2, 2, 0, 0] and st.miss.tolist() == [0, 0, 0, 0] and st.next_id == 3
    np.testing.assert_array_equal(st.kps[0], pose(103, 199))
    assert st.conf.tolist() == [np.float32(0.5), np.float32(0.9), 0, 0]


def test_ref_exact_ties_go_to_the_lower_slot_then_the_lower_pose():
    st = track_ref.TrackState(4, 17)
    assert frame(st, [pose(100, 200)])[0] == [1]
    ids, S = frame(st, [pose(101, 200), pose(101, 200)])                       # a duplicated pose: S[0,0] == S[0,1]
    assert S[0, 0] == S[0, 1] and ids == [1, 2]                                # the lower pose index continues the track, the other is new
    assert st.id.tolist() == [1, 2, 0, 0] and st.age.tolist() == [2, 1, 0, 0]
    ids, S = frame(st, [pose(101, 200)])                                       # two identical tracks, one pose: the lower slot takes it
    assert S[0, 0] == S[1, 0] == 1.0 and ids == [1]
    assert st.miss.tolist() == [0, 1, 0, 0] and st.age.tolist() == [3, 1, 0, 0]


def test_ref_similarity_equal_to_the_threshold_matches():
    st = track_ref.TrackState(2, 17)
    frame(st, [pose(100, 200)])
    ids, S = frame(st, [pose(100, 200)], match_thre=1.0)                       # a pose against itself: J / float32(J + 1e-12) = 1.0 exactly
    assert S[0, 0] == np.float64(17) / np.float64(np.float32(17) + np.float32(1e-12)) == 1.0 and ids == [1]
    ids, S = frame(st, [pose(100.5, 200)], match_thre=1.0)
    assert S[0, 0] < 1.0 and ids == [2] and st.miss.tolist() == [1, 0]


def test_ref_a_nan_pose_never_matches():
    st = track_ref.TrackState(3, 17)
    frame(st, [pose(100, 200)])
    bad = pose(100, 200)
    bad[3, 0] = np.nan
    ids, S = frame(st, [bad])
    assert np.isnan(S[0, 0]) and ids == [2] and st.miss.tolist() == [1, 0, 0]
    ids, S = frame(st, [pose(100, 200)])                                       # the clean track continues; the NaN track matches nothing
    assert S[0, 0] == 1.0 and np.isnan(S[1, 0]) and ids == [1] and st.miss.tolist() == [0, 1, 0]


def test_ref_eviction_takes_the_largest_miss_then_the_lowest_slot():
    st = track_ref.TrackState(3, 17)
    a, b, c = pose(100, 200), pose(400, 200), pose(700, 200)
    assert frame(st, [a, b, c])[0] == [1, 2, 3]
    assert frame(st, [a, b])[0] == [1, 2] and st.miss.tolist() == [0, 0, 1]
    assert frame(st, [b])[0] == [2] and st.miss.tolist() == [1, 0, 2]
    x, y = pose(100, 900), pose(700, 900)
    assert frame(st, [x, b, y])[0] == [4, 2, 5]                                # no free slot: x takes slot 2 (miss 2), y slot 0 (miss 1)
    assert st.id.tolist() == [5, 2, 4] and st.age.tolist() == [1, 4, 1] and st.miss.tolist() == [0, 0, 0] and st.next_id == 6
    st = track_ref.TrackState(3, 17)
    frame(st, [a, b, c])
    assert frame(st, [x, y, pose(400, 900)])[0] == [4, 5, 6] and st.id.tolist() == [4, 5, 6]      # equal misses: slots in order


def test_ref_ids_are_never_reused_after_max_age():
    st = track_ref.TrackState(2, 17)
    a = pose(100, 200)
    assert frame(st, [a], max_age=1)[0] == [1]
    assert frame(st, [], max_age=1)[0] == [] and st.id.tolist() == [1, 0] and st.miss.tolist() == [1, 0]
    assert frame(st, [a], max_age=1)[0] == [1] and st.age.tolist() == [2, 0]    # back inside max_age: the same person
    frame(st, [], max_age=1)
    assert frame(st, [], max_age=1)[0] == [] and st.id.tolist() == [0, 0] and st.age.tolist() == [0, 0] and st.miss.tolist() == [0, 0]
    assert frame(st, [a], max_age=1)[0] == [2] and st.id.tolist() == [2, 0] and st.next_id == 3      # after it: a new identity


def test_ref_boxes_by_hand():
    st = track_ref.TrackState(4, 17)
    k = np.zeros((17, 3))
    k[:, 0], k[:, 1], k[:, 2] = 10, 30, 1.0
    k[5] = (20, 50, 1.0)
    k[6] = (5000, -70, 0.1)                                                     # below in_vis_thre: not part of the box
    st.id[:3], st.miss[:3], st.conf[:3] = (7, 8, 9), (0, 1, 0), (0.75, 0.5, 0.25)
    st.kps[0] = st.kps[1] = k
    st.kps[2] = 0.0
    st.kps[2, :, :2] = (630, 100)                                               # nothing visible, every joint on one point near the edge
    got = track_ref.boxes(st, 0.2, 1.25, 640, 480)
    assert got.dtype == np.float32 and got.tolist() == [[8.75, 27.5, 21.25, 52.5, 0.75, 0.0], [629.5, 99.5, 630.5, 100.5, 0.25, 0.0]]
    st.kps[2, :, :2] = (700, -20)                                               # outside the image: clipped to its border
    assert track_ref.boxes(st, 0.2, 1.25, 640, 480)[1].tolist() == [640.0, 0.0, 640.0, 0.0, 0.25, 0.0]
    st.id[:] = 0
    assert track_ref.boxes(st, 0.2, 1.25, 640, 480).shape == (0, 6)


def test_ref_exp_is_a_faithful_exp():
    """track_ref.exp_f64 states an algorithm so that it can be met bit for bit; here it is held to what makes it an exp: within 1 ulp of the
    true value (the accuracy the device math library documents for its double exp; decimal at 50 digits is the truth) over the range the
    similarity uses, x <= 0 down to where the result is 0, and exact at the ends."""
    import decimal
    from fractions import Fraction
    import math
    assert track_ref._fma(0.1, 10.0, -1.0) == 2.0 ** -54 != 0.1 * 10.0 - 1.0   # one rounding, not two
    assert track_ref.exp_f64(0.0) == 1.0 == track_ref.exp_f64(-0.0)
    assert track_ref.exp_f64(-np.inf) == 0.0 == track_ref.exp_f64(-1075.5) and track_ref.exp_f64(np.inf) == np.inf == track_ref.exp_f64(800.0)
    assert np.isnan(track_ref.exp_f64(np.nan))
    rng = np.random.default_rng(5)
    xs = np.concatenate([-rng.uniform(0, 1, 100), -rng.uniform(0, 750, 200), -10.0 ** rng.uniform(-30, 0, 50), -np.arange(0, 40) * np.log(2) / 2,
                         rng.uniform(0, 700, 50)])
    worst = 0.0
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        for x in xs.tolist():
            got, true = track_ref.exp_f64(x), Fraction(decimal.Decimal(x).exp())
            worst = max(worst, float(abs(Fraction(got) - true) / Fraction(math.ulp(got))))
    print(f"MEASURED exp_f64 worst error {worst:.3f} ulp over {xs.size} points")
    assert worst <= 1.0
