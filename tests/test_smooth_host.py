"""Key-point smoothing, host side: sp_track_smooth is declared, exported and bound without an ABI bump and refuses bad arguments before
it touches the GPU; OneEuro, PoseTracker(smooth=...) and update(timestamp=...) refuse what they cannot run; PoseResult takes the new trailing
field; and tests/smooth_ref.py (the CPU restatement the GPU test compares the kernel with) gives the answers worked out by hand here."""
import ctypes
import os
import re

import numpy as np
import pytest

from simple_pose_amd import _lib
from simple_pose_amd.build import LIB_PATH
from tests import smooth_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = ctypes.c_void_p(256)          # a non-null pointer that is never dereferenced: every call below fails its argument check first


def test_new_symbol_declared_exported_bound_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(sp_\w+)\s*\(", hdr, flags=re.M))
    handle = ctypes.CDLL(LIB_PATH)
    assert "sp_track_smooth" in declared and "sp_track_smooth" in _lib.SYMBOLS and hasattr(handle, "sp_track_smooth")
    assert re.search(r"#define SP_ABI_VERSION 36\b", hdr)
    assert _lib.ABI_VERSION == 36 and _lib.lib().sp_abi_version() == 36
    assert os.path.isfile(os.path.join(ROOT, "simple_pose_amd", "csrc", "sp_smooth.h"))


def test_bad_arguments_return_einval_without_touching_the_gpu():
    lib = _lib.lib()
    names = ("kps", "box", "track_id", "keep", "keep_count", "seg", "t_id", "now", "s_id", "s_x", "s_dx", "s_t", "s_n", "out")

    def call(rows=32, joints=17, slots=32, min_cutoff=1.0, beta=0.5, d_cutoff=1.0, max_gap=0.5, vis=0.2, **ptrs):
        p = {k: ptrs.get(k, ONE) for k in names}
        return lib.sp_track_smooth(p["kps"], p["box"], p["track_id"], p["keep"], p["keep_count"], p["seg"], rows, joints, p["t_id"], slots,
                                   p["now"], min_cutoff, beta, d_cutoff, max_gap, vis, p["s_id"], p["s_x"], p["s_dx"], p["s_t"], p["s_n"],
                                   p["out"], None)

    for k in names:
        assert call(**{k: None}) == -1 and b"null" in lib.sp_last_error(), k
    for slots in (0, 257, -1):
        assert call(slots=slots) == -1 and b"slots" in lib.sp_last_error()
    for joints in (0, 65):
        assert call(joints=joints) == -1 and b"joints" in lib.sp_last_error()
    for rows in (0, -3):
        assert call(rows=rows) == -1 and b"rows" in lib.sp_last_error()
    nan, inf = float("nan"), float("inf")
    for name, bad in (("min_cutoff", (0.0, -1.0, nan, inf)), ("beta", (-0.5, nan, inf)), ("d_cutoff", (0.0, -1.0, nan, inf)),
                      ("max_gap", (0.0, -0.1, nan, inf)), ("vis", (nan, inf))):
        for v in bad:
            assert call(**{name: v}) == -1 and (b"in_vis_thre" if name == "vis" else name.encode()) in lib.sp_last_error(), (name, v)


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


def test_one_euro_and_tracker_refusals():
    from simple_pose_amd.tracking import OneEuro, PoseTracker
    f = OneEuro()
    assert (f.min_cutoff, f.beta, f.d_cutoff, f.max_gap, f.fps) == (1.0, 0.5, 1.0, 0.5, 30.0)
    assert OneEuro(beta=0).beta == 0.0 and OneEuro(2, 1, 3, 4, 25).key() == (2.0, 1.0, 3.0, 4.0)
    assert OneEuro(min_cutoff=2.0).key() != f.key()
    nan, inf = float("nan"), float("inf")
    for kw, name in (({"min_cutoff": 0.0}, "min_cutoff"), ({"min_cutoff": nan}, "min_cutoff"), ({"min_cutoff": "1"}, "min_cutoff"),
                     ({"beta": -0.1}, "beta"), ({"beta": inf}, "beta"), ({"beta": True}, "beta"), ({"d_cutoff": 0}, "d_cutoff"),
                     ({"d_cutoff": inf}, "d_cutoff"), ({"max_gap": 0.0}, "max_gap"), ({"max_gap": nan}, "max_gap"), ({"fps": 0}, "fps"),
                     ({"fps": -30.0}, "fps"), ({"fps": None}, "fps")):
        with pytest.raises(ValueError, match=name):
            OneEuro(**kw)
    est = _estimator()
    for bad in (1.0, "euro", {"beta": 1}, OneEuro):
        with pytest.raises(TypeError, match="smooth"):
            PoseTracker(est, smooth=bad)
    plain, smoothing = PoseTracker(est), PoseTracker(est, smooth=f)
    assert plain.smooth is None and not plain.smooth_state and smoothing.smooth is f
    img = np.zeros((48, 64, 3), np.uint8)
    with pytest.raises(ValueError, match="timestamp"):
        plain.update(img, timestamp=0.5)            # refused before anything is lowered or launched
    for bad in (nan, inf, "0.5", True):
        with pytest.raises(ValueError, match="timestamp"):
            smoothing.update(img, timestamp=bad)
    smoothing.reset()                               # before the first frame: nothing to forget, nothing touches the GPU


def test_pose_result_keypoints_smooth_is_a_trailing_optional_field():
    import dataclasses
    from simple_pose_amd.pipeline import PoseResult
    assert [f.name for f in dataclasses.fields(PoseResult)][-2:] == ["jpeg", "keypoints_smooth"]
    k = np.zeros((2, 17, 3))
    r = PoseResult(k, np.array([0.5, 0.25]), np.zeros((2, 5), np.float32), 3, np.array([4, 9], np.int32), None, b"x")
    assert r.keypoints_smooth is None and r.jpeg == b"x"
    r = PoseResult(k, np.array([0.5, 0.25]), np.zeros((2, 5), np.float32), 0, np.array([4, 9], np.int32), None, None, k + 1.0)
    assert r.keypoints_smooth[1, 3, 0] == 1.0
    assert "keypoints_smooth" not in r.coco(1)[0] and r.coco(1)[0]["keypoints"] == [0.0] * 51


# ---- smooth_ref on cases worked by hand -----------------------------------------------------------------------------------------------------
BOX = np.array([[100, 100, 200, 300, 0.9]], np.float32)          # size = max(100, 200) = 200


def step(st, kps, now, p, tid=1, t_id=(1,), box=BOX):
    """One row, kept, with track id `tid`."""
    kps = np.asarray(kps, np.float64).reshape(1, -1, 3)
    return smooth_ref.smooth(st, kps, box, np.array([tid], np.int32), np.array([0], np.int32), 1, [0, 1], np.array(t_id, np.int32), now, p)[0]


def test_ref_box_size():
    assert smooth_ref.box_size(BOX[0]) == 200.0
    assert smooth_ref.box_size([10, 10, 50, 20, 1]) == 40.0
    assert smooth_ref.box_size([10, 10, 10, 10, 1]) == 1.0 and smooth_ref.box_size([10, 10, 5, 7, 1]) == 1.0       # zero and negative extent
    assert smooth_ref.box_size([np.nan, 0, 5, 7, 1]) == 7.0 and smooth_ref.box_size([0, np.nan, 5, 7, 1]) == 1.0   # w > h ? w : h, then > 0
    assert smooth_ref.box_size([0.1, 0, 0.4, 0, 1]) == np.float64(np.float32(0.4) - np.float32(0.1))                 # the subtraction is float32's


def test_ref_a_constant_pose_comes_out_exactly_unchanged():
    rng = np.random.default_rng(1)
    pose = np.concatenate([rng.uniform(0, 640, (17, 2)), rng.uniform(0.3, 1, (17, 1))], 1)
    st, p = smooth_ref.SmoothState(1, 17), smooth_ref.params()
    for f in range(10):
        out = step(st, pose, f / 30.0, p)
        np.testing.assert_array_equal(out, pose)                                 # exactly: a sample equal to x^ leaves x^ as it is
    assert (st.n == 10).all() and (st.dx == 0).all()


def test_ref_beta_zero_is_the_fixed_alpha_recursion():
    """beta = 0, min_cutoff = 1 Hz, Te = 0.25 s: r = 2 pi / 4, alpha = r / (r + 1) = 0.61101547..., the same at every step.  Three steps of
    x^ = a x + (1 - a) x^ on the samples 8, 8, -4 after a start at 0, bit for bit in the stated form and to 1e-12 against the decimal values
    worked out by hand from alpha (8 a;  8 a (2 - a);  -4 a + (1 - a) x^2)."""
    p = smooth_ref.params(min_cutoff=1.0, beta=0.0, d_cutoff=1.0, max_gap=10.0)
    Te = np.float64(0.25)
    r = (np.float64(6.283185307179586) * np.float64(1.0)) * Te                   # 1.5707963267948966
    a = r / (r + 1.0)
    assert r == 1.5707963267948966 and abs(a - 0.6110154703516573) < 1e-15
    st = smooth_ref.SmoothState(1, 1)
    xs = [0.0, 8.0, 8.0, -4.0]
    outs = [step(st, [[x, 2 * x, 0.9]], f * 0.25, p)[0] for f, x in enumerate(xs)]
    h1 = a * 8.0 + (1.0 - a) * 0.0
    h2 = a * 8.0 + (1.0 - a) * h1
    h3 = a * -4.0 + (1.0 - a) * h2
    assert outs[0].tolist() == [0.0, 0.0, 0.9]                                   # the first sample is the raw one
    assert [o[0] for o in outs[1:]] == [h1, h2, h3]
    # the same three values in closed form with alpha = pi / (pi + 2), worked out in 40-digit decimals: 8a, 8a(2 - a), -4a + (1 - a) 8a(2 - a)
    assert abs(h1 - 4.888123762813258315) < 1e-12 and abs(h2 - 6.789528285554060726) < 1e-12 and abs(h3 - 0.196959585283735830) < 1e-12
    assert all(o[2] == 0.9 for o in outs) and st.n[0, 0] == 4 and st.t[0, 0] == 0.75


def test_ref_a_step_is_approached_monotonically_without_overshoot():
    st, p = smooth_ref.SmoothState(1, 1), smooth_ref.params()
    step(st, [[100.0, 50.0, 0.9]], 0.0, p)
    prev = np.array([100.0, 50.0])
    for f in range(1, 40):
        out = step(st, [[160.0, 20.0, 0.9]], f / 30.0, p)[0]
        assert prev[0] < out[0] <= 160.0 and 20.0 <= out[1] < prev[1], f
        prev = out[:2]
    assert abs(prev[0] - 160.0) < 1.0 and abs(prev[1] - 20.0) < 1.0             # and it gets there


def test_ref_a_gap_above_max_gap_restarts_from_the_raw_sample():
    st, p = smooth_ref.SmoothState(1, 1), smooth_ref.params(max_gap=0.5)
    step(st, [[10.0, 10.0, 0.9]], 0.0, p)
    inside = step(st, [[20.0, 10.0, 0.9]], 0.5, p)[0]                            # a gap of exactly max_gap still updates
    assert 10.0 < inside[0] < 20.0 and st.n[0, 0] == 2
    out = step(st, [[50.0, 70.0, 0.9]], 1.25, p)[0]
    assert out.tolist() == [50.0, 70.0, 0.9] and st.n[0, 0] == 1 and st.t[0, 0] == 1.25 and (st.dx == 0).all()
    assert st.x[0, 0].tolist() == [50.0, 70.0] and st.events["restart_gap"] == 1
    for now in (1.25, 1.0):                                                      # a repeated time and one that goes backwards restart too
        out = step(st, [[60.0, 70.0, 0.9]], now, p)[0]
        assert out.tolist() == [60.0, 70.0, 0.9] and st.n[0, 0] == 1 and st.t[0, 0] == now
    assert st.events["restart_time"] == 2


def test_ref_a_slot_handed_to_a_new_id_restarts():
    st, p = smooth_ref.SmoothState(2, 2), smooth_ref.params()
    pose = [[10.0, 10.0, 0.9], [30.0, 30.0, 0.1]]                                # joint 1 is never usable
    step(st, pose, 0.0, p, tid=5, t_id=(0, 5))
    step(st, pose, 0.1, p, tid=5, t_id=(0, 5))
    assert st.id.tolist() == [0, 5] and st.n.tolist() == [[0, 0], [2, 0]]
    out = step(st, [[90.0, 90.0, 0.9], [30.0, 30.0, 0.1]], 0.2, p, tid=7, t_id=(0, 7))       # the tracker gave slot 1 to id 7
    assert out[0].tolist() == [90.0, 90.0, 0.9] and st.id.tolist() == [0, 7] and st.n.tolist() == [[0, 0], [1, 0]]
    assert st.events["takeover"] == 2                                            # (the first use of the slot counts as one)
    # an id the slot table does not hold, an id of 0, and a row the image did not keep pass through and touch nothing
    before = st.copy()
    assert step(st, pose, 0.3, p, tid=9, t_id=(0, 7))[0].tolist() == pose[0]
    assert step(st, pose, 0.3, p, tid=0, t_id=(0, 7))[0].tolist() == pose[0]
    kps = np.asarray(pose, np.float64).reshape(1, 2, 3)
    out = smooth_ref.smooth(st, kps, BOX, np.array([7], np.int32), np.array([0], np.int32), 0, [0, 1], np.array([0, 7], np.int32), 0.3, p)
    np.testing.assert_array_equal(out, kps)
    for k in ("id", "x", "dx", "t", "n"):
        np.testing.assert_array_equal(getattr(st, k), getattr(before, k))


def test_ref_unusable_joints_pass_through_and_do_not_advance():
    st, p = smooth_ref.SmoothState(1, 4), smooth_ref.params(in_vis_thre=0.2)
    good = [[10.0, 10.0, 0.9]] * 4
    step(st, good, 0.0, p)
    step(st, good, 0.1, p)
    bad = [[20.0, 20.0, 0.2], [np.nan, 20.0, 0.9], [20.0, np.inf, 0.9], [20.0, 20.0, np.nan]]    # at the threshold, NaN x, infinite y, NaN c
    before = st.copy()
    out = step(st, bad, 0.2, p)
    np.testing.assert_array_equal(out, np.asarray(bad))                           # (NaN-aware) the raw samples
    for k in ("x", "dx", "t", "n"):
        np.testing.assert_array_equal(getattr(st, k), getattr(before, k))
    assert (st.t == 0.1).all() and st.events["pass"] == 4
    out = step(st, [[20.0, 20.0, 0.2000001]] * 4, 0.3, p)                        # just above: filtered, with Te = 0.2 (from the last ACCEPTED one)
    assert (out[:, 0] > 10.0).all() and (out[:, 0] < 20.0).all() and (st.t == 0.3).all() and (st.n == 3).all()


def test_ref_jitter_on_a_static_pose_is_reduced_for_every_joint():
    """A static 17-joint pose plus N(0, 1 px) noise (seed 2012) over 60 frames at 30 fps, on a 200 px person: the filtered RMS deviation from
    the true pose is below the raw one for every joint."""
    rng = np.random.default_rng(2012)
    true = rng.uniform(150, 450, (17, 2))
    st, p = smooth_ref.SmoothState(1, 17), smooth_ref.params()
    raw_err, out_err = [], []
    for f in range(60):
        noisy = true + rng.normal(0.0, 1.0, (17, 2))
        out = step(st, np.concatenate([noisy, np.full((17, 1), 0.8)], 1), f / 30.0, p)
        raw_err.append(noisy - true)
        out_err.append(out[:, :2] - true)
    rms = lambda e: np.sqrt((np.asarray(e) ** 2).sum(2).mean(0))
    raw, out = rms(raw_err), rms(out_err)
    print("MEASURED jitter RMS px: raw", raw.round(3).tolist(), "filtered", out.round(3).tolist())
    assert (out < raw).all()
