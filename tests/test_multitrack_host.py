"""Several streams in one call, host side: the three sp_track_*_images entries are declared, exported and bound with matching arity
without an ABI bump and refuse bad arguments before they touch the GPU, naming themselves; MultiStreamTracker refuses what it cannot run;
and the frame-kind rule (tests/multitrack_ref.py) reduces to PoseTracker's with one stream."""
import ctypes
import os
import re

import numpy as np
import pytest

from simple_pose_amd import _lib
from simple_pose_amd.build import LIB_PATH
from tests import multitrack_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sp_track_associate_images", "sp_track_boxes_images", "sp_track_smooth_images")
ONE = ctypes.c_void_p(256)          # a non-null pointer that is never dereferenced: every call below fails its argument check first


def _declared_arity(hdr, name):
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr, flags=re.M | re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_new_symbols_declared_exported_and_bound_with_matching_arity():
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert hasattr(handle, name), name
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == _declared_arity(hdr, name), name
        single = name[:-len("_images")]
        assert len(args) == len(_lib.SYMBOLS[single][1]) + 1 == _declared_arity(hdr, single) + 1      # the single entry's, plus `images`
    assert _lib.lib().sp_abi_version() == _lib.ABI_VERSION and re.search(r"#define SP_ABI_VERSION %d\b" % _lib.ABI_VERSION, hdr)


def test_bad_arguments_are_refused_by_name_without_touching_the_gpu():
    lib = _lib.lib()
    sig5 = (ctypes.c_double * 5)(*([0.05] * 5))

    def refused(rc, *words):
        msg = lib.sp_last_error()
        return rc != 0 and all(w in msg for w in words)

    def assoc(kps=ONE, keep=ONE, t_id=ONE, next_id=ONE, sim=ONE, out=ONE, images=3, rows=32, joints=17, sigmas=None, max_age=30, slots=32):
        return lib.sp_track_associate_images(kps, ONE, ONE, keep, ONE, ONE, images, rows, joints, sigmas, 0.5, max_age, slots, t_id, ONE, ONE, ONE,
                                             ONE, ONE, next_id, sim, out, None)

    def boxes(t_id=ONE, det=ONE, counts=ONE, images=3, slots=32, joints=17, max_det=300, expand=1.25, w=640, h=480):
        return lib.sp_track_boxes_images(t_id, ONE, ONE, ONE, images, slots, joints, 0.2, expand, 0.0, w, h, max_det, det, counts, None)

    def smooth(kps=ONE, now=ONE, s_n=ONE, out=ONE, images=3, rows=32, joints=17, slots=32, min_cutoff=1.0):
        return lib.sp_track_smooth_images(kps, ONE, ONE, ONE, ONE, ONE, images, rows, joints, ONE, slots, now, min_cutoff, 0.5, 1.0, 0.5, 0.2, ONE,
                                          ONE, ONE, ONE, s_n, out, None)

    for fn, name, nulls in ((assoc, b"sp_track_associate_images", ({"kps": None}, {"keep": None}, {"t_id": None}, {"next_id": None},
                                                                  {"sim": None}, {"out": None})),
                            (boxes, b"sp_track_boxes_images", ({"t_id": None}, {"det": None}, {"counts": None})),
                            (smooth, b"sp_track_smooth_images", ({"kps": None}, {"now": None}, {"s_n": None}, {"out": None}))):
        for images in (0, 257, -1):
            assert refused(fn(images=images), name + b":", b"images"), (name, images)
        for slots in (0, 257):
            assert refused(fn(slots=slots), name + b":", b"slots"), (name, slots)
        for joints in (0, 65):
            assert refused(fn(joints=joints, **({"sigmas": sig5} if fn is assoc else {})), name + b":", b"joints"), (name, joints)
        for kw in nulls:
            assert refused(fn(**kw), name + b":", b"null"), (name, kw)
    assert refused(assoc(joints=5), b"sp_track_associate_images:", b"sigmas")
    assert refused(assoc(rows=0), b"sp_track_associate_images:", b"rows")
    assert refused(assoc(max_age=-1), b"sp_track_associate_images:", b"max_age")
    assert refused(boxes(slots=32, max_det=31), b"sp_track_boxes_images:", b"max_det")
    assert refused(boxes(w=0), b"sp_track_boxes_images:", b"image")
    assert refused(boxes(expand=0.0), b"sp_track_boxes_images:", b"box_expand")
    assert refused(smooth(rows=0), b"sp_track_smooth_images:", b"rows")
    assert refused(smooth(min_cutoff=0.0), b"sp_track_smooth_images:", b"min_cutoff")
    # and the single-image entries still name themselves
    assert lib.sp_track_boxes(ONE, ONE, ONE, ONE, 0, 17, 0.2, 1.25, 0.0, 640, 480, 300, ONE, ONE, None) != 0
    assert lib.sp_last_error().startswith(b"sp_track_boxes: slots")


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


def test_multi_stream_tracker_refusals_come_before_any_launch():
    import torch
    from simple_pose_amd.tracking import MultiStreamTracker, OneEuro
    est = _estimator()
    with pytest.raises(TypeError, match="estimator"):
        MultiStreamTracker(object(), streams=2)
    for streams in (0, 257, -1, 2.0, True):
        with pytest.raises(ValueError, match="streams"):
            MultiStreamTracker(est, streams=streams)
    with pytest.raises(ValueError, match="capacity 300 exceeds .* 256"):
        MultiStreamTracker(_estimator(capacity=300), streams=2)
    with pytest.raises(ValueError, match="256"):
        MultiStreamTracker(est, streams=2, slots=257)
    with pytest.raises(ValueError, match="capacity"):
        MultiStreamTracker(est, streams=2, slots=16)                             # per stream, and still not below the shared capacity
    for kw, name in (({"match_thre": 0.0}, "match_thre"), ({"max_age": -1}, "max_age"), ({"detect_every": 0}, "detect_every"),
                     ({"box_expand": 0.0}, "box_expand"), ({"sigmas": []}, "sigmas")):
        with pytest.raises(ValueError, match=name):
            MultiStreamTracker(est, streams=2, **kw)
    with pytest.raises(TypeError, match="smooth"):
        MultiStreamTracker(est, streams=2, smooth=object())
    trk = MultiStreamTracker(est, streams=3, detect_every=4)
    assert trk.streams == 3 and trk.slots == 32 and trk.detect_every == 4 and trk.last_frame_kind is None
    trk.reset()
    trk.reset(stream=1)                             # before the first call: nothing to forget, nothing touches the GPU
    assert trk.tracks(2)["id"].size == 0
    for bad in (3, -1, None, 1.0):
        with pytest.raises(ValueError, match="stream"):
            trk.tracks(bad)
    with pytest.raises(ValueError, match="stream"):
        trk.reset(stream=3)
    img = np.zeros((48, 64, 3), np.uint8)
    with pytest.raises(ValueError, match="3 streams"):
        trk.update([img, img])                      # wrong frame count
    with pytest.raises(ValueError, match="3 streams"):
        trk.update(np.zeros((2, 48, 64, 3), np.uint8))
    with pytest.raises(ValueError, match="one size"):
        trk.update([img, img, np.zeros((48, 66, 3), np.uint8)])
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        trk.update(torch.zeros((3, 48, 64, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="does not smooth"):
        trk.update([img, img, img], timestamps=[0.0, 0.0, 0.0])
    smoothing = MultiStreamTracker(est, streams=3, smooth=OneEuro())
    for bad in ([0.0, 1.0], 0.5, [0.0, float("nan"), 1.0], [0.0, float("inf"), 1.0], [0.0, "x", 1.0]):
        with pytest.raises(ValueError, match="timestamps"):
            smoothing.update([img, img, img], timestamps=bad)


def test_golden_image_has_36_person_rows_above_the_class_tests_threshold(golden):
    """What tests/test_gpu_multitrack.py sizes its shared capacity from: 36 person rows of the golden detector output on image `a` score
    above 0.36 (tests/test_gpu_pipeline.py counts 37 candidates on the device; the sizing takes 37 per stream)."""
    d = golden("g14_detector.npz")["sp_a_dets"]
    assert int(((d[:, 5] == 0) & (d[:, 4] > 0.36)).sum()) == 36 <= 37 and 3 * 37 <= 128


@pytest.mark.parametrize("detect_every", [1, 2, 3, 5])
def test_frame_kind_rule_with_one_stream_is_the_single_trackers(detect_every):
    rng = np.random.default_rng(detect_every)
    multi, single = multitrack_ref.FrameKinds(1, detect_every), multitrack_ref.SingleKinds(detect_every)
    kinds = []
    for call in range(400):
        if rng.random() < 0.03:
            multi.reset(None if rng.random() < 0.5 else 0)
            single.reset()
        a, b = multi.next(), single.next()
        assert a == b, call
        n = int(rng.integers(0, 4)) * int(rng.random() < 0.8)                    # person counts, a fifth of them zero
        multi.done(a, [n])
        single.done(b, n)
        kinds.append(a)
    assert kinds[0] and (False in kinds) == (detect_every > 1)


def test_frame_kind_rule_with_several_streams():
    k = multitrack_ref.FrameKinds(3, 3)
    seq = []
    for counts in ([2, 0, 2], [2, 0, 2], [0, 1, 0], [2, 2, 2], [0, 0, 0], [1, 1, 1], [1, 1, 1]):
        d = k.next()
        seq.append(k.name(d))
        k.done(d, counts)
    # first; propagated although stream 1 is empty; propagated; every third; propagated; after the all-empty call; propagated
    assert seq == ["detector", "propagated", "propagated", "detector", "propagated", "detector", "propagated"]
    k.reset(stream=1)
    assert k.next()


@pytest.mark.parametrize("detect_every", [1, 2, 3, 5])
def test_the_trackers_own_frame_kind_methods_with_one_stream(detect_every):
    """The rule as the trackers run it (MultiStreamTracker._next_is_detector / _ran, host counters only), for a one-stream
    MultiStreamTracker and a PoseTracker, against both restatements; the resets and person counts of the test above."""
    from simple_pose_amd.tracking import MultiStreamTracker, PoseTracker
    rng = np.random.default_rng(detect_every)
    est = _estimator()
    multi, single = MultiStreamTracker(est, streams=1, detect_every=detect_every), PoseTracker(est, detect_every=detect_every)
    ref_multi, ref_single = multitrack_ref.FrameKinds(1, detect_every), multitrack_ref.SingleKinds(detect_every)
    kinds = []
    for call in range(400):
        if rng.random() < 0.03:
            stream = None if rng.random() < 0.5 else 0
            multi.reset(stream)
            ref_multi.reset(stream)
            single.reset()
            ref_single.reset()
        want = ref_multi.next()
        assert ref_single.next() == want, call
        assert multi._next_is_detector() is want and single._next_is_detector() is want, call
        n = int(rng.integers(0, 4)) * int(rng.random() < 0.8)                    # person counts, a fifth of them zero
        multi._ran(want, [n])
        single._ran(want, [n])
        ref_multi.done(want, [n])
        ref_single.done(want, n)
        assert multi.last_frame_kind == single.last_frame_kind == multitrack_ref.FrameKinds.name(want), call
        kinds.append(want)
    assert kinds[0] and (False in kinds) == (detect_every > 1)
    assert not multi.state and not multi.smooth_state and not single.state and not single.smooth_state     # nothing was allocated


def test_the_trackers_own_frame_kind_methods_with_three_streams():
    from simple_pose_amd.tracking import MultiStreamTracker
    trk, k = MultiStreamTracker(_estimator(), streams=3, detect_every=3), multitrack_ref.FrameKinds(3, 3)
    seq = []
    for counts in ([2, 0, 2], [2, 0, 2], [0, 1, 0], [2, 2, 2], [0, 0, 0], [1, 1, 1], [1, 1, 1]):
        d = k.next()
        assert trk._next_is_detector() is d
        trk._ran(d, counts)
        k.done(d, counts)
        seq.append(trk.last_frame_kind)
    assert seq == ["detector", "propagated", "propagated", "detector", "propagated", "detector", "propagated"]
    assert not k.next() and not trk._next_is_detector()                          # (two of three calls since the detector: propagated, but for ...)
    trk.reset(stream=1)
    k.reset(stream=1)
    assert k.next() and trk._next_is_detector() is True and not trk.state
