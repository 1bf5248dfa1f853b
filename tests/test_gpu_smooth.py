"""Key-point smoothing on the MI355X: sp_track_smooth through the C ABI against tests/smooth_ref.py, frame by frame over the sequences of
tests/smooth_scenes.py (the ones the header's CPU build filters under the sanitizers), and PoseTracker(smooth=OneEuro(...)) end to end
against an identical tracker without smoothing plus smooth_ref applied to its results.  Every double is compared bit for bit (NaN-aware):
the filter is fp64 + - * / with contraction off, which the device reproduces."""
import dataclasses

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib, synth
from simple_pose_amd.detector.nets.yolov5 import YOLOv5
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
from simple_pose_amd.pipeline import TopDownPoseEstimator
from simple_pose_amd.tracking import OneEuro, PoseTracker
from simple_pose_amd.visualize import PoseRenderer
from tests import smooth_ref, smooth_scenes
from tests.detector_ref import detector_state_dict

pytestmark = pytest.mark.gpu
G = "g14_detector.npz"
DEV = "cuda:0"
P = _lib.ptr


# ---- a. the kernel through the C ABI --------------------------------------------------------------------------------------------------------
_RUNS = {}


def _run(case):
    """One sequence through the kernel, frame by frame -> per frame (kps_smooth, the five state arrays); computed once per case."""
    if case in _RUNS:
        return _RUNS[case]
    slots, J = smooth_scenes.CASES[case]
    p = smooth_scenes.PARAMS
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(DEV)
    st = {"id": z((slots,), torch.int32), "x": z((slots, J, 2), torch.float64), "dx": z((slots, J, 2), torch.float64),
          "t": z((slots, J), torch.float64), "n": z((slots, J), torch.int32)}
    now = z((1,), torch.float64)
    stream = _lib.current_stream(torch.device(DEV))
    log = []
    for fr in smooth_scenes.sequence(case):
        rows = fr["kps"].shape[0]
        kps, box, tid, keep = d(fr["kps"], np.float64), d(fr["box"], np.float32), d(fr["track_id"], np.int32), d(fr["keep"], np.int32)
        kc, seg, t_id = d([fr["keep_count"]], np.int32), d(fr["seg"], np.int32), d(fr["t_id"], np.int32)
        out = torch.full((rows, J, 3), -7.0, dtype=torch.float64, device=DEV)
        now.fill_(fr["now"])
        _lib.check(_lib.lib().sp_track_smooth(P(kps), P(box), P(tid), P(keep), P(kc), P(seg), rows, J, P(t_id), slots, P(now), p["min_cutoff"],
                                              p["beta"], p["d_cutoff"], p["max_gap"], p["in_vis_thre"], P(st["id"]), P(st["x"]), P(st["dx"]),
                                              P(st["t"]), P(st["n"]), P(out), stream), "sp_track_smooth")
        log.append((out.cpu().numpy(), {k: v.cpu().numpy() for k, v in st.items()}))
    _RUNS[case] = log
    return log


@pytest.mark.parametrize("case", list(smooth_scenes.CASES))
def test_kernel_sequence_equals_the_reference_bitwise(case):
    want = smooth_scenes.reference(case)
    frames = smooth_scenes.sequence(case)
    changed = 0
    for f, ((got_kps, got_st), (want_kps, want_st)) in enumerate(zip(_run(case), want)):
        smooth_scenes.bits_equal(got_kps, want_kps, f"{case} frame {f} kps_smooth")
        for k in ("id", "x", "dx", "t", "n"):
            smooth_scenes.bits_equal(got_st[k], getattr(want_st, k), f"{case} frame {f} s_{k}")
        raw = frames[f]["kps"]
        changed += int(((want_kps != raw) & ~np.isnan(raw)).any())
        np.testing.assert_array_equal(want_kps[..., 2], raw[..., 2])             # c is never filtered
    ev = want[-1][1].events
    assert all(ev.values()) and changed >= 3, (ev, changed)                      # every branch of the rules was taken, and frames were filtered
    assert [f["keep_count"] for f in frames].count(0) >= 2 and frames[0]["seg"][0] > 0


# ---- b. PoseTracker(smooth=...) end to end ---------------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def est(detector, dconv, renderer):
    return TopDownPoseEstimator(detector, dconv, capacity=32, renderer=renderer)


TIMES = [0.0, 0.03, 0.08, 0.07, 0.13, 0.16, 0.21, 0.9]                           # irregular; one step backwards, one gap above max_gap


def _state_equal(trk, ref, what):
    """The tracker's filter state against the reference's, which is driven with the tracker's own slot table: bit for bit."""
    for k in ("id", "x", "dx", "t", "n"):
        smooth_scenes.bits_equal(trk.smooth_state[k].cpu().numpy(), getattr(ref.state, k), f"{what} s_{k}")


def _ref_smoother(trk, est, one_euro):
    return smooth_ref.ResultSmoother(trk.slots, 17, smooth_ref.params(min_cutoff=one_euro.min_cutoff, beta=one_euro.beta, d_cutoff=one_euro.d_cutoff,
                                                                     max_gap=one_euro.max_gap, in_vis_thre=est.in_vis_thre))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphed"])
def test_tracker_smooths_as_the_reference_and_leaves_the_raw_results_alone(golden, est, renderer, graph):
    a, b = golden(G)["sp_a_image"], golden(G)["sp_b_image"]
    keep = est.use_graph
    try:
        est.use_graph = graph
        one_euro = OneEuro(min_cutoff=1.0, beta=0.5, d_cutoff=1.0, max_gap=0.5)
        # slots above the capacity: the conditioned random nets return `capacity` "persons" per frame, few of which are found again on a
        # propagated frame, so with 32 slots nearly every track would be evicted by the next frame's births before it is seen twice
        trk, bare = PoseTracker(est, slots=256, detect_every=2, smooth=one_euro), PoseTracker(est, slots=256, detect_every=2)
        ref = _ref_smoother(trk, est, one_euro)
        persons, moved = 0, 0
        # detector and propagated frame of a, of b (the time steps backwards on it), of a again (its tracks return), of b (after the gap)
        for f, (img, t) in enumerate(zip((a, a, b, b, a, a, b, b), TIMES)):
            got, raw = trk.update(img, timestamp=t), bare.update(img)
            assert trk.last_frame_kind == bare.last_frame_kind
            np.testing.assert_array_equal(got.keypoints, raw.keypoints, err_msg=f"frame {f}")
            np.testing.assert_array_equal(got.score, raw.score, err_msg=f"frame {f}")
            np.testing.assert_array_equal(got.box, raw.box, err_msg=f"frame {f}")
            np.testing.assert_array_equal(got.track_id, raw.track_id, err_msg=f"frame {f}")
            assert raw.keypoints_smooth is None
            assert got.keypoints_smooth.dtype == np.float64 and got.keypoints_smooth.shape == got.keypoints.shape
            want = ref.update(got.keypoints, got.box, got.track_id, trk.state["id"].cpu().numpy(), t)
            smooth_scenes.bits_equal(got.keypoints_smooth, want, f"frame {f} keypoints_smooth")
            _state_equal(trk, ref, f"frame {f}")                                 # s_t holds this frame's time: a time frozen into a graph shows here
            assert float(trk.smooth_state["now"].item()) == t
            # the overlay is drawn from the smoothed poses, inside the frame
            assert torch.equal(got.image.clone(), renderer.render(img, dataclasses.replace(got, keypoints=got.keypoints_smooth))), f"frame {f}"
            persons += len(got)
            moved += int((got.keypoints_smooth != got.keypoints).any())
        ev = ref.state.events
        print("MEASURED smoothing events", "graphed" if graph else "eager", ev, "frames filtered", moved)
        # persons were tracked, the filter did filter (a frozen time would restart every frame and return the raw poses), and the gap rule fired
        assert persons >= 8 and moved >= 2 and ev["update"] > 0 and ev["restart_gap"] + ev["restart_time"] > 0
        assert (len(trk._graphs) >= 2) == graph
    finally:
        est.use_graph = keep


def test_reset_restarts_the_filter_and_the_default_clock(golden, est):
    a = golden(G)["sp_a_image"]
    one_euro = OneEuro(fps=25.0)
    trk = PoseTracker(est, slots=256, detect_every=2, smooth=one_euro)
    for rounds in range(2):                                                      # the second round, after reset(), equals the first
        ref = _ref_smoother(trk, est, one_euro)
        outs = []
        for f in range(4):                                                       # detector, propagated, detector, propagated: the crops differ
            got = trk.update(a)
            want = ref.update(got.keypoints, got.box, got.track_id, trk.state["id"].cpu().numpy(), f / 25.0)
            smooth_scenes.bits_equal(got.keypoints_smooth, want, f"round {rounds} frame {f}")
            _state_equal(trk, ref, f"round {rounds} frame {f}")
            outs.append(got)
        np.testing.assert_array_equal(outs[0].keypoints_smooth, outs[0].keypoints)            # the first frame is the raw one
        assert len(outs[0]) >= 1 and outs[0].track_id.tolist() == list(range(1, len(outs[0]) + 1))
        assert ref.state.events["update"] > 0 and any((o.keypoints_smooth != o.keypoints).any() for o in outs[1:])
        assert int(trk.smooth_state["n"].max()) >= 2
        trk.reset()
        assert all(int(v.abs().max()) == 0 for v in trk.smooth_state.values()) and trk._frame_index == [0]
