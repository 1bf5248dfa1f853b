"""tools/bench_tracker.py - what tracking costs per frame, and what leaving the detector out of three frames in four gains, on one MI355X.

    python tools/bench_tracker.py [--out profiles/tracker_bench.json] [--quick]
    python tools/bench_tracker.py --smooth [--out ...] [--quick]       what the key-point smoother adds to the tracked frame (see below)
    python tools/bench_tracker.py --streams [--out ...] [--quick]      S streams in one call against S single updates (see below)

Per frame, median wall time ending in a device synchronise, warm, the variants ALTERNATED in one process (so that clock ramps and
neighbours hit them alike), all graphed (one replay per frame):
  estimate   TopDownPoseEstimator.estimate, the untracked frame
  track1     PoseTracker.update, detect_every = 1: every frame runs the detector; track1 - estimate is the cost of the association
  track4     PoseTracker.update, detect_every = 4: one detector frame, then three frames whose boxes come from the tracks
  estimate2  the untracked frame again: the difference of the two medians is the measurement's own spread
The set-up is tools/bench_pipeline.py's: the s detector on a 640 x 640 source, capacity 32, ResNet50-DConv fp32 and ResNet50-DUC bf16, the
tests' conditioned (random) weights - the detections are not people, the work per frame is what is measured.  track4's median is over
all frames, detector frames included; its two kinds of frame are also reported apart.  The two new entry points are timed with device
events over back-to-back launches on a full state (32 tracks, 32 poses): sp_track_associate is two kernels per launch.

--smooth times the tracked frame (detect_every = 1, graphed) with and without PoseTracker(smooth=OneEuro()) in the same process, the two
ALTERNATED, plus the plain tracker a second time for the measurement's own spread, and sp_track_smooth alone with device events (32 kept
rows, every track found again, the time advancing from launch to launch so that every joint takes the update path).  The result is merged
into the output file under the key "smooth"; the other keys of the file stay as they are.

--streams times S video streams tracked in ONE call (MultiStreamTracker.update, detect_every = 1) for S in 1, 4, 8, 16 against S
PoseTracker.update calls one after the other on the same estimator in the same process, the two ALTERNATED: the same frame in every stream,
capacity 32 shared by the call, the estimator's min_box_score chosen from the detector's own scores so that every image contributes 32 / S
persons to both sides; fp32 and bf16, graphed and eager.  Reported: ms per update, ms per stream-frame, and the ratio of the S single
updates to the one call.  The four tracker launches (sp_track_associate_images' two, sp_track_boxes_images, sp_track_smooth_images) are
timed alone with device events for every S, 32 poses and tracks in total.  Merged into the output file under the key "streams".
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from simple_pose_amd import _lib  # noqa: E402
from simple_pose_amd.detector.nets.yolov5 import YOLOv5  # noqa: E402
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector  # noqa: E402
from simple_pose_amd.metrics import GaussTaylorKeyPointDecoder  # noqa: E402
from simple_pose_amd.pipeline import TopDownPoseEstimator  # noqa: E402
from simple_pose_amd.tracking import MultiStreamTracker, OneEuro, PoseTracker  # noqa: E402
from tests.detector_ref import detector_state_dict  # noqa: E402
from tools.bench_pipeline import CAPACITY, DEV, kernel_us, pose_model, summary, wall_ms  # noqa: E402

P = _lib.ptr


def kernel_times():
    """The two entry points alone, on a full state: 32 tracks that all find their pose again (the state stays full from launch to launch)."""
    rng = np.random.default_rng(3)
    slots, J = CAPACITY, 17
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    kps = d(np.concatenate([rng.uniform(0, 640, (slots, J, 2)), rng.uniform(0.3, 1, (slots, J, 1))], 2))
    area, box = d(rng.uniform(8000, 40000, slots)), d(rng.uniform(0, 1, (slots, 5)).astype(np.float32))
    keep, kc, seg = d(np.arange(slots, dtype=np.int32)), d(np.array([slots], np.int32)), d(np.array([0, slots], np.int32))
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
    st = {"id": z((slots,), torch.int32), "age": z((slots,), torch.int32), "miss": z((slots,), torch.int32), "kps": z((slots, J, 3), torch.float64),
          "area": z((slots,), torch.float64), "conf": z((slots,), torch.float32), "next_id": torch.ones((1,), dtype=torch.int32, device=DEV)}
    sim, ids = z((slots, slots), torch.float64), z((slots,), torch.int32)
    det, counts = z((1, 300, 6), torch.float32), z((1,), torch.int32)
    lib, stream = _lib.lib(), _lib.current_stream(torch.device(DEV))
    assoc = lambda: _lib.check(lib.sp_track_associate(P(kps), P(area), P(box), P(keep), P(kc), P(seg), slots, J, None, 0.5, 30, slots, P(st["id"]),
                                                      P(st["age"]), P(st["miss"]), P(st["kps"]), P(st["area"]), P(st["conf"]), P(st["next_id"]), P(sim),
                                                      P(ids), stream), "sp_track_associate")
    boxes = lambda: _lib.check(lib.sp_track_boxes(P(st["id"]), P(st["miss"]), P(st["kps"]), P(st["conf"]), slots, J, 0.2, 1.25, 0.0, 640, 640, 300,
                                                  P(det), P(counts), stream), "sp_track_boxes")
    assoc()
    out = {"sp_track_associate 32 tracks x 32 poses (2 kernels) back_to_back_us": kernel_us(assoc),
           "sp_track_boxes 32 tracks back_to_back_us": kernel_us(boxes)}
    assert int(counts.item()) == slots and sorted(ids.cpu().tolist()) == list(range(1, slots + 1))      # every launch matched all 32 again
    return out


def smooth_kernel_time():
    """sp_track_smooth alone: 32 kept rows of 17 joints whose tracks sit in slots 0..31, the time 1/30 s further at every launch."""
    rng = np.random.default_rng(4)
    slots, J = CAPACITY, 17
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
    kps = d(np.concatenate([rng.uniform(0, 640, (slots, J, 2)), rng.uniform(0.3, 1, (slots, J, 1))], 2))
    xy = rng.uniform(0, 400, (slots, 2))
    box = d(np.concatenate([xy, xy + rng.uniform(40, 200, (slots, 2)), rng.uniform(0, 1, (slots, 1))], 1).astype(np.float32))
    ids = d(np.arange(1, slots + 1, dtype=np.int32))
    keep, kc, seg = d(np.arange(slots, dtype=np.int32)), d(np.array([slots], np.int32)), d(np.array([0, slots], np.int32))
    st = {"id": z((slots,), torch.int32), "x": z((slots, J, 2), torch.float64), "dx": z((slots, J, 2), torch.float64),
          "t": z((slots, J), torch.float64), "n": z((slots, J), torch.int32)}
    now, out = z((1,), torch.float64), z((slots, J, 3), torch.float64)
    lib, stream = _lib.lib(), _lib.current_stream(torch.device(DEV))

    def launch():
        now.add_(1.0 / 30.0)                                      # (one more tiny launch inside the timed window: reported as such)
        _lib.check(lib.sp_track_smooth(P(kps), P(box), P(ids), P(keep), P(kc), P(seg), slots, J, P(ids), slots, P(now), 1.0, 0.5, 1.0, 0.5, 0.2,
                                       P(st["id"]), P(st["x"]), P(st["dx"]), P(st["t"]), P(st["n"]), P(out), stream), "sp_track_smooth")

    launch()
    us = kernel_us(launch)
    assert int(st["n"].min().item()) > 2                          # every joint was filtered at every launch
    return {"sp_track_smooth 32 rows x 17 joints + the clock's add_ back_to_back_us": us}


def smooth_main(args, det, img, decoder):
    reps, warm = (8, 4) if args.quick else (80, 8)
    out = {"device": torch.cuda.get_device_name(0), "source": [640, 640], "capacity": CAPACITY, "reps": reps, "one_euro": repr(OneEuro()),
           "kernels": smooth_kernel_time(), "runs": []}
    print(json.dumps(out["kernels"]), flush=True)
    for head, dtype in ([("dconv", "fp32")] if args.quick else [("dconv", "fp32"), ("duc", "bf16")]):
        est = TopDownPoseEstimator(det, pose_model(head, dtype), decoder=decoder, capacity=CAPACITY)
        plain, smooth, plain2 = PoseTracker(est), PoseTracker(est, smooth=OneEuro()), PoseTracker(est)
        variants = {"track": lambda: plain.update(img), "track_smooth": lambda: smooth.update(img), "track2": lambda: plain2.update(img)}
        first = {k: fn() for k, fn in variants.items()}
        times = {k: [] for k in variants}
        for r in range(warm + reps):
            for k, fn in variants.items():
                t = wall_ms(fn)
                if r >= warm:
                    times[k].append(t)
        last = smooth.update(img)
        run = {"pose": f"resnet50-{head} {dtype}", "poses_kept": len(first["track"]), "packed_bytes": int(est._frame(1, 640, 640, est.MAX_DET, 17).pack.numel()),
               "packed_bytes_smooth": int(est._frame(1, 640, 640, est.MAX_DET, 17, smooth=True).pack.numel()),
               "raw_results_equal": bool(np.array_equal(last.keypoints, first["track"].keypoints))}
        run.update({k: summary(v) for k, v in times.items()})
        run["track_self_spread_ms"] = abs(run["track"]["median_ms"] - run["track2"]["median_ms"])
        run["smoothing_cost_ms"] = run["track_smooth"]["median_ms"] - run["track"]["median_ms"]
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
    if not args.quick:
        whole = {}
        if os.path.isfile(args.out):
            with open(args.out) as fh:
                whole = json.load(fh)
        whole["smooth"] = out
        with open(args.out, "w") as fh:
            json.dump(whole, fh, indent=1)
        print("wrote", args.out)


STREAMS = (1, 4, 8, 16)


def streams_kernel_times(S):
    """The four tracker launches on S images alone: 32 / S tracks per image that all find their pose again, 32 rows in all."""
    rng = np.random.default_rng(5)
    rows, J, slots = CAPACITY, 17, CAPACITY
    per = rows // S
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
    kps = d(np.concatenate([rng.uniform(0, 640, (rows, J, 2)), rng.uniform(0.3, 1, (rows, J, 1))], 2))
    xy = rng.uniform(0, 400, (rows, 2))
    area = d(rng.uniform(8000, 40000, rows))
    box = d(np.concatenate([xy, xy + rng.uniform(40, 200, (rows, 2)), rng.uniform(0.1, 1, (rows, 1))], 1).astype(np.float32))
    keep, kc = d(np.arange(rows, dtype=np.int32)), d(np.full(S, per, np.int32))
    seg = d((np.arange(S + 1) * per).astype(np.int32))
    st = {"id": z((S, slots), torch.int32), "age": z((S, slots), torch.int32), "miss": z((S, slots), torch.int32),
          "kps": z((S, slots, J, 3), torch.float64), "area": z((S, slots), torch.float64), "conf": z((S, slots), torch.float32),
          "next_id": torch.ones((S,), dtype=torch.int32, device=DEV)}
    ss = {"id": z((S, slots), torch.int32), "x": z((S, slots, J, 2), torch.float64), "dx": z((S, slots, J, 2), torch.float64),
          "t": z((S, slots, J), torch.float64), "n": z((S, slots, J), torch.int32)}
    sim, ids, now, out = z((S, slots, slots), torch.float64), z((rows,), torch.int32), z((S,), torch.float64), z((rows, J, 3), torch.float64)
    det, counts = z((S, 300, 6), torch.float32), z((S,), torch.int32)
    lib, stream = _lib.lib(), _lib.current_stream(torch.device(DEV))
    assoc = lambda: _lib.check(lib.sp_track_associate_images(P(kps), P(area), P(box), P(keep), P(kc), P(seg), S, rows, J, None, 0.5, 30, slots,
                                                             P(st["id"]), P(st["age"]), P(st["miss"]), P(st["kps"]), P(st["area"]), P(st["conf"]),
                                                             P(st["next_id"]), P(sim), P(ids), stream), "sp_track_associate_images")
    boxes = lambda: _lib.check(lib.sp_track_boxes_images(P(st["id"]), P(st["miss"]), P(st["kps"]), P(st["conf"]), S, slots, J, 0.2, 1.25, 0.0, 640, 640,
                                                         300, P(det), P(counts), stream), "sp_track_boxes_images")

    def smooth():
        now.add_(1.0 / 30.0)                                      # (one more tiny launch inside the timed window: reported as such)
        _lib.check(lib.sp_track_smooth_images(P(kps), P(box), P(ids), P(keep), P(kc), P(seg), S, rows, J, P(st["id"]), slots, P(now), 1.0, 0.5, 1.0,
                                              0.5, 0.2, P(ss["id"]), P(ss["x"]), P(ss["dx"]), P(ss["t"]), P(ss["n"]), P(out), stream),
                   "sp_track_smooth_images")

    assoc()
    smooth()
    res = {"associate_2_kernels_us": kernel_us(assoc), "boxes_us": kernel_us(boxes), "smooth_plus_clock_add_us": kernel_us(smooth)}
    assert counts.cpu().tolist() == [per] * S and ids.cpu().tolist() == list(range(1, per + 1)) * S     # every launch matched all of them again
    assert int(ss["n"][:, :per].min().item()) > 2
    return res


def streams_main(args, det, img, decoder):
    reps, warm = (6, 3) if args.quick else (40, 6)
    boxes = det.single_predict(img)
    scores = np.sort(boxes[boxes[:, 5] == 0][:, 4].cpu().numpy())[::-1]
    assert scores.size > CAPACITY, "the detector finds fewer than capacity + 1 persons in the frame"
    out = {"device": torch.cuda.get_device_name(0), "source": [640, 640], "capacity": CAPACITY, "reps": reps, "streams": list(STREAMS),
           "kernels": {str(S): streams_kernel_times(S) for S in STREAMS}, "runs": []}
    print(json.dumps(out["kernels"]), flush=True)
    for head, dtype in ([("dconv", "fp32")] if args.quick else [("dconv", "fp32"), ("duc", "bf16")]):
        est = TopDownPoseEstimator(det, pose_model(head, dtype), decoder=decoder, capacity=CAPACITY)
        for graph in (True, False):
            est.use_graph = graph
            for S in STREAMS:
                per = CAPACITY // S
                est.min_box_score = float((scores[per - 1] + scores[per]) / 2)      # `per` detections of every image pass
                multi, singles = MultiStreamTracker(est, streams=S), [PoseTracker(est) for _ in range(S)]
                frames = np.stack([img] * S)

                def one_by_one():
                    return [t.update(img) for t in singles]

                variants = {"one_call": lambda: multi.update(frames), "single_updates": one_by_one}
                first = {k: fn() for k, fn in variants.items()}
                times = {k: [] for k in variants}
                for r in range(warm + reps):
                    for k, fn in variants.items():
                        t = wall_ms(fn)
                        if r >= warm:
                            times[k].append(t)
                same = all(np.array_equal(a.keypoints, b.keypoints) and np.array_equal(a.track_id, b.track_id)
                           for a, b in zip(first["one_call"], first["single_updates"]))
                run = {"pose": f"resnet50-{head} {dtype}", "graphed": graph, "streams": S, "persons_per_stream": [len(r) for r in first["one_call"]],
                       "dropped": int(sum(r.dropped for r in first["one_call"])), "results_equal_single_trackers": bool(same)}
                run.update({k: summary(v) for k, v in times.items()})
                run["one_call_ms_per_stream_frame"] = run["one_call"]["median_ms"] / S
                run["single_updates_ms_per_stream_frame"] = run["single_updates"]["median_ms"] / S
                run["single_updates_over_one_call"] = run["single_updates"]["median_ms"] / run["one_call"]["median_ms"]
                out["runs"].append(run)
                print(json.dumps(run), flush=True)
        est.use_graph = True
    if not args.quick:
        whole = {}
        if os.path.isfile(args.out):
            with open(args.out) as fh:
                whole = json.load(fh)
        whole["streams"] = out
        with open(args.out, "w") as fh:
            json.dump(whole, fh, indent=1)
        print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracker_bench.json"))
    ap.add_argument("--quick", action="store_true", help="DConv fp32 only, few repetitions; nothing is written")
    ap.add_argument("--smooth", action="store_true", help="the tracked frame with and without the key-point smoother; merged into --out under 'smooth'")
    ap.add_argument("--streams", action="store_true", help="S streams in one call against S single updates; merged into --out under 'streams'")
    args = ap.parse_args()
    reps, warm = (8, 4) if args.quick else (80, 8)                # multiples of 4: track4 sees whole detector / propagated cycles
    det = YOLOv5Detector(num_cls=80, scale_name="s", device=DEV, slice_idx=0, state_dict=detector_state_dict(YOLOv5(scale_name="s", num_cls=80), 14))
    det.conf_thresh, det.iou_thresh = 0.02, 0.45
    img = np.random.default_rng(0).integers(0, 256, (640, 640, 3), dtype=np.uint8)
    decoder = GaussTaylorKeyPointDecoder()
    if args.smooth:
        return smooth_main(args, det, img, decoder)
    if args.streams:
        return streams_main(args, det, img, decoder)
    out = {"device": torch.cuda.get_device_name(0), "source": [640, 640], "detector": "s fp32", "capacity": CAPACITY, "reps": reps,
           "pose_autotune": False, "kernels": kernel_times(), "runs": []}
    print(json.dumps(out["kernels"]), flush=True)
    for head, dtype in ([("dconv", "fp32")] if args.quick else [("dconv", "fp32"), ("duc", "bf16")]):
        model = pose_model(head, dtype)
        est = TopDownPoseEstimator(det, model, decoder=decoder, capacity=CAPACITY)
        trk1, trk4 = PoseTracker(est, detect_every=1), PoseTracker(est, detect_every=4)
        variants = {"estimate": lambda: est.estimate(img), "track1": lambda: trk1.update(img), "track4": lambda: trk4.update(img),
                    "estimate2": lambda: est.estimate(img)}
        first = {k: fn() for k, fn in variants.items()}
        times = {k: [] for k in variants}
        kinds = []
        for r in range(warm + reps):
            for k, fn in variants.items():
                t = wall_ms(fn)
                if r >= warm:
                    times[k].append(t)
                    if k == "track4":
                        kinds.append(trk4.last_frame_kind)
        run = {"pose": f"resnet50-{head} {dtype}", "poses_kept": len(first["estimate"]), "tracks_live": int(trk1.tracks()["id"].size),
               "track1_ids_stable": bool(trk1.update(img).track_id.tolist() == first["track1"].track_id.tolist()),
               "track4_propagated_share": kinds.count("propagated") / max(1, len(kinds))}
        run.update({k: summary(v) for k, v in times.items()})
        t4 = np.asarray(times["track4"])
        for kind in ("detector", "propagated"):
            sel = t4[np.asarray(kinds) == kind]
            if sel.size:
                run[f"track4_{kind}_frames"] = summary(sel)
        run["estimate_self_spread_ms"] = abs(run["estimate"]["median_ms"] - run["estimate2"]["median_ms"])
        run["association_cost_ms"] = run["track1"]["median_ms"] - run["estimate"]["median_ms"]
        run["track4_mean_ms"] = float(t4.mean())
        run["detect_every_4_gain_ms"] = run["estimate"]["median_ms"] - run["track4_mean_ms"]
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
    if not args.quick:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
