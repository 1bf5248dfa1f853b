"""tools/bench_yuv.py - what taking video frames (NV12 / I420) costs against taking BGR, on one MI355X.

    python tools/bench_yuv.py [--out profiles/yuv_bench.json] [--quick]

Median wall time over ALTERNATED repetitions, each ending in a device synchronise, warm, at 1920 x 1080 and 3840 x 2160 for 1, 8 and 16
frames per call:
  (a) nv12_to_bgr      NV12 surfaces in HBM -> the estimator's static BGR block [n, H, W, 3] (video.convert_into: sp_yuv420_to_bgr_u8c3 for one
                       frame, the table launch for several), against what it replaces, bgr_copy: `copy_` of the same [n, H, W, 3] block on the device
  (b) i420_host        host yuv420p frames -> that block (one pinned upload of 1.5 B/px and one launch), against bgr_host: the host BGR
                       upload of TopDownPoseEstimator._load (torch.from_numpy(...) into the block's copy_, 3 B/px from pageable memory)
  (c) bgr_to_nv12      the block -> NV12 surfaces (video.from_bgr into frames made once)
  (d) tracked frame    PoseTracker.update (tools/bench_tracker.py's setting: the s detector, 640 x 640, capacity 32, ResNet50-DConv fp32, graphed,
                       detect_every 1) fed an NV12 surface in HBM against fed the same frame as a BGR tensor in HBM
The 16-byte path is what is timed: the surfaces have 256-byte pitches.  Reported per case: the medians, effective GB/s of (a) and (c) over
the 4.5 B/px they move, and (a)'s ratio to the copy measured in the same run; (a), the copy and (c) are also timed with device events
over back-to-back calls (key device_events_us).  --quick: few repetitions, nothing is written."""
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

from simple_pose_amd.detector.nets.yolov5 import YOLOv5  # noqa: E402
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector  # noqa: E402
from simple_pose_amd.metrics import GaussTaylorKeyPointDecoder  # noqa: E402
from simple_pose_amd.pipeline import TopDownPoseEstimator  # noqa: E402
from simple_pose_amd.tracking import PoseTracker  # noqa: E402
from simple_pose_amd.video import YuvFrame, convert_into, from_bgr, to_bgr  # noqa: E402
from tests.detector_ref import detector_state_dict  # noqa: E402
from tools.bench_pipeline import CAPACITY, DEV, kernel_us, pose_model, summary, wall_ms  # noqa: E402

SIZES = ((1080, 1920), (2160, 3840))
COUNTS = (1, 8, 16)


def alternate(variants, reps, warm):
    times = {k: [] for k in variants}
    for r in range(warm + reps):
        for k, fn in variants.items():
            t = wall_ms(fn)
            if r >= warm:
                times[k].append(t)
    return {k: summary(v) for k, v in times.items()}


def surface(h, w):
    """One NV12 surface in HBM with a 256-byte pitch, random bytes."""
    pitch = (w + 255) // 256 * 256
    buf = torch.randint(0, 256, (h + (h + 1) // 2, pitch), dtype=torch.uint8, device=DEV)
    return YuvFrame.from_surface(buf, h, w, pitch, "bt709", False)


def conversion_case(h, w, n, reps, warm):
    rng = np.random.default_rng(n)
    block, src = torch.zeros((n, h, w, 3), dtype=torch.uint8, device=DEV), torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=DEV)
    nv12 = [surface(h, w) for _ in range(n)]
    outs = [surface(h, w) for _ in range(n)]
    host_i420 = [YuvFrame.from_i420(rng.integers(0, 256, h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2), dtype=np.uint8), h, w) for _ in range(n)]
    host_bgr = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    views, stage = list(block), {}
    variants = {
        "nv12_to_bgr": lambda: convert_into(nv12, views, stage, dense=block),        # as TopDownPoseEstimator._load calls it
        "bgr_copy": lambda: block.copy_(src),
        "i420_host": lambda: convert_into(host_i420, views, stage, dense=block),
        "bgr_host": lambda: block.copy_(torch.from_numpy(np.ascontiguousarray(host_bgr))),
        "bgr_to_nv12": (lambda: from_bgr(src[0], out=outs[0])) if n == 1 else (lambda: from_bgr(list(src), out=outs)),
    }
    variants["nv12_to_bgr"]()
    assert torch.equal(to_bgr(nv12[0]), block[0])                 # the timed path gives to_bgr's bytes
    run = {"height": h, "width": w, "frames": n}
    run.update(alternate(variants, reps, warm))
    px = h * w * n
    run["nv12_to_bgr_GBps"] = 4.5 * px / run["nv12_to_bgr"]["median_ms"] / 1e6
    run["bgr_to_nv12_GBps"] = 4.5 * px / run["bgr_to_nv12"]["median_ms"] / 1e6
    run["bgr_copy_GBps"] = 6.0 * px / run["bgr_copy"]["median_ms"] / 1e6
    run["nv12_to_bgr_over_bgr_copy"] = run["nv12_to_bgr"]["median_ms"] / run["bgr_copy"]["median_ms"]
    run["i420_host_over_bgr_host"] = run["i420_host"]["median_ms"] / run["bgr_host"]["median_ms"]
    return run


def device_events():
    """(a), the copy and (c) again with device events over 50 back-to-back calls (median of 5 rounds): the launches without the host's
    synchronise, so what is left of the host is its enqueue rate."""
    out = {}
    for h, w in SIZES:
        for n in (1, 16):
            block, src = torch.zeros((n, h, w, 3), dtype=torch.uint8, device=DEV), torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=DEV)
            nv12, outs = [surface(h, w) for _ in range(n)], [surface(h, w) for _ in range(n)]
            views, stage = list(block), {}
            r = {"nv12_to_bgr_us": kernel_us(lambda: convert_into(nv12, views, stage, dense=block), 50, 5),
                 "bgr_copy_us": kernel_us(lambda: block.copy_(src), 50, 5),
                 "bgr_to_nv12_us": kernel_us((lambda: from_bgr(src[0], out=outs[0])) if n == 1 else (lambda: from_bgr(list(src), out=outs)), 50, 5)}
            r["nv12_to_bgr_over_bgr_copy"] = r["nv12_to_bgr_us"] / r["bgr_copy_us"]
            out[f"{h}x{w}x{n}"] = r
    return out


def tracked_frame(reps, warm):
    det = YOLOv5Detector(num_cls=80, scale_name="s", device=DEV, slice_idx=0, state_dict=detector_state_dict(YOLOv5(scale_name="s", num_cls=80), 14))
    det.conf_thresh, det.iou_thresh = 0.02, 0.45
    est = TopDownPoseEstimator(det, pose_model("dconv", "fp32"), decoder=GaussTaylorKeyPointDecoder(), capacity=CAPACITY)
    frame = surface(640, 640)
    bgr = to_bgr(frame)
    a, b, c = PoseTracker(est), PoseTracker(est), PoseTracker(est)
    variants = {"track_bgr": lambda: a.update(bgr), "track_nv12": lambda: b.update(frame), "track_bgr2": lambda: c.update(bgr)}
    first = {k: fn() for k, fn in variants.items()}
    run = {"source": [640, 640], "pose": "resnet50-dconv fp32", "capacity": CAPACITY, "poses_kept": len(first["track_bgr"]),
           "results_equal": bool(np.array_equal(first["track_bgr"].keypoints, first["track_nv12"].keypoints))}
    run.update(alternate(variants, reps, warm))
    run["track_bgr_self_spread_ms"] = abs(run["track_bgr"]["median_ms"] - run["track_bgr2"]["median_ms"])
    run["nv12_minus_bgr_ms"] = run["track_nv12"]["median_ms"] - run["track_bgr"]["median_ms"]
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_bench.json"))
    ap.add_argument("--quick", action="store_true", help="few repetitions; nothing is written")
    args = ap.parse_args()
    reps, warm = (5, 2) if args.quick else (30, 5)
    out = {"device": torch.cuda.get_device_name(0), "reps": reps, "conversions": [], "tracked_frame": None}
    for h, w in SIZES:
        for n in COUNTS:
            run = conversion_case(h, w, n, max(5, reps // 3) if n > 1 else reps, warm)
            out["conversions"].append(run)
            print(json.dumps(run), flush=True)
    out["device_events_us"] = device_events()
    print(json.dumps(out["device_events_us"]), flush=True)
    out["tracked_frame"] = tracked_frame(*((8, 4) if args.quick else (80, 8)))
    print(json.dumps(out["tracked_frame"]), flush=True)
    if not args.quick:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
