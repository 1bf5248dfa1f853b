"""tools/bench_coco_eval.py - COCO keypoint evaluation (simple_pose_amd.metrics.coco_eval) on one MI355X against the CPU restatement.

    python tools/bench_coco_eval.py [--out profiles/coco_eval_bench.json] [--images 5000]

Workload: a seeded val2017-sized synthetic set (tests/coco_eval_ref.make_dataset: 5,000 images, about 6,000 ground-truth persons, about
100k detections, every image with detections over the 20-detection cut).  Timed: `KeypointEvaluator.evaluate()` with the detections already on
the device (HIP events on the launch stream and wall time, median of repeated runs after warm-up: the two launches of the per-image and the
accumulation kernels, the small host bookkeeping and the copy back of precision / recall), its two C-ABI calls alone, and the loop-by-loop
numpy restatement on the CPU, once.  Each step is a child process under its own time limit; the parent checks that both sides report the
same ten numbers and writes the record.  A record, not a bar.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 7
LIMITS = {"device": 600, "cpu": 1500}          # seconds


def dataset(images):
    from tests import coco_eval_ref as ref
    return ref.make_dataset(SEED, n_images=images, crowded_every=1, max_gt=2, crowded_copies=(14, 26))


def step_device(images, reps):
    import numpy as np
    import torch
    from simple_pose_amd import _lib
    from simple_pose_amd.metrics import KeypointEvaluator, KeypointGroundTruth
    gt, results, _ = dataset(images)
    truth = KeypointGroundTruth(gt)
    ev = KeypointEvaluator(truth, device="cuda:0")
    t0 = time.perf_counter()
    ev.add_results(results)
    add_ms = (time.perf_counter() - t0) * 1e3
    truth.device_tensors("cuda:0")
    runs = []
    for r in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        stats = ev.evaluate()
        e1.record()
        e1.synchronize()
        if r >= 2:
            runs.append((e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3))
    runs.sort()
    # the two C-ABI calls alone, on the tensors the last evaluate() left
    raw, lib, P = ev._raw, _lib.lib(), _lib.ptr
    from simple_pose_amd.metrics import coco_eval as ce
    import ctypes
    I, G, M = int(truth.image_ids.size), len(truth), ev.max_dets
    nbytes = ctypes.c_int64(0)
    lib.sp_coco_kp_accumulate_workspace(I, M, 10, 3, ctypes.byref(nbytes))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda:0")
    acc = []
    for r in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.sp_coco_kp_accumulate(P(raw["dt_count"]), P(raw["dt_kscore"]), P(raw["dtm"]), P(raw["dt_ignore"]), P(raw["gt_ignore"]), I, G, M,
                                             10, 3, ce._dptr(ce.REC_THRS), 101, P(ws), nbytes.value, P(raw["precision"]), P(raw["recall"]),
                                             _lib.current_stream()), "sp_coco_kp_accumulate")
        e1.record()
        e1.synchronize()
        if r >= 2:
            acc.append(e0.elapsed_time(e1))
    acc.sort()
    return {"images": I, "ground_truths": G, "detections": len(results), "kept_detections": int(sum(len(v) for v in ev.dt_ids.values())),
            "slots": I * M, "add_results_host_ms": add_ms, "evaluate_gpu_ms": runs[len(runs) // 2][0], "evaluate_wall_ms": runs[len(runs) // 2][1],
            "accumulate_gpu_ms": acc[len(acc) // 2], "per_image_gpu_ms_by_difference": runs[len(runs) // 2][0] - acc[len(acc) // 2],
            "rank_comparisons": (I * M) ** 2, "stats": [stats[k] for k in ce.STAT_NAMES], "reps": reps}


def step_cpu(images):
    from tests import coco_eval_ref as ref
    gt, results, _ = dataset(images)
    t0 = time.perf_counter()
    out = ref.evaluate(gt, results)
    return {"evaluate_wall_s": time.perf_counter() - t0, "stats": out["stats"].tolist(), "oks_threshold_margin": ref.threshold_margin(out["oks"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_eval_bench.json"))
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step", choices=["device", "cpu"], help="(internal) run one step and print its JSON")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(step_device(args.images, args.reps) if args.step == "device" else step_cpu(args.images)))
        return 0
    record = {"workload": f"make_dataset(seed={SEED}, n_images={args.images}, crowded_every=1, max_gt=2, crowded_copies=(14, 26))"}
    for step in ("device", "cpu"):                      # a step that fails or overruns ends the run: nothing is started after it
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--images", str(args.images), "--reps", str(args.reps)],
                           capture_output=True, text=True, timeout=LIMITS[step])
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            return p.returncode
        record[step] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    record["stats_equal"] = record["device"]["stats"] == record["cpu"]["stats"]
    record["speedup_wall"] = record["cpu"]["evaluate_wall_s"] * 1e3 / record["device"]["evaluate_wall_ms"]
    with open(args.out, "w") as wf:
        json.dump(record, wf, indent=1)
    print(json.dumps(record))
    return 0 if record["stats_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
