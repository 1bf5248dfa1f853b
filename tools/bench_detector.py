"""tools/bench_detector.py - YOLOv5 detector timings on one MI355X (fp32).

    python tools/bench_detector.py [--out profiles/detector_bench.json] [--quick]

Measures, with HIP events on the launch stream (median of repeated runs after warm-up): single_predict at batch 1, eager and graphed, for the
s and l models at 448x640 and 640x640 letterboxed inputs; predict throughput at batch 32; the NMS alone at conf 0.001 and 0.25.  FLOPs and
activation bytes come from the program's shapes (2 * MACs of every convolution; bytes = every buffer written once).  Weights are the tests'
conditioned ones (random: the NMS load depends on the weights, so its numbers are indicative).  The kernel breakdown comes from a run of its
own, `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o det -- python tools/bench_detector.py --quick`; its
det_kernel_stats.csv is kept as profiles/detector_kernel_stats.csv.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from simple_pose_amd.detector.nets.yolov5 import YOLOv5  # noqa: E402
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector, non_max_suppression  # noqa: E402
from tests.detector_ref import detector_state_dict  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append((e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3))
    ts.sort()
    return {"gpu_ms": ts[len(ts) // 2][0], "wall_ms": ts[len(ts) // 2][1]}


def program_cost(prog, batch):
    flops = sum(op.flops for op in prog.ops) * batch
    by = sum(int(np.prod(s)) * 4 for n, s in prog.shapes.items() if n != "input") * batch
    return flops, by


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detector_bench.json"))
    ap.add_argument("--quick", action="store_true", help="s model, 640x640 only, fewer repetitions")
    a = ap.parse_args()
    reps = 5 if a.quick else 20
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "dtype": "fp32", "runs": []}
    for scale in (("s",) if a.quick else ("s", "l")):
        m = YOLOv5(scale_name=scale, num_cls=80)
        det = YOLOv5Detector(num_cls=80, scale_name=scale, device=DEV, conf_thresh=0.25, iou_thresh=0.6, slice_idx=0,
                             state_dict=detector_state_dict(m, 14))
        for src_hw in (((640, 640),) if a.quick else ((432, 640), (640, 640))):
            img = rng.integers(0, 256, src_hw + (3,), dtype=np.uint8)
            g = det.transform.geometry(*src_hw)
            src = torch.from_numpy(img).to(DEV)
            prog = det.program(g["out_h"], g["out_w"])
            flops, by = program_cost(prog, 1)
            row = {"scale": scale, "letterboxed": [g["out_h"], g["out_w"]], "gflop_per_image": flops / 1e9, "act_mb_per_image": by / 1e6}
            for graph in (False, True):
                det.use_graph = graph
                row["single_predict_" + ("graph" if graph else "eager")] = timed(lambda: det.single_predict(src), reps)
            batch = torch.stack([src] * 32)
            t = timed(lambda: det.predict(batch), max(3, reps // 4), warmup=1)
            row["predict_b32"] = dict(t, images_per_s=32e3 / t["wall_ms"])
            pred = det._forward(src[None], g, False).clone()
            for conf in (0.001, 0.25):
                try:
                    row[f"nms_conf{conf}"] = timed(lambda: non_max_suppression(pred, conf, 0.6, merge=True), reps)
                except Exception as e:           # above the candidate cap: reported, not hidden
                    row[f"nms_conf{conf}"] = {"error": str(e)[:200]}
            res["runs"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
