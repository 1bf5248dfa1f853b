"""tools/bench_redact.py - what hiding the heads or the persons of a frame costs, on one MI355X.

    python tools/bench_redact.py [--out profiles/redact_bench.json] [--quick]

Two measurements, written the way tools/bench_render.py measures:
  kernels   sp_redact_u8c3 (two launches: the region records, then the tiles) alone, device events over back-to-back launches after a
            warm-up, at 1920 x 1080 with 32 persons (tools/bench_render.py's scene), for head and person regions and for mosaic and
            fill at the default 16 px cell, out of place; the head mosaic also in place (untouched tiles are then neither read nor
            written) and at 4 and 64 px cells.  Next to them the FLOOR of the out-of-place call: one read plus one write of the frame,
            measured as a device copy of the same bytes (Tensor.copy_) in the same run, and the tile kernel with no record at all
            (rows = 0: the copy it degenerates to).
  frame     PoseTracker.update (detect_every = 1, graphed: one replay per frame) with and without a redactor on the estimator, and with
            a redactor and a renderer, on the same box in the same run, the variants ALTERNATED (so that clock ramps and neighbours hit
            them alike), median wall ms per frame ending in a device synchronise; the bare variant runs twice, the difference of its two
            medians is the measurement's own spread.  The set-up is tools/bench_tracker.py's: the s detector on a 640 x 640 source,
            capacity 32, ResNet50-DConv fp32, the tests' conditioned (random) weights - the detections are not people, the work per
            frame is what is measured.
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

from simple_pose_amd.detector.nets.yolov5 import YOLOv5  # noqa: E402
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector  # noqa: E402
from simple_pose_amd.metrics import GaussTaylorKeyPointDecoder  # noqa: E402
from simple_pose_amd.pipeline import TopDownPoseEstimator  # noqa: E402
from simple_pose_amd.tracking import PoseTracker  # noqa: E402
from simple_pose_amd.visualize import PoseRenderer, Redactor  # noqa: E402
from tests.detector_ref import detector_state_dict  # noqa: E402
from tools.bench_pipeline import CAPACITY, DEV, kernel_us, pose_model, summary, wall_ms  # noqa: E402
from tools.bench_render import scene  # noqa: E402

VARIANTS = (("head mosaic", dict(region="head", mode="mosaic"), False), ("head fill", dict(region="head", mode="fill"), False),
            ("person mosaic", dict(region="person", mode="mosaic"), False), ("person fill", dict(region="person", mode="fill"), False),
            ("head mosaic, in place", dict(region="head", mode="mosaic"), True), ("head mosaic, cell 4", dict(region="head", mode="mosaic", cell=4), False),
            ("head mosaic, cell 64", dict(region="head", mode="mosaic", cell=64), False))


def kernel_times(quick):
    h, w, persons = 1080, 1920, 32
    launches, rounds = (20, 2) if quick else (100, 5)             # rounds x launches timed repetitions (>= 20), after one warm-up round
    s = scene(h, w, persons, seed=h)
    dst = torch.empty_like(s["src"])
    ws = Redactor.workspace(persons, DEV)
    out = {"frame": [w, h], "persons": persons, "frame_bytes_read_plus_written": 2 * h * w * 3}
    for name, kw, in_place in VARIANTS:
        r = Redactor(**kw)
        src = s["src"].clone()
        to = src if in_place else dst
        run = lambda: r.launch(src, to, s["kps"], s["box"], s["keep"], s["kc"], s["seg"], 0, persons, 17, ws)
        run()
        changed = int((to != s["src"]).any(dim=2).sum().item())
        assert changed > 0
        out[name] = {"cell": r.cell, "pixels_changed": changed, "sp_redact_u8c3 (2 kernels) back_to_back_us": kernel_us(run, launches, rounds)}
    r = Redactor()
    empty = lambda: r.launch(s["src"], dst, None, None, None, None, None, 0, 0, 17, None)
    copy = lambda: dst.copy_(s["src"])
    out["tile kernel alone, no records (rows = 0) back_to_back_us"] = kernel_us(empty, launches, rounds)
    out["floor: device copy of the frame (one read + one write) back_to_back_us"] = kernel_us(copy, launches, rounds)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "redact_bench.json"))
    ap.add_argument("--quick", action="store_true", help="few repetitions; nothing is written")
    args = ap.parse_args()
    reps, warm = (8, 4) if args.quick else (80, 8)
    out = {"device": torch.cuda.get_device_name(0), "kernels": kernel_times(args.quick)}
    print(json.dumps(out["kernels"]), flush=True)
    det = YOLOv5Detector(num_cls=80, scale_name="s", device=DEV, slice_idx=0, state_dict=detector_state_dict(YOLOv5(scale_name="s", num_cls=80), 14))
    det.conf_thresh, det.iou_thresh = 0.02, 0.45
    img = np.random.default_rng(0).integers(0, 256, (640, 640, 3), dtype=np.uint8)
    decoder, model = GaussTaylorKeyPointDecoder(), pose_model("dconv", "fp32")
    mk = lambda **kw: PoseTracker(TopDownPoseEstimator(det, model, decoder=decoder, capacity=CAPACITY, **kw))
    trk = {"track": mk(), "track_redacted": mk(redactor=Redactor()), "track_rendered": mk(renderer=PoseRenderer()),
           "track_redacted_rendered": mk(redactor=Redactor(), renderer=PoseRenderer()), "track2": mk()}
    variants = {k: (lambda t=t: t.update(img)) for k, t in trk.items()}
    first = {k: fn() for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for r in range(warm + reps):
        for k, fn in variants.items():
            t = wall_ms(fn)
            if r >= warm:
                times[k].append(t)
    run = {"pose": "resnet50-dconv fp32", "source": [640, 640], "detector": "s fp32", "capacity": CAPACITY, "reps": reps, "graphed": True,
           "poses_kept": len(first["track"]), "same_poses_with_redactor": bool(np.array_equal(first["track"].keypoints, first["track_redacted"].keypoints)),
           "pixels_changed": int((first["track_redacted"].image != torch.from_numpy(img).to(DEV)).any(dim=2).sum().item())}
    run.update({k: summary(v) for k, v in times.items()})
    run["track_self_spread_ms"] = abs(run["track"]["median_ms"] - run["track2"]["median_ms"])
    run["redaction_cost_ms"] = run["track_redacted"]["median_ms"] - run["track"]["median_ms"]
    run["redaction_cost_next_to_a_renderer_ms"] = run["track_redacted_rendered"]["median_ms"] - run["track_rendered"]["median_ms"]
    out["frame"] = run
    print(json.dumps(run), flush=True)
    if not args.quick:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
