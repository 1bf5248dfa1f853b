"""tools/bench_heat.py - what blending the kept persons' heat maps into a frame costs, on one MI355X.

    python tools/bench_heat.py [--out profiles/heat_bench.json] [--quick]

Two measurements, written the way tools/bench_redact.py measures:
  kernels   sp_heat_overlay_u8c3 (two launches: the records and u8 planes, then the tiles) alone, device events over back-to-back
            launches after a warm-up, at 1920 x 1080 with 32 persons (tools/bench_render.py's scene; every person's 17 x 64 x 48 maps are
            Gaussian bumps laid over its box), out of place and in place, with "value" and "constant" alpha.  Next to them, in the same
            run: the FLOOR of the out-of-place call - one read plus one write of the frame, measured as a device copy of the same bytes
            (Tensor.copy_) - the tile kernel with no record at all (rows = 0: the copy it degenerates to), and the redactor's and the
            renderer's two launches on the same scene.
  frame     PoseTracker.update (detect_every = 1, graphed: one replay per frame) with and without a heat overlay on the estimator, and
            with an overlay next to a renderer, on the same box in the same run, the variants ALTERNATED (so that clock ramps and
            neighbours hit them alike), median wall ms per frame ending in a device synchronise; the bare variant runs twice, the
            difference of its two medians is the measurement's own spread.  The set-up is tools/bench_tracker.py's: the s detector on a
            640 x 640 source, capacity 32, ResNet50-DConv fp32, the tests' conditioned (random) weights - the detections are not people,
            the work per frame is what is measured.
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
from simple_pose_amd.visualize import HeatOverlay, PoseRenderer, Redactor  # noqa: E402
from tests.detector_ref import detector_state_dict  # noqa: E402
from tools.bench_pipeline import CAPACITY, DEV, kernel_us, pose_model, summary, wall_ms  # noqa: E402
from tools.bench_render import scene  # noqa: E402

MH, MW, J = 64, 48, 17


def heat_scene(s, persons, seed):
    """The maps and trans_inv that go with tools/bench_render.py's scene: a bump per joint, the map laid over the person's box."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:MH, 0:MW].astype(np.float32)
    cy, cx = rng.uniform(4, MH - 4, (persons, J, 1, 1)).astype(np.float32), rng.uniform(4, MW - 4, (persons, J, 1, 1)).astype(np.float32)
    hm = (rng.uniform(0.4, 1.0, (persons, J, 1, 1)).astype(np.float32) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / 8.0)).astype(np.float32)
    box = s["box"].cpu().numpy()
    ti = np.zeros((persons, 2, 3), np.float32)
    ti[:, 0, 0], ti[:, 0, 2] = (box[:, 2] - box[:, 0]) / MW, box[:, 0]
    ti[:, 1, 1], ti[:, 1, 2] = (box[:, 3] - box[:, 1]) / MH, box[:, 1]
    return torch.from_numpy(hm).to(DEV), torch.from_numpy(ti).to(DEV)


def kernel_times(quick):
    h, w, persons = 1080, 1920, 32
    launches, rounds = (20, 2) if quick else (100, 5)             # rounds x launches timed repetitions (>= 20), after one warm-up round
    s = scene(h, w, persons, seed=h)
    hm, ti = heat_scene(s, persons, seed=7)
    dst = torch.empty_like(s["src"])
    ws = HeatOverlay.workspace(persons, MH, MW, DEV)
    out = {"frame": [w, h], "persons": persons, "maps": [J, MH, MW], "frame_bytes_read_plus_written": 2 * h * w * 3,
           "map_bytes_read": persons * J * MH * MW * 4}
    for name, kw, in_place in (("jet, value alpha", dict(), False), ("jet, constant alpha", dict(alpha="constant"), False),
                               ("jet, value alpha, in place", dict(), True)):
        o = HeatOverlay(**kw)
        src = s["src"].clone()
        to = src if in_place else dst
        run = lambda: o.launch(src, to, hm, ti, s["keep"], s["kc"], s["seg"], 0, persons, ws)
        run()
        changed = int((to != s["src"]).any(dim=2).sum().item())
        assert changed > 0
        out[name] = {"pixels_changed": changed, "sp_heat_overlay_u8c3 (2 kernels) back_to_back_us": kernel_us(run, launches, rounds)}
    o = HeatOverlay()
    empty = lambda: o.launch(s["src"], dst, None, None, None, None, None, 0, 0, None)
    copy = lambda: dst.copy_(s["src"])
    red, ren = Redactor(), PoseRenderer()
    rws, pws = Redactor.workspace(persons, DEV), PoseRenderer.workspace(persons, 17, DEV)
    redact = lambda: red.launch(s["src"], dst, s["kps"], s["box"], s["keep"], s["kc"], s["seg"], 0, persons, 17, rws)
    render = lambda: ren.launch(s["src"], dst, s["kps"], s["box"], s["tid"], s["keep"], s["kc"], s["seg"], 0, persons, 17, pws)
    out["tile kernel alone, no records (rows = 0) back_to_back_us"] = kernel_us(empty, launches, rounds)
    out["floor: device copy of the frame (one read + one write) back_to_back_us"] = kernel_us(copy, launches, rounds)
    out["sp_redact_u8c3 (2 kernels), head mosaic, same scene back_to_back_us"] = kernel_us(redact, launches, rounds)
    out["sp_render_poses_u8c3 (2 kernels), same scene back_to_back_us"] = kernel_us(render, launches, rounds)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heat_bench.json"))
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
    heat = HeatOverlay(gain=0.1, threshold=0.05)                  # the random-weight maps reach a few units: a tenth of them is visible
    trk = {"track": mk(), "track_heat": mk(heat_overlay=heat), "track_rendered": mk(renderer=PoseRenderer()),
           "track_heat_rendered": mk(heat_overlay=heat, renderer=PoseRenderer()), "track2": mk()}
    variants = {k: (lambda t=t: t.update(img)) for k, t in trk.items()}
    first = {k: fn() for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for r in range(warm + reps):
        for k, fn in variants.items():
            t = wall_ms(fn)
            if r >= warm:
                times[k].append(t)
    run = {"pose": "resnet50-dconv fp32", "source": [640, 640], "detector": "s fp32", "capacity": CAPACITY, "reps": reps, "graphed": True,
           "poses_kept": len(first["track"]), "same_poses_with_overlay": bool(np.array_equal(first["track"].keypoints, first["track_heat"].keypoints)),
           "pixels_changed": int((first["track_heat"].image != torch.from_numpy(img).to(DEV)).any(dim=2).sum().item())}
    run.update({k: summary(v) for k, v in times.items()})
    run["track_self_spread_ms"] = abs(run["track"]["median_ms"] - run["track2"]["median_ms"])
    run["heat_cost_ms"] = run["track_heat"]["median_ms"] - run["track"]["median_ms"]
    run["heat_cost_next_to_a_renderer_ms"] = run["track_heat_rendered"]["median_ms"] - run["track_rendered"]["median_ms"]
    out["frame"] = run
    print(json.dumps(run), flush=True)
    if not args.quick:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
