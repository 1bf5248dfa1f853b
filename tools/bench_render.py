"""tools/bench_render.py - what drawing the poses into the frame costs, on one MI355X.

    python tools/bench_render.py [--out profiles/render_bench.json] [--quick] [--labels]

Two measurements, written the way tools/bench_tracker.py measures:
  kernels   sp_render_poses_u8c3 (two launches: the primitive array, then the tiles) alone, device events over back-to-back launches after a
            warm-up, at 1920 x 1080 with 32 persons and at 640 x 480 with 4 persons (17 joints, COCO's 19 limbs, boxes: 40 primitives per
            person), out of place.  Next to each, the FLOOR of the call: one read plus one write of the frame, measured as a device copy of
            the same bytes (Tensor.copy_) in the same run, and the tile kernel with no primitive at all (rows = 0: the copy it degenerates to).
  frame     PoseTracker.update (detect_every = 1, graphed: one replay per frame) with and without a renderer on the estimator, on the same
            box in the same run, the variants ALTERNATED (so that clock ramps and neighbours hit them alike), median wall ms per frame
            ending in a device synchronise; the bare variant runs twice, the difference of its two medians is the measurement's own spread.
            The set-up is tools/bench_tracker.py's: the s detector on a 640 x 640 source, capacity 32, ResNet50-DConv fp32, the tests'
            conditioned (random) weights - the detections are not people, the work per frame is what is measured.

--labels measures the overlay's text instead (sp_render_labels_u8c3, two launches: the records, then the tiles, in place) and writes it
under the key "labels" of the same file, whose other keys it keeps: at 1920 x 1080 with 32 persons, label "#{id} {score}" and a caption,
both at scale 2, next to the overlay's two launches, the caption alone, and the frame copy; and the tracked frame bare, with the overlay,
and with the overlay and the text, alternated as above.
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
from simple_pose_amd.visualize import PoseRenderer  # noqa: E402
from tests.detector_ref import detector_state_dict  # noqa: E402
from tools.bench_pipeline import CAPACITY, DEV, kernel_us, pose_model, summary, wall_ms  # noqa: E402

# a standing person in a unit box (x, y in 0..1), COCO joint order
_POSE = np.array([[.5, .08], [.46, .06], [.54, .06], [.42, .08], [.58, .08], [.35, .22], [.65, .22], [.28, .38], [.72, .38], [.25, .52], [.75, .52],
                  [.4, .55], [.6, .55], [.38, .76], [.62, .76], [.37, .97], [.63, .97]], np.float64)


def scene(h, w, persons, seed):
    """`persons` standing persons, each about 0.45 of the frame high, spread over the frame: the device buffers of one frame."""
    rng = np.random.default_rng(seed)
    ph, pw = 0.45 * h, 0.2 * h
    x0, y0 = rng.uniform(0, w - pw, persons), rng.uniform(0, h - ph, persons)
    kps = np.concatenate([_POSE[None] * (pw, ph) + np.stack([x0, y0], 1)[:, None, :], rng.uniform(0.3, 1.0, (persons, 17, 1))], 2)
    box = np.stack([x0, y0, x0 + pw, y0 + ph, rng.uniform(0.3, 1, persons)], 1).astype(np.float32)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return {"src": d(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)), "kps": d(kps), "box": d(box), "tid": d(np.arange(1, persons + 1, dtype=np.int32)),
            "keep": d(np.arange(persons, dtype=np.int32)), "kc": d(np.array([persons], np.int32)), "seg": d(np.array([0, persons], np.int32))}


def kernel_times(quick):
    r = PoseRenderer()
    out = {}
    launches, rounds = (20, 2) if quick else (100, 5)             # rounds x launches timed repetitions (>= 20), after one warm-up round
    for h, w, persons in ((1080, 1920, 32), (480, 640, 4)):
        s = scene(h, w, persons, seed=h)
        dst = torch.empty_like(s["src"])
        ws = PoseRenderer.workspace(persons, 17, DEV)
        draw = lambda: r.launch(s["src"], dst, s["kps"], s["box"], s["tid"], s["keep"], s["kc"], s["seg"], 0, persons, 17, ws)
        empty = lambda: r.launch(s["src"], dst, None, None, None, None, None, None, 0, 0, 17, None)
        copy = lambda: dst.copy_(s["src"])
        draw()
        changed = int((dst != s["src"]).any(dim=2).sum().item())
        key = f"{w}x{h} {persons} persons"
        out[key] = {"primitives": persons * 40, "pixels_changed": changed, "frame_bytes_read_plus_written": 2 * h * w * 3,
                    "sp_render_poses_u8c3 (2 kernels) back_to_back_us": kernel_us(draw, launches, rounds),
                    "tile kernel alone, no primitives (rows = 0) back_to_back_us": kernel_us(empty, launches, rounds),
                    "floor: device copy of the frame (one read + one write) back_to_back_us": kernel_us(copy, launches, rounds)}
        assert changed > 0
    return out


TEXT = {"label": "#{id} {score}", "caption": "cam {image}: {n} persons"}


def label_kernel_times(quick):
    h, w, persons = 1080, 1920, 32
    launches, rounds = (20, 2) if quick else (100, 5)
    s = scene(h, w, persons, seed=h)
    score = torch.from_numpy(np.random.default_rng(1).uniform(0, 1, persons)).to(DEV)
    plain, text, only_caption = PoseRenderer(), PoseRenderer(**TEXT), PoseRenderer(caption=TEXT["caption"])
    dst = s["src"].clone()
    ws, lws = PoseRenderer.workspace(persons, 17, DEV), PoseRenderer.label_workspace(persons, DEV)
    cap = torch.from_numpy(text.caption_rows(1)).to(DEV)
    overlay = lambda: plain.launch(s["src"], dst, s["kps"], s["box"], s["tid"], s["keep"], s["kc"], s["seg"], 0, persons, 17, ws)
    labels = lambda: text.launch_labels(dst, s["box"], score, s["tid"], s["keep"], s["kc"], s["seg"], 0, persons, cap, lws)
    caption = lambda: only_caption.launch_labels(dst, s["box"], score, s["tid"], s["keep"], s["kc"], s["seg"], 0, persons, cap, lws)
    copy = lambda: dst.copy_(s["src"])
    overlay()
    before = dst.clone()
    labels()
    changed = int((dst != before).any(dim=2).sum().item())
    assert changed > 0
    return {"frame": [w, h], "persons": persons, "label": TEXT["label"], "caption": TEXT["caption"], "scale": 2, "pixels_changed_by_text": changed,
            "sp_render_labels_u8c3 (2 kernels), 32 labels + caption, back_to_back_us": kernel_us(labels, launches, rounds),
            "sp_render_labels_u8c3 (2 kernels), caption alone, back_to_back_us": kernel_us(caption, launches, rounds),
            "sp_render_poses_u8c3 (2 kernels) back_to_back_us": kernel_us(overlay, launches, rounds),
            "floor: device copy of the frame (one read + one write) back_to_back_us": kernel_us(copy, launches, rounds)}


def labels_main(args):
    reps, warm = (8, 4) if args.quick else (80, 8)
    out = {"device": torch.cuda.get_device_name(0), "kernels": label_kernel_times(args.quick)}
    print(json.dumps(out["kernels"]), flush=True)
    det = YOLOv5Detector(num_cls=80, scale_name="s", device=DEV, slice_idx=0, state_dict=detector_state_dict(YOLOv5(scale_name="s", num_cls=80), 14))
    det.conf_thresh, det.iou_thresh = 0.02, 0.45
    img = np.random.default_rng(0).integers(0, 256, (640, 640, 3), dtype=np.uint8)
    decoder, model = GaussTaylorKeyPointDecoder(), pose_model("dconv", "fp32")
    mk = lambda r: PoseTracker(TopDownPoseEstimator(det, model, decoder=decoder, capacity=CAPACITY, renderer=r))
    trk = {"track": mk(None), "track_rendered": mk(PoseRenderer()), "track_labelled": mk(PoseRenderer(**TEXT)), "track2": mk(None)}
    variants = {k: (lambda t=t: t.update(img)) for k, t in trk.items()}
    first = {k: fn() for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for r in range(warm + reps):
        for k, fn in variants.items():
            t = wall_ms(fn)
            if r >= warm:
                times[k].append(t)
    run = {"pose": "resnet50-dconv fp32", "source": [640, 640], "detector": "s fp32", "capacity": CAPACITY, "reps": reps, "graphed": True,
           "poses_kept": len(first["track"]), "same_poses_with_text": bool(np.array_equal(first["track"].keypoints, first["track_labelled"].keypoints)),
           "pixels_changed_by_text": int((first["track_labelled"].image != first["track_rendered"].image).any(dim=2).sum().item())}
    run.update({k: summary(v) for k, v in times.items()})
    run["track_self_spread_ms"] = abs(run["track"]["median_ms"] - run["track2"]["median_ms"])
    run["overlay_cost_ms"] = run["track_rendered"]["median_ms"] - run["track"]["median_ms"]
    run["text_cost_ms"] = run["track_labelled"]["median_ms"] - run["track_rendered"]["median_ms"]
    out["frame"] = run
    print(json.dumps(run), flush=True)
    if not args.quick:
        whole = {}
        if os.path.isfile(args.out):
            with open(args.out) as fh:
                whole = json.load(fh)
        whole["labels"] = out
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(whole, fh, indent=1)
        print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    ap.add_argument("--quick", action="store_true", help="few repetitions; nothing is written")
    ap.add_argument("--labels", action="store_true", help="measure the overlay's text (sp_render_labels_u8c3); written under the key \"labels\"")
    args = ap.parse_args()
    if args.labels:
        return labels_main(args)
    reps, warm = (8, 4) if args.quick else (80, 8)
    out = {"device": torch.cuda.get_device_name(0), "kernels": kernel_times(args.quick)}
    print(json.dumps(out["kernels"]), flush=True)
    det = YOLOv5Detector(num_cls=80, scale_name="s", device=DEV, slice_idx=0, state_dict=detector_state_dict(YOLOv5(scale_name="s", num_cls=80), 14))
    det.conf_thresh, det.iou_thresh = 0.02, 0.45
    img = np.random.default_rng(0).integers(0, 256, (640, 640, 3), dtype=np.uint8)
    decoder, model = GaussTaylorKeyPointDecoder(), pose_model("dconv", "fp32")
    bare = TopDownPoseEstimator(det, model, decoder=decoder, capacity=CAPACITY)
    drawn = TopDownPoseEstimator(det, model, decoder=decoder, capacity=CAPACITY, renderer=PoseRenderer())
    trk_bare, trk_drawn, trk_bare2 = PoseTracker(bare), PoseTracker(drawn), PoseTracker(bare)
    variants = {"track": lambda: trk_bare.update(img), "track_rendered": lambda: trk_drawn.update(img), "track2": lambda: trk_bare2.update(img)}
    first = {k: fn() for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for r in range(warm + reps):
        for k, fn in variants.items():
            t = wall_ms(fn)
            if r >= warm:
                times[k].append(t)
    run = {"pose": "resnet50-dconv fp32", "source": [640, 640], "detector": "s fp32", "capacity": CAPACITY, "reps": reps, "graphed": True,
           "poses_kept": len(first["track"]), "same_poses_with_renderer": bool(np.array_equal(first["track"].keypoints, first["track_rendered"].keypoints)),
           "pixels_changed": int((first["track_rendered"].image != torch.from_numpy(img).to(DEV)).any(dim=2).sum().item())}
    run.update({k: summary(v) for k, v in times.items()})
    run["track_self_spread_ms"] = abs(run["track"]["median_ms"] - run["track2"]["median_ms"])
    run["overlay_cost_ms"] = run["track_rendered"]["median_ms"] - run["track"]["median_ms"]
    run["overlay_share_of_frame"] = run["overlay_cost_ms"] / run["track_rendered"]["median_ms"]
    out["frame"] = run
    print(json.dumps(run), flush=True)
    if not args.quick:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
