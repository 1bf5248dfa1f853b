"""tools/bench_pipeline.py - the top-down frame (image -> poses) on one MI355X: staged chain vs the device-resident estimator.

    python tools/bench_pipeline.py [--out profiles/pipeline_bench.json] [--quick] [--flip-test]

Per frame, median wall time ending in a device synchronise, warm, the variants ALTERNATED in one process (so that clock ramps and
neighbours hit them alike):
  staged   single_predict -> crop_boxes -> forward_crops -> decoder -> filter_poses (the public pieces, as a user assembles them)
  staged2  the same chain again: the difference of the two medians is the measurement's own spread
  eager    TopDownPoseEstimator.estimate with use_graph = False
  graph    TopDownPoseEstimator.estimate, one graph replay per frame
for the s detector on a 640x640 source, ResNet50-DConv fp32 and ResNet50-DUC bf16, capacity 32, at n = 1, 8 and 32 live persons (n is set
through min_box_score from the detector's own scores and recorded).  Weights are the tests' conditioned ones (random), so the detections are
not people - the work per frame is what is measured.  The kernel breakdown comes from a run of its own,
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o pipe -- python tools/bench_pipeline.py --quick`; its pipe_kernel_stats.csv
is kept as profiles/pipeline_kernel_stats.csv.  The pose models run with tile timing off (autotune = False): see pose_model.

--flip-test measures what the flip test costs instead: the frame at 32 live persons with `flip_test` off and on, eager and graphed (and
the off / graphed frame a second time: the measurement's own spread), plus the two kernels it adds (sp_mirror_w on 32 crops,
sp_heat_map_flip_merge on 32 x 17 heat maps) timed with device events over back-to-back launches.  The result is merged into --out under
the key "flip_test"; the other keys of the file stay.

--mixed measures a set of differently sized images instead (mixed_bench below): `estimate` one by one against `estimate_batch` on lists of
8 and 32, in images per second, into profiles/pipeline_mixed_bench.json under "mixed".  --mixed-baseline runs the one-by-one variants only
and writes them under "baseline_one_by_one": that half uses nothing newer than `estimate`, so the same file can be run from the tree of an
older commit to measure it there on the same box.

--tiled measures tiled detection (simple_pose_amd/tiling.py) on a seeded 3840x2160 frame with the default `Tiling` (the frame and 8 x 4
tiles of 640x640), in ms per `estimate`: untiled, tiled (eager and one graph), and the staged equivalent - single_predict on the frame,
predict on contiguous copies of the tiles, the shift and the merge in numpy, then estimate_boxes - into
profiles/pipeline_tiled_bench.json.
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

from oracle import nets_oracle  # noqa: E402
from simple_pose_amd import synth  # noqa: E402
from simple_pose_amd.datasets.naive_data import crop_boxes, filter_poses  # noqa: E402
from simple_pose_amd.detector.nets.yolov5 import YOLOv5  # noqa: E402
from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector  # noqa: E402
from simple_pose_amd.metrics import GaussTaylorKeyPointDecoder  # noqa: E402
from simple_pose_amd.nets import pose_resnet_dconv, pose_resnet_duc  # noqa: E402
from simple_pose_amd.pipeline import TopDownPoseEstimator  # noqa: E402
from tests.detector_ref import detector_state_dict  # noqa: E402

DEV = "cuda:0"
CAPACITY = 32


def pose_model(head, dtype):
    m = (pose_resnet_dconv if head == "dconv" else pose_resnet_duc).resnet50(pretrained=False, num_classes=17)
    sd = synth.conditioned_state_dict(nets_oracle.state_dict_shapes_resnet50(head), 0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    m.compute_dtype = dtype
    # One Program serves every variant.  Tile timing is OFF: the first batch-32 forward would otherwise pin batch-32 tiles that the staged
    # chain's batch-1 / batch-8 forwards then run on (forward_crops never retunes downwards), to the staged side's disadvantage.  Every
    # variant runs the library's default tiles.
    m.autotune = False
    return m


def staged_frame(detector, model, decoder, img, dev_img, min_score):
    boxes = detector.single_predict(img)
    if isinstance(boxes, list):
        return [], 0
    boxes = boxes[(boxes[:, 5] == 0) & (boxes[:, 4] >= min_score)][:CAPACITY]
    if boxes.shape[0] == 0:
        return [], 0
    crops, tinv, _, _, area = crop_boxes(dev_img, boxes[:, :4].cpu().numpy())
    with torch.no_grad():
        hm = model.forward_crops(crops)
        kps, mv = decoder(hm, tinv)
    return filter_poses(torch.cat([kps, mv], -1), boxes[:, 4].double().cpu().numpy(), area, [0] * boxes.shape[0]), int(boxes.shape[0])


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(ts):
    a = np.sort(np.asarray(ts))
    return {"median_ms": float(np.median(a)), "p25_ms": float(a[len(a) // 4]), "p75_ms": float(a[(3 * len(a)) // 4]), "min_ms": float(a[0])}


def kernel_us(fn, launches=200, rounds=5):
    """Median over `rounds` of (device-event time of `launches` back-to-back launches) / launches, in microseconds."""
    out = []
    for _ in range(rounds + 1):                                   # the first round warms up
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(launches):
            fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) * 1e3 / launches)
    return float(np.median(out[1:]))


def flip_test_bench(args, det, img, decoder):
    from simple_pose_amd.metrics import merge_flipped, mirror_input
    reps, warm = (5, 2) if args.quick else (40, 5)
    crops = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (2 * CAPACITY, 256, 192, 3), dtype=np.uint8)).to(DEV)
    hm = torch.from_numpy(np.random.default_rng(2).standard_normal((2 * CAPACITY, 17, 64, 48)).astype(np.float32)).to(DEV)
    res = {"device": torch.cuda.get_device_name(0), "capacity": CAPACITY, "reps": reps, "pose_autotune": False, "kernels": {
        "sp_mirror_w u8 [32,256,192,3] back_to_back_us": kernel_us(lambda: mirror_input(crops[:CAPACITY], out=crops[CAPACITY:])),
        "sp_heat_map_flip_merge f32 [32,17,64,48] in place back_to_back_us": kernel_us(
            lambda: merge_flipped(hm[:CAPACITY], hm[CAPACITY:], out=hm[:CAPACITY]))}, "runs": []}
    print(json.dumps(res["kernels"]), flush=True)
    for head, dtype in ([("dconv", "fp32")] if args.quick else [("dconv", "fp32"), ("duc", "bf16")]):
        model = pose_model(head, dtype)
        off = TopDownPoseEstimator(det, model, decoder=decoder, capacity=CAPACITY)
        on = TopDownPoseEstimator(det, model, decoder=decoder, capacity=CAPACITY, flip_test=True)
        frame = lambda est, graph: (setattr(est, "use_graph", graph), est.estimate(img))[1]
        variants = {"off_eager": lambda: frame(off, False), "off_graph": lambda: frame(off, True), "on_eager": lambda: frame(on, False),
                    "on_graph": lambda: frame(on, True), "off_graph2": lambda: frame(off, True)}
        first = {k: fn() for k, fn in variants.items()}
        times = {k: [] for k in variants}
        for r in range(warm + reps):
            for k, fn in variants.items():
                t = wall_ms(fn)
                if r >= warm:
                    times[k].append(t)
        graphs = [next(iter(e._frames.values())).graph is not None and len(e._frames) == 1 for e in (off, on)]
        run = {"pose": f"resnet50-{head} {dtype}", "poses_kept_off": len(first["off_graph"]), "poses_kept_on": len(first["on_graph"]),
               "graph_equals_eager": bool(first["off_graph"].coco(0) == first["off_eager"].coco(0) and first["on_graph"].coco(0) == first["on_eager"].coco(0)),
               "one_graph_per_estimator": bool(all(graphs))}
        run.update({k: summary(v) for k, v in times.items()})
        run["off_graph_self_spread_ms"] = abs(run["off_graph"]["median_ms"] - run["off_graph2"]["median_ms"])
        run["flip_cost_graph_ms"] = run["on_graph"]["median_ms"] - run["off_graph"]["median_ms"]
        run["flip_cost_eager_ms"] = run["on_eager"]["median_ms"] - run["off_eager"]["median_ms"]
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    if not args.quick:
        doc = {}
        if os.path.isfile(args.out):
            with open(args.out) as fh:
                doc = json.load(fh)
        doc["flip_test"] = res
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
        print("wrote", args.out)


MIXED_SIZES = ((480, 640), (427, 640), (640, 480), (375, 500), (640, 427), (500, 375))     # COCO's common sizes: four detector net shapes
MIXED_IMAGES = 32


def git_commit():
    import subprocess
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return None


def mixed_bench(args, det, decoder):
    """Images per second over a seeded set of MIXED_IMAGES differently sized images, fp32 DConv, capacity 32 per 8 images:
      one_by_one_graph / one_by_one_eager   `estimate` per image (existing code: with --mixed-baseline only these run, so that the same
                                            file measures them on an older commit)
      batch8 / batch32                      `estimate_batch` on lists of 8 (capacity 32) and of all 32 (capacity 128)
    Every variant sees the same `min_box_score`, chosen from the detector's own scores so that the set holds about four persons per image;
    `persons` / `dropped` per variant are recorded.  `stages_ms` splits one list of 8 with a device synchronise after every stage (a
    diagnostic: the synchronisations are not in the timed calls)."""
    rng = np.random.default_rng(7)
    order = rng.integers(0, len(MIXED_SIZES), MIXED_IMAGES)
    order[:len(MIXED_SIZES)] = np.arange(len(MIXED_SIZES))                       # every size occurs
    imgs = [rng.integers(0, 256, MIXED_SIZES[k] + (3,), dtype=np.uint8) for k in order]
    nets = sorted({(g["out_h"], g["out_w"]) for g in (det.transform.geometry(*i.shape[:2]) for i in imgs)})
    assert len(nets) >= 3
    scores = np.sort(np.concatenate([(f[f[:, 5] == 0][:, 4].cpu().numpy() if not isinstance(f, list) else np.zeros(0, np.float32))
                                     for f in (det.single_predict(i) for i in imgs)]))[::-1]
    want = 4 * MIXED_IMAGES
    min_score = 0.0 if scores.size <= want else float((np.float64(scores[want - 1]) + np.float64(scores[want])) / 2)
    reps, warm = (3, 1) if args.quick else (10, 2)
    model = pose_model("dconv", "fp32")
    mk = lambda cap: TopDownPoseEstimator(det, model, decoder=decoder, capacity=cap, min_box_score=min_score)
    single, e8, e32 = mk(CAPACITY), mk(CAPACITY), mk(4 * CAPACITY)

    def one_by_one(graph):
        single.use_graph = graph
        return [single.estimate(i) for i in imgs]

    variants = {"one_by_one_graph": lambda: one_by_one(True), "one_by_one_eager": lambda: one_by_one(False)}
    if not args.mixed_baseline:
        variants["batch8"] = lambda: [r for k in range(0, MIXED_IMAGES, 8) for r in e8.estimate_batch(imgs[k:k + 8])]
        variants["batch32"] = lambda: e32.estimate_batch(imgs)
        variants["one_by_one_graph2"] = variants["one_by_one_graph"]             # again: the measurement's own spread
    first = {k: fn() for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for r in range(warm + reps):
        for k, fn in variants.items():
            t = wall_ms(fn)
            if r >= warm:
                times[k].append(t)
    res = {"device": torch.cuda.get_device_name(0), "commit": args.commit or git_commit(), "images": MIXED_IMAGES, "sizes": [list(s) for s in MIXED_SIZES],
           "net_shapes": [list(s) for s in nets], "detector": "s fp32", "pose": "resnet50-dconv fp32", "pose_autotune": False,
           "capacity_per_8_images": CAPACITY, "min_box_score": min_score, "reps": reps, "variants": {}}
    for k, ts in times.items():
        s = summary(ts)
        s.update(images_per_s=MIXED_IMAGES / (s["median_ms"] * 1e-3), ms_per_image=s["median_ms"] / MIXED_IMAGES,
                 persons=int(sum(len(r) for r in first[k])), dropped=int(sum(r.dropped for r in first[k])))
        res["variants"][k] = s
    if not args.mixed_baseline:
        from simple_pose_amd.mixed_batch import MixedBatch
        stages = {"upload": [], "detect": [], "poses": [], "fetch": []}
        for _ in range(reps):
            lst, t = imgs[:8], {}
            pose_prog = e8._pose_program()
            box = {}
            t["upload"] = wall_ms(lambda: box.update(mb=MixedBatch(lst, det.transform, e8.device, e8._stage)))
            fr = e8._mixed_frame(box["mb"], e8.MAX_DET, pose_prog.out_shape[0])
            t["detect"] = wall_ms(lambda: e8._detect_mixed(fr, box["mb"]))
            t["poses"] = wall_ms(lambda: e8._poses(fr, pose_prog, False, box["mb"].caller_table))
            t["fetch"] = wall_ms(lambda: e8._results(fr))
            for k, v in t.items():
                stages[k].append(v)
        res["stages_ms_list_of_8"] = {k: float(np.median(v)) for k, v in stages.items()}
        res["stages_ms_list_of_8"]["detector_groups"] = len(MixedBatch(imgs[:8], det.transform, e8.device, e8._stage).groups)
        v = res["variants"]
        res["batch8_over_one_by_one_graph"] = v["batch8"]["images_per_s"] / v["one_by_one_graph"]["images_per_s"]
        res["batch32_over_one_by_one_graph"] = v["batch32"]["images_per_s"] / v["one_by_one_graph"]["images_per_s"]
    print(json.dumps(res), flush=True)
    doc = {}
    if os.path.isfile(args.out):
        with open(args.out) as fh:
            doc = json.load(fh)
    doc["baseline_one_by_one" if args.mixed_baseline else "mixed"] = res
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", args.out)


def tiled_bench(args, det, decoder):
    """ms per frame on one seeded 3840x2160 frame, fp32 DConv, capacity 32, the variants alternated:
      untiled_graph            `estimate` without a tiling (one graph): what the frame cost before, finding no small person
      tiled_graph / _eager     `estimate` with the default Tiling: 33 passes, two detector forwards, the fusion on the device
      staged                   the same result from public calls through the host (its numpy merge alone: staged_merge_ms)
      tiled_graph2             tiled_graph again: the measurement's own spread"""
    from simple_pose_amd.tiling import Tiling
    from tests import tiled_ref
    H, W = 2160, 3840
    img = np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)
    tiling = Tiling()
    passes = tiling.plan(H, W)
    model = pose_model("dconv", "fp32")
    plain = TopDownPoseEstimator(det, model, decoder=decoder, capacity=CAPACITY)
    tiled = TopDownPoseEstimator(det, model, decoder=decoder, capacity=CAPACITY, tiling=tiling)
    merge_ms = []

    def staged():
        whole = det.single_predict(img)
        tiles = det.predict([np.ascontiguousarray(img[y:y + h, x:x + w]) for y, x, h, w in passes[1:]])
        rows = []
        for (y0, x0, _, _), r in zip(passes, [whole] + tiles):
            r = np.zeros((0, 6), np.float32) if isinstance(r, list) else r.cpu().numpy()
            r[:, 0] += np.float32(x0); r[:, 2] += np.float32(x0); r[:, 1] += np.float32(y0); r[:, 3] += np.float32(y0)
            rows.append(r)
        cat = np.concatenate(rows, 0)
        t0 = time.perf_counter()
        keep = tiled_ref.merge_rows_np(cat, tiling.metric, tiling.thresh, tiling.agnostic, plain.MAX_DET)
        merge_ms.append((time.perf_counter() - t0) * 1e3)
        if len(keep) == 0:
            return plain.estimate_boxes(img, np.zeros((1, 6), np.float32), [0])[0], int(cat.shape[0])
        return plain.estimate_boxes(img, cat[keep])[0], int(cat.shape[0])

    frame = lambda est, graph: (setattr(est, "use_graph", graph), est.estimate(img))[1]
    variants = {"untiled_graph": lambda: frame(plain, True), "tiled_graph": lambda: frame(tiled, True), "tiled_eager": lambda: frame(tiled, False),
                "staged": lambda: staged()[0], "tiled_graph2": lambda: frame(tiled, True)}
    first = {k: fn() for k, fn in variants.items()}
    n_cand = staged()[1]
    reps, warm = (3, 1) if args.quick else (15, 3)
    merge_ms.clear()
    times = {k: [] for k in variants}
    for r in range(warm + reps):
        for k, fn in variants.items():
            t = wall_ms(fn)
            if r >= warm:
                times[k].append(t)
    res = {"device": torch.cuda.get_device_name(0), "commit": args.commit or git_commit(), "source": [H, W], "tiling": list(tiling.key()),
           "passes": len(passes), "detector": "s fp32", "pose": "resnet50-dconv fp32", "pose_autotune": False, "capacity": CAPACITY, "reps": reps,
           "candidates_before_merge": n_cand, "poses_kept": {k: len(v) for k, v in first.items()},
           "tiled_equals_staged": bool(first["tiled_graph"].coco(0) == first["staged"].coco(0) == first["tiled_eager"].coco(0)),
           "one_graph": bool(len(tiled._frames) == 1 and next(iter(tiled._frames.values())).graph is not None)}
    res.update({k: summary(v) for k, v in times.items()})
    res["staged_merge_ms"] = float(np.median(merge_ms))
    res["tiled_graph_self_spread_ms"] = abs(res["tiled_graph"]["median_ms"] - res["tiled_graph2"]["median_ms"])
    res["staged_over_tiled_graph"] = res["staged"]["median_ms"] / res["tiled_graph"]["median_ms"]
    res["tiled_graph_over_untiled_graph"] = res["tiled_graph"]["median_ms"] / res["untiled_graph"]["median_ms"]
    print(json.dumps(res), flush=True)
    if not args.quick:
        with open(args.out, "w") as fh:
            json.dump({"tiled": res}, fh, indent=1)
        print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiled", action="store_true", help="tiled detection on a 3840x2160 frame: untiled vs tiled vs the staged equivalent "
                    "(default --out: profiles/pipeline_tiled_bench.json)")
    ap.add_argument("--mixed", action="store_true", help="a seeded set of differently sized images: estimate one by one vs estimate_batch on "
                    "lists of 8 and 32 (default --out: profiles/pipeline_mixed_bench.json)")
    ap.add_argument("--mixed-baseline", action="store_true", help="--mixed, the one-by-one variants only (runs on commits without mixed batches)")
    ap.add_argument("--commit", default=None, help="the commit to record with --mixed (default: git rev-parse of this tree)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="DConv fp32 at n = 32 only, few repetitions (the kernel-trace run)")
    ap.add_argument("--flip-test", action="store_true", help="the frame at 32 persons with the flip test off / on, and its two kernels")
    args = ap.parse_args()
    args.mixed = args.mixed or args.mixed_baseline
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "pipeline_tiled_bench.json" if args.tiled else
                                "pipeline_mixed_bench.json" if args.mixed else "pipeline_bench.json")
    reps, warm = (5, 2) if args.quick else (40, 5)
    det = YOLOv5Detector(num_cls=80, scale_name="s", device=DEV, slice_idx=0, state_dict=detector_state_dict(YOLOv5(scale_name="s", num_cls=80), 14))
    det.conf_thresh, det.iou_thresh = 0.02, 0.45
    if args.mixed:
        return mixed_bench(args, det, GaussTaylorKeyPointDecoder())
    if args.tiled:
        return tiled_bench(args, det, GaussTaylorKeyPointDecoder())
    img = np.random.default_rng(0).integers(0, 256, (640, 640, 3), dtype=np.uint8)
    dev_img = torch.from_numpy(img).to(DEV)
    found = det.single_predict(img)
    scores = np.zeros(0, np.float32) if isinstance(found, list) else found[found[:, 5] == 0][:, 4].cpu().numpy()
    decoder = GaussTaylorKeyPointDecoder()
    if args.flip_test:
        return flip_test_bench(args, det, img, decoder)
    out = {"device": torch.cuda.get_device_name(0), "source": [640, 640], "detector": "s fp32", "capacity": CAPACITY, "detections": int(scores.size),
           "reps": reps, "pose_autotune": False, "runs": []}
    models = [("dconv", "fp32")] if args.quick else [("dconv", "fp32"), ("duc", "bf16")]
    for head, dtype in models:
        model = pose_model(head, dtype)
        for n_want in ((32,) if args.quick else (1, 8, 32)):
            if scores.size < n_want:
                continue
            # the detections come out in descending score order: a threshold between the n-th and the next keeps exactly n
            min_score = 0.0 if n_want >= min(CAPACITY, scores.size) else float((np.float64(scores[n_want - 1]) + np.float64(scores[n_want])) / 2)
            est = TopDownPoseEstimator(det, model, decoder=decoder, capacity=CAPACITY, min_box_score=min_score)
            variants = {
                "staged": lambda: staged_frame(det, model, decoder, img, dev_img, min_score),
                "eager": lambda: (setattr(est, "use_graph", False), est.estimate(img))[1],
                "graph": lambda: (setattr(est, "use_graph", True), est.estimate(img))[1],
                "staged2": lambda: staged_frame(det, model, decoder, img, dev_img, min_score),
            }
            want, n_live = variants["staged"]()
            same = all(variants[k]().coco(0) == want for k in ("eager", "graph"))
            times = {k: [] for k in variants}
            for r in range(warm + reps):
                for k, fn in variants.items():
                    t = wall_ms(fn)
                    if r >= warm:
                        times[k].append(t)
            run = {"pose": f"resnet50-{head} {dtype}", "n_live": n_live, "min_box_score": min_score, "results_equal_staged": bool(same),
                   "poses_kept": len(want)}
            run.update({k: summary(v) for k, v in times.items()})
            run["staged_self_spread_ms"] = abs(run["staged"]["median_ms"] - run["staged2"]["median_ms"])
            run["graph_minus_staged_ms"] = run["graph"]["median_ms"] - run["staged"]["median_ms"]
            out["runs"].append(run)
            print(json.dumps(run), flush=True)
    if not args.quick:
        if os.path.isfile(args.out):                             # a --flip-test run's results live in the same file
            with open(args.out) as fh:
                out.update({k: v for k, v in json.load(fh).items() if k == "flip_test"})
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
