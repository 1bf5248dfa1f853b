"""tools/gen_golden_detector.py - TEST INFRASTRUCTURE.  Run in the build container (needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_detector.py [--check]

g14_detector.npz: the reference's YOLOv5 detector (detector/nets/yolov5.py, detector/yolov5_detector.py) imported as it is.  Three
in-memory stubs stand in for what is not installed: torchvision.ops.boxes.nms (tests/detector_ref.greedy_nms_np, the written-out greedy scan)
and cv.resize / cv.copyMakeBorder (the numpy restatement of tests/detector_ref).  The models are built under torch.no_grad() (the head's
in-place bias edit raises otherwise on current torch).  Weights: tests/detector_ref.detector_state_dict (synth.conditioned_state_dict, head x HEAD_GAIN); the fixture stores none.

Contents: the key lists / parameter counts of the s and l models; one s forward of a 432x640 image (r == 1: letterboxed to 448x640 without a
resize, so the forward parity does not depend on the resize restatement) - the full sliced [N, 6] output, the 85-column output on every
ROW_STEP-th row and single_predict's detections; non_max_suppression on synthetic clustered predictions (merge on / off, two thresholds, one
case keeping more than 300 boxes); make_border geometry for a list of sizes.  Every threshold is chosen so that no candidate score lies
within MARGIN of conf_thresh and no IoU the reference compares lies within MARGIN of iou_thresh.
"""
from __future__ import annotations

import importlib
import io
import os
import sys
import types
import zipfile

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from oracle import ref_import  # noqa: E402
from tests import detector_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g14_detector.npz")
SEED = 14
MARGIN = 1e-3
TIE = 1e-5          # candidate scores closer than this may swap places between fp32 forwards (measured forward error ~1e-6 of max)
ROW_STEP = 61
SRC_HW = (432, 640)
BORDER_SIZES = [(432, 640), (480, 640), (640, 480), (375, 500), (1080, 1920), (300, 301), (720, 1280), (1280, 1280), (200, 900)]


def load_reference():
    ref_import._install_stubs()
    cv2 = sys.modules["cv2"]
    cv2.INTER_LINEAR, cv2.BORDER_CONSTANT = 1, 0
    cv2.resize = lambda img, dsize, interpolation=1: detector_ref.resize_np(img, dsize[0], dsize[1])
    cv2.copyMakeBorder = lambda img, t, b, l, r, kind, value=(0, 0, 0): detector_ref.copy_make_border_np(img, t, b, l, r, value)
    tv = types.ModuleType("torchvision")
    ops = types.ModuleType("torchvision.ops")
    boxes = types.ModuleType("torchvision.ops.boxes")
    boxes.nms = lambda b, s, thr: torch.from_numpy(detector_ref.greedy_nms_np(b.numpy().astype(np.float32), s.numpy().astype(np.float32), thr))
    tv.ops, ops.boxes = ops, boxes
    sys.modules.update({"torchvision": tv, "torchvision.ops": ops, "torchvision.ops.boxes": boxes})
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    return importlib.import_module("detector.nets.yolov5"), importlib.import_module("detector.yolov5_detector")


def source_image(hw=SRC_HW, cell=16):
    """Blocky uint8 BGR image (cell x cell squares of random colour): compresses to a few kB."""
    rng = np.random.default_rng(SEED + hw[0])
    h, w = hw
    cells = rng.integers(0, 256, (h // cell, w // cell, 3), dtype=np.uint8)
    return np.repeat(np.repeat(cells, cell, 0), cell, 1)


def pick_threshold(values, lo, hi, step=0.005):
    """The first threshold in [lo, hi) with no value within MARGIN."""
    v = np.asarray(values, dtype=np.float64).ravel()
    for t in np.arange(lo, hi, step):
        if not (np.abs(v - t) < MARGIN).any():
            return float(round(t, 6))
    raise RuntimeError(f"no threshold in [{lo}, {hi}) keeps a {MARGIN} margin")


def candidate_scores(pred, conf):
    """Every value compared with conf_thresh: obj of each row, cls*obj of rows with obj > conf."""
    vals = [pred[..., 4].ravel()]
    for x in pred.astype(np.float32):
        x = x[x[:, 4] > np.float32(conf)]
        vals.append((x[:, 5:] * x[:, 4:5]).ravel())
    return np.concatenate(vals)


def compared_ious(pred, conf, merge):
    """Every IoU the reference compares with iou_thresh (all same-class candidate pairs: a superset)."""
    _, cands = detector_ref.nms_np(pred, conf, 0.5, merge=merge, return_candidates=True, max_det=10 ** 6)
    out = []
    for c in cands:
        if c is None:
            continue
        boxes, _ = c
        for i in range(len(boxes)):
            out.append(detector_ref._iou_f32(boxes[i], boxes))
    return np.concatenate(out) if out else np.zeros(0)


def pick_iou(pred, conf, lo, hi, step=0.0005, max_det=300):
    """The first iou_thresh in [lo, hi) that lies MARGIN away from every IoU deciding the single-image result at that threshold: each of the
    first max_det boxes the greedy scan keeps against every candidate (the scan's decisions up to the max_det-th kept box and the merge
    compare nothing else)."""
    _, cands = detector_ref.nms_np(pred, conf, 0.5, return_candidates=True)
    boxes, scores = cands[0]
    for t in np.arange(lo, hi, step):
        kept = detector_ref.greedy_nms_np(boxes, scores, t, limit=max_det)
        v = np.concatenate([detector_ref._iou_f32(boxes[k], boxes) for k in kept])
        if not (np.abs(v.astype(np.float64) - t) < MARGIN).any():
            return float(round(t, 6))
    raise RuntimeError(f"no iou_thresh in [{lo}, {hi}) keeps a {MARGIN} margin")


def check_ties(pred, conf, iou, max_det=300):
    """Candidates whose scores lie within TIE of each other may come out in either order from another fp32 forward.  Among the candidates the
    greedy scan visits up to its max_det-th kept box, no such pair may overlap (IoU within MARGIN of iou_thresh or above), and the last kept
    box may not tie with the next one: then a swap only reorders rows inside a tie group, and the kept set and merged boxes stay the same."""
    _, cands = detector_ref.nms_np(pred, conf, iou, return_candidates=True)
    boxes, sc = cands[0]
    order = np.lexsort((np.arange(len(sc)), -sc.astype(np.float64)))
    kept = detector_ref.greedy_nms_np(boxes, sc, iou, limit=max_det + 1)
    rank = np.empty(len(sc), np.int64)
    rank[order] = np.arange(len(sc))
    pre = order[:rank[kept[:max_det]].max() + 1]
    ss = sc[pre].astype(np.float64)
    for i in range(len(pre)):
        j = i + 1
        while j < len(pre) and ss[i] - ss[j] < TIE:
            assert detector_ref._iou_f32(boxes[pre[i]], boxes[pre[j]][None])[0] <= iou - MARGIN, "overlapping candidates with tied scores"
            j += 1
    if len(kept) > max_det:
        assert sc[kept[max_det - 1]] - sc[kept[max_det]] >= TIE, "the max_det-th kept box ties with the next one"


def check_margins(pred, conf, iou, merge):
    s = candidate_scores(pred, conf)
    assert not (np.abs(s - conf) < MARGIN).any(), "a candidate lies within the margin of conf_thresh"
    ious = compared_ious(pred, conf, merge)
    assert not (np.abs(ious - iou) < MARGIN).any(), "an IoU lies within the margin of iou_thresh"


def synthetic_predictions(rng, n_clusters, per_cluster, nc, spread, img=640.0):
    """[N, 5 + nc] xywh + obj + cls probabilities: clusters of jittered boxes around random centres."""
    rows = []
    for _ in range(n_clusters):
        cx, cy = rng.uniform(20, img - 20, 2)
        w, h = rng.uniform(10, 120, 2)
        cls = rng.integers(0, nc)
        for _ in range(per_cluster):
            r = np.zeros(5 + nc, dtype=np.float32)
            r[0:2] = (cx, cy) + rng.normal(0, spread, 2) * (w, h)
            r[2:4] = (w, h) * np.exp(rng.normal(0, spread, 2))
            r[4] = rng.uniform(0.05, 1.0)
            r[5:] = rng.uniform(0.0, 0.05, nc)
            r[5 + cls] = rng.uniform(0.3, 1.0)
            rows.append(r)
    x = np.stack(rows).astype(np.float32)
    return x[rng.permutation(len(x))]


def build():
    yolo, det = load_reference()
    out = {}
    with torch.no_grad():
        ms = yolo.YOLOv5(scale_name="s", num_cls=80)
        ml = yolo.YOLOv5(scale_name="l", num_cls=80)
    for name, m in (("s", ms), ("l", ml)):
        out[f"keys_{name}"] = np.asarray(list(m.state_dict().keys()))
        out[f"params_{name}"] = np.int64(sum(p.numel() for p in m.parameters()))
        out[f"shapes_{name}"] = np.asarray([",".join(str(d) for d in v.shape) for v in m.state_dict().values()])
    # ---- s forward + single_predict ----
    sd = detector_ref.detector_state_dict(ms, SEED)
    img = source_image()
    orig_load = torch.load
    torch.load = lambda path, map_location=None: {"ema": sd}
    try:
        with torch.no_grad():
            d = det.YOLOv5Detector("conditioned", num_cls=80, scale_name="s", scale_size=(640, 640), device="cpu", iou_thresh=0.6, conf_thresh=0.001,
                                   slice_idx=0)
    finally:
        torch.load = orig_load
    canvas, ratio, (left, top) = d.transform.make_border(img)
    assert ratio == (1.0, 1.0) and canvas.shape == (448, 640, 3)
    x = torch.from_numpy(np.ascontiguousarray(canvas[:, :, [2, 1, 0]].transpose(2, 0, 1))).unsqueeze(0).div(255.0)
    with torch.no_grad():
        sliced = d.model(x)
        ms.load_state_dict(sd)
        full = ms.eval()(x)
    # single_predict cases on real network output.  conf_thresh lies below every obj value (obj is dense in [0.13, 0.66]: no threshold
    # inside that range keeps the margin), so the margin is needed on cls * obj only; the IoUs checked are exactly those that decide the
    # output - each of the first max_det kept boxes against every candidate (the greedy prefix and the merge).
    # a: the 432x640 image (r == 1, top = 8): > 3000 candidates, no merge.  b: a 50x800 image resized to 40x640 (r = 0.8, top = 12) on a
    # 64x640 canvas (2520 rows): < 3000 candidates, merge and the redundancy filter run.
    out["pred_sliced"] = sliced[0].numpy().astype(np.float32)
    out["pred85_rows"] = np.arange(0, full.shape[1], ROW_STEP)
    out["pred85"] = full[0, ::ROW_STEP].numpy().astype(np.float32)
    for tag, im in (("a", img), ("b", source_image((50, 800), 10))):
        canvas, _, _ = d.transform.make_border(im)
        xb = torch.from_numpy(np.ascontiguousarray(canvas[:, :, [2, 1, 0]].transpose(2, 0, 1))).unsqueeze(0).div(255.0)
        with torch.no_grad():
            pred = d.model(xb).numpy()
        obj_min = float(pred[0, :, 4].min())
        cls_obj = (pred[0, :, 5] * pred[0, :, 4]).astype(np.float32)
        conf = pick_threshold(cls_obj, 0.02, obj_min - 2 * MARGIN, step=0.001)
        assert not (np.abs(candidate_scores(pred, conf) - conf) < MARGIN).any()
        iou = pick_iou(pred, conf, 0.3, 0.9)
        n = int((cls_obj > np.float32(conf)).sum())
        assert (n >= 3000) if tag == "a" else (1 < n < 3000), (tag, n)
        check_ties(pred, conf, iou)
        d.conf_thresh, d.iou_thresh = conf, iou
        boxes = d.single_predict(im)
        assert not isinstance(boxes, list) and boxes.shape[0] > 0, f"single_predict case {tag} finds nothing"
        out[f"sp_{tag}_image"] = im
        out[f"sp_{tag}_thresh"] = np.asarray([conf, iou, TIE], dtype=np.float64)
        out[f"sp_{tag}_dets"] = boxes.numpy().astype(np.float32)
        out[f"sp_{tag}_pred"] = pred[0].astype(np.float32) if tag == "b" else np.zeros((0, 6), np.float32)
    # ---- synthetic NMS ----
    rng = np.random.default_rng(SEED)
    cases = [  # (name, clusters, per cluster, classes, spread, conf, iou, merge, max_det)
        ("merge_a", 24, 9, 3, 0.08, 0.3, 0.5, True, 300),
        ("plain_a", 24, 9, 3, 0.08, 0.3, 0.5, False, 300),
        ("merge_b", 30, 7, 80, 0.12, 0.12, 0.65, True, 300),
        ("plain_b", 30, 7, 80, 0.12, 0.12, 0.65, False, 300),
        ("many", 420, 2, 4, 0.01, 0.2, 0.45, True, 300),
    ]
    nms_mod = det.non_max_suppression
    for name, ncl, per, nc, spread, conf0, iou0, merge, max_det in cases:
        for attempt in range(50):
            p = synthetic_predictions(rng, ncl, per, nc, spread)[None]
            try:
                conf = pick_threshold(candidate_scores(p, conf0), conf0, conf0 + 0.1)
                iou = pick_threshold(compared_ious(p, conf, merge), iou0, iou0 + 0.1)
                check_margins(p, conf, iou, merge)
                break
            except (RuntimeError, AssertionError):
                continue
        else:
            raise RuntimeError(f"{name}: no margin-clean draw")
        r = nms_mod(torch.from_numpy(p.copy()), conf_thresh=conf, iou_thresh=iou, merge=merge, max_det=max_det)[0]
        r = np.zeros((0, 6), np.float32) if r is None else r.numpy().astype(np.float32)
        if name == "many":
            kept = detector_ref.nms_np(p, conf, iou, merge=False, max_det=10 ** 6)[0]
            assert kept is not None and len(kept) > 300, "the 'many' case must keep more than max_det boxes"
        out[f"nms_{name}_pred"] = p
        out[f"nms_{name}_args"] = np.asarray([conf, iou, float(merge), float(max_det)], dtype=np.float64)
        out[f"nms_{name}_out"] = r
    # ---- make_border geometry ----
    geo = []
    for h, w in BORDER_SIZES:
        t = det.ScalePadding(target_size=(640, 640), minimum_rectangle=True, padding_val=(114, 114, 114))
        c, (r, _), (l, tp) = t.make_border(np.zeros((h, w, 3), np.uint8))
        geo.append([h, w, c.shape[0], c.shape[1], l, tp, r])
    out["border"] = np.asarray(geo, dtype=np.float64)
    return out


def write(arrays, path):
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(2020, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, b.getvalue())
    data = buf.getvalue()
    if path:
        with open(path, "wb") as fh:
            fh.write(data)
    return data


if __name__ == "__main__":
    arrays = build()
    if "--check" in sys.argv:
        same = open(OUT, "rb").read() == write(arrays, None)
        print("g14 up to date" if same else "g14 differs")
        sys.exit(0 if same else 1)
    write(arrays, OUT)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: getattr(v, "shape", ()) for k, v in arrays.items() if k.startswith(("sp_", "nms_")) and k.endswith(("out", "dets"))})
