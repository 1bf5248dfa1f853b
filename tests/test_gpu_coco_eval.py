"""Keypoint evaluator on the MI355X (csrc/cocoeval.hip behind simple_pose_amd.metrics.coco_eval) against the CPU checker
tests/coco_eval_ref.py on one seeded set that holds every situation at once (see make_dataset).

Bars.  OKS: 1e-12 absolute.  Both sides evaluate the same float64 operations in the same order; the one function that is not shared
bit for bit is exp, at most 1 ulp per term on either side, about 1e-16 on values in [0, 1]; the bar sits four orders above that and
three below the 1e-9 band the data keeps clear of every threshold (a precondition checked on the CPU, not a tolerance).  Everything
downstream - matches, ignore flags, precision, recall, the ten stats - is integer decisions and IEEE divisions of integer counts:
equal, bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib
from simple_pose_amd.metrics import KeypointEvaluator, KeypointGroundTruth, evaluate_map
from simple_pose_amd.metrics import coco_eval
from simple_pose_amd.metrics.pose_metrics import kps_to_dict_
from tests import coco_eval_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, N_IMAGES = 20, 300
OKS_BAR = 1e-12


@pytest.fixture(scope="module")
def data():
    gt, results, arrays = ref.make_dataset(SEED, n_images=N_IMAGES)
    want = ref.evaluate(gt, results)
    assert ref.threshold_margin(want["oks"]) > 1e-9, "precondition: change SEED, not the margin"
    return gt, results, arrays, want


def _assert_equal(ev, want, measured=None):
    worst = 0.0
    for image_id in ev.gt.image_ids.tolist():
        assert ev.oks[image_id].shape == want["oks"][image_id].shape, image_id
        if want["oks"][image_id].size:
            worst = max(worst, float(np.abs(ev.oks[image_id] - want["oks"][image_id]).max()))
        assert np.array_equal(ev.dt_ids[image_id], want["dt_ids"][image_id]), image_id
        assert np.array_equal(ev.dtm[image_id], want["dtm"][image_id]), image_id
        assert np.array_equal(ev.dt_ignore[image_id], want["dt_ignore"][image_id]), image_id
        assert np.array_equal(ev.gt_ignore[image_id], want["gt_ignore"][image_id]), image_id
    if measured is not None:
        measured("oks_max_abs_diff", worst, OKS_BAR)
    assert worst <= OKS_BAR
    np.testing.assert_array_equal(ev.precision, want["precision"])
    np.testing.assert_array_equal(ev.recall, want["recall"])
    np.testing.assert_array_equal(ev.stats, want["stats"])


def test_evaluator_equals_cpu_restatement(data, measured):
    gt, results, _, want = data
    ev = KeypointEvaluator(KeypointGroundTruth(gt), device=DEV)
    ev.add_results(results)
    stats = ev.evaluate()
    assert list(stats) == ref.STAT_NAMES and ev.precision.shape == (10, 101, 3) and ev.recall.shape == (10, 3)
    assert sum(len(v) for v in ev.dt_ids.values()) < len(results)                   # the cut to 20 really cut something
    _assert_equal(ev, want, measured)
    assert [stats[k] for k in ref.STAT_NAMES] == want["stats"].tolist()


def test_input_routes_agree(data, tmp_path):
    """Decoder tensors -> add(); the same tensors -> kps_to_dict_ -> JSON -> add_results(); the same JSON -> evaluate_map(path, path)."""
    gt, _, (xy, mv, _, img_ids), _ = data
    kps, maxvals = torch.from_numpy(xy).to(DEV), torch.from_numpy(mv).to(DEV)
    maxvals[1::7] = maxvals[0:-1:7][: maxvals[1::7].shape[0]]                     # repeated rows: tied result scores
    dicts = []
    kps_to_dict_(kps, maxvals[:, :, None], img_ids, dicts)
    res_path, ann_path = tmp_path / "res.json", tmp_path / "ann.json"
    res_path.write_text(json.dumps(dicts))
    ann_path.write_text(json.dumps(gt))
    loaded = json.loads(res_path.read_text())
    want = ref.evaluate(gt, loaded)
    assert ref.threshold_margin(want["oks"]) > 1e-9
    truth = KeypointGroundTruth(gt)
    a = KeypointEvaluator(truth)
    half = len(img_ids) // 2
    a.add(kps[:half], maxvals[:half], img_ids[:half])                               # two batches, [P,J,2] + [P,J] and [P,J,3]
    a.add(torch.cat([kps[half:], maxvals[half:, :, None]], -1), None, img_ids[half:])
    a.evaluate()
    b = KeypointEvaluator(truth)
    b.add_results(loaded)
    b.evaluate()
    for ev in (a, b):
        _assert_equal(ev, want)
    info = evaluate_map(str(res_path), str(ann_path))
    assert list(info) == ref.STAT_NAMES and [info[k] for k in ref.STAT_NAMES] == want["stats"].tolist()
    mixed = KeypointEvaluator(truth)                                                # a device batch and a list of dicts in one evaluation
    mixed.add(kps[:half], maxvals[:half], img_ids[:half])
    mixed.add_results(loaded[half:])
    mixed.evaluate()
    _assert_equal(mixed, want)
    supplied = KeypointEvaluator(truth)                                             # caller-supplied scores
    supplied.add(kps, None, img_ids, score=torch.tensor([d["score"] for d in loaded], dtype=torch.float64, device=DEV))
    supplied.evaluate()
    _assert_equal(supplied, want)


def test_custom_sigmas_and_joint_count():
    rng = np.random.default_rng(5)
    J, sig = 5, np.array([0.03, 0.05, 0.08, 0.1, 0.06])
    anns, results = [], []
    for n in range(12):
        k = np.concatenate([rng.uniform(50, 300, (J, 2)).round(), rng.integers(0, 3, (J, 1))], 1)
        k[0, 2] = 2
        anns.append({"id": n + 1, "image_id": n % 4, "keypoints": k.reshape(-1).tolist(), "num_keypoints": int((k[:, 2] > 0).sum()),
                     "bbox": [50.0, 50.0, 250.0, 250.0], "area": float(rng.uniform(500, 40000)), "iscrowd": 0})
        p = np.concatenate([(k[:, :2] + rng.normal(0, 6, (J, 2))).astype(np.float32), np.ones((J, 1), np.float32)], 1)
        results.append({"image_id": n % 4, "score": float(np.float32(rng.uniform())), "category_id": 1, "keypoints": [float(v) for v in p.reshape(-1)]})
    gt = {"images": [{"id": i} for i in range(5)], "annotations": anns}
    want = ref.evaluate(gt, results, sigmas=sig)
    assert ref.threshold_margin(want["oks"]) > 1e-9
    with pytest.raises(ValueError):
        KeypointEvaluator(KeypointGroundTruth(gt))
    ev = KeypointEvaluator(KeypointGroundTruth(gt), sigmas=sig)
    ev.add_results(results)
    ev.evaluate()
    _assert_equal(ev, want)


def test_no_detections_and_no_ground_truth():
    gt, results, _ = ref.make_dataset(1, n_images=30)
    ev = KeypointEvaluator(KeypointGroundTruth(gt), device=DEV)
    ev.evaluate()
    _assert_equal(ev, ref.evaluate(gt, []))
    assert ev.stats[0] == 0 and ev.stats[5] == 0
    empty = {"images": gt["images"], "annotations": []}
    ev = KeypointEvaluator(KeypointGroundTruth(empty), device=DEV)
    ev.add_results(results)
    ev.evaluate()
    _assert_equal(ev, ref.evaluate(empty, results))
    assert np.array_equal(ev.stats, -np.ones(10))


def test_capacity_overflow_raises():
    gt, results, _ = ref.make_dataset(1, n_images=30)
    one = results[0]
    ev = KeypointEvaluator(KeypointGroundTruth(gt), device=DEV)
    ev.add_results([one] * (_lib.SP_COCO_MAX_DT_PER_IMAGE + 1))
    with pytest.raises(_lib.HipLibraryError, match="detections in one image"):
        ev.evaluate()
    ev = KeypointEvaluator(KeypointGroundTruth(gt), device=DEV)
    ev.add_results([one] * _lib.SP_COCO_MAX_DT_PER_IMAGE)                            # exactly the capacity is evaluated
    ev.evaluate()
    assert len(ev.dt_ids[one["image_id"]]) == 20 and ev.dt_ids[one["image_id"]].tolist() == list(range(1, 21))
    a = gt["annotations"][0]
    crowd = {"images": gt["images"], "annotations": [dict(a, id=n + 1) for n in range(_lib.SP_COCO_MAX_GT_PER_IMAGE + 1)]}
    ev = KeypointEvaluator(KeypointGroundTruth(crowd), device=DEV)
    ev.add_results([one])
    with pytest.raises(_lib.HipLibraryError, match="ground truths in one image"):
        ev.evaluate()


def test_kernel_reports_overflow_the_host_did_not_announce():
    """The host-side maxima are a courtesy; the kernel checks its own capacity: dt_count -1 for the image, its neighbours untouched."""
    lib, P = _lib.lib(), _lib.ptr
    n = _lib.SP_COCO_MAX_DT_PER_IMAGE + 1
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
    gt_seg = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
    dt_seg = torch.tensor([0, n, n + 1], dtype=torch.int32, device=DEV)
    kps = torch.ones((2, 17, 3), dtype=torch.float64, device=DEV)
    xy, score = z((n + 1, 17, 2), torch.float32), z((n + 1,), torch.float32)
    count, keep = z((2,), torch.int32), z((40,), torch.int32)
    rc = lib.sp_coco_kp_eval_images(P(gt_seg), P(kps), P(z((2,), torch.float64) + 100), P(z((2, 4), torch.float64)), P(z((2,), torch.int32)), P(dt_seg),
                                    None, P(xy), P(score), 0, 2, 2, 1, 1, 17, None, 20, coco_eval._dptr(coco_eval.IOU_THRS), 10,
                                    coco_eval._dptr(coco_eval.AREA_RNG), 3, P(count), P(keep), P(z((40,), torch.float64)), P(z((40,), torch.float64)),
                                    P(z((40,), torch.float64)), P(z((3, 10, 40), torch.int32)), P(z((3, 10, 40), torch.uint8)),
                                    P(z((3, 2), torch.uint8)), _lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert count.tolist() == [-1, 1] and keep.tolist() == [-1] * 20 + [n] + [-1] * 19


def test_bad_arguments_do_not_launch():
    lib = _lib.lib()
    count = torch.full((4,), 7, dtype=torch.int32, device=DEV)
    p = _lib.ptr(count)
    thr, rng = coco_eval._dptr(coco_eval.IOU_THRS), coco_eval._dptr(coco_eval.AREA_RNG)
    rc = lib.sp_coco_kp_eval_images(p, p, p, p, p, p, None, p, p, 0, 4, 1, 1, 1, 17, None, 64, thr, 10, rng, 3, p, p, p, p, p, p, p, p, _lib.current_stream())
    assert rc == -1 and b"max_dets" in lib.sp_last_error()
    rc = lib.sp_coco_kp_accumulate(p, p, p, p, p, 4, 1, 20, 10, 3, coco_eval._dptr(coco_eval.REC_THRS), 101, p, 16, p, p, _lib.current_stream())
    assert rc == -1 and b"workspace" in lib.sp_last_error()
    torch.cuda.synchronize()
    assert count.tolist() == [7, 7, 7, 7]


# ---- the solver ---------------------------------------------------------------------------------------------------------------------------
def _solver_cfg(tmp_path, name):
    import yaml
    cfg = {"model_name": name, "gpus": "0",
           "data": {"synthetic": 8, "batch_size": 4, "num_workers": 0, "debug": False},
           "model": {"type": "pose_resnet_dconv", "name": "resnet50", "num_joints": 17, "pretrained": False},
           "optim": {"lr": 1e-3, "amp": False, "sync_bn": False, "milestones": [1], "epochs": 1, "gamma": 0.1},
           "val": {"interval": 1, "weight_path": str(tmp_path / "w")}}
    path = tmp_path / (name + ".yaml")
    path.write_text(yaml.safe_dump(cfg))
    return str(path)


def _gt_of_loader(loader):
    """Annotations from the loader's own targets: the arg-max of every target heat map, mapped to image pixels."""
    from simple_pose_amd.metrics import BasicKeyPointDecoder
    images, anns = [], []
    for _, heat_maps, masks, trans_inv, ids in loader:
        kps, _ = BasicKeyPointDecoder()(heat_maps, trans_inv.float())
        kps, vis = kps.cpu().numpy().astype(np.float64), masks.cpu().numpy() > 0
        for k, v, image_id in zip(kps, vis, ids):
            full = np.concatenate([k, np.where(v, 2.0, 0.0)[:, None]], 1)
            full[~v] = 0
            x0, y0 = k.min(0)
            w, h = k.max(0) - k.min(0)
            images.append({"id": image_id})
            anns.append(ref.annotation(len(anns) + 1, image_id, full, (x0, y0, w, h), max(float(w * h), 1.0)))
    return {"images": images, "annotations": anns}


def test_solver_reports_ap_and_writes_the_best_checkpoint(tmp_path):
    from simple_pose_amd.processors.ddp_pose_resnet_solver import DDPProcessor
    plain = DDPProcessor(_solver_cfg(tmp_path, "plain"))
    out = plain.val(0)
    assert out["val_ap"] is None and plain.best_map == 0.0                          # no ground truth: as before
    assert os.path.isfile(tmp_path / "w" / "plain_last.pth") and not os.path.isfile(tmp_path / "w" / "plain_best.pth")
    gt = _gt_of_loader(plain.vloader)
    proc = DDPProcessor(_solver_cfg(tmp_path, "dict"), val_loader=plain.vloader, val_gt=gt)
    proc.best_map = -1.0                                                            # an untrained network may well score AP 0: any AP must register
    out = proc.val(0)
    assert isinstance(out["val_ap"], float) and 0.0 <= out["val_ap"] <= 1.0
    assert proc.best_map == out["val_ap"] and os.path.isfile(tmp_path / "w" / "dict_best.pth")
    dicts = []                                                                      # the same number from the dicts val() builds
    proc.model.eval()
    with torch.no_grad():
        for x, _, _, tinv, ids in proc.vloader:
            k, s = proc.decoder(proc.model(x), tinv.float())
            kps_to_dict_(k, s, ids, dicts)
    proc.model.train()
    assert out["results"] == len(dicts) and ref.evaluate(gt, json.loads(json.dumps(dicts)))["stats"][0] == out["val_ap"]
    ann = tmp_path / "ann.json"                                                     # the same through data.val_ann_path
    ann.write_text(json.dumps(gt))
    proc.val_gt, proc.data_cfg["val_ann_path"], proc.best_map = None, str(ann), -1.0
    again = proc.val(1)
    assert again["val_ap"] == out["val_ap"] and isinstance(proc.val_gt, KeypointGroundTruth) and proc.best_map == out["val_ap"]


# ---- the estimator's output -----------------------------------------------------------------------------------------------------------------
def test_estimator_results_through_evaluate_map(golden):
    from tests.test_gpu_pipeline import G, _pose_model
    from simple_pose_amd.detector.nets.yolov5 import YOLOv5
    from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
    from simple_pose_amd.pipeline import TopDownPoseEstimator
    from tests.detector_ref import detector_state_dict
    det = YOLOv5Detector(num_cls=80, scale_name="s", device=DEV, slice_idx=0, state_dict=detector_state_dict(YOLOv5(scale_name="s", num_cls=80), 14))
    conf, iou, _ = golden(G)["sp_a_thresh"]
    det.conf_thresh, det.iou_thresh = float(conf), float(iou)
    est = TopDownPoseEstimator(det, _pose_model("dconv_fp32"), capacity=32)
    res = est.estimate(golden(G)["sp_a_image"])
    assert len(res) >= 1
    results = res.coco(7) + [dict(d, image_id=9) for d in res.coco(7)[:2]]
    rng = np.random.default_rng(11)
    anns = []
    for n, k in enumerate(res.keypoints):                                           # ground truth = the poses, disturbed at two scales
        box = (k[:, 0].min(), k[:, 1].min(), np.ptp(k[:, 0]), np.ptp(k[:, 1]))
        area = max(float(box[2] * box[3]), 1.0)
        full = np.concatenate([np.round(k[:, :2] + rng.normal(0, (0.02, 0.1)[n % 2] * np.sqrt(area), (17, 2))), np.full((17, 1), 2.0)], 1)
        anns.append(ref.annotation(n + 1, 7, full, box, area))
    gt = {"images": [{"id": 7}, {"id": 9}, {"id": 11}], "annotations": anns}
    want = ref.evaluate(gt, results)
    assert ref.threshold_margin(want["oks"]) > 1e-9
    info = evaluate_map(results, gt)
    assert [info[k] for k in ref.STAT_NAMES] == want["stats"].tolist()
    ev = coco_eval.evaluate_keypoints(results, gt)
    _assert_equal(ev, want)
