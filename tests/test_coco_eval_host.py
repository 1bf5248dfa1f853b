"""Keypoint evaluator, the part that needs no GPU: anchors that pin the CPU checker (tests/coco_eval_ref.py) to values known without
it - so that the kernels and their checker cannot share a misreading - and the host side of the package (header, bindings, ground
truth parsing, argument errors)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from simple_pose_amd import _lib
from simple_pose_amd.metrics import KeypointEvaluator, KeypointGroundTruth, evaluate_map
from simple_pose_amd.metrics import coco_eval
from tests import coco_eval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sp_coco_kp_eval_images", "sp_coco_kp_accumulate_workspace", "sp_coco_kp_accumulate")


def _det(a, score, shift=0.0):
    k = np.asarray(a["keypoints"], np.float64).reshape(17, 3)
    return ref.result(a["image_id"], k[:, :2] + shift, np.ones(17), score)


def _people(seed, sizes, image_id=1, first_id=1):
    """One fully visible person per entry of `sizes` (box height in px), side by side."""
    rng = np.random.default_rng(seed)
    out, x = [], 10.0
    for n, h in enumerate(sizes):
        w = h * 0.5
        k = ref.person(rng, x, 20.0, w, h, vis_prob=1.0)
        out.append(ref.annotation(first_id + n, image_id, k, (x, 20.0, w, h), 0.7 * w * h))
        x += w + 40
    return out


# ---- anchors of the checker -----------------------------------------------------------------------------------------------------------------
def test_identical_detections_give_ap_one():
    anns = _people(0, [20, 60, 200, 25, 80, 300])                                 # two small, two medium, two large
    gt = {"images": [{"id": 1}], "annotations": anns}
    out = ref.evaluate(gt, [_det(a, 0.9 - 0.1 * n) for n, a in enumerate(anns)])
    assert np.abs(out["stats"] - 1).max() <= 1e-12
    assert (out["stats"][5:] == 1).all()                                          # AR: n / n
    one = ref.evaluate({"images": [{"id": 1}], "annotations": anns[2:3]}, [_det(anns[2], 0.9)])
    assert one["stats"][0] == 1 / (1 + 2.0 ** -52) < 1                            # a single TP: exactly 1 is not reachable
    for oks in out["oks"].values():
        assert np.abs(np.diag(oks) - 1).max() <= 1e-15


def test_far_displaced_detections_give_zero():
    anns = _people(1, [60, 200, 80])
    gt = {"images": [{"id": 1}], "annotations": anns}
    out = ref.evaluate(gt, [_det(a, 0.9, shift=5000.0) for a in anns])
    assert np.array_equal(out["stats"], np.zeros(10))


def test_range_without_ground_truth_reports_minus_one():
    anns = _people(2, [200, 300])                                                 # large only
    gt = {"images": [{"id": 1}], "annotations": anns}
    out = ref.evaluate(gt, [_det(a, 0.9) for a in anns])
    assert out["stats"][3] == -1 and out["stats"][8] == -1                        # AP (M), AR (M)
    assert (out["precision"][:, :, 1] == -1).all() and (out["recall"][:, 1] == -1).all()
    assert abs(out["stats"][0] - 1) <= 1e-12 and abs(out["stats"][4] - 1) <= 1e-12
    crowd_only = [dict(a, iscrowd=1) for a in anns]
    out = ref.evaluate({"images": [{"id": 1}], "annotations": crowd_only}, [_det(a, 0.9) for a in anns])
    assert np.array_equal(out["stats"], -np.ones(10))


def test_hand_case_tp_fp_tp():
    """One image, two ground truths, three detections ranked TP, FP, TP at OKS 0.5: rc = 1/2, 1/2, 1; pr = 1, 1/2, 2/3 -> envelope
    1, 2/3, 2/3; recall thresholds 0 .. 0.5 (51 of them) read 1, the other 50 read 2/3."""
    a, b = _people(3, [200, 220])
    gt = {"images": [{"id": 1}], "annotations": [a, b]}
    dets = [_det(a, 0.9), _det(a, 0.8, shift=1.0), _det(b, 0.7, shift=1.0)]       # the second copy of `a` finds it taken; `b` is far from it
    out = ref.evaluate(gt, dets)
    oks = out["oks"][1]
    assert oks[1, 0] > 0.95 and oks[1, 1] < 0.5 and oks[2, 1] > 0.95 and oks[0, 1] < 0.5
    assert out["dtm"][1][0, 0].tolist() == [a["id"], 0, b["id"]]
    eps = 2.0 ** -52
    want = (51 * 1.0 / (1 + eps) + 50 * (2 / (1 + 2 + eps))) / 101
    assert abs(out["precision"][0, :, 0].mean() - (51 + 50 * (2 / 3)) / 101) <= 1e-12
    assert abs(out["precision"][0, :, 0].mean() - want) <= 1e-15
    assert out["recall"][0, 0] == 1.0
    assert abs(out["stats"][1] - (51 + 50 * (2 / 3)) / 101) <= 1e-12 and out["stats"][6] == 1.0


def test_crowd_absorbs_detections_without_false_positives():
    person, crowd = _people(4, [200, 240])
    crowd = dict(crowd, iscrowd=1)
    gt = {"images": [{"id": 1}], "annotations": [person, crowd]}
    dets = [_det(crowd, 0.8 - 0.1 * n, shift=0.1 * n) for n in range(4)] + [_det(person, 0.1)]       # the person's detection ranks last
    out = ref.evaluate(gt, dets)
    assert (out["dtm"][1][0, 0, :4] == crowd["id"]).all() and out["dt_ignore"][1][0, 0, :4].all()        # all four matched to the crowd
    assert out["dtm"][1][0, 0, 4] == person["id"] and not out["dt_ignore"][1][0, 0, 4]
    assert abs(out["stats"][0] - 1) <= 1e-12                                       # no false positive came of them
    plain = ref.evaluate({"images": [{"id": 1}], "annotations": [person, dict(crowd, iscrowd=0)]}, dets)
    assert plain["stats"][0] < 0.9                                                 # the same detections against a plain ground truth do cost


def test_zero_keypoint_ground_truth_uses_the_box_branch_and_is_ignored():
    person, = _people(5, [200])
    blank = ref.annotation(2, 1, np.zeros((17, 3)), (400.0, 100.0, 50.0, 100.0), 3500.0)
    assert blank["num_keypoints"] == 0
    gt = {"images": [{"id": 1}], "annotations": [blank, person]}
    rng = np.random.default_rng(5)
    inside = ref.result(1, np.stack([rng.uniform(360, 490, 17), rng.uniform(10, 290, 17)], 1), np.ones(17), 0.5)   # inside the doubled box
    out = ref.evaluate(gt, [_det(person, 0.9), inside])
    assert out["oks"][1][1, 0] == 1.0                                              # every distance 0 -> exp(0)
    assert out["gt_ignore"][1][:, 0].all()
    assert out["dtm"][1][0, 0].tolist() == [person["id"], blank["id"]] and out["dt_ignore"][1][0, 0].tolist() == [False, True]
    assert abs(out["stats"][0] - 1) <= 1e-12
    far = ref.result(1, np.full((17, 2), 600.0) + rng.uniform(0, 1, (17, 2)), np.ones(17), 0.5)
    got = ref.evaluate(gt, [far])["oks"][1][0, 0]                                 # x1 = 400 + 2 * 50: dx in [100, 101]; y1 = 300: dy in [300, 301]
    bound = [np.mean(np.exp(-(dx ** 2 + dy ** 2) / (2 * ref.SIGMAS) ** 2 / (3500.0 + 2.0 ** -52) / 2)) for dx, dy in ((101, 301), (100, 300))]
    assert bound[0] <= got <= bound[1] and 0 < got < 1


def test_detections_past_the_twentieth_never_count():
    anns = _people(6, [200])
    gt = {"images": [{"id": 1}], "annotations": anns}
    junk = [_det(anns[0], 0.9 - 0.01 * n, shift=5000.0) for n in range(20)]
    out = ref.evaluate(gt, junk + [_det(anns[0], 0.1)])                            # the only good detection is the 21st
    assert out["dt_ids"][1].tolist() == list(range(1, 21)) and out["stats"].tolist() == [0, 0, 0, -1, 0, 0, 0, 0, -1, 0]
    out = ref.evaluate(gt, junk[:19] + [_det(anns[0], 0.1)])                       # as the 20th it counts
    assert out["stats"][5] == 1.0 and out["stats"][0] > 0


def test_tied_scores_keep_list_order():
    anns = _people(7, [200])
    gt = {"images": [{"id": 1}, {"id": 2}], "annotations": anns}
    good, bad = _det(anns[0], 0.5), _det(anns[0], 0.5, shift=5000.0)
    first = ref.evaluate(gt, [good, bad, dict(bad, image_id=2)])
    second = ref.evaluate(gt, [bad, good, dict(bad, image_id=2)])
    assert first["dt_ids"][1].tolist() == [1, 2] and second["dt_ids"][1].tolist() == [1, 2]
    assert abs(first["stats"][0] - 1) <= 1e-12                                     # TP first: precision 1 up to recall 1
    assert abs(second["stats"][0] - 0.5) <= 1e-12                                  # FP first: precision 1/2 everywhere
    third = ref.evaluate(gt, [dict(bad, image_id=2), good])                        # across images the tie resolves in image-id order
    assert abs(third["stats"][0] - 1) <= 1e-12


# ---- the package's host side ----------------------------------------------------------------------------------------------------------------
def test_header_declares_and_bindings_bind_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(sp_\w+)\s*\(", hdr, flags=re.M))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS
    assert re.search(r"#define SP_ABI_VERSION 36\b", hdr) and _lib.ABI_VERSION == 36
    for name in ("SP_COCO_MAX_JOINTS", "SP_COCO_MAX_GT_PER_IMAGE", "SP_COCO_MAX_DT_PER_IMAGE", "SP_COCO_MAX_DETS"):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == getattr(_lib, name)
    handle = _lib.lib()
    assert handle.sp_abi_version() == 36
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name)


def test_bad_arguments_return_minus_one_on_the_host():
    lib, one = _lib.lib(), ctypes.c_void_p(16)
    nbytes = ctypes.c_int64(0)
    assert lib.sp_coco_kp_accumulate_workspace(5000, 20, 10, 3, ctypes.byref(nbytes)) == 0
    assert nbytes.value == 100000 * 4 + 30 * 100000 * 12
    assert lib.sp_coco_kp_accumulate_workspace(1, 64, 10, 3, ctypes.byref(nbytes)) == -1 and b"max_dets" in lib.sp_last_error()
    thr, rng = coco_eval._dptr(coco_eval.IOU_THRS), coco_eval._dptr(coco_eval.AREA_RNG)
    args = lambda **kw: [kw.get("ptr", one)] * 9 + [0, 1, 1, kw.get("max_gt", 1), kw.get("max_dt", 1), kw.get("joints", 17), None, kw.get("max_dets", 20),
                                                    thr, 10, rng, 3] + [one] * 8 + [None]
    assert lib.sp_coco_kp_eval_images(*args(ptr=None)) == -1 and b"null" in lib.sp_last_error()
    assert lib.sp_coco_kp_eval_images(*args(max_gt=129)) == -1 and b"ground truths in one image" in lib.sp_last_error()
    assert lib.sp_coco_kp_eval_images(*args(max_dt=2049)) == -1 and b"detections in one image" in lib.sp_last_error()
    assert lib.sp_coco_kp_eval_images(*args(joints=16)) == -1 and b"sigmas" in lib.sp_last_error()
    assert lib.sp_coco_kp_eval_images(*args(max_dets=33)) == -1 and b"max_dets" in lib.sp_last_error()
    rec = coco_eval._dptr(coco_eval.REC_THRS)
    assert lib.sp_coco_kp_accumulate(one, one, one, one, one, 10, 5, 20, 10, 3, rec, 101, one, 8, one, one, None) == -1
    assert b"workspace" in lib.sp_last_error()


def test_parameters_are_cocoeval_s():
    assert np.array_equal(coco_eval.IOU_THRS, ref.IOU_THRS) and np.array_equal(coco_eval.REC_THRS, ref.REC_THRS)
    assert np.array_equal(coco_eval.AREA_RNG, np.array(ref.AREA_RNG)) and np.array_equal(coco_eval.COCO_SIGMAS, ref.SIGMAS)
    assert coco_eval.IOU_THRS[0] == 0.5 and coco_eval.IOU_THRS[5] == 0.75 and list(coco_eval.STAT_NAMES) == ref.STAT_NAMES
    p, r = np.random.default_rng(0).uniform(size=(10, 101, 3)), np.random.default_rng(1).uniform(size=(10, 3))
    p[:, :, 1] = -1
    assert np.array_equal(coco_eval.summarize(p, r), ref.summarize(p, r))


def test_ground_truth_parsing_matches_the_dict(tmp_path):
    gt, results, _ = ref.make_dataset(3, n_images=40)
    path = tmp_path / "ann.json"
    path.write_text(json.dumps(gt))
    for source in (gt, str(path)):
        g = KeypointGroundTruth(source)
        assert g.image_ids.tolist() == sorted(im["id"] for im in gt["images"]) and len(g) == len(gt["annotations"]) and g.num_joints == 17
        assert g.seg[0] == 0 and g.seg[-1] == len(g)
        for i, image_id in enumerate(g.image_ids.tolist()):
            mine = [a for a in gt["annotations"] if a["image_id"] == image_id]                # file order
            rows = slice(int(g.seg[i]), int(g.seg[i + 1]))
            assert g.ann_ids[rows].tolist() == [a["id"] for a in mine]
            assert np.array_equal(g.keypoints[rows].reshape(len(mine), 51), np.array([a["keypoints"] for a in mine]).reshape(len(mine), 51))
            assert g.area[rows].tolist() == [a["area"] for a in mine] and g.bbox[rows].tolist() == [a["bbox"] for a in mine]
            assert [bool(f & _lib.SP_COCO_GT_CROWD) for f in g.flag[rows]] == [bool(a["iscrowd"]) for a in mine]
            assert [bool(f & _lib.SP_COCO_GT_IGNORE) for f in g.flag[rows]] == [bool(a["iscrowd"]) or a["num_keypoints"] == 0 for a in mine]
        assert g.max_per_image == max(np.diff(g.seg))
    arr = KeypointGroundTruth.from_arrays(g.image_ids[::-1], np.repeat(g.image_ids, np.diff(g.seg)), g.keypoints, g.area, g.bbox,
                                          iscrowd=g.flag & 1, ann_ids=g.ann_ids)
    assert np.array_equal(arr.flag, g.flag) and np.array_equal(arr.seg, g.seg) and np.array_equal(arr.keypoints, g.keypoints)
    with pytest.raises(ValueError):
        KeypointGroundTruth({"images": [{"id": 1}], "annotations": [dict(gt["annotations"][0], image_id=-5)]})
    with pytest.raises(ValueError):
        KeypointGroundTruth({"images": [{"id": 1}, {"id": 1}], "annotations": []})


def test_unknown_image_id_raises():
    gt, results, _ = ref.make_dataset(3, n_images=20)
    ev = KeypointEvaluator(KeypointGroundTruth(gt))
    with pytest.raises(ValueError, match="image_id 999999"):
        ev.add_results([dict(results[0], image_id=999999)])
    with pytest.raises(ValueError, match="image_id 999999"):
        evaluate_map([dict(results[0], image_id=999999)], gt)
    with pytest.raises(ValueError):
        ref.evaluate(gt, [dict(results[0], image_id=999999)])
    assert len(ev) == 0


def test_wrong_ann_type_and_bad_construction_raise():
    gt, results, _ = ref.make_dataset(3, n_images=20)
    with pytest.raises(ValueError, match="keypoints"):
        evaluate_map(results, gt, ann_type="bbox")
    with pytest.raises(ValueError):
        KeypointEvaluator(KeypointGroundTruth(gt), max_dets=64)
    with pytest.raises(ValueError):
        KeypointEvaluator(KeypointGroundTruth(gt), sigmas=[0.1] * 5)
    with pytest.raises(ValueError):
        KeypointGroundTruth({"annotations": []})


def test_generator_covers_every_situation_and_keeps_clear_of_the_thresholds():
    """The data of the GPU comparison (seed and size as tests/test_gpu_coco_eval.py uses them), checked where no GPU is needed."""
    gt, results, _ = ref.make_dataset(ref_seed(), n_images=300)
    out = ref.evaluate(gt, results)
    assert ref.threshold_margin(out["oks"]) > 1e-9
    per_image = {}
    for r in results:
        per_image[r["image_id"]] = per_image.get(r["image_id"], 0) + 1
    with_gt = {a["image_id"] for a in gt["annotations"]}
    assert max(per_image.values()) > 20 and any(i not in with_gt for i in per_image) and any(i not in per_image for i in with_gt)
    assert any(a["iscrowd"] for a in gt["annotations"]) and any(a["num_keypoints"] == 0 for a in gt["annotations"])
    areas = np.array([a["area"] for a in gt["annotations"]])
    assert (areas < 32 ** 2).any() and ((areas > 32 ** 2) & (areas < 96 ** 2)).any() and (areas > 96 ** 2).any()
    scores = [r["score"] for r in results]
    assert len(set(scores)) < len(scores) // 10                                    # ties everywhere
    vals = np.concatenate([o.reshape(-1) for o in out["oks"].values()])
    hist, _ = np.histogram(vals, bins=[0.3, 0.5, 0.7, 0.9, 1.0])
    assert (hist > 20).all()
    assert 0.05 < out["stats"][0] < 0.95 and (out["stats"] > -1).all()


def ref_seed():
    from tests.test_gpu_coco_eval import SEED
    return SEED
