"""COCO keypoint AP / AR on the MI355X: the algorithm of pycocotools' `COCOeval(gt, dt, "keypoints")` (`evaluate`, `accumulate`,
`summarize`) as HIP kernels (csrc/cocoeval.hip), the last step of the reference's `evaluate_map` (metrics/pose_metrics.py:182-209)
and `eval_kps` (eval.py:13-27).

    gt = KeypointGroundTruth("person_keypoints_val2017.json")        # or a dict with "images" / "annotations", or from_arrays(...)
    ev = KeypointEvaluator(gt)
    ev.add(pred_kps, scores, img_ids)                                 # the decoders' CUDA outputs, kept on the device
    ev.add_results(list_of_result_dicts)                              # kps_to_dict_ / PoseResult.coco / filter_poses output
    stats = ev.evaluate()                                             # {'AP': ..., 'Ap .5': ..., ...}; ev.precision, ev.recall

The host reads JSON, groups detections by image (integer bookkeeping) and takes the final ten means over `precision` / `recall`;
OKS, the per-image score order and cut, the matching, the global sort, the scans and the curves are kernels.  No torch op computes
anything here and nothing falls back to the CPU: without the library or a GPU, `evaluate()` raises."""
from __future__ import annotations

import ctypes
import json
import os
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from .. import _lib
from .._lib import HipLibraryError

STAT_NAMES = ('AP', 'Ap .5', 'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)')     # pose_metrics.py:198-199
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)                      # Params.setKpParams
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)        # all, medium, large
COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
# (stat, iouThr index or None = all, area index): summarize()'s _summarizeKps; iouThrs[0] = .5, iouThrs[5] = .75
_SUMMARY = ((1, None, 0), (1, 0, 0), (1, 5, 0), (1, None, 1), (1, None, 2), (0, None, 0), (0, 0, 0), (0, 5, 0), (0, None, 1), (0, None, 2))


def _dptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


class KeypointGroundTruth(object):
    """The ground truth of one keypoint evaluation, segment-ordered by image.

    `source`: an annotation file path, or a dict with `images` and `annotations` (the COCO layout).  Evaluated images are the `images`
    list (an image without annotations still counts its detections as false positives), in ascending id order; the annotations of an
    image keep their file order.  A ground truth is ignored when `ignore` or `iscrowd` is set or `num_keypoints == 0`.
    Host arrays: `image_ids` [I], `seg` [I+1], `ann_ids` [G], `keypoints` [G,J,3], `area` [G], `bbox` [G,4], `flag` [G] (SP_COCO_GT_*)."""

    def __init__(self, source: Union[str, os.PathLike, dict]):
        if isinstance(source, (str, os.PathLike)):
            with open(source, "r") as rf:
                source = json.load(rf)
        if not isinstance(source, dict) or "images" not in source or "annotations" not in source:
            raise ValueError("ground truth: expected an annotation file or a dict with 'images' and 'annotations'")
        anns = source["annotations"]
        n = len(anns)
        J = len(anns[0]["keypoints"]) // 3 if n else 17
        kps = np.zeros((n, J, 3), np.float64)
        for i, a in enumerate(anns):
            if len(a["keypoints"]) != J * 3:
                raise ValueError(f"annotation {a.get('id', i)}: {len(a['keypoints'])} key-point values, the first annotation has {J * 3}")
            kps[i] = np.asarray(a["keypoints"], np.float64).reshape(J, 3)
        nk = [a["num_keypoints"] if "num_keypoints" in a else int((kps[i, :, 2] > 0).sum()) for i, a in enumerate(anns)]
        self._init([im["id"] for im in source["images"]], [a["image_id"] for a in anns], kps, [a["area"] for a in anns],
                   [a["bbox"] for a in anns], [a.get("iscrowd", 0) for a in anns], [a.get("ignore", 0) for a in anns], nk,
                   [a.get("id", i + 1) for i, a in enumerate(anns)])

    @classmethod
    def from_arrays(cls, image_ids, ann_image_ids, keypoints, area, bbox, iscrowd=None, ignore=None, num_keypoints=None, ann_ids=None):
        """Explicit arrays: image_ids [I]; per annotation its image id, keypoints [G,J,3] (x, y, v), area, bbox [G,4] (x, y, w, h)."""
        self = cls.__new__(cls)
        kps = np.asarray(keypoints, np.float64)
        if kps.ndim != 3 or kps.shape[2] != 3:
            raise ValueError(f"keypoints: expected [G, J, 3], got {kps.shape}")
        n = kps.shape[0]
        zero = [0] * n
        self._init(image_ids, ann_image_ids, kps, area, bbox, zero if iscrowd is None else iscrowd, zero if ignore is None else ignore,
                   (kps[:, :, 2] > 0).sum(1) if num_keypoints is None else num_keypoints, range(1, n + 1) if ann_ids is None else ann_ids)
        return self

    def _init(self, image_ids, ann_image_ids, kps, area, bbox, iscrowd, ignore, num_keypoints, ann_ids):
        ids = np.asarray(list(image_ids), np.int64).reshape(-1)
        if ids.size == 0:
            raise ValueError("ground truth: no images")
        self.image_ids = np.unique(ids)
        if self.image_ids.size != ids.size:
            raise ValueError("ground truth: duplicate image ids")
        n = kps.shape[0]
        if not (1 <= kps.shape[1] <= _lib.SP_COCO_MAX_JOINTS):
            raise ValueError(f"ground truth: {kps.shape[1]} joints (1..{_lib.SP_COCO_MAX_JOINTS})")
        img = np.asarray(list(ann_image_ids), np.int64).reshape(-1)
        area = np.asarray(area, np.float64).reshape(-1)
        bbox = np.asarray(bbox, np.float64).reshape(-1, 4)
        crowd = np.asarray(iscrowd).reshape(-1) != 0
        ign = crowd | (np.asarray(ignore).reshape(-1) != 0) | (np.asarray(num_keypoints).reshape(-1) == 0)
        aid = np.asarray(list(ann_ids), np.int64).reshape(-1)
        if not (img.size == area.size == bbox.shape[0] == crowd.size == ign.size == aid.size == n):
            raise ValueError("ground truth: the per-annotation arrays differ in length")
        pos = self.positions(img, "annotation")
        order = np.argsort(pos, kind="stable")                # by image, annotation order within an image
        self.seg = np.zeros(self.image_ids.size + 1, np.int32)
        np.cumsum(np.bincount(pos, minlength=self.image_ids.size), out=self.seg[1:])
        self.ann_ids, self.keypoints = aid[order], np.ascontiguousarray(kps[order])
        self.area, self.bbox = np.ascontiguousarray(area[order]), np.ascontiguousarray(bbox[order])
        self.flag = (crowd[order] * _lib.SP_COCO_GT_CROWD + ign[order] * _lib.SP_COCO_GT_IGNORE).astype(np.int32)
        self.num_joints = int(kps.shape[1])
        self.max_per_image = int(np.diff(self.seg).max())
        self._device = {}

    def positions(self, img_ids, what: str = "result") -> np.ndarray:
        """Index of each image id in `image_ids`; an id that is not one of the ground truth's images is an error."""
        img = np.asarray(img_ids, np.int64).reshape(-1)
        pos = np.searchsorted(self.image_ids, img)
        bad = (pos >= self.image_ids.size) | (self.image_ids[np.minimum(pos, self.image_ids.size - 1)] != img)
        if bad.any():
            raise ValueError(f"{what} {int(np.nonzero(bad)[0][0])}: image_id {int(img[bad][0])} is not in the ground truth's images")
        return pos

    def __len__(self) -> int:
        return int(self.ann_ids.size)

    def device_tensors(self, device):
        """(seg, keypoints, area, bbox, flag) on `device`: uploaded once per device."""
        import torch
        device = torch.device(device)
        if device.type != "cuda":
            raise HipLibraryError(f"ground truth requested on {device}; simple_pose_amd runs on the MI355X only (no CPU fallback)")
        key = (device.type, _lib._device_index(device))
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(a).to(device) for a in (self.seg, self.keypoints, self.area, self.bbox, self.flag))
        return self._device[key]


class KeypointEvaluator(object):
    """`COCOeval(gt, dt, "keypoints")` on the device.  After `evaluate()`: `stats` (the ten values, STAT_NAMES order), `precision`
    [10,101,3], `recall` [10,3] and, per image id, `oks` [D,G] (detections in score order x ground truths in annotation order), `dt_ids`
    [D] (1-based position in the order the results were added), `dtm` [3,10,D] (matched annotation id, 0 = none), `dt_ignore` [3,10,D],
    `gt_ignore` [3,G] (annotation order)."""

    def __init__(self, gt: KeypointGroundTruth, sigmas: Optional[Sequence[float]] = None, max_dets: int = 20, device=None):
        if not isinstance(gt, KeypointGroundTruth):
            gt = KeypointGroundTruth(gt)
        J = gt.num_joints
        if sigmas is None:
            if J != 17:
                raise ValueError(f"the default sigmas are COCO's 17; pass sigmas for {J} joints")
            sigmas = COCO_SIGMAS
        self.sigmas = np.ascontiguousarray(np.asarray(sigmas, np.float64).reshape(-1))
        if self.sigmas.size != J:
            raise ValueError(f"sigmas: {self.sigmas.size} values for {J} joints")
        if not isinstance(max_dets, int) or not (1 <= max_dets <= _lib.SP_COCO_MAX_DETS):
            raise ValueError(f"max_dets: expected an int in 1..{_lib.SP_COCO_MAX_DETS}, got {max_dets!r}")
        self.gt, self.max_dets, self.device = gt, max_dets, device
        self.reset()

    def reset(self):
        self._chunks: List[tuple] = []                        # (xy [n,J,2] device, score [n] device, image positions [n] host)
        self.stats = self.precision = self.recall = None
        self._raw = self._count = self._per_image = None

    def __len__(self) -> int:
        return sum(int(c[2].size) for c in self._chunks)

    # -- input ----------------------------------------------------------------------------------------------------------------------------
    def add(self, pred_kps, scores, img_ids, score=None):
        """Decoder output of one batch, straight from the device: `pred_kps` CUDA fp32 [P,J,2] with the per-joint maxima `scores` [P,J]
        / [P,J,1], or `pred_kps` [P,J,3] (x, y, max_val) and `scores=None`.  The result score is `kps_to_dict_`'s rule (sp_pose_score:
        mean + max of the per-joint maxima) unless `score` [P] (CUDA fp32 / fp64) supplies it."""
        import torch
        pred_kps = _lib.require_cuda_f32(pred_kps, "pred_kps")
        J = self.gt.num_joints
        if pred_kps.dim() != 3 or pred_kps.shape[1] != J or pred_kps.shape[2] not in (2, 3):
            raise ValueError(f"pred_kps: expected [P, {J}, 2] or [P, {J}, 3], got {tuple(pred_kps.shape)}")
        P = pred_kps.shape[0]
        pos = self.gt.positions(list(img_ids))
        if pos.size != P:
            raise ValueError(f"img_ids: {pos.size} ids for {P} persons")
        if P == 0:
            return
        if pred_kps.shape[2] == 3:
            if scores is None:
                scores = pred_kps[:, :, 2]
            pred_kps = pred_kps[:, :, :2]
        if score is None:
            if scores is None:
                raise ValueError("scores: the per-joint maxima [P, J] are needed for the result score (or pass score=)")
            scores = _lib.require_cuda_f32(scores, "scores").reshape(P, -1)
            if scores.shape[1] != J:
                raise ValueError(f"scores: expected [{P}, {J}], got {tuple(scores.shape)}")
            _lib.same_device(pred_kps, scores)
            score = torch.empty(P, dtype=torch.float32, device=pred_kps.device)
            _lib.check(_lib.lib().sp_pose_score(_lib.ptr(scores), P, J, _lib.ptr(score), _lib.current_stream(pred_kps.device)), "sp_pose_score")
        else:
            if not (isinstance(score, torch.Tensor) and score.is_cuda and score.dtype in (torch.float32, torch.float64) and score.numel() == P):
                raise HipLibraryError(f"score: expected a CUDA float32 / float64 tensor of {P} values")
            _lib.same_device(pred_kps, score)
            score = score.reshape(P).contiguous()
        self._append(pred_kps.contiguous(), score, pos)

    def add_results(self, results: Sequence[dict]):
        """COCO result dicts (`image_id`, `keypoints` [3J], `score`), in list order: `kps_to_dict_`, `PoseResult.coco`, `filter_poses`."""
        import torch
        if not results:
            return
        J = self.gt.num_joints
        pos = self.gt.positions([r["image_id"] for r in results])
        kps = np.empty((len(results), J, 3), np.float64)
        for i, r in enumerate(results):
            if len(r["keypoints"]) != J * 3:
                raise ValueError(f"result {i}: {len(r['keypoints'])} key-point values, expected {J * 3}")
            kps[i] = np.asarray(r["keypoints"], np.float64).reshape(J, 3)
        sc = np.asarray([r["score"] for r in results], np.float64)
        if not np.isfinite(sc).all() or not np.isfinite(kps[:, :, :2]).all():
            raise ValueError("results: non-finite score or coordinate")
        dev = self._dev()
        self._append(torch.from_numpy(np.ascontiguousarray(kps[:, :, :2])).to(dev), torch.from_numpy(sc).to(dev), pos)

    def _dev(self):
        import torch
        if self._chunks:
            return self._chunks[0][0].device
        if self.device is not None:
            return torch.device(self.device)
        if not torch.cuda.is_available():
            raise HipLibraryError("the keypoint evaluator runs on the MI355X only (no CPU fallback)")
        return torch.device("cuda", torch.cuda.current_device())

    def _append(self, xy, score, pos):
        if self._chunks:
            _lib.same_device(self._chunks[0][0], xy)
        self._chunks.append((xy, score, pos))
        self._raw = None

    # -- evaluate() + accumulate() + summarize() ----------------------------------------------------------------------------------------------
    def evaluate(self) -> Dict[str, float]:
        import torch
        lib, gt, P = _lib.lib(), self.gt, _lib.ptr
        dev = self._dev()
        I, G, J, M = int(gt.image_ids.size), len(gt), gt.num_joints, self.max_dets
        T, A, R = IOU_THRS.size, AREA_RNG.shape[0], REC_THRS.size
        pos = np.concatenate([c[2] for c in self._chunks]) if self._chunks else np.zeros(0, np.int64)
        n_dt = int(pos.size)
        dt_seg = np.zeros(I + 1, np.int32)
        np.cumsum(np.bincount(pos, minlength=I), out=dt_seg[1:])
        max_dt = int(np.diff(dt_seg).max())
        flags, xy, score = 0, None, None
        if n_dt:
            # chunks of mixed precision are widened to float64 (exact), so one pointer serves the launch
            xy64 = any(c[0].dtype == torch.float64 for c in self._chunks)
            sc64 = any(c[1].dtype == torch.float64 for c in self._chunks)
            xy = torch.cat([c[0].to(torch.float64) if xy64 else c[0] for c in self._chunks])
            score = torch.cat([c[1].to(torch.float64) if sc64 else c[1] for c in self._chunks])
            flags = (_lib.SP_COCO_DT_XY_F64 if xy64 else 0) | (_lib.SP_COCO_DT_SCORE_F64 if sc64 else 0)
        with torch.cuda.device(dev):
            stream = _lib.current_stream(dev)
            g_seg, g_kps, g_area, g_bbox, g_flag = gt.device_tensors(dev)
            d_seg = torch.from_numpy(dt_seg).to(dev)
            d_index = torch.from_numpy(np.argsort(pos, kind="stable").astype(np.int32)).to(dev) if n_dt else None
            S = I * M
            e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
            out = {"dt_count": e((I,), torch.int32), "dt_keep": e((S,), torch.int32), "dt_kscore": e((S,), torch.float64),
                   "dt_karea": e((S,), torch.float64), "oks": e((max(G * M, 1),), torch.float64), "dtm": e((A, T, S), torch.int32),
                   "dt_ignore": e((A, T, S), torch.uint8), "gt_ignore": e((A, max(G, 1)), torch.uint8),
                   "precision": e((T, R, A), torch.float64), "recall": e((T, A), torch.float64)}
            _lib.check(lib.sp_coco_kp_eval_images(
                P(g_seg), P(g_kps), P(g_area), P(g_bbox), P(g_flag), P(d_seg), P(d_index), P(xy), P(score), flags, I, G, gt.max_per_image, max_dt, J,
                _dptr(self.sigmas), M, _dptr(IOU_THRS), T, _dptr(AREA_RNG), A, P(out["dt_count"]), P(out["dt_keep"]), P(out["dt_kscore"]),
                P(out["dt_karea"]), P(out["oks"]), P(out["dtm"]), P(out["dt_ignore"]), P(out["gt_ignore"]), stream), "sp_coco_kp_eval_images")
            nbytes = ctypes.c_int64(0)
            _lib.check(lib.sp_coco_kp_accumulate_workspace(I, M, T, A, ctypes.byref(nbytes)), "sp_coco_kp_accumulate_workspace")
            ws = e((nbytes.value,), torch.uint8)
            _lib.check(lib.sp_coco_kp_accumulate(
                P(out["dt_count"]), P(out["dt_kscore"]), P(out["dtm"]), P(out["dt_ignore"]), P(out["gt_ignore"]), I, G, M, T, A, _dptr(REC_THRS), R,
                P(ws), nbytes.value, P(out["precision"]), P(out["recall"]), stream), "sp_coco_kp_accumulate")
            count = out["dt_count"].cpu().numpy()
            if (count < 0).any():
                i = int(np.nonzero(count < 0)[0][0])
                what = (f"more than {_lib.SP_COCO_MAX_DT_PER_IMAGE} detections" if count[i] == -1
                        else f"more than {_lib.SP_COCO_MAX_GT_PER_IMAGE} ground truths")
                raise HipLibraryError(f"image {int(gt.image_ids[i])}: {what} (nothing is truncated)")
            self.precision, self.recall = out["precision"].cpu().numpy(), out["recall"].cpu().numpy()
        self._raw, self._count = out, count
        self._per_image = None
        self.stats = summarize(self.precision, self.recall)
        return {k: float(v) for k, v in zip(STAT_NAMES, self.stats)}

    # -- per-image intermediates (tests, inspection): one device-to-host copy on first use ----------------------------------------------------------
    def _images(self):
        if self._raw is None:
            raise RuntimeError("call evaluate() first")
        if self._per_image is None:
            gt, M, h = self.gt, self.max_dets, {k: v.cpu().numpy() for k, v in self._raw.items()}
            res = {"oks": {}, "dt_ids": {}, "dtm": {}, "dt_ignore": {}, "gt_ignore": {}, "dt_scores": {}, "dt_area": {}}
            for i, img in enumerate(gt.image_ids.tolist()):
                g0, g1, D, s0 = int(gt.seg[i]), int(gt.seg[i + 1]), int(self._count[i]), i * M
                res["oks"][img] = h["oks"][g0 * M:g0 * M + D * (g1 - g0)].reshape(D, g1 - g0)
                res["dt_ids"][img] = h["dt_keep"][s0:s0 + D].astype(np.int64) + 1        # dt_keep: row in the order the results were added
                m = h["dtm"][:, :, s0:s0 + D]
                res["dtm"][img] = np.where(m >= 0, gt.ann_ids[np.maximum(m, 0)] if len(gt) else 0, 0)
                res["dt_ignore"][img] = h["dt_ignore"][:, :, s0:s0 + D].astype(bool)
                res["gt_ignore"][img] = h["gt_ignore"][:, g0:g1].astype(bool)
                res["dt_scores"][img], res["dt_area"][img] = h["dt_kscore"][s0:s0 + D], h["dt_karea"][s0:s0 + D]
            self._per_image = res
        return self._per_image

    oks = property(lambda self: self._images()["oks"])
    dt_ids = property(lambda self: self._images()["dt_ids"])
    dtm = property(lambda self: self._images()["dtm"])
    dt_ignore = property(lambda self: self._images()["dt_ignore"])
    gt_ignore = property(lambda self: self._images()["gt_ignore"])
    dt_scores = property(lambda self: self._images()["dt_scores"])
    dt_area = property(lambda self: self._images()["dt_area"])


def summarize(precision: np.ndarray, recall: np.ndarray) -> np.ndarray:
    """`COCOeval.summarize` for key points: the ten means over the entries > -1 (-1 without any), STAT_NAMES order."""
    stats = np.zeros(len(_SUMMARY))
    for i, (ap, t, a) in enumerate(_SUMMARY):
        s = precision[:, :, a] if ap else recall[:, a]
        if t is not None:
            s = s[t]
        s = s[s > -1]
        stats[i] = np.mean(s) if s.size else -1
    return stats


def evaluate_keypoints(results, ground_truth, sigmas=None, max_dets: int = 20) -> KeypointEvaluator:
    """Result dicts (a JSON path or a list) against ground truth (a path, a dict or a KeypointGroundTruth): the evaluated evaluator."""
    if isinstance(results, (str, os.PathLike)):
        with open(results, "r") as rf:
            results = json.load(rf)
    ev = KeypointEvaluator(ground_truth, sigmas=sigmas, max_dets=max_dets)
    ev.add_results(results)
    ev.evaluate()
    return ev
