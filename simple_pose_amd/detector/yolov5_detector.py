"""detector/yolov5_detector.py on the MI355X: ScalePadding, non_max_suppression, clip_coords and YOLOv5Detector.

Geometry (the letterbox sizes and offsets) is host arithmetic on a few integers, as in the reference; every per-pixel and per-box operation runs
in csrc/detect.hip: the letterbox + Focus input launch, the batched NMS (candidate filter, multi-label expansion, xywh -> xyxy, sort, greedy
scan, merge, redundancy filter) and the clip + un-letterbox of the result boxes.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import _lib, engine
from .._lib import HipLibraryError
from ..video import YuvFrame, to_bgr
from .nets.yolov5 import YOLOv5

_WS: Dict[Tuple[str, int], torch.Tensor] = {}


def _workspace(batch: int, device) -> torch.Tensor:
    key = (str(device), batch)
    ws = _WS.get(key)
    if ws is None:
        n = ctypes.c_int64(0)
        _lib.check(_lib.lib().sp_yolo_nms_workspace(batch, ctypes.byref(n)), "sp_yolo_nms_workspace")
        if len(_WS) >= 4:
            _WS.pop(next(iter(_WS)))
        ws = _WS[key] = torch.empty(n.value, dtype=torch.uint8, device=device)
    return ws


def non_max_suppression(prediction: torch.Tensor, conf_thresh=0.1, iou_thresh=0.6, merge=False, agnostic=False, multi_label=True,
                        max_det=300) -> List[Optional[torch.Tensor]]:
    """yolov5_detector.py:52-128 for a CUDA fp32 [B, N, no] prediction: per image None (no candidate) or [n, 6] (x1, y1, x2, y2, conf, cls).
    Exact up to SP_YOLO_NMS_MAX_CANDIDATES candidates per image after the multi-label expansion; above that it raises."""
    pred = _lib.require_cuda_f32(prediction, "prediction")
    if pred.dim() != 3 or pred.shape[2] < 6:
        raise ValueError(f"prediction: expected [B, N, >= 6], got {tuple(pred.shape)}")
    B, N, no = pred.shape
    out = torch.zeros((B, max_det, 6), dtype=torch.float32, device=pred.device)
    counts, cands = (ctypes.c_int32 * B)(), (ctypes.c_int32 * B)()
    ws = _workspace(B, pred.device)
    _lib.check(_lib.lib().sp_yolo_nms(_lib.ptr(pred), B, N, no, float(conf_thresh), float(iou_thresh), int(bool(merge)), int(bool(multi_label)),
                                      int(bool(agnostic)), int(max_det), _lib.ptr(ws), ws.numel(), _lib.ptr(out), counts, cands,
                                      _lib.current_stream(pred.device)), "sp_yolo_nms")
    return [None if cands[b] == 0 else out[b, :counts[b]] for b in range(B)]


def boxes_to_source(det: torch.Tensor, img_hw: Tuple[int, int], left: float = 0.0, top: float = 0.0, ratio: float = 1.0) -> torch.Tensor:
    """In place on CUDA fp32 rows [..., 6]: clip_coords to the letterboxed image (h, w), then x = (x - left) / ratio, y = (y - top) / ratio."""
    if not (det.is_cuda and det.dtype == torch.float32 and det.is_contiguous() and det.shape[-1] == 6):
        raise HipLibraryError("boxes_to_source: expected a contiguous CUDA fp32 tensor [..., 6]")
    rows = det.numel() // 6
    if rows == 0:                       # candidates but no box left (merge-NMS's redundancy filter): an empty view has no pointer to pass
        return det
    _lib.check(_lib.lib().sp_yolo_boxes_to_source(_lib.ptr(det), rows, float(img_hw[0]), float(img_hw[1]), float(left), float(top), float(ratio),
                                                  _lib.current_stream(det.device)), "sp_yolo_boxes_to_source")
    return det


def clip_coords(boxes: torch.Tensor, img_shape) -> None:
    """yolov5_detector.py:9-14 (in place; the box columns of [n, 6] detections)."""
    boxes_to_source(boxes, (img_shape[0], img_shape[1]))


class ScalePadding(object):
    """The letterbox of yolov5_detector.py:131-170.  `geometry` is the reference's integer arithmetic; `make_border` runs it on the GPU
    (sp_yolo_letterbox) and returns the uint8 BGR canvas as a CUDA tensor [H, W, 3]."""

    def __init__(self, target_size=(640, 640), padding_val=(114, 114, 114), minimum_rectangle=False, scale_up=True, **kwargs):
        super().__init__(**kwargs)
        if tuple(padding_val) != (114, 114, 114):
            raise NotImplementedError("the letterbox launch pads with 114")
        self.p = 1
        self.new_shape = target_size
        self.padding_val = padding_val
        self.minimum_rectangle = minimum_rectangle
        self.scale_up = scale_up

    def geometry(self, h: int, w: int) -> dict:
        """new_h, new_w (resized image), top, bottom, left, right (borders), ratio - as make_border computes them."""
        if isinstance(self.new_shape, int):
            self.new_shape = (self.new_shape, self.new_shape)
        r = min(self.new_shape[1] / h, self.new_shape[0] / w)
        if not self.scale_up:
            r = min(r, 1.0)
        new_unpad = int(round(w * r)), int(round(h * r))
        dw, dh = self.new_shape[0] - new_unpad[0], self.new_shape[1] - new_unpad[1]
        if self.minimum_rectangle:
            dw, dh = np.mod(dw, 64), np.mod(dh, 64)
        dw /= 2
        dh /= 2
        top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
        left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
        return dict(new_h=new_unpad[1], new_w=new_unpad[0], top=top, bottom=bottom, left=left, right=right, ratio=r,
                    out_h=new_unpad[1] + top + bottom, out_w=new_unpad[0] + left + right)

    def make_border(self, img):
        src = _as_cuda_u8(img)
        g = self.geometry(src.shape[0], src.shape[1])
        out = torch.empty((g["out_h"], g["out_w"], 3), dtype=torch.uint8, device=src.device)
        _lib.check(_lib.lib().sp_yolo_letterbox(_lib.ptr(src), 1, src.shape[0], src.shape[1], g["new_h"], g["new_w"], g["top"], g["left"], g["out_h"],
                                                g["out_w"], _lib.SP_LETTERBOX_U8, _lib.ptr(out), _lib.current_stream(src.device)), "sp_yolo_letterbox")
        return out, (g["ratio"], g["ratio"]), (g["left"], g["top"])


def _as_cuda_u8(img, device=None) -> torch.Tensor:
    """uint8 BGR [H, W, 3] (or a batch [B, H, W, 3]): numpy -> CUDA; a CUDA tensor is taken as it is."""
    if isinstance(img, np.ndarray):
        if img.dtype != np.uint8:
            raise TypeError(f"expected a uint8 BGR image, got {img.dtype}")
        img = torch.from_numpy(np.ascontiguousarray(img)).to(device or "cuda")
    if not (isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.uint8 and img.dim() in (3, 4) and img.shape[-1] == 3):
        raise HipLibraryError("expected a uint8 BGR image [H, W, 3] (numpy or CUDA)")
    return img.contiguous()


class YOLOv5Detector(object):
    """yolov5_detector.py:173-239.  `state_dict=`: the model's weights directly (instead of torch.load(weights_path)['ema']).
    single_predict at batch 1 is one graph replay (letterbox + network + decode) plus the NMS; `use_graph = False` launches eagerly."""

    MAX_GRAPHS = 8

    def __init__(self, weights_path=None, num_cls=80, scale_name="l", scale_size=(640, 640), device="cuda", iou_thresh=0.6, conf_thresh=0.001,
                 slice_idx=0, state_dict=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise HipLibraryError(f"device {device}: simple_pose_amd runs on the MI355X only (no CPU fallback)")
        self.model = YOLOv5(scale_name=scale_name, num_cls=num_cls)
        if state_dict is None:
            state_dict = torch.load(weights_path, map_location="cpu")["ema"]
        self.model.load_state_dict(state_dict)
        self.transform = ScalePadding(target_size=scale_size, minimum_rectangle=True, padding_val=(114, 114, 114))
        self.iou_thresh = iou_thresh
        self.conf_thresh = conf_thresh
        self.slice_idx = slice_idx
        self.model.eval()
        self.model.to(self.device)
        self.use_graph = True
        self._graphs: Dict[tuple, object] = {}
        self._stage: dict = {}               # predict on differently sized images: the pinned staging buffer and the device arena

    def program(self, out_h: int, out_w: int) -> engine.Program:
        """The fp32 program of one letterboxed shape (uint8 source input, letterbox inside)."""
        return self.model.hip_program(out_h, out_w, self.device, slice_idx=self.slice_idx, source="u8")

    def _forward(self, src: torch.Tensor, g: dict, graph: bool) -> torch.Tensor:
        prog = self.program(g["out_h"], g["out_w"])
        engine.set_letterbox(prog, src.shape[1], src.shape[2], g["new_h"], g["new_w"], g["top"], g["left"])
        if not graph:
            return prog.run(src)
        key = (tuple(src.shape), g["out_h"], g["out_w"], id(prog))
        gf = self._graphs.get(key)
        if gf is None:
            if len(self._graphs) >= self.MAX_GRAPHS:
                self._graphs.pop(next(iter(self._graphs)))
            gf = self._graphs[key] = prog.capture(src)
        return gf(src)

    def _finish(self, dets: List[Optional[torch.Tensor]], g: dict) -> list:
        out = []
        for box in dets:
            if box is None:
                out.append([])
                continue
            boxes_to_source(box, (g["out_h"], g["out_w"]), g["left"], g["top"], g["ratio"])
            out.append(box)
        return out

    @torch.no_grad()
    def single_predict(self, img):
        """uint8 BGR [H, W, 3] (numpy or CUDA), or a video.YuvFrame -> CUDA fp32 [n, 6] (x1, y1, x2, y2, score, cls) in source pixels, or []
        when nothing is found."""
        if isinstance(img, YuvFrame):                # a video frame: converted on the device (one launch), then as a CUDA image
            img = to_bgr(img, device=self.device)
        src = _as_cuda_u8(img, self.device)
        if src.dim() != 3:
            raise ValueError("single_predict takes one image [H, W, 3]")
        g = self.transform.geometry(src.shape[0], src.shape[1])
        pred = self._forward(src[None], g, self.use_graph)
        dets = non_max_suppression(pred, multi_label=True, iou_thresh=self.iou_thresh, conf_thresh=self.conf_thresh, merge=True)
        return self._finish(dets, g)[0]

    @torch.no_grad()
    def predict(self, imgs: Union[torch.Tensor, Sequence[np.ndarray]]) -> list:
        """A batch of same-sized uint8 BGR images (CUDA [B, H, W, 3], or a list of [H, W, 3] arrays) in one forward and one NMS launch
        sequence; per image what single_predict returns.  A list of differently sized images (numpy or CUDA) is grouped by letterboxed
        net shape: one forward and one NMS sequence per group, every image letterboxed as single_predict letterboxes it alone.  A list
        may hold video.YuvFrames (or be one): it goes the grouped way, its frames converted to BGR on the device by one launch first."""
        if isinstance(imgs, torch.Tensor):
            src = _as_cuda_u8(imgs, self.device)
            if src.dim() != 4:
                raise ValueError("predict takes a batch [B, H, W, 3]")
        else:
            if isinstance(imgs, YuvFrame):
                imgs = [imgs]
            if len({tuple(np.shape(i)) for i in imgs}) != 1 or any(isinstance(i, (torch.Tensor, YuvFrame)) for i in imgs):
                return self._predict_mixed(imgs)
            src = _as_cuda_u8(np.stack([np.asarray(i) for i in imgs]), self.device)
        g = self.transform.geometry(src.shape[1], src.shape[2])
        pred = self._forward(src, g, False)
        dets = non_max_suppression(pred, multi_label=True, iou_thresh=self.iou_thresh, conf_thresh=self.conf_thresh, merge=True)
        return self._finish(dets, g)

    def _predict_mixed(self, imgs) -> list:
        """predict for a list of differently sized images: the table of sp_image_ref goes up once, each net-shape group is one eager
        forward (the letterbox launch reads its images through the table) and one NMS sequence; results in the caller's order."""
        from ..mixed_batch import MixedBatch
        mb = MixedBatch(imgs, self.transform, self.device, self._stage)
        out = [None] * mb.B
        for k, ((out_h, out_w), members) in enumerate(mb.groups):
            prog = self.program(out_h, out_w)
            engine.set_letterbox_images(prog)
            pred = prog.run(mb.group_table(k))
            dets = non_max_suppression(pred, multi_label=True, iou_thresh=self.iou_thresh, conf_thresh=self.conf_thresh, merge=True)
            for i, box in zip(members, dets):
                out[i] = self._finish([box], mb.geoms[i])[0]
        return out

    # -- tiled detection (tiling.py): the passes of large frames in one forward per net shape, fused on the device -------------------------
    TILE_CHUNK = 32                      # passes per forward at the most: bounds the activation pool; no bit depends on it

    def tile_programs(self, tp) -> tuple:
        """The programs of a TilePlan's groups, in group order."""
        return tuple(self.program(out_h, out_w) for (out_h, out_w), _, _ in tp.groups)

    def detect_tiled(self, tp, progs, det: torch.Tensor, counts: torch.Tensor, status: torch.Tensor, max_det: int, tiling,
                     single_stream: bool = False) -> None:
        """Every launch between the frames a TilePlan points into and their fused detections: per net-shape group (in chunks of
        TILE_CHUNK passes) letterbox through the table + network + head decode, sp_yolo_nms_device and the scatter into the frames'
        candidate blocks, then one sp_yolo_merge_passes into det [B, max_det, 6] / counts [B]; status [B] receives the OR of the
        passes' NMS status words.  Plain launches on the current stream (`single_stream`: the programs' too, as a capture needs it)."""
        lib, P = _lib.lib(), _lib.ptr
        stream = _lib.current_stream(self.device)
        keep = []
        status.zero_()
        for k, ((out_h, out_w), _, n) in enumerate(tp.groups):
            prog, first = progs[k], tp.groups[k][1]
            for lo in range(0, n, self.TILE_CHUNK):
                hi = min(n, lo + self.TILE_CHUNK)
                table = tp.group_table(k, lo, hi)
                engine.set_letterbox_tiles(prog)
                pred = prog.run_on_stream(table, single_stream)
                m, N, no = pred.shape
                ws = _workspace(m, pred.device)
                a, b = first + lo, first + hi
                _lib.check(lib.sp_yolo_nms_device(P(pred), m, N, no, float(self.conf_thresh), float(self.iou_thresh), 1, 1, 0, max_det, P(ws),
                                                  ws.numel(), P(tp.det[a:b]), P(tp.counts[a:b]), P(tp.status[a:b]), stream), "sp_yolo_nms_device")
                _lib.check(lib.sp_yolo_boxes_to_frame_tiles(P(tp.det[a:b]), P(tp.counts[a:b]), P(tp.status[a:b]), P(table), m, tp.P, max_det,
                                                            float(out_h), float(out_w), P(tp.cand), P(tp.cand_counts), P(status), stream),
                           "sp_yolo_boxes_to_frame_tiles")
                keep += [prog, prog.pool_for(m, pred.device), ws, pred]
        ws = _workspace(tp.B, self.device)
        _lib.check(lib.sp_yolo_merge_passes(P(tp.cand), P(tp.cand_counts), tp.B, tp.P, max_det, tiling.metric_code, tiling.thresh,
                                            int(tiling.agnostic), P(ws), ws.numel(), P(det), P(counts), stream), "sp_yolo_merge_passes")
        tp.keepalive = keep + [ws]                   # a captured graph holds their pointers

    @torch.no_grad()
    def predict_tiled(self, img, tiling, max_det: int = 300) -> list:
        """Tiled detection of one image [H, W, 3] or a same-sized batch [B, H, W, 3] (uint8 BGR, numpy or CUDA; a list of same-sized
        arrays is stacked): the detector runs on the passes `tiling` plans (tiling.Tiling: overlapping tiles at their native resolution,
        and the whole frame), one forward per net shape, and the passes' boxes are fused on the device.  Per image CUDA fp32 [n, 6]
        (x1, y1, x2, y2, score, cls) in source pixels, or [] when nothing is found; a single image gives its result, a batch a list."""
        from ..tiling import TilePlan, Tiling
        if not isinstance(tiling, Tiling):
            raise TypeError(f"tiling: expected a simple_pose_amd.tiling.Tiling, got {type(tiling).__name__}")
        if isinstance(img, YuvFrame):                # a video frame: converted on the device (one launch), then as a CUDA image
            img = to_bgr(img, device=self.device)
        if isinstance(img, (list, tuple)):
            if len(img) == 0 or len({tuple(np.shape(i)) for i in img}) != 1:
                raise ValueError("predict_tiled takes images of one size (tiling differently sized images is not supported)")
            img = torch.stack(list(img)) if isinstance(img[0], torch.Tensor) else np.stack([np.asarray(i) for i in img])
        src = _as_cuda_u8(img, self.device)
        single = src.dim() == 3
        if single:
            src = src[None]
        if 0 in tuple(src.shape):
            raise ValueError(f"expected uint8 BGR [H, W, 3] or [B, H, W, 3], got {tuple(src.shape)}")
        tp = TilePlan(tiling, self.transform, src, max_det)          # every check before the first launch
        B = src.shape[0]
        det = torch.empty((B, max_det, 6), dtype=torch.float32, device=src.device)
        cs = torch.empty((2, B), dtype=torch.int32, device=src.device)           # counts, status
        self.detect_tiled(tp, self.tile_programs(tp), det, cs[0], cs[1], max_det, tiling)
        h = cs.cpu().numpy()
        if (h[1] & 1).any():
            raise HipLibraryError(f"image {int(np.nonzero(h[1] & 1)[0][0])}: a pass has more than {_lib.SP_YOLO_NMS_MAX_CANDIDATES} detector "
                                  "candidates after the multi-label expansion (raise conf_thresh)")
        out = [det[b, :int(h[0][b])] if h[0][b] > 0 else [] for b in range(B)]
        return out[0] if single else out
