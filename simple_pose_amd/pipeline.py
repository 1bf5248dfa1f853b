"""Top-down pose estimation in one call: image in, poses out, nothing returns to the host in between.

    est = TopDownPoseEstimator(detector, pose_model, decoder=GaussTaylorKeyPointDecoder(), capacity=32)
    res = est.estimate(img)                       # uint8 BGR [H,W,3], numpy or CUDA -> PoseResult
    res = est.estimate_batch(imgs)                # same-sized batch [B,H,W,3] -> list of PoseResult
    res = est.estimate_batch([img_a, img_b, ...]) # differently sized images (numpy or CUDA) -> list of PoseResult, caller's order
    res = est.estimate_files(jpeg_files)          # JpegDecoder.decode, then that batch on the decoder's device tensors
    res = est.estimate_boxes(imgs, det, counts)   # caller-supplied detections (the reference's predicts_by_pred path)
    res = est.estimate(YuvFrame(...))             # a video frame (video.py: NV12 / I420 planes) wherever an image is taken
    est = TopDownPoseEstimator(..., tiling=Tiling())   # large frames: the detector on overlapping tiles, fused on the device

The reference runs the three stages as three offline scripts joined by JSON files (eval.py: gen_data_by_detector, predicts_by_pred,
temp_read_in_and_filter).  Here a frame is one stream of launches: letterbox + YOLOv5 + decode, sp_yolo_nms_device, sp_yolo_boxes_to_source,
sp_topdown_plan (boxes -> crop geometry), sp_warp_affine_plan_u8c3 (the crops), the pose program on `capacity` crops, the key-point decode,
sp_pose_rescore and sp_oks_nms.  The person count never reaches the host: the pose half always computes `capacity` slots (dead slots are
zero crops that OKS-NMS never sees), which is what makes the frame capturable - at batch 1 it is ONE hipGraph.  One device-to-host
transfer per call brings back the keep list, the counts, the status words and the rows.  There is no CPU fallback.
With `flip_test=True` the crops are mirrored into a second half of the crop buffer (sp_mirror_w), the pose program runs once on
`2 * capacity` crops, and sp_heat_map_flip_merge averages the un-mirrored second half into the first before the decode: two more launches
on the same stream, still one graph.
With `renderer=PoseRenderer(...)` (visualize.py) the kept poses are drawn into a copy of the source image, `PoseResult.image`, by two more
launches (sp_render_poses_u8c3) after sp_oks_nms, on the same stream and inside the same graph; without one nothing is allocated or launched.
A renderer with a `label` or a `caption` adds two more (sp_render_labels_u8c3: ids, scores and the kept count formatted on the device); the
caption's bytes are staged into the frame ahead of the launches or the replay (_stage_caption), so a captured frame shows a new caption.
With `redactor=Redactor(...)` (visualize.py) the canvas is produced from the source by sp_redact_u8c3 (two launches, out of place): the kept
persons' heads, or the whole persons, behind a mosaic or a constant colour, from this frame's raw key points and boxes.  The renderer's
launches, if there is one, then run in place on that canvas - redaction, then capsules, then text - and `PoseResult.image` exists with a
redactor or a renderer; the poses themselves are bit for bit what they are without one.
With `heat_overlay=HeatOverlay(...)` (visualize.py) the kept persons' heat maps - the tensor the decode reads, with the flip test the merged
maps - are blended into the canvas by sp_heat_overlay_u8c3 (two launches) through the frame's own `trans_inv`: after the redaction, under
the capsules and the text; out of place from the source when it is the first stage, in place on the canvas otherwise.
With `encoder=JpegEncoder(...)` (datasets.jpeg) every image's canvas - without a renderer or a redactor, the source - is encoded to a baseline JPEG file
after the frame on the same stream (sp_jpeg_encode_batch, outside the graph: it uploads its descriptors), and `PoseResult.jpeg` holds the
file's bytes; without one nothing is allocated or launched.
A list of differently sized images is one call too (mixed_batch.py): the images are grouped by letterboxed net shape, each group is one
detector forward whose letterbox launch reads every image's own geometry from a table of sp_image_ref in device memory
(sp_yolo_letterbox_images), sp_yolo_boxes_to_source_images scatters the groups' detections into the caller's order, and from
sp_topdown_plan on there is one of everything for the whole batch, the crops by sp_warp_affine_plan_images_u8c3.  Eager: the table upload
is not capturable.
With `tiling=Tiling(...)` (tiling.py) the detector half of `estimate` and same-sized `estimate_batch` runs on overlapping tiles of the
frame at their native resolution, and on the whole frame: a table of sp_tile_ref points into the frame's static source, the passes of one
net shape are one detector forward whose letterbox launch reads them through the table (sp_yolo_letterbox_tiles), sp_yolo_nms_device and
sp_yolo_boxes_to_frame_tiles bring every pass's boxes into frame coordinates, and sp_yolo_merge_passes fuses them into the `det` /
`counts` that sp_topdown_plan reads.  The table is built and uploaded once per frame shape, so `estimate` stays ONE graph."""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Dict, List, Sequence, Union

import numpy as np
import torch

from . import _lib, engine
from ._lib import HipLibraryError
from .metrics.flip import COCO_JOINT_PAIRS, check_joint_pairs, pairs_to_perm
from .datasets.jpeg import JpegDecoder, JpegEncoder
from .mixed_batch import MixedBatch, check_det_counts, check_images
from .tiling import TilePlan, Tiling, plan_pass_groups
from .video import YuvBatch, YuvFrame, convert_into, resolve
from .visualize import HeatOverlay, PoseRenderer, Redactor

P = _lib.ptr
MAX_CAPACITY = 2048                  # the OKS-NMS group limit (sp_oks_nms)


@dataclass
class PoseResult:
    """The persons of one image that survive OKS-NMS, in pick order."""
    keypoints: np.ndarray            # float64 [n, J, 3]: x, y (image px), max_val
    score: np.ndarray                # float64 [n]: box score x mean of the visible joints' max_val (eval.py:166-174)
    box: np.ndarray                  # float32 [n, 5]: x1, y1, x2, y2, detector confidence
    dropped: int = 0                 # selected detections of this image that did not fit `capacity`
    track_id: np.ndarray = None      # int32 [n]: the persons' identities (tracking.PoseTracker.update only; None from estimate*)
    image: torch.Tensor = None       # uint8 BGR [H, W, 3] on the device: the source redacted (estimators with a `redactor`), then the poses
                                     # drawn in (estimators with a `renderer`); None without both.  A VIEW of the frame's canvas, valid until
                                     # the next call with the same source shape - .clone() it to keep it
    jpeg: bytes = None               # the frame (the canvas, or the source without a renderer and a redactor) as a baseline JPEG file
                                     # (estimators with an `encoder` only)
    keypoints_smooth: np.ndarray = None     # float64 [n, J, 3]: `keypoints` through the tracker's One-Euro filter, c unfiltered
                                     # (tracking.PoseTracker(smooth=...).update only)

    def __len__(self) -> int:
        return int(self.score.shape[0])

    def coco(self, image_id) -> List[dict]:
        """The COCO result dicts `datasets.naive_data.filter_poses` returns for this image."""
        return [{"image_id": image_id, "score": float(s), "category_id": 1, "keypoints": k.reshape(-1).tolist()}
                for k, s in zip(self.keypoints, self.score)]


def capture_graph(device, warm_up, body) -> torch.cuda.CUDAGraph:
    """`body()` recorded as one graph.  `warm_up()` runs first, on a side stream outside the capture: the activation pools and workspaces
    the launches need get allocated there (a capture cannot allocate them), and the device is idle when the capture begins."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        warm_up()
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    return graph


class _Frame:
    """The device buffers of one (batch, source shape, max_det): the static source, the plan, the crops, and ONE packed result buffer
    whose slices the kernels write directly, so that a call ends in a single device-to-host copy."""

    def __init__(self, B: int, H: int, W: int, max_det: int, cap: int, J: int, in_hw, device, flip_test: bool = False, smooth: bool = False):
        self.B, self.H, self.W, self.max_det = B, H, W, max_det
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        self.src = z((B, H, W, 3), torch.uint8)
        self.det = z((B, max_det, 6), torch.float32)
        self.src_index = z((cap,), torch.int32)
        self.m_inv = z((cap, 6), torch.float64)
        self.trans_inv = z((cap, 2, 3), torch.float32)
        self.center, self.scale = z((cap, 2), torch.float32), z((cap, 2), torch.float32)
        self.area, self.box_score = z((cap,), torch.float64), z((cap,), torch.float64)
        self.crops = z(((2 * cap if flip_test else cap), in_hw[0], in_hw[1], 3), torch.uint8)    # flip test: the crops, then their mirrors
        fields = (("kps64", (cap, J, 3), torch.float64), ("score", (cap,), torch.float64), ("box", (cap, 5), torch.float32),
                  ("keep", (cap,), torch.int32), ("keep_count", (B,), torch.int32), ("seg", (B + 1,), torch.int32),
                  ("status", (B,), torch.int32), ("dropped", (B,), torch.int32), ("counts", (B,), torch.int32),
                  ("track_id", (cap,), torch.int32))             # written by tracking.PoseTracker's frames only
        if smooth:                                               # the frames of a tracker that smooths: sp_track_smooth's output rides along
            fields += (("kps_smooth", (cap, J, 3), torch.float64),)
        self.layout, off = {}, 0
        for name, shape, dt in fields:
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
            self.layout[name] = (off, nbytes, shape, dt)
            off += (nbytes + 255) // 256 * 256
        self.pack = z((off,), torch.uint8)
        self.host = torch.empty(off, dtype=torch.uint8, pin_memory=True)
        for name, (o, nbytes, shape, dt) in self.layout.items():
            setattr(self, name, self.pack[o:o + nbytes].view(dt).view(shape))
        self.graph = None
        self.params = None
        self.keepalive = None
        self.tiles = None                # tiling.TilePlan: built with the first tiled detector frame of this shape
        self.canvas = None               # [B, H, W, 3]: allocated with the first frame of an estimator that has a renderer or a redactor
        self.render_ws = None            # the primitive array (a renderer's) and the region array (a redactor's), allocated likewise
        self.redact_ws = None
        self.heat_ws = None              # the records and u8 planes of an estimator with a heat overlay, allocated likewise
        self.hm = None                   # the heat maps the last _poses decoded (kept only for a heat overlay, which reads them)
        self.label_ws = None             # the record array, the captions [B, 64] and their pinned twin: allocated with the first frame of an
        self.caption = None              # estimator whose renderer draws text
        self.caption_host = None

    def fetch(self) -> Dict[str, np.ndarray]:
        """The call's one device-to-host transfer (and its one synchronisation)."""
        self.host.copy_(self.pack, non_blocking=True)
        torch.cuda.current_stream(self.pack.device).synchronize()
        h = self.host.numpy()
        np_dt = {torch.float64: np.float64, torch.float32: np.float32, torch.int32: np.int32}
        return {name: h[o:o + nbytes].view(np_dt[dt]).reshape(shape).copy() for name, (o, nbytes, shape, dt) in self.layout.items()}


class TopDownPoseEstimator(object):
    """Detector -> crops -> pose network -> decode -> rescoring + OKS-NMS, device resident.

    `detector`: a `YOLOv5Detector`; its `conf_thresh` / `iou_thresh` are read per call.  `pose_model`: any model with `hip_program`
    (ResNet-DConv / DUC, HRNet; fp32 or bf16 through `compute_dtype`), in eval mode.  `capacity`: person slots per call (1 .. 2048), shared
    by the images of a batch; the pose network always runs on `capacity` crops, selected detections beyond it are dropped from the end of
    the (image, detection) order and reported in `PoseResult.dropped`.  `person_cls`: the detector class kept (-1: every row, as the
    reference's gen_data_by_detector does); `min_box_score`: detections below it are not cropped.
    `use_graph`: `estimate` (batch 1) replays one captured graph per source shape (an LRU of MAX_GRAPHS shapes); False launches eagerly.
    `flip_test`: every crop also goes through the pose network mirrored (one forward on 2 x capacity crops) and the two sets of heat maps
    are merged before the decode (metrics.flip); `joint_pairs`: the left/right joints that swap (default: COCO's eight pairs);
    `shift_heatmap`: Simple-Baselines' SHIFT_HEATMAP on the un-mirrored maps.  `estimate`, `estimate_batch` and `estimate_boxes` honour it.
    `tiling`: a `tiling.Tiling` - the detector runs on overlapping tiles of every frame (and on the whole frame) and the boxes are fused
    on the device, so that small persons in large frames are found; `estimate`, same-sized `estimate_batch` and the trackers' detector
    frames honour it, a list of differently sized images together with it is refused, `estimate_boxes` has no detector to tile.
    `renderer`: a `visualize.PoseRenderer` - the kept poses drawn into `PoseResult.image`; `redactor`: a `visualize.Redactor` - the kept
    persons' heads (or the persons) hidden in `PoseResult.image`, before anything is drawn; `encoder`: a `datasets.jpeg.JpegEncoder` -
    `PoseResult.jpeg`; `heat_overlay`: a `visualize.HeatOverlay` - the kept persons' joint heat maps blended into `PoseResult.image`, over the
    redaction and under the poses.  Every entry point and the trackers honour the four."""

    MAX_GRAPHS = 8
    MAX_DET = 300                    # non_max_suppression's default, what single_predict uses

    def __init__(self, detector, pose_model, decoder=None, capacity: int = 32, person_cls: int = 0, min_box_score: float = 0.0,
                 in_vis_thre: float = 0.2, oks_thre: float = 0.9, input_shape=(192, 256), output_shape=(48, 64), flip_test: bool = False,
                 joint_pairs=None, shift_heatmap: bool = False, renderer=None, encoder=None, tiling=None, redactor=None, heat_overlay=None):
        from .detector.yolov5_detector import YOLOv5Detector
        from .metrics import BasicKeyPointDecoder, GaussTaylorKeyPointDecoder
        if not isinstance(capacity, int) or isinstance(capacity, bool) or not (1 <= capacity <= MAX_CAPACITY):
            raise ValueError(f"capacity: expected an int in 1..{MAX_CAPACITY} (the OKS-NMS group limit), got {capacity!r}")
        if not isinstance(detector, YOLOv5Detector):
            raise TypeError(f"detector: expected a YOLOv5Detector, got {type(detector).__name__}")
        if not callable(getattr(pose_model, "hip_program", None)):
            raise TypeError(f"pose_model: {type(pose_model).__name__} has no hip_program (expected a simple_pose_amd.nets model)")
        if getattr(pose_model, "training", False):
            raise ValueError("pose_model is in train() mode; the estimator runs the eval-mode program (call .eval())")
        if decoder is None:
            decoder = GaussTaylorKeyPointDecoder()
        if not isinstance(decoder, BasicKeyPointDecoder):
            raise TypeError(f"decoder: expected a simple_pose_amd.metrics key-point decoder, got {type(decoder).__name__}")
        if not isinstance(person_cls, int) or person_cls < -1:
            raise ValueError(f"person_cls: a class index, or -1 for every detection; got {person_cls!r}")
        if len(input_shape) != 2 or len(output_shape) != 2 or input_shape[0] % 32 or input_shape[1] % 32 or \
                tuple(output_shape) != (input_shape[0] // 4, input_shape[1] // 4):
            raise ValueError(f"input_shape (w, h) must be multiples of 32 and output_shape a quarter of it, got {input_shape} / {output_shape}")
        # type and disjointness now; the range once the program's joint count is known (_pose_program)
        self.joint_pairs = check_joint_pairs(COCO_JOINT_PAIRS if joint_pairs is None else joint_pairs)
        self.flip_test, self.shift_heatmap = bool(flip_test), bool(shift_heatmap)
        if renderer is not None and not isinstance(renderer, PoseRenderer):
            raise TypeError(f"renderer: expected a simple_pose_amd.visualize.PoseRenderer or None, got {type(renderer).__name__}")
        self.renderer = renderer
        if redactor is not None and not isinstance(redactor, Redactor):
            raise TypeError(f"redactor: expected a simple_pose_amd.visualize.Redactor or None, got {type(redactor).__name__}")
        self.redactor = redactor
        if heat_overlay is not None and not isinstance(heat_overlay, HeatOverlay):
            raise TypeError(f"heat_overlay: expected a simple_pose_amd.visualize.HeatOverlay or None, got {type(heat_overlay).__name__}")
        self.heat_overlay = heat_overlay
        if encoder is not None and not isinstance(encoder, JpegEncoder):
            raise TypeError(f"encoder: expected a simple_pose_amd.datasets.jpeg.JpegEncoder or None, got {type(encoder).__name__}")
        if encoder is not None and encoder.device != torch.device(detector.device):
            raise HipLibraryError(f"encoder: on {encoder.device}, the detector on {detector.device}")
        self.encoder = encoder
        if tiling is not None and not isinstance(tiling, Tiling):
            raise TypeError(f"tiling: expected a simple_pose_amd.tiling.Tiling or None, got {type(tiling).__name__}")
        self.tiling = tiling
        self._perm = None
        self.detector, self.pose_model, self.decoder = detector, pose_model, decoder
        self.capacity, self.person_cls, self.min_box_score = capacity, person_cls, float(min_box_score)
        self.in_vis_thre, self.oks_thre = float(in_vis_thre), float(oks_thre)
        self.input_shape, self.output_shape = tuple(int(v) for v in input_shape), tuple(int(v) for v in output_shape)
        self.device = detector.device
        self.use_graph = True
        self._frames: Dict[tuple, _Frame] = {}
        self._stage: dict = {}           # differently sized images: the pinned staging buffer and the device arena (mixed_batch.MixedBatch)
        self._force_mixed = False        # tests: send same-sized lists down the mixed path too
        self._jpeg_decoder = None        # estimate_files' own decoder, made on first use

    # -- programs and buffers ---------------------------------------------------------------------------------------------------------
    def _pose_program(self) -> engine.Program:
        iw, ih = self.input_shape
        prog = self.pose_model.hip_program(torch.empty((0, 3, ih, iw), device=self.device))
        if tuple(prog.out_shape[1:]) != (self.output_shape[1], self.output_shape[0]):
            raise HipLibraryError(f"pose program produces heat maps {tuple(prog.out_shape)}, expected [J, {self.output_shape[1]}, {self.output_shape[0]}]")
        n = self._pose_batch()
        if getattr(self.pose_model, "autotune", False) and n >= 16 and n >= 4 * prog.tuned_for_batch:
            # as forward_crops does at this batch size: pins the fastest tile per layer (speed only, same bits); never inside a capture
            prog.autotune(torch.zeros((n, ih, iw, 3), dtype=torch.uint8, device=self.device))
        if self.flip_test:                           # per call (a few ints): `joint_pairs` may have been reassigned; the range check happens here
            J = prog.out_shape[0]
            self._perm = (ctypes.c_int32 * J)(*pairs_to_perm(self.joint_pairs, J))
        return prog

    def _pose_batch(self) -> int:
        """Crops per run of the pose program: the slots, and with the flip test their mirrors."""
        return 2 * self.capacity if self.flip_test else self.capacity

    def _frame(self, B: int, H: int, W: int, max_det: int, J: int, smooth: bool = False) -> _Frame:
        key = (B, H, W, max_det, J, self.flip_test) + ((True,) if smooth else ())
        fr = self._frames.get(key)
        if fr is None:
            if len(self._frames) >= self.MAX_GRAPHS:
                self._frames.pop(next(iter(self._frames)))
            fr = _Frame(B, H, W, max_det, self.capacity, J, (self.input_shape[1], self.input_shape[0]), self.device, self.flip_test, smooth)
        else:
            self._frames.pop(key)                # most recently used last
        self._frames[key] = fr
        if self._draws() and fr.canvas is None:
            fr.canvas = torch.zeros((B, H, W, 3), dtype=torch.uint8, device=self.device)
        if self.renderer is not None and fr.render_ws is None:
            fr.render_ws = PoseRenderer.workspace(self.capacity, J, self.device)
        if self.redactor is not None and fr.redact_ws is None:
            fr.redact_ws = Redactor.workspace(self.capacity, self.device)
        if self.heat_overlay is not None and fr.heat_ws is None:
            fr.heat_ws = HeatOverlay.workspace(self.capacity, self.output_shape[1], self.output_shape[0], self.device)
        if self.heat_overlay is not None:
            self.heat_overlay.table(self.device)         # uploaded here, ahead of any capture
        if self.renderer is not None and self.renderer.has_text and fr.label_ws is None:
            fr.label_ws = PoseRenderer.label_workspace(self.capacity, self.device)
            fr.caption = torch.zeros((B, _lib.SP_LABEL_CAPTION_BYTES), dtype=torch.uint8, device=self.device)
            fr.caption_host = torch.zeros((B, _lib.SP_LABEL_CAPTION_BYTES), dtype=torch.uint8).pin_memory()
        return fr

    def _draws(self) -> bool:
        """Does a frame have a canvas (`PoseResult.image`) ?  With a redactor, a heat overlay or a renderer."""
        return self.renderer is not None or self.redactor is not None or self.heat_overlay is not None

    def _stage_caption(self, fr: _Frame) -> None:
        """`renderer.caption` as it reads now into the frame's caption buffer: through the pinned twin, by a copy on the frame's stream
        ahead of the launches or the replay that read it, never inside a capture (as a tracker stages its times) - so a captured frame
        shows a reassigned caption with its next replay.  A list of another length than the frame has images: ValueError, before any
        launch.  Nothing without a caption."""
        if self.renderer is None or self.renderer.caption is None:
            return
        fr.caption_host.copy_(torch.from_numpy(self.renderer.caption_rows(fr.B)))
        fr.caption.copy_(fr.caption_host, non_blocking=True)

    def _load(self, fr: _Frame, imgs) -> None:
        """The images into the frame's static source buffer (host -> device, or a device copy; video frames by one conversion launch in
        place of the copy: sp_yuv420_to_bgr_u8c3, or the table launch for several frames or host planes)."""
        if isinstance(imgs, YuvBatch):
            for i, f in enumerate(imgs.frames):
                if not f.is_host and f.device != fr.src.device:
                    raise HipLibraryError(f"image {i}: on {f.device}, the detector on {fr.src.device}")
            convert_into(imgs.frames, list(fr.src), self._stage.setdefault("yuv", {}), dense=fr.src)
            return
        if isinstance(imgs, np.ndarray):
            if imgs.dtype != np.uint8:
                raise TypeError(f"expected a uint8 BGR image, got {imgs.dtype}")
            imgs = torch.from_numpy(np.ascontiguousarray(imgs))
        elif not imgs.is_cuda:
            raise HipLibraryError(f"image tensor is on {imgs.device}; simple_pose_amd runs on the MI355X only (no CPU fallback)")
        if imgs.dtype != torch.uint8:
            raise TypeError(f"expected a uint8 BGR image, got {imgs.dtype}")
        fr.src.copy_(imgs.reshape(fr.src.shape))

    @staticmethod
    def _shape_of(imgs, batched: bool):
        """The image or batch as the frame takes it.  A video.YuvFrame passes as the [H, W, 3] image it stands for (`frame[None]` is its
        batch of one), same-sized frames as a YuvBatch; they were checked when they were made."""
        if isinstance(imgs, YuvFrame) and not batched:
            return imgs
        if isinstance(imgs, YuvBatch) and batched:
            return imgs
        if isinstance(imgs, (list, tuple)):
            if not batched:
                raise ValueError("estimate takes one image [H, W, 3]")
            shapes = {tuple(np.shape(i)) for i in imgs}
            if len(shapes) != 1:
                raise ValueError("the images of one batch share one size")
            if all(isinstance(i, YuvFrame) for i in imgs):
                return YuvBatch(imgs)
            imgs = resolve(imgs)                     # frames next to BGR images: converted, then stacked with them
            if any(isinstance(i, torch.Tensor) for i in imgs):
                imgs = torch.stack(list(imgs))
            else:
                imgs = np.stack([np.asarray(i) for i in imgs])
        if not isinstance(imgs, (np.ndarray, torch.Tensor)):
            raise TypeError(f"expected a uint8 BGR image (numpy or CUDA), got {type(imgs).__name__}")
        if isinstance(imgs, torch.Tensor) and not imgs.is_cuda:
            raise HipLibraryError(f"image tensor is on {imgs.device}; simple_pose_amd runs on the MI355X only (no CPU fallback)")
        want = 4 if batched else 3
        if len(imgs.shape) != want or imgs.shape[-1] != 3 or 0 in tuple(imgs.shape):
            raise ValueError(f"expected uint8 BGR {'[B, H, W, 3]' if batched else '[H, W, 3]'}, got {tuple(imgs.shape)}")
        return imgs

    # -- the frame: every launch between the source image and the packed result -------------------------------------------------------
    def _params(self, det_prog, pose_prog) -> tuple:
        d = self.detector
        det_id = tuple(id(p) for p in det_prog) if isinstance(det_prog, tuple) else id(det_prog)
        return (float(d.conf_thresh), float(d.iou_thresh), self.person_cls, self.min_box_score, self.in_vis_thre, self.oks_thre,
                det_id, id(pose_prog), id(self.decoder), self.flip_test, tuple(self._perm or ()), self.shift_heatmap,
                None if self.renderer is None else self.renderer.key(), None if self.tiling is None else self.tiling.key(),
                None if self.redactor is None else self.redactor.key()) + \
            (() if self.heat_overlay is None else ((self.heat_overlay.key(), id(self.heat_overlay)),))

    def _det_program(self, B: int, H: int, W: int):
        """What `_detect` runs on B frames of H x W: the detector program of their letterboxed shape, or, with a tiling, the programs of
        the passes' net-shape groups (a tuple, in group order).  Raises before any launch what the tiling refuses for this shape."""
        d = self.detector
        if self.tiling is None:
            g = d.transform.geometry(H, W)
            return d.program(g["out_h"], g["out_w"])
        _, groups = plan_pass_groups(self.tiling.plan_call(B, H, W), d.transform)
        return tuple(d.program(out_h, out_w) for (out_h, out_w), _ in groups)

    def _det_keepalive(self, fr: _Frame, det_prog) -> tuple:
        """What a captured detector half points into: the programs, their activation pools and the NMS workspaces."""
        if det_prog is None:
            return (None, None, None)
        if isinstance(det_prog, tuple):
            return (det_prog, fr.tiles, tuple(fr.tiles.keepalive))
        return (det_prog, det_prog.pool_for(fr.B, self.device), getattr(fr, "ws", None))

    def _detect_tiled(self, fr: _Frame, det_progs: tuple, single_stream: bool) -> None:
        """_detect with a tiling: detector.detect_tiled over the table that points into the frame's static source.  The table is built
        and uploaded with the first call of a frame shape (never inside a capture: every capture here is preceded by a warm-up run)."""
        d = self.detector
        if fr.tiles is None or fr.tiles.key != TilePlan.key_of(self.tiling, d.transform, fr.src, fr.max_det):
            if torch.cuda.is_current_stream_capturing():
                raise HipLibraryError("tiled detection: the table of passes cannot be uploaded inside a stream capture")
            fr.tiles = TilePlan(self.tiling, d.transform, fr.src, fr.max_det)
        d.detect_tiled(fr.tiles, det_progs, fr.det, fr.counts, fr.status, fr.max_det, self.tiling, single_stream)

    def _detect(self, fr: _Frame, det_prog, single_stream: bool = False) -> None:
        """letterbox + network + head decode, NMS and the un-letterbox, all on the device (what single_predict / predict compute)."""
        if isinstance(det_prog, tuple):              # the programs of a tiling's groups (_det_program)
            return self._detect_tiled(fr, det_prog, single_stream)
        lib, d = _lib.lib(), self.detector
        from .detector.yolov5_detector import _workspace
        g = d.transform.geometry(fr.H, fr.W)
        engine.set_letterbox(det_prog, fr.H, fr.W, g["new_h"], g["new_w"], g["top"], g["left"])
        pred = det_prog.run_on_stream(fr.src, single_stream)
        B, N, no = pred.shape
        ws = _workspace(B, pred.device)
        stream = _lib.current_stream(self.device)
        fr.det.zero_()
        _lib.check(lib.sp_yolo_nms_device(P(pred), B, N, no, float(d.conf_thresh), float(d.iou_thresh), 1, 1, 0, fr.max_det, P(ws), ws.numel(),
                                          P(fr.det), P(fr.counts), P(fr.status), stream), "sp_yolo_nms_device")
        # every row: the rows past counts[b] are zeros, and the plan never reads them
        _lib.check(lib.sp_yolo_boxes_to_source(P(fr.det), B * fr.max_det, float(g["out_h"]), float(g["out_w"]), float(g["left"]), float(g["top"]),
                                               float(g["ratio"]), stream), "sp_yolo_boxes_to_source")
        fr.ws = ws                                   # (a captured graph holds its pointer)

    def _poses(self, fr: _Frame, pose_prog, single_stream: bool, images: torch.Tensor = None) -> None:
        """plan -> crops -> pose forward -> decode -> rescore -> OKS-NMS over the frame's `det` / `counts`.  `images`: the table of
        sp_image_ref of a batch of differently sized images, in the caller's order (the crops then come from it instead of `fr.src`)."""
        lib, cap = _lib.lib(), self.capacity
        stream = _lib.current_stream(self.device)
        iw, ih = self.input_shape
        ow, oh = self.output_shape
        J = pose_prog.out_shape[0]
        _lib.check(lib.sp_topdown_plan(P(fr.det), P(fr.counts), fr.B, fr.max_det, self.person_cls, self.min_box_score, cap, iw, ih, ow, oh,
                                       P(fr.seg), P(fr.src_index), P(fr.m_inv), P(fr.trans_inv), P(fr.center), P(fr.scale), P(fr.area),
                                       P(fr.box_score), P(fr.box), P(fr.dropped), stream), "sp_topdown_plan")
        if images is None:
            _lib.check(lib.sp_warp_affine_plan_u8c3(P(fr.src), fr.B, fr.H, fr.W, P(fr.m_inv), P(fr.src_index), P(fr.seg), cap, P(fr.crops), ih, iw,
                                                    stream), "sp_warp_affine_plan_u8c3")
        else:
            _lib.check(lib.sp_warp_affine_plan_images_u8c3(P(images), fr.B, P(fr.m_inv), P(fr.src_index), P(fr.seg), cap, P(fr.crops), ih, iw,
                                                           stream), "sp_warp_affine_plan_images_u8c3")
        if self.flip_test:
            half = fr.crops[:cap]
            _lib.check(lib.sp_mirror_w(P(half), P(fr.crops[cap:]), cap * ih, iw, 3, stream), "sp_mirror_w")     # dead slots: zeros mirror to zeros
        hm = pose_prog.run_on_stream(fr.crops, single_stream)
        if self.flip_test:
            hm = hm[:cap]                            # merged in place; the decode sees the first `capacity` maps only
            _lib.check(lib.sp_heat_map_flip_merge(P(hm), P(hm) + hm.numel() * 4, self._perm, cap, J, oh, ow, int(self.shift_heatmap), P(hm),
                                                  stream), "sp_heat_map_flip_merge")
        if self.heat_overlay is not None:
            fr.hm = hm                               # what the decode reads is what the overlay shows (_render)
        kps, mv = self.decoder(hm, fr.trans_inv)
        kps3 = torch.cat([kps, mv], -1)              # eval.py:138
        _lib.check(lib.sp_pose_rescore(P(kps3), P(fr.box_score), cap, J, self.in_vis_thre, P(fr.kps64), P(fr.score), stream), "sp_pose_rescore")
        _lib.check(lib.sp_oks_nms(P(fr.kps64), P(fr.score), P(fr.area), P(fr.seg), fr.B, cap, J, None, self.oks_thre, -1.0, P(fr.keep),
                                  P(fr.keep_count), stream), "sp_oks_nms")

    def _render(self, fr: _Frame, J: int, tracked: bool = False, kps: torch.Tensor = None) -> None:
        """The overlay of every image's kept poses into the frame's canvas: one sp_render_poses_u8c3 (two launches) per image index, reading
        the buffers sp_oks_nms (and, `tracked`, sp_track_associate) just wrote; `kps`: the poses to draw instead of the frame's own (a
        smoothing tracker's kps_smooth).  A renderer with text then labels the canvas (sp_render_labels_u8c3, two more launches) from the
        frame's scores, ids and staged captions (_stage_caption, which the caller ran outside any capture).  With a redactor the canvas
        comes from sp_redact_u8c3 first (two launches, source -> canvas, always from the frame's raw kps64) and the renderer then draws in
        place on it.  With a heat overlay sp_heat_overlay_u8c3 (two launches) runs between the two - from the source when nothing was
        redacted, in place on the canvas otherwise - so the order is redaction, heat, capsules, text.  Nothing without any of the three."""
        if not self._draws():
            return
        for b in range(fr.B):
            src = fr.src[b]
            if self.redactor is not None:
                self.redactor.launch(src, fr.canvas[b], fr.kps64, fr.box, fr.keep, fr.keep_count, fr.seg, b, self.capacity, J, fr.redact_ws)
                src = fr.canvas[b]
            if self.heat_overlay is not None:
                self.heat_overlay.launch(src, fr.canvas[b], fr.hm, fr.trans_inv, fr.keep, fr.keep_count, fr.seg, b, self.capacity, fr.heat_ws)
                src = fr.canvas[b]
            if self.renderer is not None:
                self.renderer.launch(src, fr.canvas[b], fr.kps64 if kps is None else kps, fr.box, fr.track_id if tracked else None, fr.keep,
                                     fr.keep_count, fr.seg, b, self.capacity, J, fr.render_ws, score=fr.score, caption=fr.caption,
                                     label_workspace=fr.label_ws)

    def _issue(self, fr: _Frame, det_prog, pose_prog, single_stream: bool) -> None:
        """The frame's launches: detector, poses, redaction and overlay."""
        self._detect(fr, det_prog, single_stream)
        self._poses(fr, pose_prog, single_stream)
        self._render(fr, pose_prog.out_shape[0])

    def _capture(self, fr: _Frame, det_prog, pose_prog) -> None:
        issue = lambda: self._issue(fr, det_prog, pose_prog, True)
        fr.graph, fr.params = capture_graph(self.device, issue, issue), self._params(det_prog, pose_prog)
        # the nodes hold raw pointers into both programs' activation pools: keep them alive whatever Program._alloc evicts later
        # (and, with a heat overlay, into the heat maps of the captured run: a fresh tensor per run, so the tensor itself is kept)
        fr.keepalive = (pose_prog, pose_prog.pool_for(self._pose_batch(), self.device), fr.hm) + self._det_keepalive(fr, det_prog)

    def _results(self, fr: _Frame, tracked: bool = False, detected: bool = True) -> List[PoseResult]:
        """`tracked`: the frame carries track ids; `detected`: the detector's NMS wrote the status words of this frame."""
        # the frames as JPEG files: launched behind the frame on its stream, before the fetch that waits for both
        drawn = self._draws()
        enc = None if self.encoder is None else self.encoder.encode_device(fr.canvas if drawn else fr.src)
        h = fr.fetch()
        files = [None] * fr.B if enc is None else self.encoder.collect(*enc)
        if detected and (h["status"] & 1).any():
            b = int(np.nonzero(h["status"] & 1)[0][0])
            raise HipLibraryError(f"image {b}: more than {_lib.SP_YOLO_NMS_MAX_CANDIDATES} detector candidates after the multi-label expansion "
                                  "(raise the detector's conf_thresh)")
        out = []
        for b in range(fr.B):
            lo, n = int(h["seg"][b]), int(h["keep_count"][b])
            if n < 0:
                raise HipLibraryError(f"image {b}: more than {MAX_CAPACITY} persons")
            rows = h["keep"][lo:lo + n]
            out.append(PoseResult(h["kps64"][rows], h["score"][rows], h["box"][rows], int(h["dropped"][b]),
                                  h["track_id"][rows] if tracked else None, fr.canvas[b] if drawn else None, files[b],
                                  h["kps_smooth"][rows] if tracked and "kps_smooth" in h else None))
        return out

    # -- public surface -----------------------------------------------------------------------------------------------------------------
    def _run(self, imgs, graph: bool) -> List[PoseResult]:
        # Both program lookups validate their cache against every parameter's (data_ptr, version) - a walk over a few hundred tensors per
        # call, replays included.  It is what notices in-place weight updates (and forces the re-capture); it is also host time that a
        # replay does not get back, one reason the graphed frame is no faster than the eager one while the GPU is the longer side.
        B, H, W = imgs.shape[0], imgs.shape[1], imgs.shape[2]
        det_prog = self._det_program(B, H, W)
        pose_prog = self._pose_program()
        fr = self._frame(B, H, W, self.MAX_DET, pose_prog.out_shape[0])
        self._stage_caption(fr)
        self._load(fr, imgs)
        if graph:
            if fr.graph is None or fr.params != self._params(det_prog, pose_prog):
                self._capture(fr, det_prog, pose_prog)
            fr.hm = fr.keepalive[2]                  # the heat maps the graph writes (an eager run in between left its own; None without an overlay)
            fr.graph.replay()
        else:
            self._issue(fr, det_prog, pose_prog, False)
        return self._results(fr)

    @torch.no_grad()
    def estimate(self, img) -> PoseResult:
        """One uint8 BGR image [H, W, 3] (numpy or CUDA), or one video.YuvFrame (NV12 / I420 planes) -> the persons in it."""
        img = self._shape_of(img, batched=False)
        return self._run(img[None], self.use_graph)[0]

    # -- differently sized images ---------------------------------------------------------------------------------------------------------
    def _is_mixed(self, imgs) -> bool:
        """A list whose images differ in size (or any list, with the tests' private switch); an empty list fails in check_images.  A list
        in which video frames stand next to BGR images goes this way too: its frames become BGR tensors by one table launch."""
        if not isinstance(imgs, (list, tuple)):
            return False
        if len({isinstance(i, YuvFrame) for i in imgs}) == 2:
            return True
        return self._force_mixed or len({tuple(np.shape(i)) for i in imgs}) != 1

    def _mixed_frame(self, mb: MixedBatch, max_det: int, J: int) -> _Frame:
        """The frame of a mixed batch: keyed without a source shape (H = W = 0: no dense source block); `src` is the call's list of images
        and `canvas` a list of per-image canvases, which _render, the encoder and _results index like the dense blocks."""
        fr = self._frame(mb.B, 0, 0, max_det, J)
        fr.src = mb.srcs
        if self._draws():
            fr.canvas = [torch.empty_like(s) for s in mb.srcs]
        return fr

    def _detect_mixed(self, fr: _Frame, mb: MixedBatch) -> None:
        """_detect per net-shape group: letterbox (through the table) + network + head decode, NMS on the device, then the un-letterbox
        with every image's own offsets, which also scatters the group's rows into the frame's `det` / `counts` / `status` in caller order."""
        lib, d = _lib.lib(), self.detector
        from .detector.yolov5_detector import _workspace
        stream = _lib.current_stream(self.device)
        for k, ((out_h, out_w), members) in enumerate(mb.groups):
            prog = d.program(out_h, out_w)
            engine.set_letterbox_images(prog)
            table = mb.group_table(k)
            pred = prog.run_on_stream(table, False)
            n, N, no = pred.shape
            ws = _workspace(n, pred.device)
            det = torch.empty((n, fr.max_det, 6), dtype=torch.float32, device=pred.device)
            cnt = torch.empty((2, n), dtype=torch.int32, device=pred.device)     # counts, status
            _lib.check(lib.sp_yolo_nms_device(P(pred), n, N, no, float(d.conf_thresh), float(d.iou_thresh), 1, 1, 0, fr.max_det, P(ws), ws.numel(),
                                              P(det), P(cnt[0]), P(cnt[1]), stream), "sp_yolo_nms_device")
            _lib.check(lib.sp_yolo_boxes_to_source_images(P(det), P(cnt[0]), P(cnt[1]), P(table), n, fr.max_det, float(out_h), float(out_w),
                                                          P(fr.det), P(fr.counts), P(fr.status), stream), "sp_yolo_boxes_to_source_images")

    def _run_mixed(self, imgs, det=None, counts=None) -> List[PoseResult]:
        """estimate_batch / estimate_boxes on a list of differently sized images.  Eager: the table upload is not capturable."""
        n = len(check_images(imgs))                  # every check before the first launch
        if det is None and self.tiling is not None:
            raise ValueError("tiling: the images of one call share one size (tiled detection of differently sized images is not supported)")
        M = self.MAX_DET if det is None else check_det_counts(n, det, counts)
        if getattr(self.detector, "transform", None) is None:
            # without the detector's letterbox the images cannot be grouped by net shape: the dense path's rule is all that is left
            raise ValueError("the images of one batch share one size (differently sized images are grouped by the detector's letterbox, "
                             "detector.transform, which this detector does not have)")
        if det is not None:
            det, cnt = self._det_counts(n, det, counts)
        pose_prog = self._pose_program()
        mb = MixedBatch(imgs, self.detector.transform, self.device, self._stage)
        fr = self._mixed_frame(mb, M, pose_prog.out_shape[0])
        self._stage_caption(fr)
        if det is None:
            self._detect_mixed(fr, mb)
        else:
            fr.det.copy_(det)
            fr.counts.copy_(cnt)
            fr.status.zero_()
        self._poses(fr, pose_prog, False, mb.caller_table)
        self._render(fr, pose_prog.out_shape[0])
        return self._results(fr, detected=det is None)         # `mb` holds the caller's CUDA images until this fetch

    @torch.no_grad()
    def estimate_batch(self, imgs: Union[torch.Tensor, np.ndarray, Sequence]) -> List[PoseResult]:
        """A batch of images -> one PoseResult per image, in the caller's order.  Same-sized ([B, H, W, 3], or a list of [H, W, 3]): one
        forward of the detector on B images.  A list of differently sized images (numpy or CUDA): one detector forward per letterboxed net
        shape, every image letterboxed as `estimate` letterboxes it alone.  Either way one pose forward on the `capacity` slots the images
        share and one device-to-host transfer.  video.YuvFrames stand where images stand: same-sized frames are converted into the static
        source by one launch, a list of other sizes (or of frames next to BGR images) has its frames converted by one launch first."""
        if self._is_mixed(imgs):
            return self._run_mixed(imgs)
        return self._run(self._shape_of(imgs, batched=True), False)

    @torch.no_grad()
    def estimate_files(self, files, decoder=None) -> List[PoseResult]:
        """JPEG files (paths or bytes, of any sizes) -> one PoseResult per file: `JpegDecoder.decode`, then the batch on the decoder's device
        tensors; nothing goes through the host in between.  `decoder`: a datasets.jpeg.JpegDecoder (default: one on this device, kept)."""
        if decoder is None:
            if self._jpeg_decoder is None:
                self._jpeg_decoder = JpegDecoder(device=self.device)
            decoder = self._jpeg_decoder
        if not isinstance(decoder, JpegDecoder):
            raise TypeError(f"decoder: expected a simple_pose_amd.datasets.jpeg.JpegDecoder or None, got {type(decoder).__name__}")
        if not isinstance(files, (list, tuple)) or len(files) == 0:
            raise ValueError("estimate_files takes a non-empty list of JPEG files")
        datas = []
        for f in files:
            if isinstance(f, (str, os.PathLike)):
                with open(f, "rb") as fh:
                    f = fh.read()
            datas.append(f)
        return self.estimate_batch(list(decoder.decode(datas)))

    @torch.no_grad()
    def estimate_boxes(self, imgs, det, counts=None) -> List[PoseResult]:
        """Caller-supplied detections instead of the detector (the reference's predicts_by_pred path): imgs [B, H, W, 3] (or one image
        [H, W, 3]), det fp32 [B, M, 6] (or [M, 6]) rows (x1, y1, x2, y2, score, cls) in source pixels, counts int [B] valid rows per image
        (default: all M).  Selection (`person_cls`, `min_box_score`, `capacity`) applies as in `estimate`.  A list of differently sized
        images is taken as in `estimate_batch`, with det [B, M, 6] / counts [B] in the list's order."""
        if self._is_mixed(imgs):
            return self._run_mixed(imgs, det, counts)
        single = len(getattr(imgs, "shape", ())) == 3
        imgs = self._shape_of(imgs[None] if single else imgs, batched=True)
        B, H, W = imgs.shape[0], imgs.shape[1], imgs.shape[2]
        det, cnt = self._det_counts(B, det, counts)
        M = det.shape[1]
        pose_prog = self._pose_program()
        fr = self._frame(B, H, W, M, pose_prog.out_shape[0])
        self._stage_caption(fr)
        self._load(fr, imgs)
        fr.det.copy_(det)
        fr.counts.copy_(cnt)
        fr.status.zero_()
        self._poses(fr, pose_prog, False)
        self._render(fr, pose_prog.out_shape[0])
        return self._results(fr)

    def _det_counts(self, B: int, det, counts):
        """Caller-supplied detections of B images -> (det fp32 [B, M, 6], counts int32 [B]) on the device."""
        if isinstance(det, np.ndarray):
            det = torch.from_numpy(np.ascontiguousarray(det, dtype=np.float32)).to(self.device)
        if not (isinstance(det, torch.Tensor) and det.is_cuda and det.dtype == torch.float32):
            raise HipLibraryError("det: expected float32 detections [B, M, 6] (numpy or CUDA)")
        if det.dim() == 2:
            det = det[None]
        if det.dim() != 3 or det.shape[0] != B or det.shape[2] != 6 or det.shape[1] == 0:
            raise ValueError(f"det: expected [{B}, M, 6], got {tuple(det.shape)}")
        M = det.shape[1]
        if counts is None:
            counts = [M] * B
        if isinstance(counts, torch.Tensor):
            cnt = counts.to(device=self.device, dtype=torch.int32).reshape(-1)
        else:
            cnt = torch.from_numpy(np.ascontiguousarray(np.asarray(counts, dtype=np.int32).reshape(-1))).to(self.device)
        if cnt.numel() != B:
            raise ValueError(f"counts: expected {B} values")
        return det, cnt
