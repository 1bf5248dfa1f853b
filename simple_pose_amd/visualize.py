"""Poses drawn into frames on the device: skeleton limbs, joints and boxes, coloured by person (track id) or by part.

    r = PoseRenderer(skeleton=COCO_SKELETON, joint_radius=3.0, limb_width=2.0, box_width=1.0, opacity=1.0, in_vis_thre=0.2,
                     colour_by="person", palette=None, label=None, label_scale=2, label_opacity=1.0,
                     caption=None, caption_scale=2, caption_corner="tl", caption_opacity=0.75)
    out = r.render(img, result)                                   # uint8 BGR [H,W,3] (numpy or CUDA) + a PoseResult -> CUDA uint8 [H,W,3]
    est = TopDownPoseEstimator(detector, pose_model, renderer=r)  # in the frame: PoseResult.image, drawn inside the frame's own graph

The rasteriser is sp_render_poses_u8c3 (csrc/render.hip, the pixel rules in csrc/sp_render.h and include/simple_pose_hip.h): every
primitive is a capsule in 1/16 px, covered pixels are blended by 16 samples each, persons are painted in reverse pick order so that the
best pose lies on top.  Inside an estimator or a tracker the two launches follow sp_oks_nms / sp_track_associate on the same stream and
read the frame's buffers directly; the person count never reaches the host.  `render` is the same kernels on the rows of a PoseResult that
is already on the host.  There is no CPU fallback.

Text is sp_render_labels_u8c3 (csrc/labels.hip, the rules in csrc/sp_label.h, the 5 x 7 font in csrc/sp_font.h), two more launches behind
the overlay's, in place on the canvas.  `label="#{id} {score}"` puts a plate in the person's colour at the first corner of every kept
person's box: `{id}` is the track id (the pick position + 1 without a tracker), `{score}` the pose score, `{conf}` the detector's
confidence, formatted on the device from the frame's buffers.  `caption="cam 3: {n} persons"` (one string, or one per image) puts a black
plate into a corner of the frame: `{n}` is the image's kept count, `{image}` its index.  `{{` and `}}` are literal braces.  The caption
can be reassigned at any time (`renderer.caption = ...`): an estimator stages its bytes through a pinned buffer ahead of the launches or
the replay, so a captured frame shows the new text without being captured again.  The font is ASCII only.

    x = Redactor(region="head", mode="mosaic", cell=16)            # or region="person", mode="fill", fill=(0, 0, 0)
    out = x.redact(img, result)                                   # the heads of the result's persons behind a mosaic
    est = TopDownPoseEstimator(detector, pose_model, redactor=x)  # in the frame: PoseResult.image is redacted before anything is drawn

Redaction is sp_redact_u8c3 (csrc/redact.hip, the rules in csrc/sp_redact.h and include/simple_pose_hip.h), two launches: the frame is cut
into `cell` x `cell` pixel cells, and every cell that a person's region meets - a disc around the visible head joints, or the box - becomes
the mean of its source pixels (mosaic) or a constant colour (fill), as a whole.  Inside an estimator or a tracker it produces the canvas
from the source ahead of the renderer's launches, from the RAW key points of this frame (under a smoothing tracker as well).

    h = HeatOverlay(colormap="jet", opacity=0.6, alpha="value", threshold=0.1)
    out = h.overlay(img, heat_maps, trans_inv)                    # CUDA fp32 [n, J, h, w] maps through [n, 2, 3] maps -> image
    est = TopDownPoseEstimator(detector, pose_model, heat_overlay=h)   # in the frame: the kept persons' maps, under the skeleton

The heat overlay is sp_heat_overlay_u8c3 (csrc/heat.hip, the rules in csrc/sp_heat.h and include/simple_pose_hip.h), two launches: what
the reference's draw_heat_map shows in a window - the maximum over the joints' maps times 255 - warped back into the frame through each
kept person's trans_inv and blended in through a colour table."""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from ._lib import HipLibraryError

P = _lib.ptr
# the usual 19 COCO limbs, 0-based (pycocotools' person skeleton minus one)
COCO_SKELETON = ((15, 13), (13, 11), (16, 14), (14, 12), (11, 12), (5, 11), (6, 12), (5, 6), (5, 7), (6, 8), (7, 9), (8, 10), (1, 2), (0, 1),
                 (0, 2), (1, 3), (2, 4), (3, 5), (4, 6))
# BGR, told apart at a glance; ids and parts cycle through it
DEFAULT_PALETTE = ((56, 56, 255), (31, 112, 255), (29, 178, 255), (49, 210, 207), (10, 249, 72), (23, 204, 146), (134, 219, 61), (52, 147, 26),
                   (187, 212, 0), (168, 153, 44), (255, 194, 0), (255, 115, 100), (236, 24, 0), (255, 56, 132), (133, 0, 82), (255, 56, 203),
                   (200, 149, 255), (199, 55, 255), (151, 157, 255), (128, 128, 128))
MAX_RADIUS_PX = _lib.SP_RENDER_MAX_RADIUS / 16.0


LABEL_FIELDS = ("id", "score", "conf")       # what a label may hold; a caption holds the other two
CAPTION_FIELDS = ("n", "image")


def parse_template(text, fields, limit: int, what: str) -> bytes:
    """"#{id} {score}" -> the bytes sp_render_labels_u8c3 takes: printable ASCII stays, `{name}` becomes the field's byte (0x01 .. 0x05),
    `{{` and `}}` are literal braces.  ValueError for a field that is not in `fields`, a lone brace, a character outside printable ASCII or
    more than `limit` bytes."""
    if not isinstance(text, str):
        raise ValueError(f"{what}: expected a string, got {type(text).__name__}")
    out, i = bytearray(), 0
    while i < len(text):
        c = text[i]
        if c in "{}" and text[i:i + 2] == c + c:
            out.append(ord(c))
            i += 2
        elif c == "{":
            j = text.find("}", i)
            name = text[i + 1:j] if j > 0 else None
            if name is None or name not in _lib.SP_LABEL_FIELDS:
                raise ValueError(f"{what}: unknown field {text[i:j + 1] if j > 0 else text[i:]!r} in {text!r} (fields: "
                                 f"{', '.join('{' + f + '}' for f in fields)}; a literal brace is doubled)")
            if name not in fields:
                raise ValueError(f"{what}: {{{name}}} is not a field of this text (fields: {', '.join('{' + f + '}' for f in fields)})")
            out.append(_lib.SP_LABEL_FIELDS[name])
            i = j + 1
        elif c == "}":
            raise ValueError(f"{what}: a lone '}}' in {text!r} (a literal brace is doubled)")
        elif not (0x20 <= ord(c) <= 0x7E):
            raise ValueError(f"{what}: {c!r} in {text!r} is not printable ASCII (the built-in font has nothing else)")
        else:
            out.append(ord(c))
            i += 1
    if len(out) > limit:
        raise ValueError(f"{what}: {len(out)} bytes, at most {limit} (a field counts as one)")
    return bytes(out)


def _number(name, v, lo, hi, what):
    if not isinstance(v, (int, float)) or isinstance(v, bool) or not (lo <= float(v) <= hi):
        raise ValueError(f"{name}: {what}, got {v!r}")
    return float(v)


def _image_and_out(img, out):
    """`img` (uint8 BGR [H, W, 3], numpy or CUDA) as a contiguous CUDA tensor, and `out` checked against it (a new tensor when None)."""
    if isinstance(img, np.ndarray):
        if img.dtype != np.uint8:
            raise TypeError(f"expected a uint8 BGR image, got {img.dtype}")
        img = torch.from_numpy(np.ascontiguousarray(img)).to("cuda")
    if not isinstance(img, torch.Tensor):
        raise TypeError(f"expected a uint8 BGR image (numpy or CUDA), got {type(img).__name__}")
    if not img.is_cuda:
        raise HipLibraryError(f"image tensor is on {img.device}; simple_pose_amd runs on the MI355X only (no CPU fallback)")
    if img.dtype != torch.uint8:
        raise TypeError(f"expected a uint8 BGR image, got {img.dtype}")
    if img.dim() != 3 or img.shape[2] != 3 or 0 in tuple(img.shape):
        raise ValueError(f"expected uint8 BGR [H, W, 3], got {tuple(img.shape)}")
    img = img.contiguous()
    if out is None:
        out = torch.empty_like(img)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.shape == img.shape and out.is_contiguous()
              and out.device == img.device):
        raise ValueError(f"out: expected a contiguous CUDA uint8 tensor {tuple(img.shape)} on {img.device}")
    return img, out


def _joint_indices(values, least: int, most, message: str, pairs: bool = False) -> list:
    """`values` (with `pairs`: pairs of them, returned flat) as a list of `least` .. `most` (None: any number of) joint indices in 0..63;
    anything else: ValueError(message)."""
    try:
        flat = [v for a, b in values for v in (a, b)] if pairs else list(values)
        ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in flat)
        out = [int(v) for v in flat] if ok else []
    except (TypeError, ValueError):
        out, ok = [], False
    if not ok or len(out) < least or (most is not None and len(out) > most) or any(v < 0 or v >= 64 for v in out):
        raise ValueError(message)
    return out


def _workspace(entry: str, least: int, device, *shape) -> torch.Tensor:
    """What the library's `entry`(*shape, &bytes) asks for as a zeroed uint8 tensor, of at least `least` bytes (so that it has a pointer)."""
    n = ctypes.c_int64()
    _lib.check(getattr(_lib.lib(), entry)(*shape, ctypes.byref(n)), entry)
    return torch.zeros((max(int(n.value), least),), dtype=torch.uint8, device=device)


def _copy_through(img, out):
    """Nothing is kept, so nothing is drawn: `out` holds the image."""
    if out.data_ptr() != img.data_ptr():
        out.copy_(img)
    return out


def _host_frame(img, out, result, image):
    """A PoseResult that is on the host as the frame's buffers of one image at index `image`, whose keep list is rows 0 .. n.  Checks the
    index, the images (`_image_and_out`) and, with n > 0, the key points and boxes; returns img, out, image, n, J, `up` (numpy -> the image's
    device), the host arrays counts and segs and, with n > 0 (nothing is uploaded without), kps, box, keep, keep_count and seg on the device."""
    if not isinstance(image, (int, np.integer)) or isinstance(image, bool) or not (0 <= image < 4096):
        raise ValueError(f"image: an image index in 0..4095, got {image!r}")
    image = int(image)
    img, out = _image_and_out(img, out)
    kps = np.ascontiguousarray(result.keypoints, dtype=np.float64)
    n = int(kps.shape[0])
    J = int(kps.shape[1]) if kps.ndim == 3 else 0
    up = lambda a: torch.from_numpy(a).to(img.device)
    counts, segs = np.zeros(image + 1, np.int32), np.zeros(image + 2, np.int32)
    counts[image], segs[image + 1:] = n, n
    f = SimpleNamespace(img=img, out=out, image=image, n=n, J=J, up=up, counts=counts, segs=segs)
    if n == 0:
        return f
    if kps.ndim != 3 or kps.shape[2] != 3 or not (1 <= J <= 64):
        raise ValueError(f"result.keypoints: expected [n, J <= 64, 3], got {tuple(kps.shape)}")
    box = np.ascontiguousarray(result.box, dtype=np.float32)
    if box.shape != (n, 5):
        raise ValueError(f"result.box: expected [{n}, 5], got {tuple(box.shape)}")
    f.kps, f.box, f.keep, f.keep_count, f.seg = up(kps), up(box), up(np.arange(n, dtype=np.int32)), up(counts), up(segs)
    return f


class PoseRenderer(object):
    """`skeleton`: the limbs as pairs of joint indices (at most 64; default COCO's 19).  `joint_radius`, `limb_width`, `box_width`: pixels
    (radius 0 .. 64, widths 0 .. 128), quantised to 1/16 px (a limb or box edge is a capsule of half the width); `box_width=0` draws no
    boxes.  `opacity`: 0 .. 1, quantised to 1/16.  `in_vis_thre`: a joint is drawn when its max_val exceeds it, a limb when both ends do.
    `colour_by`: "person" (the track id's palette entry, the pick position's without ids) or "part" (one entry per limb / joint; boxes keep
    the person's).  `palette`: up to 32 BGR triples (default: 20 colours).

    `label`: None (no labels) or a template of at most 32 bytes, printable ASCII with the fields {id}, {score}, {conf} (a field is one
    byte; `{{` / `}}` are literal braces); the formatted text is cut at 24 characters.  `label_scale`, `caption_scale`: 1 .. 8 image pixels
    per font pixel.  `label_opacity`, `caption_opacity`: 0 .. 1, quantised to 1/16.  `caption`: None, a string or a list with one string
    per image, each at most 64 bytes with the fields {n} and {image}; `caption_corner`: "tl", "tr", "bl" or "br".  With `label` and
    `caption` both None nothing is allocated or launched for text."""

    def __init__(self, skeleton=COCO_SKELETON, joint_radius: float = 3.0, limb_width: float = 2.0, box_width: float = 1.0, opacity: float = 1.0,
                 in_vis_thre: float = 0.2, colour_by: str = "person", palette=None, label=None, label_scale: int = 2,
                 label_opacity: float = 1.0, caption=None, caption_scale: int = 2, caption_corner: str = "tl", caption_opacity: float = 0.75):
        ends = _joint_indices(skeleton, 0, 2 * _lib.SP_RENDER_MAX_EDGES,
                              f"skeleton: expected at most {_lib.SP_RENDER_MAX_EDGES} pairs of joint indices in 0..63, got {skeleton!r}", pairs=True)
        sk = list(zip(ends[0::2], ends[1::2]))
        jr = _number("joint_radius", joint_radius, 0.0, MAX_RADIUS_PX, f"a radius in 0..{MAX_RADIUS_PX:g} px")
        lw = _number("limb_width", limb_width, 0.0, 2 * MAX_RADIUS_PX, f"a width in 0..{2 * MAX_RADIUS_PX:g} px")
        bw = _number("box_width", box_width, 0.0, 2 * MAX_RADIUS_PX, f"a width in 0..{2 * MAX_RADIUS_PX:g} px (0: no boxes)")
        op = _number("opacity", opacity, 0.0, 1.0, "a value in 0..1")
        if not isinstance(in_vis_thre, (int, float)) or isinstance(in_vis_thre, bool) or in_vis_thre != in_vis_thre:
            raise ValueError(f"in_vis_thre: a number, got {in_vis_thre!r}")
        if colour_by not in ("person", "part"):
            raise ValueError(f"colour_by: 'person' or 'part', got {colour_by!r}")
        pal = np.asarray(DEFAULT_PALETTE if palette is None else palette)
        if pal.ndim != 2 or pal.shape[1] != 3 or not (1 <= pal.shape[0] <= _lib.SP_RENDER_MAX_PALETTE) or pal.dtype.kind not in "iu" or \
                pal.min() < 0 or pal.max() > 255:
            raise ValueError(f"palette: expected 1..{_lib.SP_RENDER_MAX_PALETTE} BGR triples of ints in 0..255")
        self.skeleton = tuple(sk)
        self.joint_r, self.limb_r, self.box_r = int(round(jr * 16)), int(round(lw * 8)), int(round(bw * 8))      # 1/16 px
        self.opacity16 = int(round(op * 16))
        self.in_vis_thre, self.colour_by = float(in_vis_thre), colour_by
        self.palette = pal.astype(np.uint8)
        st = _lib.RenderStyle()
        st.edges = len(sk)
        for e, (a, b) in enumerate(sk):
            st.edge[e][0], st.edge[e][1] = a, b
        st.joint_r, st.limb_r, st.box_r, st.opacity = self.joint_r, self.limb_r, self.box_r, self.opacity16
        st.in_vis_thre = self.in_vis_thre
        st.colour_by = _lib.SP_RENDER_COLOUR_PART if colour_by == "part" else _lib.SP_RENDER_COLOUR_PERSON
        st.palette_n = int(pal.shape[0])
        for i, c in enumerate(self.palette.tolist()):
            st.palette[i][0], st.palette[i][1], st.palette[i][2] = c
        self._style = st
        # ---- text
        self.label = None if label is None else parse_template(label, LABEL_FIELDS, _lib.SP_LABEL_MAX_TEMPLATE, "label")
        for name, v in (("label_scale", label_scale), ("caption_scale", caption_scale)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not (1 <= v <= _lib.SP_LABEL_MAX_SCALE):
                raise ValueError(f"{name}: an integer in 1..{_lib.SP_LABEL_MAX_SCALE} (image pixels per font pixel), got {v!r}")
        lo = _number("label_opacity", label_opacity, 0.0, 1.0, "a value in 0..1")
        co = _number("caption_opacity", caption_opacity, 0.0, 1.0, "a value in 0..1")
        if caption_corner not in _lib.SP_LABEL_CORNERS:
            raise ValueError(f"caption_corner: 'tl', 'tr', 'bl' or 'br', got {caption_corner!r}")
        self.label_scale, self.caption_scale, self.caption_corner = int(label_scale), int(caption_scale), caption_corner
        self.label_opacity16, self.caption_opacity16 = int(round(lo * 16)), int(round(co * 16))
        self.caption = caption
        ls = _lib.LabelStyle()
        ls.template_len = len(self.label or b"")
        for i, c in enumerate(self.label or b""):
            ls.label_template[i] = c
        ls.label_scale, ls.label_opacity = self.label_scale, self.label_opacity16
        ls.caption_scale, ls.caption_opacity = self.caption_scale, self.caption_opacity16
        ls.caption_corner = _lib.SP_LABEL_CORNERS[caption_corner]
        ls.palette_n = st.palette_n
        for i, c in enumerate(self.palette.tolist()):
            ls.palette[i][0], ls.palette[i][1], ls.palette[i][2] = c
        self._label_style = ls

    @property
    def caption(self):
        """None, a string, or a list with one string per image; assign at any time (the text is checked at once)."""
        return self._caption

    @caption.setter
    def caption(self, value) -> None:
        if value is None:
            self._caption, self._caption_bytes = None, None
            return
        texts = list(value) if isinstance(value, (list, tuple)) else [value]
        if len(texts) == 0:
            raise ValueError("caption: a string, or a list with one string per image; got an empty list")
        parsed = [parse_template(t, CAPTION_FIELDS, _lib.SP_LABEL_CAPTION_BYTES, "caption") for t in texts]
        self._caption = list(value) if isinstance(value, (list, tuple)) else value
        self._caption_bytes = parsed if isinstance(value, (list, tuple)) else parsed[0]

    @property
    def has_text(self) -> bool:
        return self.label is not None or self._caption is not None

    def caption_rows(self, images: int) -> np.ndarray:
        """The captions of `images` images as sp_render_labels_u8c3 reads them: uint8 [images, 64], NUL padded.  A list of another
        length: ValueError."""
        cb = self._caption_bytes
        if cb is None:
            raise ValueError("caption: this renderer has none")
        if isinstance(cb, list) and len(cb) != images:
            raise ValueError(f"caption: a list of {len(cb)} strings for {images} image{'s' if images != 1 else ''} (one per image)")
        out = np.zeros((images, _lib.SP_LABEL_CAPTION_BYTES), np.uint8)
        for b in range(images):
            t = cb[b] if isinstance(cb, list) else cb
            out[b, :len(t)] = list(t)
        return out

    def key(self) -> tuple:
        """Everything the launches depend on: two renderers with equal keys draw the same pixels (a captured graph is reused only then) -
        but for the caption's text, which the launches read from device memory: only whether there is one is part of the key."""
        return (self.skeleton, self.joint_r, self.limb_r, self.box_r, self.opacity16, self.in_vis_thre, self.colour_by, self.palette.tobytes(),
                self.label, self.label_scale, self.label_opacity16, self._caption is not None, self.caption_scale, self.caption_corner,
                self.caption_opacity16)

    @staticmethod
    def workspace(rows: int, joints: int, device) -> torch.Tensor:
        """The primitive array of `rows` person slots, sized for any skeleton (64 limbs)."""
        return _workspace("sp_render_workspace_bytes", 8, device, rows, joints, _lib.SP_RENDER_MAX_EDGES)

    @staticmethod
    def label_workspace(rows: int, device) -> torch.Tensor:
        """The record array of `rows` person slots and the caption."""
        return _workspace("sp_render_labels_workspace_bytes", 0, device, rows)

    def launch(self, src, dst, kps, box, track_id, keep, keep_count, seg, image: int, rows: int, joints: int, workspace, score=None,
               caption=None, label_workspace=None) -> None:
        """sp_render_poses_u8c3 on the current stream of src's device; every argument a CUDA tensor (track_id may be None).  A renderer with
        text then issues sp_render_labels_u8c3 on `dst`: `score` fp64 [rows] (needed with a `label`), `caption` uint8 [images, 64] on the
        device (needed with a caption: `caption_rows` uploaded by the caller), `label_workspace` from `label_workspace(rows, device)`."""
        h, w = int(src.shape[0]), int(src.shape[1])
        _lib.check(_lib.lib().sp_render_poses_u8c3(P(src), P(dst), h, w, P(kps), P(box), P(track_id), P(keep), P(keep_count), P(seg), image, rows,
                                                   joints, ctypes.byref(self._style), P(workspace), _lib.current_stream(src.device)),
                   "sp_render_poses_u8c3")
        if self.has_text:
            self.launch_labels(dst, box, score, track_id, keep, keep_count, seg, image, rows, caption, label_workspace)

    def launch_labels(self, img, box, score, track_id, keep, keep_count, seg, image: int, rows: int, caption, label_workspace) -> None:
        """sp_render_labels_u8c3 on `img` in place, on the current stream of its device."""
        if self.label is not None and rows > 0 and score is None:
            raise ValueError("launch: this renderer has a label, which needs score= (fp64 [rows] on the device)")
        if self._caption is not None and caption is None:
            raise ValueError("launch: this renderer has a caption, which needs caption= (caption_rows(images) on the device)")
        if label_workspace is None:
            raise ValueError("launch: this renderer draws text, which needs label_workspace= (PoseRenderer.label_workspace(rows, device))")
        h, w = int(img.shape[0]), int(img.shape[1])
        _lib.check(_lib.lib().sp_render_labels_u8c3(P(img), h, w, P(box), P(score), P(track_id), P(keep), P(keep_count), P(seg), image, rows,
                                                    ctypes.byref(self._label_style), P(caption) if self._caption is not None else None,
                                                    P(label_workspace), _lib.current_stream(img.device)), "sp_render_labels_u8c3")

    @torch.no_grad()
    def render(self, img, result, out=None, image: int = 0) -> torch.Tensor:
        """`img`: uint8 BGR [H, W, 3], numpy or CUDA; `result`: a PoseResult (its track_id colours the persons when present).  Returns a
        CUDA uint8 [H, W, 3]: `out` when given (contiguous; it may be `img` itself when that is a contiguous CUDA tensor, drawn in
        place), a new tensor otherwise.  A non-contiguous `img` is copied first, so it cannot also be `out`.  Labels take `result.score`
        and `result.track_id`; `image`: the index {image} prints and, with a list of captions, the one that is drawn."""
        f = _host_frame(img, out, result, image)
        dev, n = f.img.device, f.n
        cap = None
        if self._caption is not None:
            cb = self._caption_bytes
            if isinstance(cb, list) and f.image >= len(cb):
                raise ValueError(f"caption: a list of {len(cb)} strings has none for image {f.image}")
            cap = f.up(self.caption_rows(len(cb) if isinstance(cb, list) else f.image + 1))
        if n == 0:
            _copy_through(f.img, f.out)
            if cap is not None:
                with torch.cuda.device(dev):
                    self.launch_labels(f.out, None, None, None, None, f.up(f.counts), f.up(f.segs), f.image, 0, cap, self.label_workspace(0, dev))
            return f.out
        tid = None if result.track_id is None else f.up(np.ascontiguousarray(result.track_id, dtype=np.int32).reshape(n))
        score = lws = None
        if self.has_text:
            score = f.up(np.ascontiguousarray(result.score, dtype=np.float64).reshape(n))
            lws = self.label_workspace(n, dev)
        with torch.cuda.device(dev):
            self.launch(f.img, f.out, f.kps, f.box, tid, f.keep, f.keep_count, f.seg, f.image, n, f.J, self.workspace(n, f.J, dev), score=score,
                        caption=cap, label_workspace=lws)
        return f.out


class Redactor(object):
    """`region`: "head" (a disc around the visible head joints) or "person" (the box).  `mode`: "mosaic" (a redacted cell becomes the mean
    of its source pixels) or "fill" (the constant BGR colour `fill`).  `cell`: 4, 8, 16, 32 or 64 pixels; a cell is redacted as a whole or
    left alone.  Head regions: `head_joints`: 1 .. 8 joint indices (default COCO's nose, eyes and ears); a head joint counts when its
    max_val exceeds `in_vis_thre`; the disc's radius is half the longer side of the visible head joints' bounding box, at least `head_min`
    (0 .. 1, quantised to 1/256) of the box's longer side, times `expand` (1 .. 4, quantised to 1/16).  `fallback`: what hides a person
    without a visible head joint - "box_top" (the top `top_frac`, 0 .. 1 quantised to 1/256, of the box: the default fails closed), "box"
    (the whole box) or "none"."""

    def __init__(self, region: str = "head", mode: str = "mosaic", cell: int = 16, expand: float = 1.5, head_min: float = 20 / 256,
                 head_joints=(0, 1, 2, 3, 4), fallback: str = "box_top", top_frac: float = 0.25, in_vis_thre: float = 0.2, fill=(0, 0, 0)):
        if region not in _lib.SP_REDACT_REGIONS:
            raise ValueError(f"region: 'head' or 'person', got {region!r}")
        if mode not in _lib.SP_REDACT_MODES:
            raise ValueError(f"mode: 'mosaic' or 'fill', got {mode!r}")
        if not isinstance(cell, (int, np.integer)) or isinstance(cell, bool) or cell not in _lib.SP_REDACT_CELLS:
            raise ValueError(f"cell: one of {', '.join(str(c) for c in _lib.SP_REDACT_CELLS)} pixels, got {cell!r}")
        ex = _number("expand", expand, 1.0, 4.0, "a factor in 1..4")
        hm = _number("head_min", head_min, 0.0, 1.0, "a fraction of the box side in 0..1")
        tf = _number("top_frac", top_frac, 0.0, 1.0, "a fraction of the box height in 0..1")
        hj = _joint_indices(head_joints, 1, _lib.SP_REDACT_MAX_HEAD_JOINTS,
                            f"head_joints: expected 1..{_lib.SP_REDACT_MAX_HEAD_JOINTS} joint indices in 0..63, got {head_joints!r}")
        if fallback not in _lib.SP_REDACT_FALLBACKS:
            raise ValueError(f"fallback: 'box_top', 'box' or 'none', got {fallback!r}")
        if not isinstance(in_vis_thre, (int, float)) or isinstance(in_vis_thre, bool) or in_vis_thre != in_vis_thre:
            raise ValueError(f"in_vis_thre: a number, got {in_vis_thre!r}")
        try:
            col = np.asarray(fill)
        except (TypeError, ValueError):
            col = np.zeros(0)
        if col.shape != (3,) or col.dtype.kind not in "iu" or col.min() < 0 or col.max() > 255:
            raise ValueError(f"fill: a BGR triple of ints in 0..255, got {fill!r}")
        self.region, self.mode, self.cell, self.fallback = region, mode, int(cell), fallback
        self.expand16, self.head_min256, self.top_frac256 = int(round(ex * 16)), int(round(hm * 256)), int(round(tf * 256))
        self.head_joints, self.in_vis_thre = tuple(hj), float(in_vis_thre)
        self.fill = tuple(int(c) for c in col)
        st = _lib.RedactStyle()
        st.region, st.mode, st.cell = _lib.SP_REDACT_REGIONS[region], _lib.SP_REDACT_MODES[mode], self.cell
        st.expand, st.head_min, st.top_frac = self.expand16, self.head_min256, self.top_frac256
        st.head_joints = len(hj)
        for i, j in enumerate(hj):
            st.head_joint[i] = j
        st.fallback = _lib.SP_REDACT_FALLBACKS[fallback]
        st.in_vis_thre = self.in_vis_thre
        st.fill[0], st.fill[1], st.fill[2] = self.fill
        self._style = st

    def key(self) -> tuple:
        """Everything the launches depend on: two redactors with equal keys write the same pixels (a captured graph is reused only then)."""
        return (self.region, self.mode, self.cell, self.expand16, self.head_min256, self.head_joints, self.fallback, self.top_frac256,
                self.in_vis_thre, self.fill)

    @staticmethod
    def workspace(rows: int, device) -> torch.Tensor:
        """The region array of `rows` person slots."""
        return _workspace("sp_redact_workspace_bytes", 4, device, rows)

    def launch(self, src, dst, kps, box, keep, keep_count, seg, image: int, rows: int, joints: int, workspace) -> None:
        """sp_redact_u8c3 on the current stream of src's device; every argument a CUDA tensor.  `dst` may be `src` (in place)."""
        h, w = int(src.shape[0]), int(src.shape[1])
        _lib.check(_lib.lib().sp_redact_u8c3(P(src), P(dst), h, w, P(kps), P(box), P(keep), P(keep_count), P(seg), image, rows, joints,
                                             ctypes.byref(self._style), P(workspace), _lib.current_stream(src.device)), "sp_redact_u8c3")

    @torch.no_grad()
    def redact(self, img, result, out=None, image: int = 0) -> torch.Tensor:
        """`img`: uint8 BGR [H, W, 3], numpy or CUDA; `result`: a PoseResult (its `keypoints`, never `keypoints_smooth`, and its `box`).
        Returns a CUDA uint8 [H, W, 3]: `out` when given (contiguous; it may be `img` itself when that is a contiguous CUDA tensor,
        redacted in place), a new tensor otherwise.  `image`: the index the rows are filed under (any index gives the same pixels)."""
        f = _host_frame(img, out, result, image)
        if f.n == 0:
            return _copy_through(f.img, f.out)
        with torch.cuda.device(f.img.device):
            self.launch(f.img, f.out, f.kps, f.box, f.keep, f.keep_count, f.seg, f.image, f.n, f.J, self.workspace(f.n, f.img.device))
        return f.out


def _colormap(name: str) -> np.ndarray:
    """The named table as uint8 [256, 3] BGR, by integer formulas (v = 0 .. 255, clamp to 0 .. 255):
    "gray"  B = G = R = v;
    "hot"   R = clamp(3 v), G = clamp(3 v - 255), B = clamp(3 v - 510): black, red, yellow, white;
    "jet"   R = clamp((765 - |8 v - 1530|) >> 1), G = clamp((765 - |8 v - 1020|) >> 1), B = clamp((765 - |8 v - 510|) >> 1): the classic
            piecewise-linear 255 * clamp(1.5 - |4 t - k|, 0, 1), t = v / 255, k = 3, 2, 1: dark blue, blue, cyan, yellow, red, dark red."""
    v = np.arange(256, dtype=np.int64)
    if name == "gray":
        b = g = r = v
    elif name == "hot":
        r, g, b = 3 * v, 3 * v - 255, 3 * v - 510
    elif name == "jet":
        r, g, b = ((765 - np.abs(8 * v - k)) >> 1 for k in (1530, 1020, 510))
    else:
        raise ValueError(f"colormap: 'gray', 'hot', 'jet' or a [256, 3] uint8 BGR array, got {name!r}")
    return np.clip(np.stack([b, g, r], 1), 0, 255).astype(np.uint8)


class HeatOverlay(object):
    """The kept persons' joint heat maps blended into the frame (sp_heat_overlay_u8c3: csrc/heat.hip, the rules in csrc/sp_heat.h and
    include/simple_pose_hip.h), two launches: per person the maximum over the joints' maps, quantised to 0 .. 255 (`gain` 1 maps [0, 1]
    onto it: the reference's draw_heat_map, `(merge_map * 255).astype(np.uint8)`), warped into the image through the inverse of the
    person's `trans_inv` with bilinear sampling in fixed point; a pixel takes the maximum over the persons, and where that reaches
    `threshold` it is blended with the colour the table gives it.

    `colormap`: "gray" (the reference's GRAY2BGR), "hot", "jet" (integer formulas: `_colormap`) or a [256, 3] uint8 BGR array; uploaded
    once per device.  `opacity`: 0 .. 1, quantised to 1/16.  `alpha`: "value" (the weight grows with the heat) or "constant".
    `threshold`: 0 .. 1 of the quantised range, min(255, max(1, int(threshold * 255))).  `gain`: finite, >= 0; the maps are multiplied by
    float32(255 * gain).  `joints`: None (every joint) or the joint indices (< 64) whose maps take part.  There is no CPU fallback.

        h = HeatOverlay(colormap="jet", opacity=0.6, alpha="value", threshold=0.1, gain=1.0, joints=None)
        out = h.overlay(img, heat_maps, trans_inv)                    # every row of heat_maps [n, J, h, w] / trans_inv [n, 2, 3]
        est = TopDownPoseEstimator(detector, pose_model, heat_overlay=h)   # in the frame: under the skeleton, over the redaction"""

    def __init__(self, colormap="jet", opacity: float = 0.6, alpha: str = "value", threshold: float = 0.1, gain: float = 1.0, joints=None):
        if isinstance(colormap, str):
            lut = _colormap(colormap)
        else:
            try:
                lut = np.asarray(colormap)
            except (TypeError, ValueError):
                lut = np.zeros(0)
            if lut.shape != (256, 3) or lut.dtype != np.uint8:
                raise ValueError(f"colormap: 'gray', 'hot', 'jet' or a [256, 3] uint8 BGR array, got {type(colormap).__name__}"
                                 f"{' ' + str(lut.shape) + ' ' + str(lut.dtype) if isinstance(colormap, np.ndarray) else ''}")
        op = _number("opacity", opacity, 0.0, 1.0, "a value in 0..1")
        if alpha not in _lib.SP_HEAT_ALPHAS:
            raise ValueError(f"alpha: 'value' or 'constant', got {alpha!r}")
        th = _number("threshold", threshold, 0.0, 1.0, "a fraction of the quantised range in 0..1")
        g = _number("gain", gain, 0.0, float("inf"), "a finite factor >= 0")
        with np.errstate(over="ignore"):
            scale = np.float32(255.0 * g)
        if not np.isfinite(scale):
            raise ValueError(f"gain: a finite factor >= 0 (255 * gain must fit float32), got {gain!r}")
        if joints is None:
            mask, js = (1 << 64) - 1, None
        else:
            js = _joint_indices(joints, 1, None, f"joints: None (every joint) or a non-empty list of joint indices in 0..63, got {joints!r}")
            mask = 0
            for j in js:
                mask |= 1 << j
            js = tuple(sorted(set(js)))
        self.lut = np.ascontiguousarray(lut).copy()
        self.colormap = colormap if isinstance(colormap, str) else None
        self.opacity16, self.alpha = int(round(op * 16)), alpha
        self.threshold = min(255, max(1, int(th * 255)))
        self.gain, self.scale, self.joints, self.joint_mask = g, scale, js, mask
        st = _lib.HeatStyle()
        st.joint_mask, st.scale, st.threshold, st.opacity16, st.alpha = mask, float(scale), self.threshold, self.opacity16, _lib.SP_HEAT_ALPHAS[alpha]
        self._style = st
        self._lut_dev = {}

    def key(self) -> tuple:
        """Everything the launches depend on: two overlays with equal keys write the same pixels.  (A captured graph also holds the
        pointer of one overlay's uploaded table, so an estimator adds the overlay's identity to its own key.)"""
        return (self.lut.tobytes(), self.opacity16, self.alpha, self.threshold, float(self.scale), self.joint_mask)

    def table(self, device) -> torch.Tensor:
        """The colour table on `device`, uploaded with the first call (never inside a capture: an estimator's frame asks for it ahead)."""
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        t = self._lut_dev.get(dev)
        if t is None:
            t = self._lut_dev[dev] = torch.from_numpy(self.lut).to(dev)
        return t

    @staticmethod
    def workspace(rows: int, hm_h: int, hm_w: int, device) -> torch.Tensor:
        """The records and the u8 planes of `rows` person slots with hm_h x hm_w maps."""
        return _workspace("sp_heat_overlay_workspace_bytes", 8, device, rows, hm_h, hm_w)

    def launch(self, src, dst, hm, trans_inv, keep, keep_count, seg, image: int, rows: int, workspace) -> None:
        """sp_heat_overlay_u8c3 on the current stream of src's device; every argument a CUDA tensor (hm: contiguous fp32 [>= rows, J, h, w]).
        `dst` may be `src` (in place)."""
        h, w = int(src.shape[0]), int(src.shape[1])
        if rows > 0 and not (hm.is_cuda and hm.dtype == torch.float32 and hm.dim() == 4 and hm.is_contiguous() and hm.shape[0] >= rows):
            raise ValueError(f"heat maps: expected contiguous CUDA float32 [>= {rows}, J, h, w], got {hm.dtype} {tuple(hm.shape)}")
        J, mh, mw = (int(v) for v in hm.shape[1:]) if rows > 0 else (1, 1, 1)
        _lib.check(_lib.lib().sp_heat_overlay_u8c3(P(src), P(dst), h, w, P(hm) if rows > 0 else None, J, mh, mw, P(trans_inv), P(keep),
                                                   P(keep_count), P(seg), image, rows, ctypes.byref(self._style),
                                                   P(self.table(src.device)), P(workspace), _lib.current_stream(src.device)),
                   "sp_heat_overlay_u8c3")

    @torch.no_grad()
    def overlay(self, img, heat_maps, trans_inv, out=None) -> torch.Tensor:
        """`img`: uint8 BGR [H, W, 3], numpy or CUDA; `heat_maps`: CUDA float32 [n, J <= 64, h, w] (h, w <= 256); `trans_inv`: CUDA
        float32 [n, 2, 3], heat-map px -> image px.  Every row is drawn.  Returns a CUDA uint8 [H, W, 3]: `out` when given (contiguous;
        it may be `img` itself when that is a contiguous CUDA tensor, drawn in place), a new tensor otherwise."""
        img, out = _image_and_out(img, out)
        for name, t in (("heat_maps", heat_maps), ("trans_inv", trans_inv)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name}: expected a CUDA float32 tensor, got {type(t).__name__}")
            if not t.is_cuda or t.device != img.device:
                raise HipLibraryError(f"{name} is on {t.device}, the image on {img.device}; simple_pose_amd runs on the MI355X only (no CPU fallback)")
            if t.dtype != torch.float32:
                raise TypeError(f"{name}: expected float32, got {t.dtype}")
        if heat_maps.dim() != 4:
            raise ValueError(f"heat_maps: expected [n, J, h, w], got {tuple(heat_maps.shape)}")
        n, J, mh, mw = (int(v) for v in heat_maps.shape)
        if n > 2048 or not (1 <= J <= 64) or not (1 <= mh <= _lib.SP_HEAT_MAX_MAP and 1 <= mw <= _lib.SP_HEAT_MAX_MAP):
            raise ValueError(f"heat_maps: expected [n <= 2048, J <= 64, h <= {_lib.SP_HEAT_MAX_MAP}, w <= {_lib.SP_HEAT_MAX_MAP}], got {tuple(heat_maps.shape)}")
        if tuple(trans_inv.shape) != (n, 2, 3):
            raise ValueError(f"trans_inv: expected [{n}, 2, 3], got {tuple(trans_inv.shape)}")
        if n == 0:
            return _copy_through(img, out)
        dev = img.device
        keep = torch.arange(n, dtype=torch.int32, device=dev)
        keep_count = torch.full((1,), n, dtype=torch.int32, device=dev)
        seg = torch.tensor([0, n], dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            self.launch(img, out, heat_maps.contiguous(), trans_inv.contiguous(), keep, keep_count, seg, 0, n, self.workspace(n, mh, mw, dev))
        return out
