"""Poses drawn into frames on the device: skeleton limbs, joints and boxes, coloured by person (track id) or by part.

    r = PoseRenderer(skeleton=COCO_SKELETON, joint_radius=3.0, limb_width=2.0, box_width=1.0, opacity=1.0, in_vis_thre=0.2,
                     colour_by="person", palette=None)
    out = r.render(img, result)                                   # uint8 BGR [H,W,3] (numpy or CUDA) + a PoseResult -> CUDA uint8 [H,W,3]
    est = TopDownPoseEstimator(detector, pose_model, renderer=r)  # in the frame: PoseResult.image, drawn inside the frame's own graph

The rasteriser is sp_render_poses_u8c3 (csrc/render.hip, the pixel rules in csrc/sp_render.h and include/simple_pose_hip.h): every
primitive is a capsule in 1/16 px, covered pixels are blended by 16 samples each, persons are painted in reverse pick order so that the
best pose lies on top.  Inside an estimator or a tracker the two launches follow sp_oks_nms / sp_track_associate on the same stream and
read the frame's buffers directly; the person count never reaches the host.  `render` is the same kernels on the rows of a PoseResult that
is already on the host.  There is no CPU fallback and no text."""
from __future__ import annotations

import ctypes

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


def _number(name, v, lo, hi, what):
    if not isinstance(v, (int, float)) or isinstance(v, bool) or not (lo <= float(v) <= hi):
        raise ValueError(f"{name}: {what}, got {v!r}")
    return float(v)


class PoseRenderer(object):
    """`skeleton`: the limbs as pairs of joint indices (at most 64; default COCO's 19).  `joint_radius`, `limb_width`, `box_width`: pixels
    (radius 0 .. 64, widths 0 .. 128), quantised to 1/16 px (a limb or box edge is a capsule of half the width); `box_width=0` draws no
    boxes.  `opacity`: 0 .. 1, quantised to 1/16.  `in_vis_thre`: a joint is drawn when its max_val exceeds it, a limb when both ends do.
    `colour_by`: "person" (the track id's palette entry, the pick position's without ids) or "part" (one entry per limb / joint; boxes keep
    the person's).  `palette`: up to 32 BGR triples (default: 20 colours)."""

    def __init__(self, skeleton=COCO_SKELETON, joint_radius: float = 3.0, limb_width: float = 2.0, box_width: float = 1.0, opacity: float = 1.0,
                 in_vis_thre: float = 0.2, colour_by: str = "person", palette=None):
        try:
            sk = [(int(a), int(b)) for a, b in skeleton]
            ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for e in skeleton for v in e)
        except (TypeError, ValueError):
            sk, ok = [], False
        if not ok or len(sk) > _lib.SP_RENDER_MAX_EDGES or any(v < 0 or v >= 64 for e in sk for v in e):
            raise ValueError(f"skeleton: expected at most {_lib.SP_RENDER_MAX_EDGES} pairs of joint indices in 0..63, got {skeleton!r}")
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

    def key(self) -> tuple:
        """Everything the launches depend on: two renderers with equal keys draw the same pixels (a captured graph is reused only then)."""
        return (self.skeleton, self.joint_r, self.limb_r, self.box_r, self.opacity16, self.in_vis_thre, self.colour_by, self.palette.tobytes())

    @staticmethod
    def workspace(rows: int, joints: int, device) -> torch.Tensor:
        """The primitive array of `rows` person slots, sized for any skeleton (64 limbs)."""
        n = ctypes.c_int64()
        _lib.check(_lib.lib().sp_render_workspace_bytes(rows, joints, _lib.SP_RENDER_MAX_EDGES, ctypes.byref(n)), "sp_render_workspace_bytes")
        return torch.zeros((max(int(n.value), 8),), dtype=torch.uint8, device=device)

    def launch(self, src, dst, kps, box, track_id, keep, keep_count, seg, image: int, rows: int, joints: int, workspace) -> None:
        """sp_render_poses_u8c3 on the current stream of src's device; every argument a CUDA tensor (track_id may be None)."""
        h, w = int(src.shape[0]), int(src.shape[1])
        _lib.check(_lib.lib().sp_render_poses_u8c3(P(src), P(dst), h, w, P(kps), P(box), P(track_id), P(keep), P(keep_count), P(seg), image, rows,
                                                   joints, ctypes.byref(self._style), P(workspace), _lib.current_stream(src.device)),
                   "sp_render_poses_u8c3")

    @torch.no_grad()
    def render(self, img, result, out=None) -> torch.Tensor:
        """`img`: uint8 BGR [H, W, 3], numpy or CUDA; `result`: a PoseResult (its track_id colours the persons when present).  Returns a
        CUDA uint8 [H, W, 3]: `out` when given (contiguous; it may be `img` itself when that is a contiguous CUDA tensor, drawn in
        place), a new tensor otherwise.  A non-contiguous `img` is copied first, so it cannot also be `out`."""
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
        kps = np.ascontiguousarray(result.keypoints, dtype=np.float64)
        n = int(kps.shape[0])
        J = int(kps.shape[1]) if kps.ndim == 3 else 0
        if n == 0:
            if out.data_ptr() != img.data_ptr():
                out.copy_(img)
            return out
        if kps.ndim != 3 or kps.shape[2] != 3 or not (1 <= J <= 64):
            raise ValueError(f"result.keypoints: expected [n, J <= 64, 3], got {tuple(kps.shape)}")
        box = np.ascontiguousarray(result.box, dtype=np.float32)
        if box.shape != (n, 5):
            raise ValueError(f"result.box: expected [{n}, 5], got {tuple(box.shape)}")
        dev = img.device
        up = lambda a: torch.from_numpy(a).to(dev)
        tid = None if result.track_id is None else up(np.ascontiguousarray(result.track_id, dtype=np.int32).reshape(n))
        d_kps, d_box = up(kps), up(box)
        keep, keep_count, seg = up(np.arange(n, dtype=np.int32)), up(np.array([n], np.int32)), up(np.array([0, n], np.int32))
        ws = self.workspace(n, J, dev)
        with torch.cuda.device(dev):
            self.launch(img, out, d_kps, d_box, tid, keep, keep_count, seg, 0, n, J, ws)
        return out
