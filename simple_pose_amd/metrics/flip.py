"""The flip test of top-down evaluation (Simple-Baselines / HRNet `TEST.FLIP_TEST`), device resident.

    x2 = torch.empty((2 * B,) + x.shape[1:], ...); x2[:B] = x; mirror_input(x2[:B], out=x2[B:])
    hm2 = model.forward_crops(x2)                       # ONE forward on both halves
    hm = merge_flipped(hm2[:B], hm2[B:], out=hm2[:B])   # un-mirror, swap left/right joints, average

(`forward_crops(crops, flip_test=True)` and `TopDownPoseEstimator(..., flip_test=True)` do exactly this.)  Each function is ONE kernel
launch (sp_mirror_w / sp_heat_map_flip_merge) on the stream of the tensor's device, with no host sync; the left/right permutation travels
in the kernel's arguments, so both launches can be captured into a graph.  The arithmetic is stated in include/simple_pose_hip.h."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from .. import _lib
from .._lib import HipLibraryError

COCO_JOINT_PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))   # left/right key points (datasets/coco.py)
MAX_JOINTS = 64


def check_joint_pairs(joint_pairs) -> tuple:
    """Type and disjointness of left/right pairs (what can be said without the joint count) -> a tuple of (int, int)."""
    try:
        pairs = [tuple(p) for p in joint_pairs]
    except TypeError:
        raise ValueError(f"joint_pairs: expected a sequence of (left, right) index pairs, got {joint_pairs!r}") from None
    seen = set()
    for p in pairs:
        if len(p) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in p):
            raise ValueError(f"joint_pairs: every pair is two ints, got {p!r}")
        if p[0] < 0 or p[1] < 0:
            raise ValueError(f"joint_pairs: pair {p!r} is out of range (negative index)")
        if p[0] == p[1] or p[0] in seen or p[1] in seen:
            raise ValueError(f"joint_pairs: the pairs must be disjoint, joint of {p!r} appears twice")
        seen.update(p)
    return tuple(pairs)


def pairs_to_perm(joint_pairs, num_joints: int) -> list:
    """The joint permutation of a horizontal flip (commons.joint_utils.flip_joints' `perm`): perm[a] = b and perm[b] = a for every pair,
    identity elsewhere.  ValueError unless the pairs are ints, disjoint and inside 0..num_joints-1."""
    if isinstance(num_joints, bool) or not isinstance(num_joints, int) or not (1 <= num_joints <= MAX_JOINTS):
        raise ValueError(f"num_joints: expected an int in 1..{MAX_JOINTS}, got {num_joints!r}")
    perm = list(range(num_joints))
    for a, b in check_joint_pairs(joint_pairs):
        if a >= num_joints or b >= num_joints:
            raise ValueError(f"joint_pairs: pair {(a, b)!r} is out of range for {num_joints} joints")
        perm[a], perm[b] = b, a
    return perm


def _require_cuda(t, name: str):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise HipLibraryError(f"{name}: tensor is on {t.device}; simple_pose_amd runs on the MI355X only (no CPU fallback)")
    return t


def _check_out(out, like: torch.Tensor, name: str):
    if out is None:
        return torch.empty_like(like)
    _require_cuda(out, name)
    if out.shape != like.shape or out.dtype != like.dtype or out.device != like.device or not out.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous {like.dtype} tensor {tuple(like.shape)} on {like.device}")
    return out


@torch.no_grad()
def mirror_input(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The horizontally mirrored network input: CUDA uint8 BGR crops [B,H,W,3] or fp32 images [B,3,H,W].  `out`: where to write it (a
    contiguous tensor like `x` that does not overlap it, e.g. the second half of one [2B,...] buffer); default: a new tensor."""
    _require_cuda(x, "x")
    if x.dim() == 4 and x.dtype == torch.uint8 and x.shape[3] == 3:
        rows, w, eb = x.shape[0] * x.shape[1], x.shape[2], 3
    elif x.dim() == 4 and x.dtype == torch.float32 and x.shape[1] == 3:
        rows, w, eb = x.shape[0] * 3 * x.shape[2], x.shape[3], 4
    else:
        raise TypeError(f"mirror_input: expected uint8 [B,H,W,3] or float32 [B,3,H,W], got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    out = _check_out(out, x, "out")
    if x.numel() == 0:
        return out
    _lib.check(_lib.lib().sp_mirror_w(_lib.ptr(x), _lib.ptr(out), rows, w, eb, _lib.current_stream(x.device)), "sp_mirror_w")
    return out


@torch.no_grad()
def merge_flipped(hm: torch.Tensor, hm_flipped: torch.Tensor, joint_pairs: Sequence = COCO_JOINT_PAIRS, shift: bool = False,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(hm + unflip(hm_flipped)) / 2 for fp32 heat maps [B,J,h,w]: `hm_flipped` is the network's answer to the mirrored input; it is
    mirrored back and its left/right joints (`joint_pairs`) are swapped.  `shift`: Simple-Baselines' SHIFT_HEATMAP (the un-mirrored map
    moves one pixel to the right, column 0 kept).  `out` may be `hm` itself (in place); it must not overlap `hm_flipped`."""
    hm = _lib.require_cuda_f32(hm, "hm")
    hm_flipped = _lib.require_cuda_f32(hm_flipped, "hm_flipped")
    if hm.dim() != 4 or hm_flipped.shape != hm.shape:
        raise ValueError(f"merge_flipped: expected two heat maps [B,J,h,w] of one shape, got {tuple(hm.shape)} and {tuple(hm_flipped.shape)}")
    B, J, H, W = hm.shape
    perm = (ctypes.c_int32 * J)(*pairs_to_perm(joint_pairs, J))
    out = _check_out(out, hm, "out")
    _lib.same_device(hm, hm_flipped, out)
    if hm.numel() == 0:
        return out
    _lib.check(_lib.lib().sp_heat_map_flip_merge(_lib.ptr(hm), _lib.ptr(hm_flipped), perm, B, J, H, W, int(bool(shift)), _lib.ptr(out),
                                                 _lib.current_stream(hm.device)), "sp_heat_map_flip_merge")
    return out
