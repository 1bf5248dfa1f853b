"""Batches of differently sized images: the host side of the `sp_image_ref` table.

The detector letterboxes every image to its own net shape (ScalePadding.geometry with minimum_rectangle: the reference's semantics), so
a list of differently sized images splits into groups of one net shape (out_h, out_w) each.  One group is one detector forward; inside it
every image keeps its own source size, resize target and placement, which the kernels read per image from a table in device memory
(sp_yolo_letterbox_images, sp_yolo_boxes_to_source_images, sp_warp_affine_plan_images_u8c3).  This module checks the images, groups them,
packs the table (pure Python over `geometry`, no GPU) and stages table and host images with ONE host-to-device copy (`MixedBatch`).

Table layout of a call over B images: entries [0, B) in the caller's order (what the crop launch indexes with sp_topdown_plan's
src_index), then the same images again group by group, each group contiguous (what a group's letterbox and un-letterbox launches read);
`dst_index` is the image's position in the caller's order in both halves."""
from __future__ import annotations

import ctypes
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from ._lib import HipLibraryError, ImageRef, _device_index
from .video import YuvFrame, resolve

MAX_SIDE = 32767                     # the warp's fixed-point sample position holds source coordinates in a short
REF_BYTES = ctypes.sizeof(ImageRef)


def check_images(imgs) -> List[Tuple[int, int]]:
    """A list of uint8 BGR images [H_i, W_i, 3], numpy or CUDA -> their (h, w).  Raises before anything is launched: ValueError for an empty
    list and a bad or zero-sized shape, TypeError for another dtype, HipLibraryError for a CPU tensor.  A video.YuvFrame (checked when it
    was made) stands for the BGR image it converts to."""
    if not isinstance(imgs, (list, tuple)):
        raise TypeError(f"expected a list of uint8 BGR images, got {type(imgs).__name__}")
    if len(imgs) == 0:
        raise ValueError("an empty list of images")
    shapes = []
    for i, im in enumerate(imgs):
        if isinstance(im, YuvFrame):
            shapes.append((im.height, im.width))
            continue
        if isinstance(im, torch.Tensor):
            if not im.is_cuda:
                raise HipLibraryError(f"image {i}: tensor is on {im.device}; simple_pose_amd runs on the MI355X only (no CPU fallback)")
            ok = im.dtype == torch.uint8
        elif isinstance(im, np.ndarray):
            ok = im.dtype == np.uint8
        else:
            raise TypeError(f"image {i}: expected a uint8 BGR image (numpy or CUDA), got {type(im).__name__}")
        if not ok:
            raise TypeError(f"image {i}: expected a uint8 BGR image, got {im.dtype}")
        shape = tuple(int(v) for v in im.shape)
        if len(shape) != 3 or shape[2] != 3 or 0 in shape:
            raise ValueError(f"image {i}: expected uint8 BGR [H, W, 3], got {shape}")
        if shape[0] > MAX_SIDE or shape[1] > MAX_SIDE:
            raise ValueError(f"image {i}: {shape[0]}x{shape[1]} is above {MAX_SIDE} pixels a side")
        shapes.append((shape[0], shape[1]))
    return shapes


def check_det_counts(n_images: int, det, counts) -> int:
    """Shapes of caller-supplied detections for `n_images` images: det [n_images, M, 6] with M >= 1, counts (or None) n_images values.
    Returns M.  ValueError otherwise; nothing is uploaded or launched."""
    shape = tuple(det.shape) if hasattr(det, "shape") else tuple(np.shape(det))
    if len(shape) != 3 or shape[0] != n_images or shape[2] != 6 or shape[1] == 0:
        raise ValueError(f"det: expected [{n_images}, M, 6], got {shape}")
    if counts is not None:
        n = counts.numel() if isinstance(counts, torch.Tensor) else int(np.asarray(counts).size)
        if n != n_images:
            raise ValueError(f"counts: expected {n_images} values, got {n}")
    return shape[1]


def plan_groups(shapes: Sequence[Tuple[int, int]], transform) -> Tuple[List[dict], List[Tuple[Tuple[int, int], List[int]]]]:
    """Per image `transform.geometry(h, w)` (what single_predict letterboxes it with), and the images grouped by their net shape:
    [((out_h, out_w), [caller indices, ascending])], groups in the order their first image appears."""
    geoms = [transform.geometry(h, w) for h, w in shapes]
    groups: Dict[Tuple[int, int], List[int]] = {}
    for i, g in enumerate(geoms):
        groups.setdefault((int(g["out_h"]), int(g["out_w"])), []).append(i)
    return geoms, list(groups.items())


def pack_image_refs(ptrs: Sequence[int], shapes, geoms, groups):
    """The table of one call (module docstring) as a ctypes array of 2 * B `ImageRef`, and per group the index of its first entry."""
    B = len(shapes)
    refs = (ImageRef * (2 * B))()

    def fill(r, i):
        g, (h, w) = geoms[i], shapes[i]
        if not (g["new_h"] >= 1 and g["new_w"] >= 1 and g["top"] >= 0 and g["left"] >= 0 and g["top"] + g["new_h"] <= g["out_h"]
                and g["left"] + g["new_w"] <= g["out_w"] and g["out_h"] % 2 == 0 and g["out_w"] % 2 == 0):
            raise ValueError(f"image {i}: letterbox {h}x{w} -> {g['new_h']}x{g['new_w']} at ({g['top']}, {g['left']}) does not fit an even "
                             f"{g['out_h']}x{g['out_w']} canvas")
        r.data, r.h, r.w = int(ptrs[i]), h, w
        r.new_h, r.new_w, r.top, r.left = int(g["new_h"]), int(g["new_w"]), int(g["top"]), int(g["left"])
        r.ratio, r.dst_index = float(g["ratio"]), i

    for i in range(B):
        fill(refs[i], i)
    starts, k = [], B
    for _, members in groups:
        starts.append(k)
        for i in members:
            fill(refs[k], i)
            k += 1
    return refs, starts


class MixedBatch(object):
    """One call's images on the device and their table.  CUDA inputs are referenced in place (a non-contiguous one is made contiguous);
    numpy inputs and the table share one pinned staging buffer and reach the device in one copy on the current stream.  YuvFrames among
    the inputs are converted to BGR CUDA tensors first, all of them by one table launch (video.resolve), and then are CUDA inputs.  `stage`: a dict
    the owner keeps between calls, so that the pinned buffer and the device arena are allocated once and grown on demand; the owner
    synchronises with the stream before it starts the next call (every public call here ends in a fetch or a synchronous NMS).
      srcs          the B images as CUDA tensors [H_i, W_i, 3] (this object keeps them, and the arena, alive)
      table         uint8 [2 * B, sizeof(sp_image_ref)] on the device; `caller_table` its first half
      groups        [((out_h, out_w), [caller indices])]; `group_table(k)` the entries of group k"""

    def __init__(self, imgs, transform, device, stage: dict = None):
        self.shapes = check_images(imgs)
        device = torch.device("cuda", _device_index(torch.device(device)))
        for i, im in enumerate(imgs):
            if isinstance(im, torch.Tensor) and im.device != device:
                raise HipLibraryError(f"image {i}: on {im.device}, the detector on {device}")
            if isinstance(im, YuvFrame) and not im.is_host and im.device != device:
                raise HipLibraryError(f"image {i}: on {im.device}, the detector on {device}")
        stage = {} if stage is None else stage
        self.B = B = len(imgs)
        self.geoms, self.groups = plan_groups(self.shapes, transform)
        imgs = resolve(imgs, device, stage.setdefault("yuv", {}))
        align = lambda n: (n + 255) // 256 * 256
        off, where = align(2 * B * REF_BYTES), {}
        for i, im in enumerate(imgs):
            if isinstance(im, np.ndarray):
                where[i] = off
                off += align(im.size)
        if stage.get("host") is None or stage["host"].numel() < off or stage["dev"].device != device:
            stage["host"] = torch.empty(off, dtype=torch.uint8, pin_memory=True)
            stage["dev"] = torch.empty(off, dtype=torch.uint8, device=device)
        host, dev = stage["host"], stage["dev"]
        hview = host.numpy()
        self.srcs = []
        for i, im in enumerate(imgs):
            if i in where:
                h, w = self.shapes[i]
                o = where[i]
                np.copyto(hview[o:o + im.size].reshape(h, w, 3), im)
                self.srcs.append(dev[o:o + im.size].view(h, w, 3))
            else:
                self.srcs.append(im.contiguous())
        refs, self._starts = pack_image_refs([s.data_ptr() for s in self.srcs], self.shapes, self.geoms, self.groups)
        ctypes.memmove(hview.ctypes.data, ctypes.addressof(refs), ctypes.sizeof(refs))
        dev[:off].copy_(host[:off], non_blocking=True)           # the call's one host-to-device copy
        self.table = dev[:2 * B * REF_BYTES].view(2 * B, REF_BYTES)
        self.caller_table = self.table[:B]
        self._arena = dev

    def group_table(self, k: int) -> torch.Tensor:
        lo = self._starts[k]
        return self.table[lo:lo + len(self.groups[k][1])]
