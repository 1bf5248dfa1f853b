"""Tiled ("sliced") detection: the host side of the `sp_tile_ref` table.

The detector letterboxes a frame onto one 640-pixel canvas whatever its size, so a small person in a large frame reaches the network a
few pixels tall.  Tiled detection runs the detector on overlapping tiles of the frame at their native resolution, optionally on the
whole frame as well, and fuses the boxes.  A "pass" is one such rectangle.  This module plans the passes of a frame (`Tiling.plan`),
checks the limits, and packs the table that the launches read from device memory (`pack_tile_refs`, the counterpart of
mixed_batch.pack_image_refs): pure Python, no GPU.  `TilePlan` is the table on the device together with the buffers the launches of one
call write: sp_yolo_letterbox_tiles (inside the detector program), sp_yolo_nms_device, sp_yolo_boxes_to_frame_tiles per net-shape group,
then sp_yolo_merge_passes per call.

Table layout: the passes group by group (a group is one letterboxed net shape, so one detector forward: the tiles share one shape, the
whole frame usually has another), groups in the order their first pass appears, inside a group by (frame, slot)."""
from __future__ import annotations

import ctypes
from typing import Dict, List, Sequence, Tuple

from ._lib import SP_TILE_IOS, SP_TILE_IOU, SP_TILE_MAX_TILES, TileRef

MAX_TILES = SP_TILE_MAX_TILES        # per frame: 65 passes x 300 rows stay below SP_YOLO_NMS_MAX_CANDIDATES
MAX_PASSES_PER_CALL = 256
REF_BYTES = ctypes.sizeof(TileRef)
_METRICS = {"iou": SP_TILE_IOU, "ios": SP_TILE_IOS}


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _is_real(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def axis_positions(n: int, t: int, overlap: float) -> Tuple[int, List[int]]:
    """Tile side and tile origins along one axis of length n: t = min(t, n), lap = int(t * overlap), step = t - lap, positions
    0, step, 2 * step, ... while p + t < n, then a last position n - t."""
    t = min(t, n)
    step = t - int(t * overlap)
    pos, p = [], 0
    while p + t < n:
        pos.append(p)
        p += step
    pos.append(n - t)
    return t, pos


class Tiling(object):
    """How a frame is cut into detector passes and how their boxes are fused.

    `tile`: (w, h) of a tile in source pixels, the order of `input_shape`; a frame smaller than the tile along an axis is taken whole
    along it.  `overlap`: the fraction of a tile side that neighbours share at least (0 <= overlap < 1).  `full_frame`: the whole frame
    is pass 0 and the tiles follow (it finds the persons too large for a tile).  `metric`, `thresh`, `agnostic`: the fusion of the
    passes' boxes (sp_yolo_merge_passes) - sorted by score, a box is dropped when a kept box of its class (`agnostic`: of any class) has
    IoU ("iou") or intersection over the smaller area ("ios") above `thresh`; "ios" also removes the part of a person that a tile cut
    off, which lies inside the whole person's box but has a small IoU with it.

    The defaults are design choices, not tuned values: there are no trained weights here to tune them on."""

    def __init__(self, tile=(640, 640), overlap: float = 0.2, full_frame: bool = True, metric: str = "ios", thresh: float = 0.5,
                 agnostic: bool = False):
        if not isinstance(tile, (tuple, list)) or len(tile) != 2 or not all(_is_int(v) for v in tile):
            raise TypeError(f"tile: expected (w, h) as two ints, got {tile!r}")
        if tile[0] <= 0 or tile[1] <= 0:
            raise ValueError(f"tile: sides must be positive, got {tuple(tile)}")
        if not _is_real(overlap):
            raise TypeError(f"overlap: expected a number, got {overlap!r}")
        if not (0.0 <= overlap < 1.0):
            raise ValueError(f"overlap: expected 0 <= overlap < 1, got {overlap!r}")
        if not isinstance(metric, str):
            raise TypeError(f"metric: expected 'iou' or 'ios', got {metric!r}")
        if metric not in _METRICS:
            raise ValueError(f"metric: expected 'iou' or 'ios', got {metric!r}")
        if not _is_real(thresh):
            raise TypeError(f"thresh: expected a number, got {thresh!r}")
        if not (0.0 < thresh <= 1.0):
            raise ValueError(f"thresh: expected 0 < thresh <= 1, got {thresh!r}")
        self.tile = (int(tile[0]), int(tile[1]))
        self.overlap, self.full_frame = float(overlap), bool(full_frame)
        self.metric, self.thresh, self.agnostic = metric, float(thresh), bool(agnostic)

    def key(self) -> tuple:
        """Everything a launch depends on (captured graphs are keyed on it)."""
        return (self.tile, self.overlap, self.full_frame, self.metric, self.thresh, self.agnostic)

    @property
    def metric_code(self) -> int:
        return _METRICS[self.metric]

    def tiles(self, H: int, W: int) -> List[Tuple[int, int, int, int]]:
        """The tiles of an H x W frame as (y0, x0, h, w), row-major.  ValueError above MAX_TILES."""
        if not (_is_int(H) and _is_int(W)) or H <= 0 or W <= 0:
            raise ValueError(f"frame: expected positive sizes, got {H}x{W}")
        th, ys = axis_positions(H, self.tile[1], self.overlap)
        tw, xs = axis_positions(W, self.tile[0], self.overlap)
        if len(ys) * len(xs) > MAX_TILES:
            raise ValueError(f"a {H}x{W} frame gives {len(ys)} x {len(xs)} tiles of {th}x{tw}, above the limit of {MAX_TILES} per frame "
                             "(larger tiles or less overlap)")
        return [(y, x, th, tw) for y in ys for x in xs]

    def plan(self, H: int, W: int) -> List[Tuple[int, int, int, int]]:
        """The passes of one H x W frame as (y0, x0, h, w): with `full_frame` the whole frame first, then the tiles; a single tile that
        equals the frame is one pass only."""
        tiles = self.tiles(H, W)
        if self.full_frame and tiles != [(0, 0, H, W)]:
            return [(0, 0, H, W)] + tiles
        return tiles

    def plan_call(self, B: int, H: int, W: int) -> List[Tuple[int, int, int, int]]:
        """`plan` for a call over B frames of one size.  ValueError above MAX_PASSES_PER_CALL passes in all."""
        passes = self.plan(H, W)
        if B < 1 or B * len(passes) > MAX_PASSES_PER_CALL:
            raise ValueError(f"{B} frames x {len(passes)} passes = {B * len(passes)} passes, above the limit of {MAX_PASSES_PER_CALL} per call")
        return passes


def plan_pass_groups(passes: Sequence[Tuple[int, int, int, int]], transform):
    """Per pass `transform.geometry(h, w)` (what single_predict letterboxes a contiguous copy of it with), and the passes grouped by
    their net shape: [((out_h, out_w), [slots, ascending])], groups in the order their first pass appears."""
    geoms = [transform.geometry(h, w) for _, _, h, w in passes]
    groups: Dict[Tuple[int, int], List[int]] = {}
    for s, g in enumerate(geoms):
        if not (g["new_h"] >= 1 and g["new_w"] >= 1 and g["top"] >= 0 and g["left"] >= 0 and g["top"] + g["new_h"] <= g["out_h"]
                and g["left"] + g["new_w"] <= g["out_w"] and g["out_h"] % 2 == 0 and g["out_w"] % 2 == 0):
            raise ValueError(f"pass {s}: letterbox {passes[s][2]}x{passes[s][3]} -> {g['new_h']}x{g['new_w']} at ({g['top']}, {g['left']}) "
                             f"does not fit an even {g['out_h']}x{g['out_w']} canvas")
        groups.setdefault((int(g["out_h"]), int(g["out_w"])), []).append(s)
    return geoms, list(groups.items())


def pack_tile_refs(base_ptr: int, B: int, H: int, W: int, passes, geoms, groups):
    """The table of one call over B frames [B, H, W, 3] that start at device address `base_ptr` (module docstring): a ctypes array of
    B * len(passes) `TileRef`, and per group (index of its first entry, number of entries)."""
    P = len(passes)
    refs = (TileRef * (B * P))()
    spans, k = [], 0
    for _, slots in groups:
        spans.append((k, B * len(slots)))
        for b in range(B):
            for s in slots:
                y0, x0, h, w = passes[s]
                if not (0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= H and x0 + w <= W):
                    raise ValueError(f"pass {s}: ({y0}, {x0}) {h}x{w} does not lie inside the {H}x{W} frame")
                g, r = geoms[s], refs[k]
                r.data = int(base_ptr) + ((b * H + y0) * W + x0) * 3
                r.h, r.w, r.pitch = h, w, W
                r.new_h, r.new_w, r.top, r.left = int(g["new_h"]), int(g["new_w"]), int(g["top"]), int(g["left"])
                r.ratio = float(g["ratio"])
                r.x0, r.y0, r.image, r.slot = x0, y0, b, s
                k += 1
    return refs, spans


class TilePlan(object):
    """One call shape's passes on the device: the table of sp_tile_ref pointing into `src` (uint8 [B, H, W, 3], which the owner keeps at
    its address for as long as the plan lives), and the buffers of the launches.  Built once; nothing in it changes between calls, so a
    captured graph can point into it.
      passes        (y0, x0, h, w) per slot;  groups [((out_h, out_w), first entry, entries)]
      table         uint8 [B * passes, sizeof(sp_tile_ref)];  `group_table(k, lo, hi)` a chunk of group k's entries
      det, counts, status    sp_yolo_nms_device's output per table entry: [B * passes, max_det, 6], [B * passes], [B * passes]
      cand, cand_counts      the frames' candidate blocks: [B, passes, max_det, 6], [B, passes]"""

    def __init__(self, tiling: Tiling, transform, src, max_det: int):
        import numpy as np
        import torch
        B, H, W = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
        self.key = self.key_of(tiling, transform, src, max_det)
        self.passes = tiling.plan_call(B, H, W)
        self.P = len(self.passes)
        self.geoms, groups = plan_pass_groups(self.passes, transform)
        refs, spans = pack_tile_refs(src.data_ptr(), B, H, W, self.passes, self.geoms, groups)
        self.groups = [(shape, lo, n) for (shape, _), (lo, n) in zip(groups, spans)]
        n = B * self.P
        host = np.frombuffer(bytes(refs), dtype=np.uint8).reshape(n, REF_BYTES).copy()
        dev = src.device
        self.table = torch.from_numpy(host).to(dev)
        self.det = torch.zeros((n, max_det, 6), dtype=torch.float32, device=dev)
        self.counts = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.status = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.cand = torch.zeros((B, self.P, max_det, 6), dtype=torch.float32, device=dev)
        self.cand_counts = torch.zeros((B, self.P), dtype=torch.int32, device=dev)
        self.B, self.max_det = B, max_det
        self.keepalive: list = []            # what the launches of a captured call point into besides this plan (pools, workspaces)

    @staticmethod
    def key_of(tiling: Tiling, transform, src, max_det: int) -> tuple:
        """What a plan was built from: another key needs another plan."""
        return (tiling.key(), tuple(src.shape), src.data_ptr(), max_det, str(transform.new_shape), transform.minimum_rectangle,
                transform.scale_up)

    def group_table(self, k: int, lo: int, hi: int):
        """Entries [lo, hi) of group k."""
        first = self.groups[k][1]
        return self.table[first + lo:first + hi]
