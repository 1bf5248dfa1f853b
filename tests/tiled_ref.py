"""Tiled detection restated in numpy (include/simple_pose_hip.h: sp_tile_ref and its three launches; simple_pose_amd/tiling.py):
the plan, the scatter (box_to_source's float32 arithmetic, then the add of the pass's origin) and the merge (float32, in the
operation order of the header).  No GPU; imports nothing from the package's tiling module, so that the two can disagree."""
from __future__ import annotations

import numpy as np

from tests.detector_ref import _iou_f32

F = np.float32


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
def axis_np(n, t, overlap):
    t = min(t, n)
    step = t - int(t * overlap)
    pos, p = [], 0
    while p + t < n:
        pos.append(p)
        p += step
    return t, pos + [n - t]


def plan_np(H, W, tile=(640, 640), overlap=0.2, full_frame=True):
    """Passes (y0, x0, h, w) of one frame: the whole frame first (unless the one tile equals it), then the tiles row-major."""
    th, ys = axis_np(H, tile[1], overlap)
    tw, xs = axis_np(W, tile[0], overlap)
    tiles = [(y, x, th, tw) for y in ys for x in xs]
    if full_frame and tiles != [(0, 0, H, W)]:
        return [(0, 0, H, W)] + tiles
    return tiles


# ---- the scatter --------------------------------------------------------------------------------------------------------------------------
def to_frame_np(rows, img_h, img_w, left, top, ratio, x0, y0):
    """rows float32 [n, 6] in letterboxed pixels -> frame pixels: clip to the canvas, (v - offset) / ratio, + origin; all float32."""
    r = np.array(rows, dtype=F, copy=True).reshape(-1, 6)
    lim = (F(img_w), F(img_h), F(img_w), F(img_h))
    off = (F(left), F(top), F(left), F(top))
    org = (F(x0), F(y0), F(x0), F(y0))
    for k in range(4):
        v = np.minimum(np.maximum(r[:, k], F(0)), lim[k])
        r[:, k] = ((v - off[k]) / F(ratio)).astype(F) + org[k]
    return r


def scatter_np(det, counts, status, refs, frames, passes, max_det, img_h, img_w, cand=None, cand_counts=None, status_frames=None):
    """sp_yolo_boxes_to_frame_tiles: refs[p] = dict(left, top, ratio, x0, y0, image, slot).  Buffers are created (cand with NaN, so that an
    unwritten row shows) or updated in place."""
    if cand is None:
        cand = np.full((frames, passes, max_det, 6), np.nan, F)
        cand_counts = np.full((frames, passes), -1, np.int32)
        status_frames = np.zeros((frames,), np.int32)
    for p, r in enumerate(refs):
        n = int(counts[p])
        blk = cand[r["image"], r["slot"]]
        blk[...] = 0
        blk[:n] = to_frame_np(det[p, :n], img_h, img_w, r["left"], r["top"], r["ratio"], r["x0"], r["y0"])
        cand_counts[r["image"], r["slot"]] = n
        status_frames[r["image"]] |= int(status[p])
    return cand, cand_counts, status_frames


# ---- the merge ----------------------------------------------------------------------------------------------------------------------------
def _ios_f32(a, b):
    """_iou_f32's intersection over the smaller area."""
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.maximum(np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]), F(0))
    h = np.maximum(np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]), F(0))
    inter = w * h
    with np.errstate(divide="ignore", invalid="ignore"):
        return (inter / np.minimum(area_a, area_b)).astype(F)


def merge_rows_np(rows, metric="ios", thresh=0.5, agnostic=False, max_det=300):
    """Greedy fusion of candidate rows float32 [n, 6] (in candidate order): indices kept, in pick order."""
    rows = np.asarray(rows, dtype=F).reshape(-1, 6)
    order = np.lexsort((np.arange(len(rows)), -rows[:, 4].astype(np.float64)))
    fn = _ios_f32 if metric == "ios" else _iou_f32
    keep = []
    for i in order:
        if keep:
            k = np.asarray(keep)
            with np.errstate(divide="ignore", invalid="ignore"):
                m = fn(rows[i][:4], rows[k][:, :4]) > F(thresh)          # NaN > thresh is False: no suppression
            if not agnostic:
                m &= rows[k][:, 5] == rows[i][5]
            if m.any():
                continue
        keep.append(int(i))
        if len(keep) >= max_det:
            break
    return np.asarray(keep, dtype=np.int64)


def merge_np(cand, cand_counts, metric="ios", thresh=0.5, agnostic=False, max_det=300):
    """sp_yolo_merge_passes: cand [frames, passes, M, 6], cand_counts [frames, passes] -> det [frames, max_det, 6] (zeros past the
    count), counts [frames]."""
    frames, passes = cand_counts.shape
    det = np.zeros((frames, max_det, 6), F)
    counts = np.zeros((frames,), np.int32)
    for b in range(frames):
        rows = np.concatenate([cand[b, p, :int(cand_counts[b, p])] for p in range(passes)], 0).astype(F)
        keep = merge_rows_np(rows, metric, thresh, agnostic, max_det)
        det[b, :len(keep)] = rows[keep]
        counts[b] = len(keep)
    return det, counts
