"""Box -> crop geometry of the detector-driven path: the two helpers of the reference's `commons/joint_utils.py` that sit
next to the hot path - `box_to_center_scale` (:39-56) and `get_affine_transform` (:115-152).  A few float operations per person
on the host (they only produce the 2x3 matrices); the pixel work, `cv.warpAffine`, runs on the GPU
(`simple_pose_amd.datasets.naive_data.crop_boxes`).  Arithmetic types follow the reference step by step (float32 points,
float64 solve) so that the matrices agree to the last bits."""
from __future__ import annotations

import math
import random

import numpy as np

_F32 = np.float32


def box_to_center_scale(x, y, w, h, aspect_ratio=1.0, scale_mult=1.25):
    """(center [2] float32, scale [2] float32): box centre; the box grown to `aspect_ratio` (= w/h of the network input) on its
    short side, then enlarged by `scale_mult` - unless the centre's x is the sentinel -1."""
    cx, cy = x + w * 0.5, y + h * 0.5
    if w > aspect_ratio * h:
        h = w / aspect_ratio
    elif w < aspect_ratio * h:
        w = h * aspect_ratio
    center = np.array([cx, cy], dtype=_F32)
    scale = np.array([w, h], dtype=_F32)
    return center, (scale * scale_mult if center[0] != -1 else scale)


def _solve_affine(p: np.ndarray, q: np.ndarray) -> np.ndarray:
    """cv.getAffineTransform(p, q): the 2x3 float64 map taking the three points p[i] to q[i].  Cramer's rule in Python floats
    (fixed operation order, so the matrix is bit-identical on every host; a LAPACK solve is not)."""
    (x0, y0), (x1, y1), (x2, y2) = [(float(a), float(b)) for a, b in p]
    det = x0 * (y1 - y2) - y0 * (x1 - x2) + (x1 * y2 - x2 * y1)
    out = np.empty((2, 3), np.float64)
    for k in range(2):
        u0, u1, u2 = float(q[0][k]), float(q[1][k]), float(q[2][k])
        out[k, 0] = (u0 * (y1 - y2) - y0 * (u1 - u2) + (u1 * y2 - u2 * y1)) / det
        out[k, 1] = (x0 * (u1 - u2) - u0 * (x1 - x2) + (x1 * u2 - x2 * u1)) / det
        out[k, 2] = (x0 * (y1 * u2 - y2 * u1) - y0 * (x1 * u2 - x2 * u1) + u0 * (x1 * y2 - x2 * y1)) / det
    return out


def _triangle(p0, p1) -> np.ndarray:
    """Three float32 points: p0, p1 (each rounded to float32 once), and the corner that makes a right angle at p1."""
    pts = np.zeros((3, 2), dtype=_F32)
    pts[0] = p0
    pts[1] = p1
    d = pts[0] - pts[1]
    pts[2] = pts[1] + np.array([-d[1], d[0]], dtype=_F32)
    return pts


def get_affine_transform(center, scale, rot, output_size, shift=np.array([0, 0], dtype=_F32)):
    """(trans, trans_inv), both 2x3 float64: `trans` maps image coordinates of the (center, scale) box, rotated by `rot`
    degrees, onto an `output_size` = (w, h) crop; `trans_inv` goes back (what the decoders take).  Only the box WIDTH sets the
    zoom (the reference's convention)."""
    if not isinstance(scale, (np.ndarray, list)):
        scale = np.array([scale, scale])
    out_w, out_h = output_size[0], output_size[1]
    theta = math.pi * rot / 180
    sn, cs = np.sin(theta), np.cos(theta)
    half = scale[0] * -0.5                                       # the "up" vector of the box: (0, -w/2), rotated
    offset = scale * shift
    up = np.array([0 * cs - half * sn, 0 * sn + half * cs])       # float64
    src = _triangle(center + offset, center + up + offset)
    mid = np.array([out_w * 0.5, out_h * 0.5])
    dst = _triangle(mid, mid + np.array([0, out_w * -0.5], _F32))
    return _solve_affine(src, dst), _solve_affine(dst, src)


# ---- the training-side augmentation geometry (reference `commons/joint_utils.py`: box_crop :6-36, center_scale_to_box :59-68,
# affine_transform_batch :89-101, the joint half of flip_joints :104-113).  Host numpy per sample; the pixels are warped on the GPU.

def box_crop(bbox, img_width, img_ht, rng=None):
    """Random crop / jitter of a person box (x1, y1, x2, y2) inside a `img_width` x `img_ht` image.  `rng` = (random.Random,
    np.random.RandomState) pair (default: the global `random` / `np.random` modules).  Draws, in order: one `random.uniform(0, 1)`
    for the branch; then either two more `random.uniform(0, 1)` (a shrunken patch at a random place, path_scale > 0.85) or four
    `np.random.normal` (per-side jitter clamped to the image).  Returns a NEW box of the caller's container type - a float32 array
    stays a float32 array, so its stores round as the reference's in-place stores do; the caller's box is not mutated."""
    py, npr = rng if rng is not None else (random, np.random)
    out = bbox.copy() if isinstance(bbox, np.ndarray) else list(bbox)
    x1, y1, x2, y2 = out[0], out[1], out[2], out[3]
    width, ht = x2 - x1, y2 - y1
    path_scale = py.uniform(0, 1)
    if path_scale > 0.85:
        ratio = ht / width
        if width < ht:
            pw = path_scale * width
            ph = pw * ratio
        else:
            ph = path_scale * ht
            pw = ph / ratio
        xmin = x1 + py.uniform(0, 1) * (width - pw)
        ymin = y1 + py.uniform(0, 1) * (ht - ph)
        xmax, ymax = xmin + pw + 1, ymin + ph + 1
    else:
        xmin = max(1, min(x1 + npr.normal(-0.0142, 0.1158) * width, img_width - 3))
        ymin = max(1, min(y1 + npr.normal(0.0043, 0.068) * ht, img_ht - 3))
        xmax = min(max(xmin + 2, x2 + npr.normal(0.0154, 0.1337) * width), img_width - 3)
        ymax = min(max(ymin + 2, y2 + npr.normal(-0.0013, 0.0711) * ht), img_ht - 3)
    out[0], out[1], out[2], out[3] = xmin, ymin, xmax, ymax
    return out


def center_scale_to_box(center, scale):
    """(xmin, ymin, xmax, ymax) of the box `scale` = (w, h) wide around `center` (float32 in, float32 scalars out)."""
    w, h = scale[0] * 1.0, scale[1] * 1.0
    xmin, ymin = center[0] - w * 0.5, center[1] - h * 0.5
    return xmin, ymin, xmin + w, ymin + h


def affine_transform_batch(joints, t):
    """joints [..., J, 3] float32 (x, y, vis) through the 2x3 float64 map(s) `t` ([2,3], or [..., 2, 3] one per leading index):
    only joints with vis > 0 move; x' = x*t00 + y*t01 + t02 evaluated in float64 (separately rounded products, left to right - no
    FMA) and rounded back to float32.  Returns a new array."""
    joints = np.asarray(joints, _F32)
    t = np.asarray(t, np.float64)
    out = joints.copy()
    x, y = joints[..., 0].astype(np.float64), joints[..., 1].astype(np.float64)
    tt = t[..., None, :, :] if t.ndim > 2 else t
    nx = x * tt[..., 0, 0] + y * tt[..., 0, 1] + tt[..., 0, 2]
    ny = x * tt[..., 1, 0] + y * tt[..., 1, 1] + tt[..., 1, 2]
    vis = joints[..., 2] > 0
    out[..., 0] = np.where(vis, nx.astype(_F32), joints[..., 0])
    out[..., 1] = np.where(vis, ny.astype(_F32), joints[..., 1])
    return out


def flip_joints(joints, width, joint_pairs):
    """The joint half of a horizontal flip of a `width` px wide image: x -> width - x - 1 (float32), then the left/right pairs
    swap rows.  Returns a new array; the image itself is flipped at read time by the warp kernel."""
    out = np.array(joints, _F32, copy=True)
    out[:, 0] = width - out[:, 0] - 1
    perm = np.arange(out.shape[0])
    for a, b in joint_pairs:
        perm[a], perm[b] = perm[b], perm[a]
    return out[perm]


def _solve_affine_batch(p: np.ndarray, q: np.ndarray) -> np.ndarray:
    """`_solve_affine` for a batch: p [B,3,2], q [3,2] or [B,3,2] (float32) -> [B,2,3] float64.  The same float64 operations in the
    same order, element-wise (numpy ufuncs round every operation, nothing is fused), so every matrix has the per-sample bits."""
    p, q = np.asarray(p, np.float64), np.broadcast_to(np.asarray(q, np.float64), p.shape)
    x0, y0, x1, y1, x2, y2 = p[:, 0, 0], p[:, 0, 1], p[:, 1, 0], p[:, 1, 1], p[:, 2, 0], p[:, 2, 1]
    det = x0 * (y1 - y2) - y0 * (x1 - x2) + (x1 * y2 - x2 * y1)
    out = np.empty((p.shape[0], 2, 3), np.float64)
    for k in range(2):
        u0, u1, u2 = q[:, 0, k], q[:, 1, k], q[:, 2, k]
        out[:, k, 0] = (u0 * (y1 - y2) - y0 * (u1 - u2) + (u1 * y2 - u2 * y1)) / det
        out[:, k, 1] = (x0 * (u1 - u2) - u0 * (x1 - x2) + (x1 * u2 - x2 * u1)) / det
        out[:, k, 2] = (x0 * (y1 * u2 - y2 * u1) - y0 * (x1 * u2 - x2 * u1) + u0 * (x1 * y2 - x2 * y1)) / det
    return out


def _triangle_batch(p0, p1) -> np.ndarray:
    """`_triangle` for a batch: p0, p1 [B,2] -> [B,3,2] float32 (same element-wise float32 operations)."""
    pts = np.zeros((p0.shape[0], 3, 2), dtype=_F32)
    pts[:, 0] = p0
    pts[:, 1] = p1
    d = pts[:, 0] - pts[:, 1]
    pts[:, 2] = pts[:, 1] + np.stack([-d[:, 1], d[:, 0]], axis=-1)
    return pts


def get_affine_transform_batch(center, scale, rot, output_sizes):
    """`get_affine_transform(center[i], scale[i], rot[i], size)` for every sample i and every size in `output_sizes`, with the bits
    of the per-sample calls: center, scale [B,2] float32, rot [B] -> [(trans [B,2,3], trans_inv [B,2,3]) per size].  The sine and
    cosine are taken one sample at a time, as the per-sample call does (a vectorised libm loop may round differently)."""
    center, scale = np.asarray(center, _F32), np.asarray(scale, _F32)
    theta = [math.pi * r / 180 for r in rot]
    sn = np.array([np.sin(t) for t in theta], np.float64)
    cs = np.array([np.cos(t) for t in theta], np.float64)
    half = scale[:, 0] * -0.5                                    # float32, as scale[0] * -0.5
    offset = scale * np.zeros(2, _F32)
    up = np.stack([0 * cs - half * sn, 0 * sn + half * cs], axis=-1)
    src = _triangle_batch(center + offset, center + up + offset)
    out = []
    for size in output_sizes:
        out_w, out_h = size[0], size[1]
        mid = np.array([out_w * 0.5, out_h * 0.5])
        dst = _triangle(mid, mid + np.array([0, out_w * -0.5], _F32))
        out.append((_solve_affine_batch(src, dst), _solve_affine_batch(np.broadcast_to(dst, src.shape), src)))
    return out
