"""The heat overlay's rules (include/simple_pose_hip.h above sp_heat_overlay_u8c3; simple_pose_amd/csrc/sp_heat.h) restated in numpy: what
the kernels of heat.hip and the CPU program tests/heat_core_main.cpp are compared with, bit for bit.  float32 and float64 operations in the
stated order (one fp32 multiply under the quantisation; the inversion statement by statement in Python floats, tests/warp_edges.py; one
fp64 multiply under the rint of the coefficients), int64 for the fixed point.  No bounding box here: every person is sampled at every
pixel, which is what a box must never change."""
import numpy as np

from tests.warp_edges import invert_affine

ALPHAS = {"constant": 0, "value": 1}
ALL_JOINTS = (1 << 64) - 1


class Style(object):
    """sp_heat_style in the C ABI's units: joint_mask (int, bit j = joint j), scale (float32), threshold 1..255, opacity16 0..16, alpha."""

    def __init__(self, joint_mask=ALL_JOINTS, scale=255.0, threshold=26, opacity16=10, alpha="value"):
        self.joint_mask, self.scale, self.threshold, self.opacity16, self.alpha = int(joint_mask), np.float32(scale), int(threshold), int(opacity16), alpha


def gray_lut():
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)


def q8(m, scale):
    """sp_heat_q on an array: v = m * scale in float32; NaN 0, >= 255 255, > 0 truncated, else 0."""
    with np.errstate(all="ignore"):
        v = np.asarray(m, np.float32) * np.float32(scale)
        out = np.zeros(v.shape, np.uint8)
        big = v >= np.float32(255.0)
        pos = (v > np.float32(0.0)) & ~big
        out[big] = 255
        out[pos] = v[pos].astype(np.int32).astype(np.uint8)
    return out


def plane(maps, joint_mask, scale):
    """maps float32 [J, h, w] -> the u8 plane, or None when no bit below J is set.  np.fmax: a NaN loses against every number."""
    js = [j for j in range(maps.shape[0]) if (joint_mask >> j) & 1]
    if not js:
        return None
    m = maps[js[0]]
    for j in js[1:]:
        m = np.fmax(m, maps[j])
    return q8(m, scale)


def forward(trans_inv):
    """trans_inv float32 [2, 3] -> the six int coefficients c (1/65536 px), or None when the person is skipped."""
    with np.errstate(all="ignore"):
        F = invert_affine(np.asarray(trans_inv, np.float32).astype(np.float64))
    for i in range(6):
        if not (abs(F[i]) <= (1048576.0 if i in (2, 5) else 1024.0)):
            return None
    if F[0] == 0.0 and F[1] == 0.0 and F[3] == 0.0 and F[4] == 0.0:
        return None
    return [int(np.rint(float(F[i]) * 65536.0)) for i in range(6)]


def sample(pl, c, H, W):
    """val of every pixel of an H x W image for one person's plane: int64 [H, W] in 0..255."""
    mh, mw = pl.shape
    X, Y = np.arange(W, dtype=np.int64)[None, :], np.arange(H, dtype=np.int64)[:, None]
    U, V = c[0] * X + c[1] * Y + c[2], c[3] * X + c[4] * Y + c[5]
    u, v = U >> 8, V >> 8
    xi, fx, yi, fy = u >> 8, u & 255, v >> 8, v & 255
    inside = (xi >= -1) & (xi <= mw - 1) & (yi >= -1) & (yi <= mh - 1)
    xs, ys = np.clip(xi, -1, mw - 1) + 1, np.clip(yi, -1, mh - 1) + 1        # into the plane padded by one cell of zeros each way
    pp = np.pad(pl.astype(np.int64), 1)
    p00, p10, p01, p11 = pp[ys, xs], pp[ys, xs + 1], pp[ys + 1, xs], pp[ys + 1, xs + 1]
    val = ((256 - fx) * (256 - fy) * p00 + fx * (256 - fy) * p10 + (256 - fx) * fy * p01 + fx * fy * p11 + 32768) >> 16
    return np.where(inside, val, 0)


def live_rows(keep, keep_count, seg, image, rows):
    """sp_render_live + the row check: the rows of the image's live persons that are drawn."""
    lo = int(seg[image])
    if lo < 0 or lo > rows:
        return []
    n = min(max(int(keep_count[image]), 0), rows, rows - lo)
    return [int(r) for r in keep[lo:lo + n] if 0 <= int(r) < rows]


def vmax(H, W, style, hm, trans_inv, rows):
    """Vmax int64 [H, W]: the maximum of val over the persons `rows` (any order)."""
    out = np.zeros((H, W), np.int64)
    for row in rows:
        pl = plane(hm[row], style.joint_mask, style.scale)
        c = forward(trans_inv[row])
        if pl is None or c is None:
            continue
        out = np.maximum(out, sample(pl, c, H, W))
    return out


def overlay(img, style, hm, trans_inv, rows, lut):
    """The overlay of the persons `rows` (indices into hm / trans_inv) on img uint8 [H, W, 3] -> a new image."""
    H, W = img.shape[:2]
    vm = vmax(H, W, style, hm, trans_inv, rows)
    a = 256 if style.alpha == "constant" else vm + (vm >> 7)
    w = (style.opacity16 * a * np.ones_like(vm))[..., None]
    colour = np.asarray(lut, np.uint8).astype(np.int64)[vm]
    out = (img.astype(np.int64) * (4096 - w) + colour * w + 2048) >> 12
    return np.where((vm >= style.threshold)[..., None], out, img).astype(np.uint8)
