"""How a layer becomes a launch descriptor (`sp_conv_desc`, include/simple_pose_hip.h): the one place that knows.

Pure host arithmetic: no library call, no tensor.  engine.py (inference lowering) and train.py (ConvT) build every ConvDesc through
these functions; what stays with the callers is what differs between them - weight packing, buffer shapes, FLOP counts, tile pinning.

The kernel reads input pixel (g * stride + d0 + phase + tap * d_step) for grid point g and writes output pixel (g * o_mul + o_add + phase),
per axis, for every (phase_y, phase_x) of the launch; K runs over (tap row, tap, channel), channel fastest.
"""
from __future__ import annotations

from typing import Iterator, Optional, Tuple

from ._lib import ConvDesc, SP_CONV_OUT_F32, SP_CONV_OUT_SLICE, SP_CONV_PIXEL_SHUFFLE


def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def n_pad_for(c_out: int) -> int:
    """Packed row count: the kernel's N tile must divide it (128 / 64 / 32 wide tiles)."""
    if c_out >= 128:
        return round_up(c_out, 128)
    if c_out > 32:
        return round_up(c_out, 64)
    return 32


def dgrad_store_flag(bf16: bool, g16: bool) -> int:
    """Output flag of an input-gradient launch: activation gradients are fp32 unless grad_dtype is bf16."""
    return SP_CONV_OUT_F32 if (bf16 and not g16) else 0


def grouped_panel(name: str, groups: int, cpg: int, channels: int) -> int:
    """Channels per N tile of a grouped launch: block-diagonal panels of whole groups, one per N tile; K per tap is the panel, not c_in.
    64 = one bf16 K tile / two fp32 ones and a legal tile_n of the implicit GEMM."""
    panel = 64
    while panel % cpg:
        panel *= 2
    if channels % panel or panel > 128:
        raise NotImplementedError(f"{name}: no panel width for {groups} groups of {cpg} channels in {channels}")
    return panel


def _desc(in_hwc, grid, c_out, n_pad, taps, k_pad, stride, origin, step, out_hwc, out_map=(1, 0, 1, 0), phases=1, flags=0, panel=0) -> ConvDesc:
    d = ConvDesc()
    d.batch, (d.in_h, d.in_w, d.c_in) = 1, in_hwc
    (d.grid_h, d.grid_w), d.c_out, d.n_pad = grid, c_out, n_pad
    (d.taps_h, d.taps_w), d.k_pad, d.stride = taps, k_pad, stride
    (d.dy0, d.dx0), d.dy_step, d.dx_step = origin, step, step
    d.out_h, d.out_w, d.out_c = out_hwc
    d.oy_mul, d.oy_add, d.ox_mul, d.ox_add = out_map
    d.phases_y = d.phases_x = phases
    d.flags = flags
    if panel:               # grouped launch: N tile t reads channels [t * panel, (t + 1) * panel) of every tap
        d.c_in_group, d.tile_m, d.tile_n = panel, 128, panel
    return d


def conv_fwd(h: int, w: int, c_buf: int, c_out: int, n_pad: int, kh: int, kw: int, taps_h: int, taps_w: int, k_pad: int, stride: int, pad: int,
             flags: int = 0, *, pixel_shuffle: bool = False, pair_half: Optional[int] = None, slice_of: Optional[int] = None, panel: int = 0) -> ConvDesc:
    """Conv2d(kh x kw, stride, pad) of an [h, w, c_buf] activation: grid and output size from the real kernel, taps and K from the packed
    one (tap rows padded to fill K tiles), origin -pad, unit output map.
    `pixel_shuffle`: nn.PixelShuffle(2) in the epilogue (out = 2 * grid, c_out / 4 channels; rows packed sub-pixel-major).
    `pair_half`: the x-paired bf16 stem - the NHWC4 image read as pixel pairs [h, w / 2, 8], one pair per stride-2 step, origin -pair_half.
    `slice_of`: the launch writes c_out channels of a `slice_of`-channel buffer (a producer of a concat).  `panel`: grouped launch."""
    gh, gw = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    out_hwc, out_map = (gh, gw, slice_of or c_out), (1, 0, 1, 0)
    if pixel_shuffle:
        assert c_out % 4 == 0 and n_pad == c_out
        out_hwc, out_map, flags = (gh * 2, gw * 2, c_out // 4), (2, 0, 2, 0), flags | SP_CONV_PIXEL_SHUFFLE
    if slice_of is not None:
        flags |= SP_CONV_OUT_SLICE
    d = _desc((h, w, c_buf), (gh, gw), c_out, n_pad, (taps_h, taps_w), k_pad, stride, (-pad, -pad), 1, out_hwc, out_map, flags=flags, panel=panel)
    if pair_half is not None:
        d.in_w, d.stride_x, d.dx0 = w // 2, 1, -pair_half
    return d


def deconv_k4s2p1_fwd(h: int, w: int, c_in: int, c_out: int, n_pad: int, flags: int = 0) -> ConvDesc:
    """ConvTranspose2d(k=4, s=2, p=1): 2x2 output phases in one launch, each a 2x2-tap conv walking backwards from (g + phase); out = 2 * g + phase."""
    return _desc((h, w, c_in), (h, w), c_out, n_pad, (2, 2), 4 * c_in, 1, (0, 0), -1, (2 * h, 2 * w, c_out), (2, 0, 2, 0), phases=2, flags=flags)


def deconv_k4s2p1_dgrad(h: int, w: int, c_in: int, c_out: int, n_pad: int, flags: int = 0) -> ConvDesc:
    """Input gradient of that layer ([h, w, c_in] -> [2h, 2w, c_out]): Conv2d(k=4, s=2, p=1) of dy back onto the input grid."""
    return conv_fwd(2 * h, 2 * w, c_out, c_in, n_pad, 4, 4, 4, 4, 16 * c_out, 2, 1, flags)


def conv_dgrad_s1(oh: int, ow: int, c_dy: int, c_in: int, n_pad: int, kh: int, kw: int, k_pad: int, pad: int, flags: int = 0, *, panel: int = 0) -> ConvDesc:
    """Input gradient of a stride-1 Conv2d: the conv of dy [oh, ow, c_dy] with the flipped taps, padded by kh - 1 - pad."""
    return conv_fwd(oh, ow, c_dy, c_in, n_pad, kh, kw, kh, kw, k_pad, 1, kh - 1 - pad, flags, panel=panel)


Phase = Tuple[int, int, int, int, int, int, int, int]


def stride2_dgrad_phases(kh: int, kw: int, pad: int) -> Iterator[Phase]:
    """Input gradient of a stride-2 Conv2d, one launch per output phase (py, px): dx[2g + py] sums the ky with (2g + py + pad - ky) even, at
    oy = (2g + py + pad - ky) / 2.  Tap t of phase py is ky = ky0 + 2t (< kh) and reads oy = g + dy0 - t.  Yields
    (py, px, ky0, kx0, taps_h, taps_w, dy0, dx0); a phase without taps receives no gradient and is skipped (1x1: only phase (0, 0))."""
    for py in range(2):
        for px in range(2):
            ky0, kx0 = (py + pad) % 2, (px + pad) % 2
            th, tw = len(range(ky0, kh, 2)), len(range(kx0, kw, 2))
            if th and tw:
                yield py, px, ky0, kx0, th, tw, (py + pad - ky0) // 2, (px + pad - kx0) // 2


def conv_dgrad_s2(h: int, w: int, oh: int, ow: int, c_dy: int, c_in: int, n_pad: int, phase: Phase, k_pad: int, flags: int = 0, *, panel: int = 0) -> ConvDesc:
    """The launch of one `stride2_dgrad_phases` phase: dy [oh, ow, c_dy] -> pixels (2g + py, 2g + px) of dx [h, w, c_in]."""
    py, px, _, _, th, tw, dy0, dx0 = phase
    return _desc((oh, ow, c_dy), (h // 2, w // 2), c_in, n_pad, (th, tw), k_pad, 1, (dy0, dx0), -1, (h, w, c_in), (2, py, 2, px), flags=flags, panel=panel)


def _full_range(grid: int, size: int, stride: int, d0: int, taps: int, step: int) -> Tuple[int, int]:
    """Grid points [lo, hi) of one axis whose every tap lies inside the image (the kernel's own arithmetic, conv_igemm.hip)."""
    far = (taps - 1) * step
    a, b = -(d0 + min(far, 0)), size - 1 - d0 - max(far, 0)
    lo = 0 if a <= 0 else (a + stride - 1) // stride
    hi = min(0 if b < 0 else b // stride + 1, grid)
    return min(lo, hi), hi


def tap_skip_positions(d: ConvDesc, py: int = 0, px: int = 0) -> list:
    """Output positions (gy, gx) of phase (py, px) in the order the tap-skipping kernel hands them out: every tap inside the image on both axes
    first, then partial on x only, partial on y only, partial on both (interior, edges, corners of a padded 3x3)."""
    ylo, yhi = _full_range(d.grid_h, d.in_h, d.stride, d.dy0 + py, d.taps_h, d.dy_step)
    xlo, xhi = _full_range(d.grid_w, d.in_w, d.stride_x or d.stride, d.dx0 + px, d.taps_w, d.dx_step)
    fy, fx = list(range(ylo, yhi)), list(range(xlo, xhi))
    qy = [g for g in range(d.grid_h) if not ylo <= g < yhi]
    qx = [g for g in range(d.grid_w) if not xlo <= g < xhi]
    return [(gy, gx) for ys, xs in ((fy, fx), (fy, qx), (qy, fx), (qy, qx)) for gy in ys for gx in xs]


def tap_mask(d: ConvDesc, gy: int, gx: int, py: int = 0, px: int = 0) -> int:
    """Bit (ty * taps_w + tx) set when that tap of output position (gy, gx) reads inside the image."""
    m = 0
    for ty in range(d.taps_h):
        for tx in range(d.taps_w):
            iy = gy * d.stride + d.dy0 + py + ty * d.dy_step
            ix = gx * (d.stride_x or d.stride) + d.dx0 + px + tx * d.dx_step
            if 0 <= iy < d.in_h and 0 <= ix < d.in_w:
                m |= 1 << (ty * d.taps_w + tx)
    return m


def tap_skip_k_tiles(d: ConvDesc, batch: int, tile_m: int, k_tile: int = 32) -> Tuple[int, int]:
    """K tiles one column of N tiles executes over the whole launch (every phase, every M tile): (with tap skipping, without).
    With skipping, rows are ordered (position in `tap_skip_positions` order, image) and a tile of `tile_m` rows runs the K tiles of the taps
    that lie inside the image for at least one of its rows, `c_in / k_tile` per tap.  A launch the kernel's launcher would not take
    (one tap, batch < tile_m / 2, c_in not in whole K tiles) executes everything: both counts are equal.  The launcher's other conditions
    (fp32 inference, NHWC store, no groups) are the caller's to know."""
    taps = d.taps_h * d.taps_w
    M = batch * d.grid_h * d.grid_w
    tiles_m = (M + tile_m - 1) // tile_m
    phases = d.phases_y * d.phases_x
    full = phases * tiles_m * (d.k_pad // k_tile)
    if taps <= 1 or taps > 32 or 2 * batch < tile_m or d.c_in % k_tile or d.k_pad != taps * d.c_in:
        return full, full
    per_tap, done = d.c_in // k_tile, 0
    for ph in range(phases):
        py, px = ph // d.phases_x, ph % d.phases_x
        masks = [tap_mask(d, gy, gx, py, px) for gy, gx in tap_skip_positions(d, py, px)]
        for t in range(tiles_m):
            first, last = t * tile_m // batch, (min((t + 1) * tile_m, M) - 1) // batch
            union = 0
            for i in range(first, last + 1):
                union |= masks[i]
            done += max(bin(union).count("1"), 1) * per_tap
    return done, full
