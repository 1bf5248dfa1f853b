"""The redaction's rules (include/simple_pose_hip.h above sp_redact_u8c3) restated in numpy and Python ints: a CHECKER only, never imported
by the package.  The kernels (simple_pose_amd/csrc/redact.hip) and the CPU program (tests/redact_core_main.cpp) are compared with `redact`
bit for bit.  Everything is exact integer arithmetic (Python ints) behind the overlay's quantisation, render_ref.quantise."""
import numpy as np

from tests.render_ref import kept, quantise            # noqa: F401  (`kept` is re-exported for the scenes)

CELLS = (4, 8, 16, 32, 64)
MAX_RADIUS = 1 << 20


class Style:
    """expand in sixteenths, head_min and top_frac in 1/256, fill BGR."""

    def __init__(self, region="head", mode="mosaic", cell=16, expand=24, head_min=20, head_joints=(0, 1, 2, 3, 4), fallback="box_top",
                 top_frac=64, in_vis_thre=0.2, fill=(0, 0, 0)):
        assert region in ("head", "person") and mode in ("mosaic", "fill") and cell in CELLS and fallback in ("box_top", "box", "none")
        self.region, self.mode, self.cell, self.fallback = region, mode, int(cell), fallback
        self.expand, self.head_min, self.top_frac = int(expand), int(head_min), int(top_frac)
        self.head_joints, self.in_vis_thre = tuple(int(j) for j in head_joints), float(in_vis_thre)
        self.fill = tuple(int(c) for c in fill)


def quantised_box(box):
    """(x1, y1, x2, y2) in 1/16 px with both axes ordered by min / max, or None when q rejects one of the four."""
    q = [quantise(np.float64(v)) for v in box[:4]]
    if any(v is None for v in q):
        return None
    return min(q[0], q[2]), min(q[1], q[3]), max(q[0], q[2]), max(q[1], q[3])


def region(style, kps, box):
    """One kept person's region: ("disc", cx, cy, r), ("rect", ax, ay, bx, by) or None (empty)."""
    qb = quantised_box(box)
    if style.region == "person":
        return None if qb is None else ("rect",) + qb
    pts = []
    for j in style.head_joints:
        x, y, c = kps[j]
        if not bool(np.float64(c) > np.float64(style.in_vis_thre)):          # a NaN compares false
            continue
        qx, qy = quantise(x), quantise(y)
        if qx is None or qy is None:
            continue
        pts.append((qx, qy))
    if pts:
        minx, maxx = min(p[0] for p in pts), max(p[0] for p in pts)
        miny, maxy = min(p[1] for p in pts), max(p[1] for p in pts)
        e = max(maxx - minx, maxy - miny)
        s = 0 if qb is None else max(qb[2] - qb[0], qb[3] - qb[1])
        r0 = max(e >> 1, (s * style.head_min) >> 8)
        return ("disc", (minx + maxx) >> 1, (miny + maxy) >> 1, min((r0 * style.expand) >> 4, MAX_RADIUS))
    if style.fallback == "none" or qb is None:
        return None
    if style.fallback == "box":
        return ("rect",) + qb
    x1, y1, x2, y2 = qb
    return ("rect", x1, y1, x2, y1 + (((y2 - y1) * style.top_frac) >> 8))


def regions(style, kps, box):
    """The regions of the kept persons (kps [n, J, 3], box [n, >= 4]); None where a slot is empty."""
    return [region(style, np.asarray(kps[p], np.float64), np.asarray(box[p])) for p in range(len(kps))]


def meets(reg, X0, Y0, X1, Y1):
    """Does the region meet the closed rectangle [16 X0, 16 X1 + 15] x [16 Y0, 16 Y1 + 15] ?"""
    if reg is None:
        return False
    lx, hx, ly, hy = 16 * X0, 16 * X1 + 15, 16 * Y0, 16 * Y1 + 15
    if reg[0] == "rect":
        _, ax, ay, bx, by = reg
        return ax <= hx and bx >= lx and ay <= hy and by >= ly
    _, cx, cy, r = reg
    dx, dy = max(lx - cx, 0, cx - hx), max(ly - cy, 0, cy - hy)
    return dx * dx + dy * dy <= r * r


def hit_cells(regs, h, w, cell):
    """bool [ceil(h / cell), ceil(w / cell)]: the cells some region meets."""
    ny, nx = (h + cell - 1) // cell, (w + cell - 1) // cell
    hit = np.zeros((ny, nx), bool)
    for cy in range(ny):
        for cx in range(nx):
            X0, Y0 = cx * cell, cy * cell
            X1, Y1 = min(X0 + cell, w) - 1, min(Y0 + cell, h) - 1
            hit[cy, cx] = any(meets(r, X0, Y0, X1, Y1) for r in regs)
    return hit


def apply(img, hit, style):
    """The hit cells of a uint8 BGR image redacted: a new uint8 array.  The sums come from `img`, never from the output."""
    src = np.asarray(img)
    out = src.copy()
    h, w = src.shape[:2]
    c = style.cell
    for cy, cx in zip(*np.nonzero(hit)):
        ys, xs = slice(cy * c, min(cy * c + c, h)), slice(cx * c, min(cx * c + c, w))
        if style.mode == "fill":
            out[ys, xs] = np.asarray(style.fill, np.uint8)
            continue
        block = src[ys, xs].astype(np.int64).reshape(-1, 3)
        n = block.shape[0]
        out[ys, xs] = ((block.sum(axis=0) + n // 2) // n).astype(np.uint8)
    return out


def redact(img, style, kps, box):
    """The redaction of the kept persons (kps [n, J, 3], box [n, >= 4]) on a uint8 BGR image: a new uint8 array."""
    h, w = np.asarray(img).shape[:2]
    return apply(img, hit_cells(regions(style, kps, box), h, w, style.cell), style)


def tile_hits(regs, h, w, cell, tile_w=64):
    """Per tile of 64 x max(16, cell) pixels, how many of its cells are hit: int [tiles_y, tiles_x].  A tile with 0 is one the device
    leaves alone in place."""
    tile_h = max(16, cell)
    hit = hit_cells(regs, h, w, cell)
    out = np.zeros(((h + tile_h - 1) // tile_h, (w + tile_w - 1) // tile_w), np.int64)
    for cy, cx in zip(*np.nonzero(hit)):
        out[cy * cell // tile_h, cx * cell // tile_w] += 1
    return out
