"""The pose overlay's pixel rules (include/simple_pose_hip.h above sp_render_poses_u8c3) restated in numpy and Python ints: a CHECKER only,
never imported by the package.  The kernels (simple_pose_amd/csrc/render.hip) and the CPU program (tests/render_core_main.cpp) are compared
with `render` bit for bit.  Integers are exact (int64 / Python ints); the one floating-point comparison is the fp64 form the rules name,
(double)c * (double)c <= (double)(r * r) * (double)L, not an exact integer comparison."""
import numpy as np

BOX_SLOTS = 4
COCO_SKELETON = ((15, 13), (13, 11), (16, 14), (14, 12), (11, 12), (5, 11), (6, 12), (5, 6), (5, 7), (6, 8), (7, 9), (8, 10), (1, 2), (0, 1),
                 (0, 2), (1, 3), (2, 4), (3, 5), (4, 6))


class Style:
    """Radii in 1/16 px, opacity in sixteenths, palette uint8 [P, 3] BGR, colour_by "person" or "part"."""

    def __init__(self, skeleton=COCO_SKELETON, joint_r=48, limb_r=16, box_r=8, opacity=16, in_vis_thre=0.2, colour_by="person", palette=None):
        self.skeleton = [(int(a), int(b)) for a, b in skeleton]
        self.joint_r, self.limb_r, self.box_r, self.opacity = int(joint_r), int(limb_r), int(box_r), int(opacity)
        self.in_vis_thre, self.colour_by = float(in_vis_thre), colour_by
        if palette is None:
            palette = [[(37 * i + 11) % 256, (91 * i + 60) % 256, (153 * i + 200) % 256] for i in range(7)]
        self.palette = np.asarray(palette, np.uint8).reshape(-1, 3)


def quantise(v):
    """q(v) = (int32) rint(v * 16.0), ties to even; None for a coordinate that is not finite or has |v| > 32768."""
    v = np.float64(v)
    if not np.isfinite(v) or abs(v) > 32768.0:
        return None
    return int(np.rint(v * np.float64(16.0)))


def capsule(ax, ay, bx, by, r, colour):
    """(ax, ay, bx, by, r, (b, g, r)) in 1/16 px, or None: the empty primitive."""
    q = [quantise(v) for v in (ax, ay, bx, by)]
    if any(v is None for v in q):
        return None
    return (q[0], q[1], q[2], q[3], int(r), tuple(int(c) for c in colour))


def person_primitives(style, kps, box, pick, track_id):
    """The 4 + E + J slots of one kept person, in slot order; None where the slot is empty."""
    P = style.palette.shape[0]
    person = style.palette[(track_id - 1) % P] if track_id is not None and track_id > 0 else style.palette[pick % P]
    part = style.colour_by == "part"
    vis = [bool(np.float64(c) > np.float64(style.in_vis_thre)) for c in kps[:, 2]]          # a NaN compares false
    out = []
    x1, y1, x2, y2 = (np.float64(v) for v in box[:4])
    for a, b in (((x1, y1), (x2, y1)), ((x2, y1), (x2, y2)), ((x2, y2), (x1, y2)), ((x1, y2), (x1, y1))):
        out.append(None if style.box_r == 0 else capsule(a[0], a[1], b[0], b[1], style.box_r, person))
    for e, (a, b) in enumerate(style.skeleton):
        ok = vis[a] and vis[b]
        out.append(capsule(kps[a, 0], kps[a, 1], kps[b, 0], kps[b, 1], style.limb_r, style.palette[e % P] if part else person) if ok else None)
    for j in range(kps.shape[0]):
        out.append(capsule(kps[j, 0], kps[j, 1], kps[j, 0], kps[j, 1], style.joint_r, style.palette[j % P] if part else person) if vis[j] else None)
    return out


def primitives(style, kps, box, track_id=None):
    """Every primitive of the kept persons (kps [n, J, 3], box [n, >=4], track_id [n] or None, all in pick order) in PAINTING order:
    persons in reverse pick order, slots in order.  Index p * (4 + E + J) + slot, as the device's array."""
    n = kps.shape[0]
    out = []
    for p in range(n):
        pick = n - 1 - p
        out += person_primitives(style, kps[pick], box[pick], pick, None if track_id is None else int(track_id[pick]))
    return out


def coverage(prim, h, w):
    """k (0..16) of every pixel the capsule can touch: (y0, x0, k int [ny, nx]) over a generous window clipped to the image, or None."""
    ax, ay, bx, by, r, _ = prim
    x0, x1 = max(0, (min(ax, bx) - r) // 16 - 1), min(w - 1, (max(ax, bx) + r) // 16 + 1)
    y0, y1 = max(0, (min(ay, by) - r) // 16 - 1), min(h - 1, (max(ay, by) + r) // 16 + 1)
    if x0 > x1 or y0 > y1:
        return None
    off = np.array([2, 6, 10, 14], np.int64)
    sx = (16 * np.arange(x0, x1 + 1, dtype=np.int64)[:, None] + off[None, :]).reshape(1, -1)
    sy = (16 * np.arange(y0, y1 + 1, dtype=np.int64)[:, None] + off[None, :]).reshape(-1, 1)
    abx, aby = np.int64(bx - ax), np.int64(by - ay)
    asx, asy = sx - ax, sy - ay
    t = asx * abx + asy * aby
    L = abx * abx + aby * aby
    r2 = np.int64(r) * np.int64(r)
    c = asx * aby - asy * abx
    in_a = asx * asx + asy * asy <= r2
    in_b = (sx - bx) ** 2 + (sy - by) ** 2 <= r2
    cd = c.astype(np.float64)
    in_s = cd * cd <= np.float64(r2) * np.float64(L)
    inside = np.where((L == 0) | (t <= 0), in_a, np.where(t >= L, in_b, in_s))
    k = inside.reshape(y1 - y0 + 1, 4, x1 - x0 + 1, 4).sum(axis=(1, 3)).astype(np.int64)
    return y0, x0, k


def blend(img, prim, opacity):
    """One primitive onto img (int64 [h, w, 3]) in place: out = (in * (256 - a) + colour * a + 128) >> 8, a = k * opacity."""
    cov = coverage(prim, img.shape[0], img.shape[1])
    if cov is None:
        return
    y0, x0, k = cov
    a = (k * opacity)[:, :, None]
    win = img[y0:y0 + k.shape[0], x0:x0 + k.shape[1]]
    win[...] = (win * (256 - a) + np.asarray(prim[5], np.int64)[None, None, :] * a + 128) >> 8


def render(img, style, kps, box, track_id=None):
    """The overlay of the kept persons on a uint8 BGR image: a new uint8 array."""
    out = np.asarray(img).astype(np.int64)
    for prim in primitives(style, np.asarray(kps, np.float64), np.asarray(box), track_id):
        if prim is not None:
            blend(out, prim, style.opacity)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def kept(kps, box, track_id, keep, keep_count, seg, image):
    """The image's kept rows as the device selects them from the frame's buffers: (kps [n, J, 3], box [n, 5], track_id [n] or None)."""
    rows = kps.shape[0]
    lo = int(seg[image])
    n = 0
    if 0 <= lo <= rows:
        n = min(max(int(keep_count[image]), 0), rows, rows - lo)
    sel = np.asarray(keep[lo:lo + n], np.int64)
    assert ((sel >= 0) & (sel < rows)).all()
    return kps[sel], box[sel], None if track_id is None else track_id[sel]


def tile_hits(prims, h, w, tile_w=64, tile_h=16):
    """Per tile, how many primitives cover at least one sample of one of its pixels: int [tiles_y, tiles_x].  Every one of them is in the
    tile's list on the device (whose box test can only add more)."""
    hits = np.zeros(((h + tile_h - 1) // tile_h, (w + tile_w - 1) // tile_w), np.int64)
    for prim in prims:
        cov = None if prim is None else coverage(prim, h, w)
        if cov is None:
            continue
        y0, x0, k = cov
        ys, xs = np.nonzero(k)
        for ty, tx in {((y0 + y) // tile_h, (x0 + x) // tile_w) for y, x in zip(ys.tolist(), xs.tolist())}:
            hits[ty, tx] += 1
    return hits
