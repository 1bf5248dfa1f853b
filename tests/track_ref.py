"""The tracker's rules on the CPU, written for this project from include/simple_pose_hip.h (sp_track_associate, sp_track_boxes): numpy
float64 for the association, numpy float32 scalars for the boxes, the state in plain arrays.  The reference project has no tracker; this
file is what the device kernels are compared with."""
import math

import numpy as np

COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0


class TrackState:
    def __init__(self, slots, joints):
        self.slots, self.joints = slots, joints
        self.id = np.zeros(slots, np.int32)
        self.age = np.zeros(slots, np.int32)
        self.miss = np.zeros(slots, np.int32)
        self.kps = np.zeros((slots, joints, 3), np.float64)
        self.area = np.zeros(slots, np.float64)
        self.conf = np.zeros(slots, np.float32)
        self.next_id = 1

    def copy(self):
        c = TrackState(self.slots, self.joints)
        for k in ("id", "age", "miss", "kps", "area", "conf"):
            setattr(c, k, getattr(self, k).copy())
        c.next_id = self.next_id
        return c


def _fma(a, b, c):
    """a * b + c of finite Python floats, rounded once: the sum as an exact ratio of integers, which int / int rounds correctly."""
    (na, da), (nb, db), (nc, dc) = a.as_integer_ratio(), b.as_integer_ratio(), c.as_integer_ratio()
    return (na * nb * dc + nc * da * db) / (da * db * dc)


_LOG2E, _LN2_HI, _LN2_LO = float.fromhex("0x1.71547652b82fep+0"), float.fromhex("0x1.62e42fefa39efp-1"), float.fromhex("0x1.abc9e3b39803fp-56")
_EXP_POLY = [float.fromhex(c) for c in (
    "0x1.ade156a5dcb37p-26", "0x1.28af3fca7ab0cp-22", "0x1.71dee623fde64p-19", "0x1.a01997c89e6b0p-16", "0x1.a01a014761f6ep-13",
    "0x1.6c16c1852b7b0p-10", "0x1.1111111122322p-7", "0x1.55555555502a1p-5", "0x1.5555555555511p-3", "0x1.000000000000bp-1", "1.0", "1.0")]


def exp_f64(x):
    """exp of one float64 as the device math library's double-precision exp evaluates it (ROCm device-libs, ocml expD): n = rint(x log2 e),
    t = x - n ln2 with ln2 in two parts, a degree-11 polynomial in t, the result scaled by 2^n; every multiply-add is fused.  A float64 exp is
    not correctly rounded anywhere, and numpy's differs between machines (its SIMD loops against the C library's), so a reference that is to
    be met bit for bit has to state the algorithm too.  tests/test_track_host.py holds it within 1 ulp of the true value."""
    x = float(x)
    if x != x:
        return x
    if x < -1075.0:
        return 0.0
    if x > 1024.0:
        return float("inf")
    n = round(x * _LOG2E)                                        # ties to even, as rint
    t = _fma(-float(n), _LN2_LO, _fma(-float(n), _LN2_HI, x))
    p = _EXP_POLY[0]
    for c in _EXP_POLY[1:]:
        p = _fma(t, p, c)
    try:
        return math.ldexp(p, n)                                  # rounds to nearest even where the result is subnormal
    except OverflowError:
        return float("inf")


def oks_pair(a, b, area_a, area_b, var):
    """oks_iou (datasets/naive_data.py) of two poses [J, 3] without a visibility threshold, operation by operation."""
    J = a.shape[0]
    denom = (np.float64(area_a) + np.float64(area_b)) / 2 + 1e-12
    dx, dy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
    with np.errstate(all="ignore"):
        e = (dx * dx + dy * dy) / var / denom / 2
        term = np.array([exp_f64(v) for v in (-e).tolist()], np.float64)
    den = np.float32(J) + np.float32(1e-12)                      # float32 + weak python float stays float32
    return np.sum(term) / np.float64(den)


def similarity(state, kps, area, sigmas=None):
    """S [slots, slots]: oks of live track t and pose p, -1 elsewhere."""
    sig = COCO_SIGMAS if sigmas is None else np.asarray(sigmas, np.float64)
    var = (sig * 2) * (sig * 2)
    S = np.full((state.slots, state.slots), -1.0, np.float64)
    for t in range(state.slots):
        if state.id[t] == 0:
            continue
        for p in range(min(kps.shape[0], state.slots)):
            S[t, p] = oks_pair(state.kps[t], kps[p], state.area[t], area[p], var)
    return S


def associate(state, kps, area, conf, match_thre=0.5, max_age=30, sigmas=None):
    """One frame: kps float64 [n, J, 3], area float64 [n], conf float32 [n], in pick order (n <= slots).  Updates `state` in place and
    returns (track ids int32 [n], S)."""
    kps, area, conf = np.asarray(kps, np.float64), np.asarray(area, np.float64), np.asarray(conf, np.float32)
    n, slots = kps.shape[0], state.slots
    assert n <= slots
    S = similarity(state, kps, area, sigmas)
    live = state.id != 0
    pairs = [(-S[t, p], t, p) for t in range(slots) if live[t] for p in range(n) if S[t, p] >= match_thre]      # a NaN fails the comparison
    pairs.sort()
    track_pose, pose_track = {}, {}
    for _, t, p in pairs:
        if t not in track_pose and p not in pose_track:
            track_pose[t], pose_track[p] = p, t
    free = [t for t in range(slots) if not live[t]]
    evict = sorted((t for t in range(slots) if live[t] and t not in track_pose), key=lambda t: (-int(state.miss[t]), t))
    born = set()
    for p in range(n):
        if p in pose_track:
            continue
        t = free.pop(0) if free else evict.pop(0)
        pose_track[p] = t
        born.add(t)
        state.id[t], state.age[t], state.miss[t] = state.next_id, 0, 0
        state.next_id += 1
    for p, t in pose_track.items():
        state.kps[t], state.area[t], state.conf[t] = kps[p], area[p], conf[p]
        state.miss[t] = 0
        state.age[t] += 1
    for t in range(slots):
        if live[t] and t not in track_pose and t not in born:
            state.miss[t] += 1
            if state.miss[t] > max_age:
                state.id[t] = state.age[t] = state.miss[t] = 0
    return np.array([state.id[pose_track[p]] for p in range(n)], np.int32).reshape(n), S


def boxes(state, in_vis_thre, box_expand, img_w, img_h, cls=0.0):
    """Detector rows float32 [k, 6] of the tracks with id != 0 and miss == 0, in slot order; float32 scalar arithmetic."""
    f = np.float32
    rows = []
    with np.errstate(all="ignore"):
        for t in range(state.slots):
            if state.id[t] == 0 or state.miss[t] != 0:
                continue
            q = state.kps[t].astype(np.float32)
            use = q[:, 2] > f(in_vis_thre)
            if use.sum() < 2:
                use[:] = True
            x1 = y1 = f(np.inf)
            x2 = y2 = f(-np.inf)
            for (x, y, _), u in zip(q, use):
                if not u:
                    continue
                x1, x2 = (x if x < x1 else x1), (x if x > x2 else x2)         # a NaN coordinate fails both comparisons
                y1, y2 = (y if y < y1 else y1), (y if y > y2 else y2)
            cx, cy = (x1 + x2) * f(0.5), (y1 + y2) * f(0.5)
            w, h = (x2 - x1) * f(box_expand), (y2 - y1) * f(box_expand)
            w = w if w >= f(1) else f(1)
            h = h if h >= f(1) else f(1)
            hw, hh = w * f(0.5), h * f(0.5)
            b = [cx - hw, cy - hh, cx + hw, cy + hh]
            for i in range(4):
                hi = f(img_h) if i & 1 else f(img_w)
                b[i] = b[i] if b[i] > f(0) else f(0)
                b[i] = b[i] if b[i] < hi else hi
            rows.append(b + [state.conf[t], f(cls)])
    return np.array(rows, np.float32).reshape(len(rows), 6)
