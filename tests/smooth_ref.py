"""The key-point smoother's rules on the CPU, written for this project from include/simple_pose_hip.h (sp_track_smooth) and
simple_pose_amd/csrc/sp_smooth.h: the One-Euro filter (Casiez, Roussel, Vogel, CHI 2012) per track and joint, numpy float64 scalars,
operation by operation in the header's order, the state in plain arrays.  The reference project has no tracker and no smoother; this file is
what the device kernel and the header's CPU build are compared with.  It imports nothing of the library."""
import numpy as np

TWO_PI = np.float64(6.283185307179586)
F = np.float64
DEFAULTS = {"min_cutoff": 1.0, "beta": 0.5, "d_cutoff": 1.0, "max_gap": 0.5, "in_vis_thre": 0.2}


class SmoothState:
    def __init__(self, slots, joints):
        self.slots, self.joints = slots, joints
        self.id = np.zeros(slots, np.int32)
        self.x = np.zeros((slots, joints, 2), np.float64)
        self.dx = np.zeros((slots, joints, 2), np.float64)
        self.t = np.zeros((slots, joints), np.float64)
        self.n = np.zeros((slots, joints), np.int32)
        self.events = {"start": 0, "restart_gap": 0, "restart_time": 0, "update": 0, "pass": 0, "takeover": 0}     # what the calls went through

    def copy(self):
        c = SmoothState(self.slots, self.joints)
        for k in ("id", "x", "dx", "t", "n"):
            setattr(c, k, getattr(self, k).copy())
        c.events = dict(self.events)
        return c


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def box_size(box_row):
    """max(x2 - x1, y2 - y1) in float32 (w > h ? w : h), widened; 1.0 unless that is > 0."""
    b = np.asarray(box_row, np.float32)
    with np.errstate(all="ignore"):
        w, h = np.float32(b[2] - b[0]), np.float32(b[3] - b[1])
    size = F(w if w > h else h)
    return size if size > 0 else F(1.0)


def joint(st, slot, j, x, y, c, now, size, p):
    """One sample of one joint -> (x, y, c) out; the state of (slot, j) advances."""
    x, y, c, now, size = F(x), F(y), F(c), F(now), F(size)
    ev = st.events
    if not (c > F(p["in_vis_thre"])) or not np.isfinite(x) or not np.isfinite(y):
        ev["pass"] += 1
        return x, y, c
    with np.errstate(all="ignore"):
        Te = now - st.t[slot, j]
        if st.n[slot, j] == 0 or not (Te > 0) or Te > F(p["max_gap"]):
            ev["start" if st.n[slot, j] == 0 else ("restart_gap" if Te > 0 else "restart_time")] += 1
            st.x[slot, j] = (x, y)
            st.dx[slot, j] = 0.0
            st.n[slot, j] = 1
            st.t[slot, j] = now
            return x, y, c
        out = [x, y]
        for a, s in enumerate((x, y)):
            xh, dxh = st.x[slot, j, a], st.dx[slot, j, a]
            d = (s - xh) / Te
            rd = (TWO_PI * F(p["d_cutoff"])) * Te
            ad = rd / (rd + F(1.0))
            dxh = ad * d + (F(1.0) - ad) * dxh
            fc = F(p["min_cutoff"]) + F(p["beta"]) * (np.abs(dxh) / size)
            r = (TWO_PI * fc) * Te
            al = r / (r + F(1.0))
            if s != xh:                                                          # equal: x^ stays exactly (the blend would round within an ulp)
                xh = al * s + (F(1.0) - al) * xh
            st.x[slot, j, a], st.dx[slot, j, a] = xh, dxh
            out[a] = xh
    st.n[slot, j] += 1
    st.t[slot, j] = now
    ev["update"] += 1
    return out[0], out[1], c


def kept_rows(rows, keep, keep_count, seg, slots):
    """The rows the image kept, the count clamped as sp_track_associate clamps it."""
    lo = int(seg[0])
    if lo < 0 or lo > rows:
        return []
    n = min(max(int(keep_count), 0), slots, rows - lo)
    return [int(r) for r in np.asarray(keep)[lo:lo + n]]


def smooth(st, kps, box, track_id, keep, keep_count, seg, t_id, now, p):
    """One frame: kps [rows, J, 3], box [rows, 5] float32, track_id [rows], keep / keep_count / seg of one image, t_id [slots] ->
    kps_smooth [rows, J, 3]; `st` advances."""
    kps = np.asarray(kps, np.float64)
    rows, J = kps.shape[0], kps.shape[1]
    out = kps.copy()
    kept = set(kept_rows(rows, keep, keep_count, seg, st.slots))
    for row in range(rows):
        tid = int(track_id[row])
        where = np.nonzero(np.asarray(t_id) == tid)[0]
        if row not in kept or tid <= 0 or where.size == 0:
            continue
        slot = int(where[0])
        if st.id[slot] != tid:
            st.n[slot, :] = 0
            st.id[slot] = tid
            st.events["takeover"] += 1
        size = box_size(box[row])
        for j in range(J):
            out[row, j] = joint(st, slot, j, kps[row, j, 0], kps[row, j, 1], kps[row, j, 2], now, size, p)
    return out


class ResultSmoother:
    """smooth() over the host rows of a tracked PoseResult (pick order): what PoseTracker(smooth=...) returns in keypoints_smooth."""

    def __init__(self, slots, joints, p):
        self.state, self.p = SmoothState(slots, joints), p

    def update(self, keypoints, box, track_id, t_id, now):
        n = int(np.asarray(keypoints).shape[0])
        if n == 0:
            return np.zeros((0, self.state.joints, 3), np.float64)
        return smooth(self.state, keypoints, box, track_id, np.arange(n), n, [0, n], t_id, now, self.p)
