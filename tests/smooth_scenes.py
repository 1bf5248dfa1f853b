"""The 12-frame sequences the smoother's tests share (tests/test_gpu_smooth.py on the kernel, tests/test_smooth_core_cpu.py on the header's
CPU build): for every frame exactly the buffers sp_track_associate leaves behind for one image, made by a scripted tracker (persons keep
their id while they are seen or missed for at most MAX_AGE frames, new persons take the lowest free slot and, when none is free, the
unseen track with the largest miss), plus the frame's time.  Births, empty frames, a return inside max_gap and one after it, a repeated
timestamp and one that goes backwards, slots handed to new ids, NaN coordinates and confidences, confidences exactly at in_vis_thre, boxes
of zero and negative extent, and the rows scattered behind seg[0] > 0."""
import numpy as np

from tests import smooth_ref

MAX_AGE = 2
FRAMES = 12
TIMES = [0.0, 0.04, 0.07, 0.11, 0.15, 0.15, 0.5, 0.8, 0.78, 0.83, 0.86, 0.9]      # f5 repeats f4's; f7 comes 0.65 s after f5; f8 goes backwards
CASES = {"slots1_j17": (1, 17), "slots4_j17": (4, 17), "slots40_j17": (40, 17), "slots4_j5": (4, 5), "slots2_j64": (2, 64)}
PARAMS = smooth_ref.params(min_cutoff=1.0, beta=0.5, d_cutoff=1.0, max_gap=0.5, in_vis_thre=0.2)


class _Tracks:
    """The scripted tracker: slot table t_id [slots], miss [slots]; step(persons seen) -> their ids."""

    def __init__(self, slots):
        self.id, self.miss, self.person, self.next_id = np.zeros(slots, np.int32), np.zeros(slots, np.int32), {}, 1

    def step(self, who):
        seen = {self.person[w] for w in who if w in self.person}
        unseen = sorted((t for t in range(self.id.size) if self.id[t] != 0 and t not in seen), key=lambda t: (-int(self.miss[t]), t))
        free = [t for t in range(self.id.size) if self.id[t] == 0]
        born = set()
        for w in who:
            if w in self.person:
                continue
            t = free.pop(0) if free else unseen.pop(0)
            self.person = {k: v for k, v in self.person.items() if v != t}
            self.person[w], self.id[t], self.next_id = t, self.next_id, self.next_id + 1
            born.add(t)
        for t in range(self.id.size):
            if self.id[t] == 0:
                continue
            if t in seen or t in born:
                self.miss[t] = 0
            else:
                self.miss[t] += 1
                if self.miss[t] > MAX_AGE:
                    self.id[t] = self.miss[t] = 0
                    self.person = {k: v for k, v in self.person.items() if v != t}
        return np.array([self.id[self.person[w]] for w in who], np.int32).reshape(len(who))


def sequence(case):
    """-> list of FRAMES dicts: now, kps [rows, J, 3], box [rows, 5] f32, track_id [rows], keep [rows], keep_count, seg [2], t_id [slots]."""
    slots, J = CASES[case]
    rng = np.random.default_rng(31 * slots + J)
    people = 2 * slots
    half = max(1, (slots + 1) // 2)
    first, everyone, late = list(range(half)), list(range(slots)), list(range(slots, 2 * slots))
    plan = [first, first, everyone, [], first, first, [], first, first, late, late, first + late[:slots - half]]
    assert len(plan) == FRAMES == len(TIMES)
    base, shape = rng.uniform(100, 1900, (people, 1, 2)), rng.uniform(-60, 60, (people, J, 2))
    conf = rng.uniform(0.05, 1.0, (people, J, 1))                                 # some joints sit below in_vis_thre for the whole sequence
    tracks = _Tracks(slots)
    rows, lo = slots + 5, 2
    frames = []
    for f, who in enumerate(plan):
        n = len(who)
        ids = tracks.step(who)
        pos = base + rng.normal(0, 2.0, (people, 1, 2)) + rng.normal(0, 0.7, (people, J, 2))
        k = np.concatenate([pos + shape, np.clip(conf + rng.normal(0, 0.02, (people, J, 1)), 0.01, 1.0)], 2)[who].reshape(n, J, 3)
        for _ in range(n):                                                        # a few bad samples per frame
            p, j = int(rng.integers(0, n)), int(rng.integers(0, J))
            kind = int(rng.integers(0, 4))
            if kind == 0:
                k[p, j, int(rng.integers(0, 2))] = np.nan
            elif kind == 1:
                k[p, j, 2] = np.nan
            elif kind == 2:
                k[p, j, 2] = PARAMS["in_vis_thre"]                                # exactly at the threshold: not usable
            else:
                k[p, j, 0] = np.inf
        where = lo + rng.permutation(rows - lo)[:n]                               # the kept rows, scattered; keep lists them in pick order
        kps = np.concatenate([rng.uniform(0, 2000, (rows, J, 2)), rng.uniform(0.3, 1, (rows, J, 1))], 2)
        x1y1 = rng.uniform(0, 1500, (rows, 2))
        box = np.concatenate([x1y1, x1y1 + rng.uniform(40, 400, (rows, 2)), rng.uniform(0, 1, (rows, 1))], 1).astype(np.float32)
        kps[where] = k
        if n >= 1 and f % 3 == 1:
            box[where[0], 2:4] = box[where[0], 0:2]                               # zero extent: size 1
        if n >= 1 and f % 3 == 2:
            box[where[-1], 2:4] = box[where[-1], 0:2] - np.float32(3.0)           # negative extent: size 1
        track_id = np.zeros(rows, np.int32)
        track_id[where] = ids
        keep = np.full(rows, -1, np.int32)
        keep[lo:lo + n] = where
        frames.append({"now": TIMES[f], "kps": kps, "box": box, "track_id": track_id, "keep": keep, "keep_count": n, "seg": [lo, rows],
                       "t_id": tracks.id.copy()})
    return frames


_REF = {}


def reference(case):
    """smooth_ref over the sequence, computed once per case and left unchanged: a list of (kps_smooth, state after the frame)."""
    if case not in _REF:
        slots, J = CASES[case]
        st, out = smooth_ref.SmoothState(slots, J), []
        for fr in sequence(case):
            k = smooth_ref.smooth(st, fr["kps"], fr["box"], fr["track_id"], fr["keep"], fr["keep_count"], fr["seg"], fr["t_id"], fr["now"], PARAMS)
            out.append((k, st.copy()))
        _REF[case] = out
    return _REF[case]


def bits_equal(got, want, what=""):
    """Bit for bit, NaN-aware: same NaN-ness everywhere, the same bits wherever the value is a number (and the same sign of zero)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        np.testing.assert_array_equal(gn, wn, err_msg=f"{what}: NaN positions")
        view = {8: np.uint64, 4: np.uint32}[got.dtype.itemsize]
        np.testing.assert_array_equal(got.view(view)[~gn], want.view(view)[~wn], err_msg=what)
    else:
        np.testing.assert_array_equal(got, want, err_msg=what)
