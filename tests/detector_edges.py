"""TEST HELPER: inputs that put the detector's NMS kernels at their option and chunk edges, with every decision exact.

Corner coordinates are integers below 512 (centres are half-integers, sizes integers: xywh -> xyxy is exact), objectness and class scores are
multiples of 1/8 (their fp32 product is exact, a multiple of 1/64), so the class-offset boxes (4096 * class + coordinate < 2^24), their areas
and intersections are exact integers and every IoU is ONE correctly rounded fp32 division of exact operands - computed in the same order by
detect.hip's box_iou1 and by detector_ref._iou_f32.  Every comparison against a threshold therefore decides identically on both sides.  With
at most 64 members per merge group the score-weighted sums (multiples of 1/64 below 2^15) are exact in fp32 in any order, so merged boxes are
one division too.  check_exact() asserts all of this on a case's own data; each builder asserts, on detector_ref.nms_np's result alone, that
its case reaches the edge it is named after.

tests/test_detector_edges_host.py builds every case without a GPU; tests/test_gpu_detector_edges.py runs them through sp_yolo_nms and
sp_yolo_nms_device.  The head-decode inputs of the latter are built here as well.
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from tests.detector_ref import _iou_f32, nms_np, nms_trace_np

CHUNK = 256            # detect.hip: NT, the candidates one pass of the greedy scan takes
CONF, IOU = 0.1, 0.47  # strictly between attainable values: scores are k / 64 (6 / 64 < 0.1 < 7 / 64); check_exact() keeps every IoU away from 0.47


@dataclass
class NmsCase:
    name: str
    pred: np.ndarray                   # float32 [B, N, no]
    merge: bool = False
    multi_label: bool = True
    agnostic: bool = False
    max_det: int = 300
    want: List[Optional[np.ndarray]] = field(default_factory=list)      # nms_np's result per image
    facts: dict = field(default_factory=dict)

    def kwargs(self):
        return dict(conf_thresh=CONF, iou_thresh=IOU, merge=self.merge, agnostic=self.agnostic, multi_label=self.multi_label, max_det=self.max_det)


def rows(boxes, obj8, cls8) -> np.ndarray:
    """Prediction rows [n, 5 + classes] (cx, cy, w, h, obj, cls...) from integer corners [n, 4] and scores in eighths."""
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    cls8 = np.asarray(cls8, dtype=np.int64).reshape(len(b), -1)
    assert (b >= 0).all() and (b < 512).all() and (b[:, 2] > b[:, 0]).all() and (b[:, 3] > b[:, 1]).all()
    assert (np.asarray(obj8) >= 0).all() and (np.asarray(obj8) <= 8).all() and (cls8 >= 0).all() and (cls8 <= 8).all()
    f = b.astype(np.float32)
    out = np.zeros((len(b), 5 + cls8.shape[1]), dtype=np.float32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = (f[:, 0] + f[:, 2]) / 2, (f[:, 1] + f[:, 3]) / 2, f[:, 2] - f[:, 0], f[:, 3] - f[:, 1]
    out[:, 4] = np.asarray(obj8, dtype=np.float32) / 8
    out[:, 5:] = cls8.astype(np.float32) / 8
    return out


def stack(images, n_rows=None) -> np.ndarray:
    """Images of different row counts -> [B, N, no]; the rows added have objectness 0 (never a candidate)."""
    n = n_rows or max(len(i) for i in images)
    out = np.zeros((len(images), n, images[0].shape[1]), dtype=np.float32)
    for b, im in enumerate(images):
        out[b, :len(im)] = im
    return out


def _pairwise_iou(boxes):
    return np.stack([_iou_f32(boxes[k], boxes) for k in range(len(boxes))]) if len(boxes) else np.zeros((0, 0), np.float32)


def check_exact(c: NmsCase) -> dict:
    """The conditions of the module's docstring on the case's own data; returns the figures (candidates and largest merge group per image)."""
    out = {"candidates": [], "largest_group": []}
    p = c.pred.astype(np.float64)
    x1, y1, x2, y2 = p[..., 0] - p[..., 2] / 2, p[..., 1] - p[..., 3] / 2, p[..., 0] + p[..., 2] / 2, p[..., 1] + p[..., 3] / 2
    for t in (x1, y1, x2, y2):
        assert np.array_equal(t, np.round(t)) and (t >= 0).all() and (t < 512).all()            # integer corners below 512
    assert np.array_equal(p[..., 4:] * 8, np.round(p[..., 4:] * 8))                              # scores in eighths: exact products
    assert (c.pred.shape[2] - 5) * 4096 + 512 < 2 ** 24                                          # 4096 * class + coordinate below 2^24
    _, cands = nms_np(c.pred, return_candidates=True, **c.kwargs())
    for cand in cands:
        if cand is None:
            out["candidates"].append(0); out["largest_group"].append(0)
            continue
        boxes, scores = cand
        assert np.array_equal(boxes, np.round(boxes)) and (boxes < 2 ** 24).all()
        assert np.array_equal(scores.astype(np.float64) * 64, np.round(scores.astype(np.float64) * 64))
        assert (scores > 6 / 64).all()
        iou = _pairwise_iou(boxes)
        assert (np.abs(iou - np.float32(IOU)) > 1e-6).all()                                      # the threshold lies strictly between attainable values
        keep = nms_trace_np(boxes, scores, IOU, c.max_det)[0]
        groups = (iou[keep] > np.float32(IOU)).sum(1)
        out["candidates"].append(len(scores)); out["largest_group"].append(int(groups.max()))
        if c.merge:
            assert groups.max() <= 64, groups.max()                                              # the weighted sums are exact in any order
    return out


def _finish(c: NmsCase) -> NmsCase:
    c.want = nms_np(c.pred, **c.kwargs())
    return c


def _cluster(rng, x0, y0, n, size, small, large, n_large):
    """n integer boxes around (x0, y0): the first is the cluster's head, `n_large` members are displaced by up to `large` pixels (they escape the
    head), the others by up to `small` (the head suppresses them)."""
    d = rng.integers(-small, small + 1, (n, 2))
    if n_large:
        d[1:1 + n_large] = rng.integers(-large, large + 1, (n_large, 2))
    d[0] = 0
    wh = size + rng.integers(-2, 3, (n, 2))
    return np.concatenate([np.stack([x0 + d[:, 0], y0 + d[:, 1]], 1), np.stack([x0 + d[:, 0] + wh[:, 0], y0 + d[:, 1] + wh[:, 1]], 1)], 1)


def _chunk_rows(seed=1):
    """36 clusters of a head (score 56/64 or 1) and 16 members (8/64 .. 48/64) on a 64-pixel grid, then 16 isolated boxes of the lowest score:
    about 630 candidates in three chunks; the heads are kept in chunk 0 and suppress members ranked in chunks 1 and 2."""
    rng = np.random.default_rng(seed)
    boxes, obj, cls = [], [], []
    for k in range(36):
        b = _cluster(rng, 14 + 64 * (k % 6), 14 + 64 * (k // 6), 17, 36, 3, 13, 5)
        boxes.append(b)
        obj += [8] + list(rng.integers(4, 9, 16))
        cls += [int(rng.integers(7, 9))] + list(rng.integers(2, 7, 16))
    for k in range(16):                                                    # isolated, last in row order: they rank last among the 8/64 ties
        x0, y0 = 398 + 56 * (k % 2), 4 + 62 * (k // 2)
        boxes.append(np.array([[x0, y0, x0 + 40, y0 + 44]]))
        obj.append(4); cls.append(2)
    return rows(np.concatenate(boxes), obj, np.asarray(cls)[:, None])


def _trace(c: NmsCase, image=0, limit=None):
    _, cands = nms_np(c.pred, return_candidates=True, **c.kwargs())
    boxes, scores = cands[image]
    return nms_trace_np(boxes, scores, IOU, limit) + (len(scores),)


def case_chunks(merge=False) -> NmsCase:
    c = NmsCase("chunks_merge" if merge else "chunks", _chunk_rows()[None], merge=merge, max_det=1024)
    keep, order, suppressed, n = _trace(c)
    rank_of = {int(i): r for r, i in enumerate(order)}
    kept_ranks = sorted(rank_of[int(i)] for i in keep)
    far = [(s, k) for s, k in suppressed if s - k >= CHUNK]
    c.facts = dict(n=n, kept=len(keep), kept_per_chunk=[sum(1 for r in kept_ranks if r // CHUNK == q) for q in range(3)],
                   suppressed_across=len([1 for s, k in suppressed if s // CHUNK > k // CHUNK]), gap_256=len(far),
                   from_chunk0_into=[len([1 for s, k in suppressed if k < CHUNK and s // CHUNK == q]) for q in (1, 2)])
    assert 2 * CHUNK < n <= 3 * CHUNK, n                                    # three chunks
    assert c.facts["gap_256"] >= 1 and min(c.facts["from_chunk0_into"]) >= 1, c.facts    # boxes kept in chunk 0 suppress candidates of chunks 1 and 2
    assert min(c.facts["kept_per_chunk"]) >= 1, c.facts                     # and every chunk keeps some of its own
    return _finish(c)


def case_max_det(which: str) -> NmsCase:
    """The chunk rows cut by max_det: "mid0" - 7, in the middle of chunk 0; "end0" - exactly the number kept when chunk 0 ends; "mid1" - three
    more than that, in the middle of chunk 1."""
    full = case_chunks()
    k0, k1 = full.facts["kept_per_chunk"][:2]
    assert k0 > 7 and k1 > 3, full.facts
    max_det = {"mid0": 7, "end0": k0, "mid1": k0 + 3}[which]
    c = NmsCase(f"max_det_{which}", full.pred, max_det=max_det)
    keep, order, _, n = _trace(c, limit=max_det)
    rank_of = {int(i): r for r, i in enumerate(order)}
    last = rank_of[int(keep[-1])]
    c.facts = dict(max_det=max_det, kept_unlimited=full.facts["kept"], last_kept_rank=last)
    assert len(keep) == max_det < full.facts["kept"]
    assert last // CHUNK == (1 if which == "mid1" else 0)
    if which != "end0":
        assert last % CHUNK != CHUNK - 1                                    # the scan stops inside a chunk
    _finish(c)
    assert len(c.want[0]) == max_det and np.array_equal(c.want[0], full.want[0][:max_det])
    return c


def case_agnostic(agnostic: bool) -> NmsCase:
    """24 pairs of overlapping boxes: 16 of different classes (kept per class, suppressed class-agnostically), 8 of the same class."""
    rng = np.random.default_rng(2)
    boxes, obj, cls = [], [], []
    for k in range(24):
        x0, y0 = 10 + 80 * (k % 6), 10 + 80 * (k // 6)
        d = rng.integers(-3, 4, 2)
        boxes += [[x0, y0, x0 + 50, y0 + 44], [x0 + d[0] + 4, y0 + d[1] + 4, x0 + d[0] + 52, y0 + d[1] + 50]]
        ca = int(rng.integers(0, 3))
        cb = ca if k % 3 == 2 else (ca + 1 + int(rng.integers(0, 2))) % 3
        for cc, s in ((ca, int(rng.integers(5, 9))), (cb, int(rng.integers(2, 5)))):
            v = [0, 0, 0]
            v[cc] = s
            cls.append(v); obj.append(8)
    c = _finish(NmsCase("agnostic" if agnostic else "per_class", rows(boxes, obj, cls)[None], agnostic=agnostic))
    c.facts = dict(kept=len(c.want[0]))
    assert len(c.want[0]) == (24 if agnostic else 40), c.facts              # 16 pairs of different classes: both kept only per class
    return c


def case_best_class() -> NmsCase:
    """multi_label = 0 on four classes: rows with two classes above the threshold (one candidate, the larger), rows with two classes tied for
    the maximum (the first wins, as np.argmax), rows whose objectness passes but whose best product does not (no candidate)."""
    rng = np.random.default_rng(3)
    boxes, obj, cls, kind = [], [], [], []
    for k in range(48):
        x0, y0 = 6 + 60 * (k % 8) + int(rng.integers(0, 5)), 6 + 70 * (k // 8) + int(rng.integers(0, 5))
        boxes.append([x0, y0, x0 + 40 + int(rng.integers(0, 9)), y0 + 50])
        t = k % 3
        v = [0, 0, 0, 0]
        if t == 0:                                                          # two above the threshold, the larger second
            a, b = rng.choice(4, 2, replace=False)
            v[a], v[b] = 3, 6
            obj.append(8)
        elif t == 1:                                                        # tied maximum at classes lo < hi, a smaller third
            lo, hi, other = np.sort(rng.choice(4, 3, replace=False))[[0, 2, 1]]
            v[lo], v[hi], v[other] = 5, 5, 2
            obj.append(int(rng.integers(4, 9)))
        else:                                                               # objectness 2/8 > 0.1, best product 6/64 < 0.1
            v[int(rng.integers(0, 4))] = 3
            obj.append(2)
        cls.append(v); kind.append(t)
    # overlapping neighbours of the same best class: one of each such pair is suppressed
    for k in range(0, 48, 6):
        boxes.append([boxes[k][0] + 2, boxes[k][1] + 2, boxes[k][2] + 2, boxes[k][3] + 2])
        v = list(cls[k]); obj.append(8); cls.append([min(e, 5) for e in v]); kind.append(3)
    c = _finish(NmsCase("best_class", rows(boxes, obj, cls)[None], multi_label=False))
    multi = nms_np(c.pred, return_candidates=True, **dict(c.kwargs(), multi_label=True))[1][0]
    _, order, suppressed, n = _trace(c)
    kind = np.asarray(kind)
    c.facts = dict(n=n, n_multi_label=len(multi[1]), rows=len(kind), dropped=int((kind == 2).sum()), suppressed=len(suppressed))
    assert n == int((kind != 2).sum()) and c.facts["n_multi_label"] > n and suppressed     # one candidate per row; rows of kind 2 give none
    want = c.want[0]
    cls8 = np.asarray(cls)
    for r in want:                                                          # every kept row names the FIRST of its row's largest classes
        src = np.nonzero((np.abs(rows(boxes, obj, cls)[:, :4] - _xywh(r[:4])) == 0).all(1))[0]
        assert any(int(r[5]) == int(np.argmax(cls8[s])) for s in src), r
    tied = [r for r in want if any(kind[s] == 1 for s in np.nonzero((np.abs(rows(boxes, obj, cls)[:, :4] - _xywh(r[:4])) == 0).all(1))[0])]
    assert len(tied) >= 8
    return c


def _xywh(b):
    return np.array([(b[0] + b[2]) / 2, (b[1] + b[3]) / 2, b[2] - b[0], b[3] - b[1]], dtype=np.float32)


def case_ties() -> NmsCase:
    """Overlapping boxes of exactly equal score, one index, 40 and 300 rows apart (the same and another 256-row block of the rank kernel): the
    lower candidate index survives."""
    rng = np.random.default_rng(4)
    n_pairs = 330
    first, second, score = [], [], []
    for k in range(n_pairs):
        x0, y0 = 2 + 22 * (k % 22), 2 + 30 * (k // 22)
        first.append([x0, y0, x0 + 18, y0 + 26])
        second.append([x0 + 1, y0 + 1, x0 + 20, y0 + 27])                   # larger: were it kept instead, the output would differ
        score.append(int(rng.integers(1, 5)) * 2)                           # obj 8/8 x cls in {2, 4, 6, 8} / 8: only four distinct scores
    boxes, cls, partner = [None] * (2 * n_pairs), [0] * (2 * n_pairs), {}
    # partner of pair k sits 1, 40 or 300 rows after its first box: lay the pairs out in three sections
    slots = list(range(2 * n_pairs))
    pos = 0
    for k in range(n_pairs):
        while boxes[pos] is not None:
            pos += 1
        gap = (1, 40, 300)[k % 3]
        q = pos + gap
        while q < 2 * n_pairs and boxes[q] is not None:
            q += 1
        if q >= 2 * n_pairs:
            q = next(i for i in slots if i > pos and boxes[i] is None)
        boxes[pos], boxes[q], cls[pos], cls[q] = first[k], second[k], score[k], score[k]
        partner[pos] = q
    c = _finish(NmsCase("ties", rows(boxes, [8] * len(boxes), np.asarray(cls)[:, None])[None], max_det=1024))
    keep, order, suppressed, n = _trace(c)
    gaps = [q - p for p, q in partner.items()]
    c.facts = dict(n=n, kept=len(keep), gaps_at_least_256=sum(g >= 256 for g in gaps), distinct_scores=len(set(cls)))
    assert n == 2 * n_pairs and sorted(int(i) for i in keep) == sorted(partner) and c.facts["gaps_at_least_256"] >= 20, c.facts
    assert len(suppressed) == n_pairs and c.facts["distinct_scores"] == 4
    return c


def case_merge_groups() -> NmsCase:
    """merge = 1: groups of 1 (dropped by the redundancy filter), 2, 3, 10, 30 and 64 members (merged)."""
    rng = np.random.default_rng(5)
    boxes, obj, cls, sizes = [], [], [], []
    for k, n in enumerate((1, 2, 3, 10, 30, 1, 2, 1, 5, 1, 17, 1)):
        x0, y0 = 8 + 70 * (k % 4), 8 + 70 * (k // 4)
        b = _cluster(rng, x0, y0, n, 44, 2, 2, 0)
        boxes.append(b); sizes.append(n)
        obj += [8] * n
        cls += [8] + list(rng.integers(1, 8, n - 1))
    big = np.array([[300 + dx, 300 + dy, 400 + dx, 400 + dy] for dy in range(8) for dx in range(8)])      # 64 boxes, all within 4 pixels of (3, 3)
    boxes.append(big)
    obj += [8] * 64
    cls += [8 if (i % 8, i // 8) == (3, 3) else int(rng.integers(1, 8)) for i in range(64)]
    c = _finish(NmsCase("merge_groups", rows(np.concatenate(boxes), obj, np.asarray(cls)[:, None])[None], merge=True))
    _, cands = nms_np(c.pred, return_candidates=True, **c.kwargs())
    b, s = cands[0]
    keep = nms_trace_np(b, s, IOU)[0]
    groups = sorted(int(g) for g in (_pairwise_iou(b)[keep] > np.float32(IOU)).sum(1))
    c.facts = dict(n=len(s), groups=groups, out=len(c.want[0]))
    assert groups == sorted(sizes + [64]), groups                           # one kept box per cluster, its group the whole cluster
    assert len(c.want[0]) == sum(g > 1 for g in groups) and groups.count(1) == 5
    plain = nms_np(c.pred, **dict(c.kwargs(), merge=False))[0]
    assert len(plain) == len(groups)
    assert sum(not any(np.array_equal(w[:4], q[:4]) for q in plain) for w in c.want[0]) >= 5                # the merge moves boxes
    return c


def case_single_merge() -> NmsCase:
    """n == 1 with merge = 1: neither merge nor the redundancy filter applies, the box comes out as it is."""
    c = _finish(NmsCase("single_merge", rows([[10, 20, 110, 220]], [8], [[5]])[None], merge=True))
    assert len(c.want[0]) == 1 and np.array_equal(c.want[0][0], np.array([10, 20, 110, 220, 5 / 8, 0], dtype=np.float32))
    return c


def case_batch3() -> NmsCase:
    """Three images in one call: no candidate (the objectness passes, no product does), one candidate, about 300 in two chunks; merge = 1."""
    rng = np.random.default_rng(6)
    none = rows([[5 + 9 * k, 7, 40 + 9 * k, 90] for k in range(12)], [2] * 12, [[3]] * 12)
    one = np.concatenate([none[:5], rows([[33, 44, 133, 244]], [8], [[7]]), none[5:]])
    boxes, obj, cls = [], [], []
    for k in range(30):
        n = int(rng.integers(8, 13))
        boxes.append(_cluster(rng, 16 + 80 * (k % 6), 16 + 80 * (k // 6), n, 40, 3, 14, 2))
        obj += [8] + list(rng.integers(4, 9, n - 1))
        cls += [8] + list(rng.integers(2, 7, n - 1))
    many = rows(np.concatenate(boxes), obj, np.asarray(cls)[:, None])
    c = _finish(NmsCase("batch3", stack([none, one, many]), merge=True))
    ex = check_exact(c)
    c.facts = dict(candidates=ex["candidates"], out=[None if w is None else len(w) for w in c.want])
    assert ex["candidates"][:2] == [0, 1] and CHUNK < ex["candidates"][2] <= 2 * CHUNK, ex
    assert c.want[0] is None and len(c.want[1]) == 1 and len(c.want[2]) > 10
    return c


NMS_CASES = {
    "chunks": case_chunks, "chunks_merge": lambda: case_chunks(True),
    "max_det_mid0": lambda: case_max_det("mid0"), "max_det_end0": lambda: case_max_det("end0"), "max_det_mid1": lambda: case_max_det("mid1"),
    "per_class": lambda: case_agnostic(False), "agnostic": lambda: case_agnostic(True),
    "best_class": case_best_class, "ties": case_ties, "merge_groups": case_merge_groups, "single_merge": case_single_merge, "batch3": case_batch3,
}


# ---- head decode ----------------------------------------------------------------------------------------------------------------------------
HEAD_GRIDS = ((3, 5), (2, 3), (1, 2))
HEAD_STRIDES = (8.0, 16.0, 32.0)
HEAD_LAYOUTS = ((3, 6, 8), (3, 85, 88), (1, 5, 8), (4, 6, 8))             # (anchors, no, a_stride)
HEAD_BATCH = 2
SPECIAL_LOGITS = (30.0, -30.0, 88.0, -88.0, 100.0, -100.0)


def head_anchors(anchors: int) -> np.ndarray:
    """[3][anchors][2]: a distinct integer per level, anchor and axis."""
    l, a, k = np.meshgrid(np.arange(3), np.arange(anchors), np.arange(2), indexing="ij")
    return (10 + 64 * l + 8 * a + 3 * k).astype(np.float32)


def head_inputs(anchors, no, a_stride, kind, seed=0):
    """The three packed head tensors [B, ny, nx, anchors * a_stride] (float32) with NaN in every padding column.  kind "zero": all logits 0;
    "distinct": every logit another value in [-4, 4) (shuffled); "random": uniform in [-6, 6] with SPECIAL_LOGITS planted in every column."""
    rng = np.random.default_rng(seed)
    total = sum(HEAD_BATCH * ny * nx * anchors * no for ny, nx in HEAD_GRIDS)
    pool = rng.permutation(total).astype(np.float64) * (8.0 / total) - 4.0
    heads, used = [], 0
    for ny, nx in HEAD_GRIDS:
        t = np.full((HEAD_BATCH, ny, nx, anchors, a_stride), np.nan, dtype=np.float32)
        shape = (HEAD_BATCH, ny, nx, anchors, no)
        if kind == "zero":
            v = np.zeros(shape)
        elif kind == "distinct":
            v = pool[used:used + int(np.prod(shape))].reshape(shape)
            used += v.size
        else:
            v = rng.uniform(-6, 6, shape)
            flat = v.reshape(-1, no)                                        # (a view: v is contiguous)
            m = min(len(flat), len(SPECIAL_LOGITS))
            for k in range(no):                                             # (a level with fewer rows takes what fits, another part per column)
                flat[rng.choice(len(flat), m, replace=False), k] = np.roll(SPECIAL_LOGITS, k)[:m]
        t[..., :no] = v
        heads.append(t.reshape(HEAD_BATCH, ny, nx, anchors * a_stride))
    return heads


def head_logits_in_output_order(heads, anchors, no, a_stride) -> np.ndarray:
    """The logits of head_inputs() where the decode puts their results: [B, N, no], rows ordered (level, anchor, y, x)."""
    z = []
    for h in heads:
        B, ny, nx, _ = h.shape
        z.append(h.reshape(B, ny, nx, anchors, a_stride)[..., :no].transpose(0, 3, 1, 2, 4).reshape(B, -1, no))
    return np.concatenate(z, 1)
