"""The detector edge cases (tests/detector_edges.py) without a GPU: every NMS case builds, meets the conditions that make its comparison exact and
reaches the edge it is named after (asserted on detector_ref.nms_np's result alone), so that a changed generator cannot silently empty a case;
the float64 head decode restates the interpreter's; the head inputs hold what the GPU module relies on."""
import numpy as np
import pytest
import torch

from tests import detector_edges as de
from tests.detector_ref import head_decode_torch, nms_np


@pytest.mark.parametrize("name", sorted(de.NMS_CASES))
def test_nms_case_is_exact_and_reaches_its_edge(name):
    c = de.NMS_CASES[name]()                       # (the builder asserts the edge)
    ex = de.check_exact(c)
    print(name, c.pred.shape, c.facts, ex)
    assert c.pred.dtype == np.float32 and c.pred.ndim == 3 and len(c.want) == c.pred.shape[0]
    for w in c.want:
        assert w is None or (w.dtype == np.float32 and w.shape[1] == 6 and len(w) <= c.max_det)
    again = de.NMS_CASES[name]()                   # deterministic: the GPU module builds the same case
    assert np.array_equal(again.pred, c.pred)


def test_the_two_agnostic_runs_share_their_input_and_differ():
    a, b = de.NMS_CASES["per_class"](), de.NMS_CASES["agnostic"]()
    assert np.array_equal(a.pred, b.pred) and len(a.want[0]) > len(b.want[0])
    kept = {tuple(r) for r in a.want[0]}
    assert all(tuple(r) in kept for r in b.want[0])                        # class-agnostic keeps a subset: boxes of other classes are suppressed


def test_the_max_det_cases_are_prefixes_of_the_full_scan():
    full = de.NMS_CASES["chunks"]().want[0]
    for which in ("mid0", "end0", "mid1"):
        c = de.NMS_CASES[f"max_det_{which}"]()
        assert np.array_equal(c.want[0], full[:c.max_det]) and len(c.want[0]) == c.max_det < len(full)


def test_equal_scores_keep_the_lower_index():
    c = de.NMS_CASES["ties"]()
    p = c.pred[0]
    kept = {tuple(r[:4]) for r in c.want[0]}
    x1, y1 = p[:, 0] - p[:, 2] / 2, p[:, 1] - p[:, 3] / 2
    firsts = (p[:, 2] == 18)                                               # the first box of a pair is 18 wide, its partner 19
    assert firsts.sum() == len(p) // 2 == len(kept)
    for i in np.nonzero(firsts)[0]:
        assert (x1[i], y1[i], x1[i] + 18, y1[i] + 26) in kept
        j = np.nonzero((x1 == x1[i] + 1) & (y1 == y1[i] + 1))[0]
        assert len(j) == 1 and j[0] > i and p[j[0], 5] == p[i, 5]          # the partner: a higher row, the same score


@pytest.mark.parametrize("anchors,no,a_stride", de.HEAD_LAYOUTS)
def test_head_inputs_and_the_float64_decode(anchors, no, a_stride):
    ag = de.head_anchors(anchors)
    assert len(np.unique(ag)) == ag.size
    # all logits 0: s = 0.5, xy = (grid + 0.5) * stride, wh = anchor, every value an fp32 number
    heads = [torch.from_numpy(h) for h in de.head_inputs(anchors, no, a_stride, "zero")]
    for h in heads:
        t = h.view(h.shape[:3] + (anchors, a_stride))
        assert bool(torch.isnan(t[..., no:]).all()) and not bool(torch.isnan(t[..., :no]).any())
    z = head_decode_torch(heads, anchors, no, a_stride, de.HEAD_STRIDES, ag)
    n = sum(anchors * ny * nx for ny, nx in de.HEAD_GRIDS)
    assert z.shape == (de.HEAD_BATCH, n, no) and not bool(torch.isnan(z).any())
    assert torch.equal(z.float().double(), z) and bool((z[..., 4:] == 0.5).all())
    row = 0
    for l, (ny, nx) in enumerate(de.HEAD_GRIDS):
        for a in range(anchors):
            for y in range(ny):
                for x in range(nx):
                    want = [(x + 0.5) * de.HEAD_STRIDES[l], (y + 0.5) * de.HEAD_STRIDES[l], float(ag[l, a, 0]), float(ag[l, a, 1])]
                    assert z[:, row, :4].tolist() == [want] * de.HEAD_BATCH, (l, a, y, x)
                    row += 1
    # distinct logits: distinct in fp32, and sigmoids far enough apart that a tolerance of 1e-6 names the input element
    heads = de.head_inputs(anchors, no, a_stride, "distinct")
    vals = np.concatenate([h.reshape(-1)[~np.isnan(h.reshape(-1))] for h in heads])
    assert len(np.unique(vals)) == vals.size == de.HEAD_BATCH * n * no
    s = np.sort(1 / (1 + np.exp(-vals.astype(np.float64))))
    assert np.diff(s).min() > 1e-5
    # random logits: the special values are present in every column of the first level
    heads = de.head_inputs(anchors, no, a_stride, "random", seed=7)
    first = heads[0].reshape(-1, a_stride)[:, :no]
    for k in range(no):
        assert set(de.SPECIAL_LOGITS) <= set(first[:, k].tolist())
    allv = np.concatenate([h.reshape(-1, a_stride)[:, :no].reshape(-1) for h in heads])
    assert np.abs(allv[~np.isin(allv, de.SPECIAL_LOGITS)]).max() <= 6.0


def test_the_float64_decode_equals_the_program_interpreter_formula():
    """head_decode_torch in float32 is the formula of detector_ref.run_yolo_program_cpu's yolo_decode branch (itself pinned to the reference
    network): the same values on the same inputs."""
    anchors, no, a_stride = 3, 6, 8
    heads = [torch.from_numpy(np.nan_to_num(h, nan=0.0)) for h in de.head_inputs(anchors, no, a_stride, "random", seed=3)]
    ag = de.head_anchors(anchors)
    got = head_decode_torch(heads, anchors, no, a_stride, de.HEAD_STRIDES, ag, dtype=torch.float32)
    z, B = [], de.HEAD_BATCH
    for l, t in enumerate(heads):
        ny, nx = de.HEAD_GRIDS[l]
        v = t.view(B, ny, nx, anchors, a_stride)[..., :no].permute(0, 3, 1, 2, 4).sigmoid()
        yv, xv = torch.meshgrid(torch.arange(ny), torch.arange(nx), indexing="ij")
        g = torch.stack((xv, yv), 2).view(1, 1, ny, nx, 2).float()
        xy = (v[..., 0:2] * 2. - 0.5 + g) * de.HEAD_STRIDES[l]
        wh = (v[..., 2:4] * 2) ** 2 * torch.tensor(ag)[l].view(1, anchors, 1, 1, 2)
        z.append(torch.cat([xy, wh, v[..., 4:]], -1).reshape(B, -1, no))
    assert torch.equal(got, torch.cat(z, 1))


def test_nms_np_options_are_reached_by_the_cases():
    """Every option of nms_np away from its default occurs in the table."""
    cases = [f() for f in de.NMS_CASES.values()]
    assert any(c.merge for c in cases) and any(not c.multi_label for c in cases) and any(c.agnostic for c in cases)
    assert any(c.max_det < 300 for c in cases) and any(c.pred.shape[0] > 1 for c in cases)
    assert nms_np(cases[0].pred, **cases[0].kwargs())[0].shape == cases[0].want[0].shape
