"""The detector's head decode and NMS kernels (csrc/detect.hip) called directly, at the edges the end-to-end goldens do not reach.

Head decode: the index arithmetic (level, anchor, y, x, row order, a padded anchor stride) on all-zero logits, where every output is exact, and
on distinct logits; the accuracy of the sigmoid / square chain against float64 at a bar taken from the same formula in fp32 on the CPU; the
refusals of the entry point.  NMS: the cases of tests/detector_edges.py - every option, the 256-candidate chunk edges, score ties, merge groups,
several images per call - bit for bit against detector_ref.nms_np through sp_yolo_nms and sp_yolo_nms_device."""
import ctypes

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib
from tests import detector_edges as de
from tests.detector_ref import head_decode_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = _lib.ptr
SENTINEL = -12345.5          # prefill of every output: a value no case produces


def _stream():
    return _lib.current_stream(torch.device(DEV))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- head decode ----------------------------------------------------------------------------------------------------------------------------
def _decode_call(heads, anchors, no, a_stride, grids=de.HEAD_GRIDS, batch=de.HEAD_BATCH):
    """sp_yolo_head_decode on numpy heads: (return code, output [B, N, no] prefilled with SENTINEL)."""
    dev = [torch.from_numpy(np.ascontiguousarray(h)).to(DEV) for h in heads]
    flat = [float(v) for v in de.head_anchors(min(anchors, 4)).reshape(-1)] + [0.0] * 64      # (room for what a refused call could read)
    n = sum(max(anchors, 1) * max(ny, 1) * max(nx, 1) for ny, nx in grids)
    out = torch.full((batch, n, max(no, 1)), SENTINEL, dtype=torch.float32, device=DEV)
    grid = [v for g in grids for v in g]
    rc = _lib.lib().sp_yolo_head_decode(P(dev[0]), P(dev[1]), P(dev[2]), batch, (ctypes.c_int32 * 6)(*grid), anchors, no, a_stride,
                                        (ctypes.c_float * 3)(*de.HEAD_STRIDES), (ctypes.c_float * len(flat))(*flat), P(out), _stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _ref64(heads, anchors, no, a_stride, dtype=torch.float64):
    return head_decode_torch([torch.from_numpy(h) for h in heads], anchors, no, a_stride, de.HEAD_STRIDES, de.head_anchors(anchors), dtype=dtype).numpy()


@pytest.mark.parametrize("anchors,no,a_stride", de.HEAD_LAYOUTS)
def test_head_decode_index_arithmetic_is_exact(anchors, no, a_stride):
    """All logits 0: expf(-0) = 1, s = 0.5 exactly, so xy = (grid + 0.5) * stride and wh = anchor carry no rounding - array_equal on all
    B x N x no elements pins level, anchor, y, x and the row order independently of expf.  The padding columns hold NaN and must not be read.
    Then distinct logits: the objectness and class columns (plain sigmoids) follow the expected permutation of the inputs."""
    heads = de.head_inputs(anchors, no, a_stride, "zero")
    rc, got = _decode_call(heads, anchors, no, a_stride)
    assert rc == 0
    want = _ref64(heads, anchors, no, a_stride)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want.astype(np.float32)))
    heads = de.head_inputs(anchors, no, a_stride, "distinct")
    rc, got = _decode_call(heads, anchors, no, a_stride)
    assert rc == 0 and not np.isnan(got).any()
    want = _ref64(heads, anchors, no, a_stride)
    # sigmoids of distinct inputs lie more than 1e-5 apart (tests/test_detector_edges_host.py): within 1e-6 means "of that input element"
    assert np.abs(got[..., 4:] - want[..., 4:]).max() <= 1e-6
    assert np.array_equal(np.argsort(got[..., 4:].reshape(-1), kind="stable"), np.argsort(want[..., 4:].reshape(-1), kind="stable"))
    # and the box columns read their own element too: s from the column's own logit, at fp32 accuracy
    for lo, hi in ((0, 2), (2, 4)):
        assert np.abs(got[..., lo:hi] - want[..., lo:hi]).max() <= 1e-5 * np.abs(want[..., lo:hi]).max()


@pytest.mark.parametrize("anchors,no,a_stride", de.HEAD_LAYOUTS)
def test_head_decode_accuracy_against_float64(anchors, no, a_stride, measured):
    """Logits uniform in [-6, 6] plus +-30, +-88, +-100 in every column.  Per column group (xy, wh, obj, cls) the largest error against the
    float64 decode, relative to the group's maximum.  The bar per group: 4 x the error of the same formula in fp32 torch on the CPU against
    float64 on the same inputs (the device's expf is allowed a few ulp where the CPU's is nearly correctly rounded), at least 4 fp32 ulp of
    the group's maximum.  At -100, expf(100) = inf and 1 / (1 + inf) = 0: no NaN, the sigmoid and wh exactly 0, xy exactly (grid - 0.5) * stride."""
    heads = de.head_inputs(anchors, no, a_stride, "random", seed=11)
    rc, got = _decode_call(heads, anchors, no, a_stride)
    assert rc == 0 and not np.isnan(got).any() and np.isfinite(got).all()
    want = _ref64(heads, anchors, no, a_stride)
    cpu32 = _ref64(heads, anchors, no, a_stride, dtype=torch.float32).astype(np.float64)
    tag = f"A{anchors}_no{no}"
    failed = []
    for name, lo, hi in (("xy", 0, 2), ("wh", 2, 4), ("obj", 4, 5), ("cls", 5, no)):
        if hi <= lo:
            continue
        top = np.abs(want[..., lo:hi]).max()
        err = np.abs(got[..., lo:hi] - want[..., lo:hi]).max() / top
        err_cpu = np.abs(cpu32[..., lo:hi] - want[..., lo:hi]).max() / top
        bar = max(4 * err_cpu, 4 * float(np.spacing(np.float32(top))) / top)
        measured(f"{tag}_{name}_cpu_fp32_rel_err", err_cpu)
        measured(f"{tag}_{name}_rel_err", err, bar)
        if err > bar:
            failed.append((name, err, bar))
    assert not failed, failed
    logit = de.head_logits_in_output_order(heads, anchors, no, a_stride)
    low, high = logit == -100.0, logit == 100.0
    assert low[..., :2].any() and low[..., 2:4].any() and low[..., 4:].any() and high[..., 4:].any()
    assert (got[..., 2:][low[..., 2:]] == 0).all()                          # wh, objectness, classes: exactly 0
    assert np.array_equal(got[..., :2][low[..., :2]], want[..., :2][low[..., :2]].astype(np.float32))
    assert (got[..., 4:][high[..., 4:]] == 1).all()


def test_head_decode_refusals_leave_the_output_untouched():
    anchors, no, a_stride = 3, 6, 8
    heads = de.head_inputs(anchors, no, a_stride, "zero")
    lib = _lib.lib()
    bad = [
        (dict(anchors=5), "anchors 5"),
        (dict(no=4), "no 4"),
        (dict(no=10), "a_stride 8"),                                        # a_stride < no
        (dict(a_stride=10, no=6), "a_stride 10"),                           # a_stride % 4 != 0
        (dict(grids=((3, 5), (0, 3), (1, 2))), "level 1 grid 0x3"),
        (dict(grids=((3, 5), (2, 3), (1, 0))), "level 2 grid 1x0"),
    ]
    for change, message in bad:
        args = dict(anchors=anchors, no=no, a_stride=a_stride)
        args.update(change)
        rc, out = _decode_call(heads, **args)
        text = lib.sp_last_error().decode()
        assert rc != 0 and text.startswith("sp_yolo_head_decode:") and message in text, (change, rc, text)
        assert (out == np.float32(SENTINEL)).all(), change
    rc, out = _decode_call(heads, anchors, no, a_stride)                    # the same inputs, unchanged, are accepted
    assert rc == 0 and not (out == np.float32(SENTINEL)).any()


# ---- NMS ------------------------------------------------------------------------------------------------------------------------------------
def _workspace(batch):
    n = ctypes.c_int64(0)
    _lib.check(_lib.lib().sp_yolo_nms_workspace(batch, ctypes.byref(n)), "sp_yolo_nms_workspace")
    return torch.empty(n.value, dtype=torch.uint8, device=DEV)


def _nms_both(c: de.NmsCase):
    """The case through sp_yolo_nms (host counts) and sp_yolo_nms_device (device counts): (out, counts, candidates), (out, counts, status)."""
    lib = _lib.lib()
    pred = torch.from_numpy(c.pred).to(DEV)
    B, N, no = pred.shape
    args = (B, N, no, float(de.CONF), float(de.IOU), int(c.merge), int(c.multi_label), int(c.agnostic), int(c.max_det))
    ws = _workspace(B)
    out_h = torch.full((B, c.max_det, 6), SENTINEL, dtype=torch.float32, device=DEV)
    counts, cands = (ctypes.c_int32 * B)(*([-1] * B)), (ctypes.c_int32 * B)(*([-1] * B))
    _lib.check(lib.sp_yolo_nms(P(pred), *args, P(ws), ws.numel(), P(out_h), counts, cands, _stream()), "sp_yolo_nms")
    torch.cuda.synchronize()
    ws2 = _workspace(B)                                                     # (a workspace of its own: nothing carries over)
    out_d = torch.full((B, c.max_det, 6), SENTINEL, dtype=torch.float32, device=DEV)
    counts_d = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    status = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _lib.check(lib.sp_yolo_nms_device(P(pred), *args, P(ws2), ws2.numel(), P(out_d), P(counts_d), P(status), _stream()), "sp_yolo_nms_device")
    torch.cuda.synchronize()
    return (out_h.cpu().numpy(), list(counts), list(cands)), (out_d.cpu().numpy(), counts_d.cpu().tolist(), status.cpu().tolist())


@pytest.mark.parametrize("name", sorted(de.NMS_CASES))
def test_nms_edges_bit_for_bit_against_the_restatement(name):
    """Rows, order, scores, classes and boxes equal nms_np's bit for bit through both entry points (the case's inputs make every IoU one
    correctly rounded division of exact operands and every merged box one division of exact sums: tests/detector_edges.py; no merged case
    needed a tolerance).  Of the rows from the count on, only what the header promises: sp_yolo_nms_device does not write them."""
    c = de.NMS_CASES[name]()
    de.check_exact(c)
    (out_h, counts_h, cands_h), (out_d, counts_d, status) = _nms_both(c)
    assert status == [0] * len(c.want)
    for b, want in enumerate(c.want):
        n = 0 if want is None else len(want)
        assert (cands_h[b] == 0) == (want is None), (b, cands_h[b])
        assert counts_h[b] == n and counts_d[b] == n, (b, counts_h[b], counts_d[b], n)
        if n:
            for what, got in (("sp_yolo_nms", out_h[b, :n]), ("sp_yolo_nms_device", out_d[b, :n])):
                diff = (_bits(got) != _bits(want)).any(1)
                assert not diff.any(), f"{name} image {b} {what}: {int(diff.sum())} of {n} rows differ, first row {int(np.nonzero(diff)[0][0])}: " \
                                       f"got {got[np.nonzero(diff)[0][0]]}, want {want[np.nonzero(diff)[0][0]]}"
        assert np.array_equal(_bits(out_h[b, :n]), _bits(out_d[b, :n]))
        assert (out_d[b, n:] == np.float32(SENTINEL)).all()                 # "rows from counts[b] on are not written"
    print(name, c.facts, counts_h)


def test_nms_agnostic_and_per_class_runs_differ_as_the_restatement_says():
    a, b = de.NMS_CASES["per_class"](), de.NMS_CASES["agnostic"]()
    (_, counts_a, _), _ = _nms_both(a)
    (_, counts_b, _), _ = _nms_both(b)
    assert counts_a == [len(a.want[0])] and counts_b == [len(b.want[0])] and counts_a[0] > counts_b[0]
