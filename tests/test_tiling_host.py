"""The host side of tiled detection (simple_pose_amd/tiling.py): the plan, the refusals, the limits, the table's ABI, and the merge
reference against the detector's greedy NMS.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from simple_pose_amd import _lib
from simple_pose_amd.detector.yolov5_detector import ScalePadding
from simple_pose_amd.tiling import MAX_PASSES_PER_CALL, MAX_TILES, Tiling, axis_positions, pack_tile_refs, plan_pass_groups
from tests import tiled_ref
from tests.detector_ref import greedy_nms_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_axis_rule_exhaustive():
    """Every pixel covered, every tile inside, one size, strictly increasing positions, neighbours overlap by at least `lap`."""
    for t0 in (1, 2, 5, 16, 17):
        for overlap in (0.0, 0.2, 0.5, 0.9):
            for n in range(1, 80):
                t, pos = axis_positions(n, t0, overlap)
                assert (t, pos) == tiled_ref.axis_np(n, t0, overlap)
                lap = int(t * overlap)
                assert t == min(t0, n) and pos[0] == 0 and pos[-1] == n - t
                assert all(b > a for a, b in zip(pos, pos[1:]))
                assert all(0 <= p and p + t <= n for p in pos)
                covered = np.zeros(n, bool)
                for p in pos:
                    covered[p:p + t] = True
                assert covered.all()
                assert all(a + t - b >= lap for a, b in zip(pos, pos[1:]))


def test_plan_is_the_row_major_product_and_matches_the_reference():
    for (H, W, tile, ov) in ((37, 53, (16, 17), 0.2), (79, 5, (5, 16), 0.5), (16, 16, (16, 16), 0.0), (10, 40, (64, 64), 0.9)):
        for full in (True, False):
            t = Tiling(tile=tile, overlap=ov, full_frame=full)
            got = t.plan(H, W)
            assert got == tiled_ref.plan_np(H, W, tile, ov, full)
            th, ys = axis_positions(H, tile[1], ov)
            tw, xs = axis_positions(W, tile[0], ov)
            tiles = [(y, x, th, tw) for y in ys for x in xs]
            assert got[-len(tiles):] == tiles
            assert len(got) == len(tiles) + (1 if full and tiles != [(0, 0, H, W)] else 0)


def test_worked_examples():
    p = Tiling().plan(2160, 3840)
    assert len(p) == 1 + 8 * 4 and p[0] == (0, 0, 2160, 3840)
    assert sorted({y for y, _, _, _ in p[1:]}) == [0, 512, 1024, 1520]
    assert sorted({x for _, x, _, _ in p[1:]}) == [0, 512, 1024, 1536, 2048, 2560, 3072, 3200]
    assert all((h, w) == (640, 640) for _, _, h, w in p[1:])
    q = Tiling(tile=(320, 256), overlap=0.25, full_frame=False).plan(432, 640)
    assert q == [(0, 0, 256, 320), (0, 240, 256, 320), (0, 320, 256, 320), (176, 0, 256, 320), (176, 240, 256, 320), (176, 320, 256, 320)]
    # a single tile that equals the frame: one pass, with or without full_frame
    assert Tiling(tile=(640, 640)).plan(480, 640) == [(0, 0, 480, 640)]
    assert Tiling(tile=(64, 64), full_frame=True).plan(64, 65)[0] == (0, 0, 64, 65)


@pytest.mark.parametrize("kw, exc", [
    (dict(tile=(0, 640)), ValueError), (dict(tile=(640, -1)), ValueError), (dict(tile=640), TypeError), (dict(tile=(640.0, 640)), TypeError),
    (dict(tile=(1, 2, 3)), TypeError), (dict(overlap=-0.1), ValueError), (dict(overlap=1.0), ValueError), (dict(overlap="a"), TypeError),
    (dict(metric="giou"), ValueError), (dict(metric=1), TypeError), (dict(thresh=0.0), ValueError), (dict(thresh=1.5), ValueError),
    (dict(thresh=None), TypeError), (dict(thresh=float("nan")), ValueError), (dict(overlap=float("nan")), ValueError)])
def test_refusals(kw, exc):
    with pytest.raises(exc):
        Tiling(**kw)


def test_accepts_the_edges_and_key_holds_every_field():
    t = Tiling(tile=(1, 1), overlap=0.0, thresh=1.0, metric="iou", agnostic=True, full_frame=False)
    assert t.key() == ((1, 1), 0.0, False, "iou", 1.0, True)
    assert Tiling().key() == ((640, 640), 0.2, True, "ios", 0.5, False)
    assert Tiling().key() != Tiling(thresh=0.6).key() and Tiling().key() != Tiling(metric="iou").key()
    assert (Tiling(metric="iou").metric_code, Tiling(metric="ios").metric_code) == (_lib.SP_TILE_IOU, _lib.SP_TILE_IOS)


def test_limits():
    t = Tiling(tile=(8, 8), overlap=0.0)
    assert len(t.plan(64, 64)) == 65                                             # 64 tiles: the most
    with pytest.raises(ValueError, match="tiles"):
        t.plan(64, 72)                                                           # 8 x 9
    with pytest.raises(ValueError, match="tiles"):
        Tiling(tile=(8, 8), overlap=0.0, full_frame=False).plan(72, 64)
    # 256 passes per call: 3 x 65 = 195 fit, 4 x 65 = 260 do not; 256 x 1 fit, 257 x 1 do not
    assert len(t.plan_call(3, 64, 64)) == 65
    with pytest.raises(ValueError, match="passes"):
        t.plan_call(4, 64, 64)
    one = Tiling(tile=(64, 64))
    assert one.plan_call(256, 64, 64) == [(0, 0, 64, 64)]
    with pytest.raises(ValueError, match="passes"):
        one.plan_call(257, 64, 64)
    assert (MAX_TILES, MAX_PASSES_PER_CALL) == (64, 256) and (MAX_TILES + 1) * 300 <= _lib.SP_YOLO_NMS_MAX_CANDIDATES


def test_tile_ref_mirror_matches_the_header():
    with open(os.path.join(ROOT, "include", "simple_pose_hip.h")) as fh:
        text = fh.read()
    m = re.search(r"\}\s*sp_tile_ref;\s*/\*\s*(\d+) bytes\s*\*/", text)
    assert m and ctypes.sizeof(_lib.TileRef) == int(m.group(1)) == 56
    body = re.search(r"typedef struct sp_tile_ref \{(.*?)\}\s*sp_tile_ref;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [w for w in re.findall(r"[A-Za-z_][A-Za-z_0-9]*", body) if w not in ("const", "unsigned", "char", "int32_t", "float")]
    assert names == [f[0] for f in _lib.TileRef._fields_]
    for macro, val in (("SP_TILE_MAX_TILES", _lib.SP_TILE_MAX_TILES), ("SP_TILE_MAX_PASSES", _lib.SP_TILE_MAX_PASSES),
                       ("SP_TILE_IOU", _lib.SP_TILE_IOU), ("SP_TILE_IOS", _lib.SP_TILE_IOS)):
        assert int(re.search(rf"#define {macro} (\d+)", text).group(1)) == val


def test_pack_tile_refs():
    tf = ScalePadding(target_size=(640, 640), minimum_rectangle=True)
    passes = Tiling(tile=(320, 256), overlap=0.25).plan(432, 640)
    geoms, groups = plan_pass_groups(passes, tf)
    assert [g[0] for g in groups] == [(448, 640), (512, 640)] and [g[1] for g in groups] == [[0], [1, 2, 3, 4, 5, 6]]
    base, B, H, W = 1 << 20, 2, 432, 640
    refs, spans = pack_tile_refs(base, B, H, W, passes, geoms, groups)
    assert spans == [(0, 2), (2, 12)] and len(refs) == 14
    seen = set()
    for k, r in enumerate(refs):
        y0, x0, h, w = passes[r.slot]
        g = tf.geometry(h, w)
        assert (r.h, r.w, r.pitch, r.x0, r.y0) == (h, w, W, x0, y0)
        assert r.data == base + ((r.image * H + y0) * W + x0) * 3
        assert (r.new_h, r.new_w, r.top, r.left) == (g["new_h"], g["new_w"], g["top"], g["left"]) and r.ratio == np.float32(g["ratio"])
        assert (k < 2) == (r.slot == 0)
        seen.add((r.image, r.slot))
    assert seen == {(b, s) for b in range(B) for s in range(7)}
    with pytest.raises(ValueError):
        pack_tile_refs(base, 1, 100, 100, [(0, 0, 101, 100)], [tf.geometry(101, 100)], [((128, 128), [0])])


def test_merge_reference_with_one_pass_and_iou_is_the_greedy_nms():
    rng = np.random.default_rng(3)
    n = 200
    xy = rng.integers(0, 4 * 80, (n, 2)).astype(np.float32) / 4
    wh = rng.integers(4, 4 * 60, (n, 2)).astype(np.float32) / 4
    rows = np.concatenate([xy, xy + wh, rng.integers(1, 50, (n, 1)).astype(np.float32) / 64, np.zeros((n, 1), np.float32)], 1)
    for thr, limit in ((0.5, 300), (0.3, 300), (0.5, 7)):
        want = greedy_nms_np(rows[:, :4], rows[:, 4], thr, limit)
        assert 7 <= len(want) < n
        got = tiled_ref.merge_rows_np(rows, "iou", thr, False, limit)
        assert np.array_equal(got, want)
        det, counts = tiled_ref.merge_np(rows[None, None], np.array([[n]], np.int32), "iou", thr, False, limit)
        assert counts[0] == len(want) and np.array_equal(det[0, :len(want)], rows[want]) and not det[0, len(want):].any()


def test_merge_reference_properties():
    f = np.float32
    big = [10, 10, 110, 210, 0.9, 0]
    inside = [20.25, 20.25, 60.25, 100.25, 0.8, 0]                               # IoU 0.16, IoS 1
    other_cls = [10, 10, 110, 210, 0.7, 1]
    empty = [50, 50, 50, 120, 0.6, 0]                                            # zero area: IoS is 0 / 0
    rows = np.array([big, inside, other_cls, empty], f)
    assert tiled_ref.merge_rows_np(rows, "iou", 0.5).tolist() == [0, 1, 2, 3]
    assert tiled_ref.merge_rows_np(rows, "ios", 0.5).tolist() == [0, 2, 3]
    assert tiled_ref.merge_rows_np(rows, "ios", 0.5, agnostic=True).tolist() == [0, 3]
    tie = np.array([big, big], f)
    assert tiled_ref.merge_rows_np(tie, "iou", 0.5).tolist() == [0]
