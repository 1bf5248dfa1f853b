"""CPU side of the decoder edge tests: the fixture frozen from the real reference (tests/golden/g4b_decode_shapes.npz) loads and holds what
it should, the C oracle reproduces it within the bars the GPU tests use, every hand-built map takes the branch it is named for, and the
launcher refuses what it cannot run by name, before any launch."""
import ctypes
import os

import numpy as np
import pytest

from oracle import pose_oracle
from simple_pose_amd import _lib, synth
from tests import decode_edges as de

# tests/test_gpu_parity.py's decoder bars (px per unit of |trans_inv|); that module needs no GPU to import
from tests.test_gpu_parity import BASIC_BAR, GT_ORACLE_BAR, GT_REFERENCE_BAR


def test_fixture_loads_and_holds_the_issue_shapes(golden):
    g = golden(de.FIXTURE)
    assert [tuple(s) for s in g["shapes"]] == list(de.SHAPES)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", de.FIXTURE)) < 500_000
    for H, W, ks in de.SHAPES:
        nm = [str(s) for s in g[f"{H}x{W}/names"]]
        assert g[f"{H}x{W}/maps"].shape[1:] == (de.B, de.J, H, W)
        assert [str(r) for r in g[f"{H}x{W}/raised"]] == [""], "the reference raised on no map when the fixture was made"
        for kind in ("interior_gauss", "all_zero", "all_negative", "constant_positive", "single_nan", "inf_at_peak"):
            assert kind in nm, (H, W, kind)
        if H * W > 1024 + H * W // 3:
            assert {"tie_2_apart", "tie_64_apart", "tie_256_apart", "tie_1024_apart"} <= set(nm)
        if H >= 40 and W >= 32:
            assert "clamp_plateau_det0" in nm
        for n, maps, exp in de.groups(g, H, W, ks):
            assert set(exp) == {"axis", "axis_max"} | {f"{t}/{k}" for t in ("ident4", "rand") for k in ("gt_kps", "gt_max", "basic_kps")}


@pytest.mark.parametrize("H,W,ks", de.SHAPES, ids=de.IDS)
def test_oracle_reproduces_the_reference_fixture(golden, H, W, ks):
    """The bars of the GPU test, with no kernel involved: index work bit exact, GaussTaylor within GT_REFERENCE_BAR x scale, Basic within
    BASIC_BAR x scale, NaN exactly where the reference has it."""
    g = golden(de.FIXTURE)
    for n, maps, exp in de.groups(g, H, W, ks):
        co, mv = pose_oracle.heat_map_to_axis(maps)
        assert de.same_bits(co, exp["axis"]) and de.same_bits(mv, exp["axis_max"]), n
        for tname, tinv in de.trans_sets():
            scale = de.scale_of(tinv)
            kps, mv = pose_oracle.decode_gauss_taylor(maps, tinv, ks)
            assert de.same_bits(mv, exp[f"{tname}/gt_max"])
            assert de.max_err(kps, exp[f"{tname}/gt_kps"]) <= GT_REFERENCE_BAR * scale, (n, tname)
            bk, _ = pose_oracle.decode_basic(maps, tinv)
            assert de.max_err(bk, exp[f"{tname}/basic_kps"]) <= BASIC_BAR * scale, (n, tname)
    assert GT_ORACLE_BAR <= GT_REFERENCE_BAR


@pytest.mark.parametrize("H,W,ks", de.SHAPES, ids=de.IDS)
def test_every_hand_built_map_takes_the_branch_it_is_named_for(golden, H, W, ks):
    """Refined and unrefined joints counted on the REFERENCE's outputs (a joint is refined when its key point is not the affine image of its
    arg-max) against the two guards restated in numpy, map by map."""
    g = golden(de.FIXTURE)
    nm = de.names(g, H, W)
    tinv = synth.trans_inv_batch(de.B)
    first = 4 * ((H * W // 3) // 4)
    refined = {"gt": 0, "basic": 0}
    for n, maps, exp in de.groups(g, H, W, ks):
        basic_ok, gt_ok, xi, yi = de.guards(maps)
        assert np.array_equal(exp["axis"][..., 0], xi) and np.array_equal(exp["axis"][..., 1], yi)
        raw = de.affine(exp["axis"], tinv)
        with np.errstate(invalid="ignore"):
            gt_moved = (exp["ident4/gt_kps"] != raw).any(-1)
            basic_moved = (exp["ident4/basic_kps"] != raw).any(-1)
        for b in range(de.B):
            for j in range(de.J):
                name, where = nm[n * de.B * de.J + b * de.J + j], (H, W, ks, n, b, j)
                x, y, mx = int(xi[b, j]), int(yi[b, j]), exp["axis_max"][b, j, 0]
                kind, _, arg = name.rpartition("_")
                if name in ("all_zero", "all_negative", "single_nan"):
                    assert (x, y) == (0, 0) and not gt_moved[b, j] and not basic_moved[b, j], where
                    assert (np.isnan(mx) if name == "single_nan" else mx <= 0), where
                elif name == "constant_positive":
                    assert (x, y) == (0, 0) and mx == 0.5 and not gt_moved[b, j] and not basic_moved[b, j], where
                elif name.startswith("tie_"):
                    assert (x, y) == (first % W, first // W) and mx == 2.0, where
                elif kind in ("peak_x", "peak_y"):
                    assert (x if kind == "peak_x" else y) == int(arg), where
                    assert gt_moved[b, j] == gt_ok[b, j] and basic_moved[b, j] == basic_ok[b, j], where
                elif name == "clamp_plateau_det0":
                    assert gt_ok[b, j] and not gt_moved[b, j] and mx == 10.0, where
                elif name == "inf_at_peak":
                    assert mx == np.inf and (x, y) == (W // 2, H // 2), where
                    assert np.isnan(exp["ident4/gt_kps"][b, j]).all() == bool(gt_ok[b, j]), where     # inf * inf / inf through clamp and log
                else:
                    assert name == "interior_gauss" and gt_moved[b, j] == gt_ok[b, j] and basic_moved[b, j] == basic_ok[b, j], where
                refined["gt"] += int(gt_moved[b, j]); refined["basic"] += int(basic_moved[b, j])
    if (H, W) in ((5, 4), (3, 50), (1, 1)):
        assert refined["gt"] == 0, "the GaussTaylor guard can never hold at this size"
    if (H, W) == (5, 4):
        assert refined["basic"] > 0, "the Basic guard can (x = 2, y in 2..3)"
    if min(H, W) >= 13:
        assert refined["gt"] > 0 and refined["basic"] > refined["gt"] - 2, refined


def test_peaks_at_w_minus_2_separate_the_two_guards(golden):
    g = golden(de.FIXTURE)
    for H, W, ks in de.SHAPES:
        if min(H, W) < 13:
            continue
        nm = de.names(g, H, W)
        maps = g[f"{H}x{W}/maps"].reshape(-1, 1, H, W)
        for name in (f"peak_x_{W - 2}", f"peak_y_{H - 2}"):
            basic_ok, gt_ok, _, _ = de.guards(maps[nm.index(name)][None])
            assert basic_ok.all() and not gt_ok.any(), (H, W, name)
        for name in (f"peak_x_{W - 3}", f"peak_y_{H - 3}", "peak_x_2", "peak_y_2"):
            basic_ok, gt_ok, _, _ = de.guards(maps[nm.index(name)][None])
            assert basic_ok.all() and gt_ok.all(), (H, W, name)
        for name in ("peak_x_1", "peak_y_1"):
            basic_ok, gt_ok, _, _ = de.guards(maps[nm.index(name)][None])
            assert not basic_ok.any() and not gt_ok.any(), (H, W, name)


def test_round_trip_bounds_hold_at_96x72_on_the_oracle():
    """What tests/test_gpu_decode_edges.py relies on: decode(encode(j)) recovers joints >= 8 px from the border of a 96 x 72 map within the
    bounds asserted at 64 x 48 (max < 5e-3 px, median < 1e-3 px).  Measured here: max 3.3e-4, median 6.0e-5 px."""
    Bn, H, W = 4, 96, 72
    j = synth.joints_batch(Bn, 17, seed=78, w=W, h=H)
    j[..., 0] = np.clip(j[..., 0], 8.0, W - 9.0)
    j[..., 1] = np.clip(j[..., 1], 8.0, H - 9.0)
    j[..., 2] = 1.0
    ot, ow = pose_oracle.encode_refine(j, 2.0, (W, H))
    ident = np.zeros((Bn, 2, 3), np.float32); ident[:, 0, 0] = 1; ident[:, 1, 1] = 1
    okps, _ = pose_oracle.decode_gauss_taylor(ot, ident)
    err = np.abs(okps - j[..., :2])
    assert err.max() < 5e-3 and np.median(err) < 1e-3 and (ow == 1).all(), (err.max(), np.median(err))


def _lds_need(H, W, ks):
    pw = (((W + 11) // 12 * 12 + ks + 6) // 4) * 4 + 4
    return ((H + 2 * (ks // 2)) * pw + H * W) * 4


def test_decoder_refusals_are_by_name_and_launch_nothing():
    """kernel_size 0, 2 and 17, and maps beyond one workgroup's 160 KiB of LDS, the message carrying the bytes needed.  The pointers are
    not device memory: every one of these returns before a launch."""
    lib = _lib.lib()
    one = ctypes.c_void_p(16)
    for ks in (0, 2, 17):
        rc = lib.sp_decode_gauss_taylor(one, one, 1, 3, 16, 12, ks, one, one, None)
        msg = lib.sp_last_error()
        assert rc == -1 and b"kernel_size=%d " % ks in msg and b"odd" in msg, msg
    assert (_lds_need(96, 72, 11), _lds_need(72, 96, 11), _lds_need(128, 96, 11)) == (66656, 65696, 113184)       # accepted sizes
    for H, W in ((256, 192), (160, 120)):
        need = _lds_need(H, W, 11)
        assert need > 160 * 1024 - 32
        rc = lib.sp_decode_gauss_taylor(one, one, 1, 3, H, W, 11, one, one, None)
        msg = lib.sp_last_error()
        assert rc == -1 and b"sp_decode_gauss_taylor" in msg and b"%dx%d" % (H, W) in msg and b"%d B" % need in msg and b"160 KiB" in msg, msg
    assert _lds_need(256, 192, 11) == 422176
    rc = lib.sp_decode_basic(one, one, 1, 3, 256, 192, one, one, None)                  # the raw map alone: 196,608 B
    assert rc == -1 and b"sp_decode_basic" in lib.sp_last_error() and b"196608 B" in lib.sp_last_error(), lib.sp_last_error()
    rc = lib.sp_heat_map_to_axis(one, 1, 3, 256, 192, one, one, None)
    assert rc == -1 and b"sp_heat_map_to_axis" in lib.sp_last_error() and b"196608 B" in lib.sp_last_error(), lib.sp_last_error()
    rc = lib.sp_decode_gauss_taylor(None, one, 1, 3, 16, 12, 11, one, one, None)
    assert rc == -1 and b"null" in lib.sp_last_error()
