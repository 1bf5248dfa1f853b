"""The key-point decoders (csrc/decode.hip) on the MI355X at the map sizes, kernel sizes and edges the 64 x 48 / kernel_size 11 tests do not
reach: against the real reference's outputs (tests/golden/g4b_decode_shapes.npz) and against the C oracle, on hand-built maps from 1 x 1 to
128 x 96 (more than 64 KiB of LDS), with the bars tests/test_gpu_parity.py holds the 64 x 48 path to and no share of joints left out."""
import numpy as np
import pytest
import torch

from oracle import pose_oracle
from simple_pose_amd import _lib, synth
from simple_pose_amd.commons.transforms import RefineSimpleTransform
from simple_pose_amd.metrics import BasicKeyPointDecoder, GaussTaylorKeyPointDecoder
from tests import decode_edges as de
from tests.test_gpu_parity import BASIC_BAR, GT_ORACLE_BAR, GT_REFERENCE_BAR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = _lib.ptr
TAIL = 64          # guard floats behind kps and max_val


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return _lib.current_stream(torch.device(DEV))


def _decode(mode, hm, tinv, ks=None):
    """One launch through the C ABI into NaN-prefilled outputs with a guard tail: returns (kps [B,J,2], max_val [B,J,1]) as numpy after
    checking that the tails are intact.  Whether every output was written is the caller's comparison: an unwritten one is still NaN where
    the expected value is not."""
    Bn, Jn, H, W = hm.shape
    n = Bn * Jn
    kps = torch.full((2 * n + TAIL,), float("nan"), device=DEV)
    mv = torch.full((n + TAIL,), float("nan"), device=DEV)
    sentinel = torch.tensor(-12345.5, device=DEV)
    kps[2 * n:], mv[n:] = sentinel, sentinel
    lib = _lib.lib()
    if mode == "axis":
        rc = lib.sp_heat_map_to_axis(P(hm), Bn, Jn, H, W, P(kps), P(mv), _stream())
    elif mode == "basic":
        rc = lib.sp_decode_basic(P(hm), P(tinv), Bn, Jn, H, W, P(kps), P(mv), _stream())
    else:
        rc = lib.sp_decode_gauss_taylor(P(hm), P(tinv), Bn, Jn, H, W, ks, P(kps), P(mv), _stream())
    _lib.check(rc, f"decode {mode} {H}x{W} ks={ks}")
    kps, mv = kps.cpu().numpy(), mv.cpu().numpy()
    assert (kps[2 * n:] == -12345.5).all() and (mv[n:] == -12345.5).all(), "wrote behind its outputs"
    return kps[:2 * n].reshape(Bn, Jn, 2), mv[:n].reshape(Bn, Jn, 1)


@pytest.mark.parametrize("H,W,ks", de.SHAPES, ids=de.IDS)
def test_decoders_at_other_sizes_vs_reference_fixture_and_oracle(golden, measured, H, W, ks):
    """Every map of the fixture at this (size, kernel size).  Index work is bit exact; key points meet the three bars of the 64 x 48 tests,
    every joint, NaN where the reference has NaN (the +inf peak); the input is unchanged, every output written, nothing behind them."""
    g = golden(de.FIXTURE)
    worst = dict(ref=0.0, oracle=0.0, basic=0.0)
    for n, maps, exp in de.groups(g, H, W, ks):
        hm = _cuda(maps)
        before = hm.clone()
        co, mv = _decode("axis", hm, None)
        assert de.same_bits(co, exp["axis"]), (n, co, exp["axis"])
        assert de.same_bits(mv, exp["axis_max"]), n
        for tname, tinv in de.trans_sets():
            scale = de.scale_of(tinv)
            t = _cuda(tinv)
            kps, mv = _decode("gauss_taylor", hm, t, ks)
            assert de.same_bits(mv, exp[f"{tname}/gt_max"]), (n, tname)
            okps, omv = pose_oracle.decode_gauss_taylor(maps, tinv, ks)
            assert de.same_bits(mv, omv), (n, tname)
            e_ref, e_or = de.max_err(kps, exp[f"{tname}/gt_kps"]) / scale, de.max_err(kps, okps) / scale
            bk, bmv = _decode("basic", hm, t)
            assert de.same_bits(bmv, exp["axis_max"]), (n, tname)
            e_b = de.max_err(bk, exp[f"{tname}/basic_kps"]) / scale
            print(f"MEASURED-RAW {H}x{W} ks{ks} group {n} {tname}: vs reference {e_ref:.3g}  vs oracle {e_or:.3g}  basic {e_b:.3g}")
            worst = dict(ref=max(worst["ref"], e_ref), oracle=max(worst["oracle"], e_or), basic=max(worst["basic"], e_b))
        assert torch.equal(hm.view(torch.int32), before.view(torch.int32)), "decoder must not modify its input"
    measured("gauss_taylor_vs_reference_px_over_scale", worst["ref"], GT_REFERENCE_BAR)
    measured("gauss_taylor_vs_oracle_px_over_scale", worst["oracle"], GT_ORACLE_BAR)
    measured("basic_vs_reference_px_over_scale", worst["basic"], BASIC_BAR)
    assert worst["ref"] <= GT_REFERENCE_BAR, worst
    assert worst["oracle"] <= GT_ORACLE_BAR, worst
    assert worst["basic"] <= BASIC_BAR, worst


def test_generic_decoder_path_every_joint_within_the_oracle_bar(measured):
    """Strict companion of test_decoder_other_shapes_and_kernel_sizes on its four shapes: every joint carries a bump of 8x the noise's
    standard deviation or more (amplitude 8 over 0.01 x N(0, 1)), and EVERY joint is within GT_ORACLE_BAR x scale of the oracle."""
    worst = 0.0
    for (Bn, Jn, H, W, ks) in [(2, 5, 32, 24, 7), (1, 3, 40, 52, 11), (3, 17, 64, 48, 5), (2, 4, 17, 13, 3)]:
        maps = synth.tensor_normal(5, f"dec/{H}x{W}", (Bn, Jn, H, W), std=1.0)
        yy, xx = np.mgrid[0:H, 0:W]
        for b in range(Bn):
            for j in range(Jn):
                cx, cy = 3 + (7 * j + 3 * b) % (W - 6), 3 + (5 * j + b) % (H - 6)
                maps[b, j] = 8 * np.exp(-((xx - cx - 0.3) ** 2 + (yy - cy + 0.2) ** 2) / 8.0) + 0.01 * maps[b, j]
        tinv = synth.trans_inv_batch(Bn, seed=4)
        kps, mv = _decode("gauss_taylor", _cuda(maps), _cuda(tinv), ks)
        okps, omv = pose_oracle.decode_gauss_taylor(maps, tinv, ks)
        assert np.array_equal(mv, omv)
        err = de.max_err(kps, okps) / de.scale_of(tinv)
        print(f"MEASURED-RAW generic {H}x{W} ks{ks}: {err:.3g}")
        worst = max(worst, err)
    measured("generic_path_vs_oracle_px_over_scale", worst, GT_ORACLE_BAR)
    assert worst <= GT_ORACLE_BAR, worst


def test_encode_decode_round_trip_at_96x72(measured):
    """decode(encode(j)) == j at the 384 x 288 configuration's map size (66,656 B of LDS): B = 4, 17 joints, sigma 2, joints >= 8 px from
    the border, identity trans_inv - the bounds test_encode_decode_round_trip_full_batch asserts at 64 x 48.  (The oracle's round trip on
    these joints sits at max 3.3e-4 / median 6.0e-5 px: tests/test_decode_edges_host.py.)"""
    Bn, H, W = 4, 96, 72
    j = synth.joints_batch(Bn, 17, seed=78, w=W, h=H)
    j[..., 0] = np.clip(j[..., 0], 8.0, W - 9.0)
    j[..., 1] = np.clip(j[..., 1], 8.0, H - 9.0)
    j[..., 2] = 1.0
    t, w = RefineSimpleTransform.get_heat_map(_cuda(j), 2.0, (W, H))
    ident = np.zeros((Bn, 2, 3), np.float32); ident[:, 0, 0] = 1; ident[:, 1, 1] = 1
    kps, mv = GaussTaylorKeyPointDecoder()(t, _cuda(ident))
    err = np.abs(kps.cpu().numpy() - j[..., :2])
    measured("round_trip_96x72_max_px", err.max(), 5e-3)
    measured("round_trip_96x72_median_px", np.median(err), 1e-3)
    assert err.max() < 5e-3 and np.median(err) < 1e-3, (err.max(), np.median(err))
    assert torch.all(w == 1)
    ot, _ = pose_oracle.encode_refine(j, 2.0, (W, H))
    okps, _ = pose_oracle.decode_gauss_taylor(ot, ident)
    assert np.abs(kps.cpu().numpy() - okps).max() <= 1e-4
    co, _ = BasicKeyPointDecoder.heat_map_to_axis(t)
    assert np.array_equal(co.cpu().numpy(), np.round(j[..., :2]))                       # the arg-max is the nearest pixel
