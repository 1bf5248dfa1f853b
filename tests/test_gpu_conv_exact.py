"""Every convolution launcher against an exact integer reference, bit for bit (tests/conv_exact.py): small integer operands make every fp32
partial sum exact in any order, so a float64 convolution on the CPU predicts every stored bit of every launch - forward through sp_conv2d_fwd /
sp_conv3x3_direct on every (tile, kernel) the tuner may pick (the detector's hardswish / channel-slice epilogues among them: the activation's
one division and the residual add round once each on an exact pre-activation, so their bits are unique too), input and weight gradients through train.ConvT, the grouped launches and the
BatchNorm statistics epilogue.  There is no tolerance in this module: every comparison is torch.equal on the stored bits."""
import types

import pytest
import torch

from simple_pose_amd import _lib, engine
from simple_pose_amd.train import ConvT, FlatParams
from tests import conv_exact as ce
from tests.test_conv_exact_host import BACKWARD_LAYERS, GROUPED, STATS, STEM
from tests.test_gpu_backward_kernels import LAYERS, STATS_CASES, _nhwc, _OneLayer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 4096       # guard elements behind every output: a store beyond the tensor would land here
P = _lib.ptr


@pytest.fixture(autouse=True)
def _knob_back_on():
    yield
    _lib.lib().sp_conv_set_tap_skip(1)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(got, want, what):
    """torch.equal on the stored bits; a mismatch reports how many elements differ and the first of them."""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if torch.equal(_bits(got), _bits(want)):
        return
    diff = _bits(got) != _bits(want)
    first = tuple(diff.nonzero()[0].tolist())
    raise AssertionError(f"{what}: {int(diff.sum())} of {diff.numel()} elements differ; first at {first}: got {got[first].item()!r}, exact {want[first].item()!r}")


def _guarded(n, dtype, fill=float("nan")):
    """A flat output of n elements pre-filled with NaN (every element must be written) and PAD guard elements behind it."""
    y = torch.full((n + PAD,), float("nan"), dtype=dtype, device=DEV)
    if fill == 0:
        y[:n] = 0
    return y


def _take(y, n, shape, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[n:]).all()), f"{what}: stored behind the tensor"
    out = y[:n].view(shape)
    assert not bool(torch.isnan(out).any()), f"{what}: elements left unwritten"
    return out


# ---- forward: one launch per (case, dtype, candidate) -------------------------------------------------------------------------------------------
class _Sweep:
    """Runs a (case, dtype) once, whoever asks first (its own test or the coverage test), and remembers which kernels ran."""

    def __init__(self):
        self.done, self.seen = {}, set()

    def run(self, case, dtype, only=None, tap_skip=1):
        key = (case.name, dtype, only, tap_skip)
        if key not in self.done:
            try:
                self.done[key] = (self._run(case, dtype, only, tap_skip), None)
            except AssertionError as e:
                self.done[key] = (0, e)
        ran, err = self.done[key]
        if err is not None:
            raise err
        return ran

    def _run(self, case, dtype, only, tap_skip):
        lib = _lib.lib()
        _lib.check(lib.sp_conv_set_tap_skip(tap_skip), "sp_conv_set_tap_skip")
        d = ce.make(case, dtype)
        ce.conditions(d)                               # a changed generator cannot silently empty the case
        low = ce.lower(d, engine.HipPacker(), DEV)
        op, desc, st = low.op, low.op.desc, _lib.current_stream()
        x = low.x
        if case.kind == "stem":
            x = torch.empty((case.B, case.H, case.width(dtype), 4), dtype=torch.bfloat16 if dtype == "bf16" else torch.float32, device=DEV)
            fn = lib.sp_nchw_to_nhwc4_bf16 if dtype == "bf16" else lib.sp_nchw_to_nhwc4
            _lib.check(fn(P(low.x), P(x), case.B, 3, case.H, case.width(dtype), st), "to_nhwc4")
        want = d.expected()
        n = want.numel()
        out_c, c0 = case.slice_of or (case.c_out, 0)
        if case.slice_of:                              # the guarded buffer is the whole out_c-channel tensor; the launch gets channel c0 of it
            n = n // case.c_out * out_c
            assert tuple(low.out_shape) == tuple(want.shape[:3]) + (out_c,) and op.c0 == c0
        cands = [only] if only else ce.candidates(low, case)
        assert cands, case.name
        for cand in cands:
            what = f"{case.name} {dtype} {cand}"
            fam = ce.family(low, cand, case.residual)
            y = _guarded(n, d.store_dtype)
            res = low.res
            if case.inplace:                           # residual == y: the accumulate form
                y[:n] = low.res.reshape(-1)
                res = y
            if cand[0] < 0:
                _lib.check(lib.sp_conv3x3_direct(desc, P(x), P(op.w), P(op.scale), P(op.shift), P(res), P(y), st), what)
            else:
                desc.tile_m, desc.tile_n, desc.kernel = cand
                _lib.check(lib.sp_conv2d_fwd(desc, P(x), P(op.w), P(op.scale), P(op.shift), P(res), P(y) + 4 * c0, st), what)
            if case.slice_of:
                torch.cuda.synchronize()
                full = y[:n].view(low.out_shape)
                outside = torch.cat([full[..., :c0], full[..., c0 + case.c_out:]], -1)
                prefill = _bits(torch.full((1,), float("nan"), dtype=d.store_dtype, device=DEV))
                assert bool((_bits(y[n:]) == prefill).all()), f"{what}: stored behind the tensor"
                assert bool((_bits(outside) == prefill).all()), f"{what}: stored outside channels [{c0}, {c0 + case.c_out})"
                got = full[..., c0:c0 + case.c_out]
                assert not bool(torch.isnan(got).any()), f"{what}: elements of the slice left unwritten"
                _same_bits(got, want, what)
            else:
                _same_bits(_take(y, n, want.shape, what), want, what)
            self.seen.add(fam)
            self.seen |= ce.detector_families(case, fam)
        return len(cands)


_SWEEP = _Sweep()
PAIRS = [(c, dt) for c in ce.FORWARD_CASES for dt in c.dtypes]
TAP_SKIP = [(h, w, t) for h, w in ((3, 2), (5, 4)) for t in ((64, 64), (128, 64), (128, 128))]


@pytest.mark.parametrize("case,dtype", PAIRS, ids=lambda v: v if isinstance(v, str) else v.name)
def test_forward_every_candidate_stores_the_exact_bits(case, dtype):
    ran = _SWEEP.run(case, dtype)
    print(f"{case.name} {dtype}: {ran} launches bit-exact")


@pytest.mark.parametrize("h,w,tile", TAP_SKIP, ids=[f"{h}x{w}_{t[0]}x{t[1]}" for h, w, t in TAP_SKIP])
def test_tap_skipping_on_and_off_store_the_exact_bits(h, w, tile):
    """3x3 at batch 70 on maps with and without interior (ragged M, tiles that straddle positions): the tap-skipping kernel and the full K loop."""
    case = ce.tap_skip_case(h, w, tile)
    cand = (tile[0], tile[1], _lib.SP_CONV_KERNEL_IGEMM)
    low = ce.lower(ce.make(case, "fp32"), engine.HipPacker(), DEV)
    low.op.desc.tile_m, low.op.desc.tile_n = tile
    _lib.lib().sp_conv_set_tap_skip(1)
    assert _lib.conv_kernel_name(low.op.desc, True) == f"conv_igemm_tapskip_kernel<{tile[0]}, {tile[1]}, 2, 2>"
    _lib.lib().sp_conv_set_tap_skip(0)
    assert _lib.conv_kernel_name(low.op.desc, True).startswith("conv_igemm_kernel<")
    _SWEEP.run(case, "fp32", cand, 1)
    _SWEEP.run(case, "fp32", cand, 0)


DETECTOR_3X3 = [c for c in ce.DETECTOR_CASES if c.k == 3]


@pytest.mark.parametrize("case", DETECTOR_3X3, ids=lambda c: c.name)
def test_detector_3x3_tap_skipping_on_and_off_store_the_exact_bits(case):
    """The detector's 3x3 convolutions (hardswish, residual after it, slice store) on every tile with the tap-skipping kernel allowed and with
    the full K loop.  The batch-70 cases resolve to conv_igemm_tapskip_kernel on the tiles of up to 128 rows (batch >= tile_m / 2), the
    Focus conv (c_in = 12 fills no K tile) and the small batches to the plain kernel: asserted on the library's own dispatch."""
    low = ce.lower(ce.make(case, "fp32"), engine.HipPacker(), DEV)
    lib = _lib.lib()
    for cand in ce.candidates(low, case):
        low.op.desc.tile_m, low.op.desc.tile_n, low.op.desc.kernel = cand
        lib.sp_conv_set_tap_skip(1)
        name = _lib.conv_kernel_name(low.op.desc, case.residual)
        skips = case.c_in % 32 == 0 and case.B >= cand[0] // 2
        assert name.startswith("conv_igemm_tapskip_kernel<" if skips else "conv_igemm_kernel<"), (cand, name)
        lib.sp_conv_set_tap_skip(0)
        assert _lib.conv_kernel_name(low.op.desc, case.residual).startswith("conv_igemm_kernel<")
    ran = _SWEEP.run(case, "fp32", None, 1), _SWEEP.run(case, "fp32", None, 0)
    print(f"{case.name}: {ran[0]} launches with tap skipping allowed, {ran[1]} without, all bit-exact")


def test_every_kernel_family_ran():
    """The coverage condition: over the whole table each implicit-GEMM tile in both dtypes, the tap-skipping kernel, the three ring kernels, the
    streaming 1x1 kernel and the direct kernel at 32, 64 and 128 channels stored exact bits, and so did the detector's epilogues on every fp32
    tile and in the tap-skipping kernel (cases that have not run yet run here)."""
    for case, dtype in PAIRS:
        _SWEEP.run(case, dtype)
    for h, w, tile in TAP_SKIP:
        _SWEEP.run(ce.tap_skip_case(h, w, tile), "fp32", (tile[0], tile[1], _lib.SP_CONV_KERNEL_IGEMM), 1)
    # the detector's epilogues: every fp32 tile stored exact bits with hardswish, with a slice at c0 > 0 and with hardswish + residual, the
    # tap-skipping kernel with hardswish and with a slice (conv_exact.required_detector_families)
    missing = ce.missing_families(_SWEEP.seen)
    assert not missing, missing
    assert ce.required_detector_families() <= _SWEEP.seen
    print(sorted(map(str, _SWEEP.seen)))


# ---- backward: train.ConvT ----------------------------------------------------------------------------------------------------------------------
MODES = [(False, False), (True, False), (True, True)]          # (bf16 operands, bf16 gradients)
MODE_IDS = ["fp32", "bf16", "bf16_grads"]


@pytest.mark.parametrize("bf16,g16", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", BACKWARD_LAYERS)
def test_dgrad_and_wgrad_store_the_exact_bits(name, bf16, g16):
    _, kind, I, O, k, s, p, H, W, B = next(c for c in LAYERS if c[0] == name)
    r = ce.backward_reference(kind, I, O, k, s, p, H, W, B, seed=1)
    ce.backward_conditions(r, acc_mag=4)
    one = _OneLayer(kind, r["w"].float(), H, W, bf16, g16=g16, stride=s, pad=p)
    L = one.layer
    lib, st = _lib.lib(), _lib.current_stream()
    adt = torch.bfloat16 if bf16 else torch.float32
    gdt = one.grad_dtype
    xd = _nhwc(r["x"], dtype=adt)
    dzd = _nhwc(r["dz"], c_buf=L.c_out_buf, dtype=adt)
    # ---- wgrad into the NaN-prefilled flat gradient: the integer dW ----
    L.d_wgrad.batch = B
    gt, at = (dzd, xd) if kind == "conv" else (xd, dzd)
    one.flat.grad.fill_(float("nan"))
    _lib.check(lib.sp_conv2d_wgrad(L.d_wgrad, P(gt), gt.shape[-1], P(at), L.wg["n_valid"], L.wg["c_valid"], L.wg["kw_valid"], L.wg["s_n"],
                                   L.wg["s_c"], P(one.flat.view("c.weight", grad=True)), P(one.wgrad_ws), one.wgrad_ws.numel() * 4, st), name)
    torch.cuda.synchronize()
    _same_bits(one.flat.view("c.weight", grad=True).view(r["w"].shape), r["dw"].float(), f"{name} wgrad")
    # ---- dgrad: every launch of the family; phases a 1x1 stride-2 layer never reaches stay zero ----
    want = r["dx"].permute(0, 2, 3, 1).contiguous()
    n = want.numel()
    full = L.dgrad_full_cover
    dx = _guarded(n, gdt, fill=float("nan") if full else 0)
    for d, wd in zip(L.d_dgrad, L.w_dgrad):
        d.batch = B
        _lib.check(lib.sp_conv2d_fwd(d, P(dzd), P(wd), None, None, None, P(dx), st), name + ".dgrad")
    _same_bits(_take(dx, n, want.shape, name + ".dgrad"), want.to(gdt), f"{name} dgrad")
    # the product path (ConvT.dgrad): a stride-2 family whose phases cover the input runs as ONE launch (sp_conv2d_dgrad_phases)
    _same_bits(L.dgrad(dzd, B, None), want.to(gdt), f"{name} ConvT.dgrad")
    if full:                                           # accumulate form (residual fan-out): dx = acc + dgrad, in place
        acc0 = ce.ints(tuple(want.shape), 4, ce.generator(name, 9))
        acc = _guarded(n, gdt)
        acc[:n] = acc0.reshape(-1).to(gdt)
        for d, wd in zip(L.d_dgrad, L.w_dgrad):
            _lib.check(lib.sp_conv2d_fwd(d, P(dzd), P(wd), None, None, P(acc), P(acc), st), name + ".dgrad+")
        _same_bits(_take(acc, n, want.shape, name + ".dgrad+"), (want + acc0).to(gdt), f"{name} dgrad accumulate")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_stem_7x7_wgrad_stores_the_exact_bits(bf16):
    """conv1 (3 -> 64, 7x7 s2 p3) reads the image as NHWC4 (fp32) / NHWC8 (bf16) with 8 packed taps per row; only its weight gradient exists."""
    I, O, k, s, p, H, W, B = STEM
    r = ce.backward_reference("conv", *STEM, seed=4)
    ce.backward_conditions(r)
    cbuf = 8 if bf16 else 4
    one = _OneLayer("conv", r["w"].float(), H, W, bf16, stride=s, pad=p, c_in_buf=cbuf, need_dgrad=False)
    L = one.layer
    adt = torch.bfloat16 if bf16 else torch.float32
    xd, dzd = _nhwc(r["x"], c_buf=cbuf, dtype=adt), _nhwc(r["dz"], dtype=adt)
    L.d_wgrad.batch = B
    one.flat.grad.fill_(float("nan"))
    _lib.check(_lib.lib().sp_conv2d_wgrad(L.d_wgrad, P(dzd), dzd.shape[-1], P(xd), L.wg["n_valid"], L.wg["c_valid"], L.wg["kw_valid"], L.wg["s_n"],
                                          L.wg["s_c"], P(one.flat.view("c.weight", grad=True)), P(one.wgrad_ws), one.wgrad_ws.numel() * 4,
                                          _lib.current_stream()), "stem")
    torch.cuda.synchronize()
    _same_bits(one.flat.view("c.weight", grad=True).view(r["w"].shape), r["dw"].float(), "stem wgrad")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C,groups,stride,B,H,W", GROUPED)
def test_grouped_forward_dgrad_wgrad_store_the_exact_bits(C, groups, stride, B, H, W, dtype):
    bf = dtype == "bf16"
    adt = torch.bfloat16 if bf else torch.float32
    r = ce.backward_reference("conv", C, C, 3, stride, 1, H, W, B, seed=2, groups=groups)
    ce.backward_conditions(r, acc_mag=4)
    conv = torch.nn.Conv2d(C, C, 3, stride=stride, padding=1, groups=groups, bias=False)
    conv.weight.data.copy_(r["w"].float())
    holder = torch.nn.Module()
    holder.add_module("g", conv)
    holder = holder.to(DEV)
    flat = FlatParams(holder)
    tr = types.SimpleNamespace(bf16=bf, g16=bf, grad_dtype=adt, flat=flat, kernel_events=None)
    layer = ConvT(tr, "g", "conv", holder.g.weight.detach(), H, W, stride=stride, pad=1, groups=groups)
    layer.pack_grouped(_lib.current_stream())
    xg, dzg = _nhwc(r["x"], dtype=adt), _nhwc(r["dz"], dtype=adt)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    z = layer.forward(xg, B)
    dx = layer.dgrad(dzg, B, None)
    flat.grad.fill_(float("nan"))
    layer.wgrad_grouped(xg, dzg, B)
    acc0 = ce.ints(tuple(nhwc(r["dx"]).shape), 4, ce.generator("grouped", C))
    dx2 = layer.dgrad(dzg, B, acc0.to(adt).to(DEV))
    torch.cuda.synchronize()
    _same_bits(z, nhwc(r["y"]).to(adt), "grouped forward")
    _same_bits(dx, nhwc(r["dx"]).to(adt), "grouped dgrad")
    _same_bits(dx2, (nhwc(r["dx"]) + acc0).to(adt), "grouped dgrad accumulate")
    _same_bits(flat.view("g.weight", grad=True).view(r["w"].shape), r["dw"].float(), "grouped wgrad")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(STATS))
def test_statistics_epilogue_sums_are_the_integer_column_sums(name, bf16):
    _, I, O, k, s, p, H, W, B = next(c for c in STATS_CASES if c[0] == name)
    r = ce.backward_reference("conv", I, O, k, s, p, H, W, B, seed=3, mag=STATS[name])
    ce.backward_conditions(r)
    adt = torch.bfloat16 if bf16 else torch.float32
    z64 = r["y"].permute(0, 2, 3, 1).contiguous()
    ce.stats_conditions(z64.reshape(-1, O), adt)
    one = _OneLayer("conv", r["w"].float(), H, W, bf16, stride=s, pad=p)
    z, part, prow = one.layer.forward_bn_stats(_nhwc(r["x"], dtype=adt), B)
    torch.cuda.synchronize()
    assert part.shape[1] == prow and prow > 0
    _same_bits(z, z64.to(adt), f"{name} z")
    cols = z64.reshape(-1, O)
    assert torch.equal(part[0].double().sum(0).cpu()[:O], cols.sum(0)), f"{name}: column sums"
    assert torch.equal(part[1].double().sum(0).cpu()[:O], (cols * cols).sum(0)), f"{name}: column sums of squares"
