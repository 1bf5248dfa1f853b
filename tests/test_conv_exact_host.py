"""The exact-integer convolution cases (tests/conv_exact.py) without a GPU: every case's conditions hold on its reference, the descriptor
interpreter (tests/desc_interp.conv_desc_cpu on TorchPacker's layouts) reproduces the integer reference exactly - packing and geometry against an
independent float64 convolution - the case table reaches every kernel family the GPU module must run, and the method catches what it is for: one
dropped product at K = 4608, and a store that truncates."""
import pytest
import torch

from simple_pose_amd import _lib
from tests import conv_exact as ce
from tests.desc_interp import TorchPacker, conv_desc_cpu
from tests.test_gpu_backward_kernels import LAYERS, STATS_CASES

PAIRS = [(c, dt) for c in ce.FORWARD_CASES for dt in c.dtypes]
TAP_SKIP = [ce.tap_skip_case(h, w, t) for h, w in ((3, 2), (5, 4)) for t in ((64, 64), (128, 64), (128, 128))]
BACKWARD_LAYERS = ("1x1", "1x1_wide_m", "3x3_s1", "3x3_s2", "1x1_s2_shortcut", "final_1x1_17", "deconv_k4s2p1")
GROUPED = [(128, 32, 1, 3, 12, 10), (256, 32, 2, 2, 16, 12)]
STEM = (3, 64, 7, 2, 3, 32, 24, 3)                                      # conv1: I, O, k, stride, pad, H, W, B (only its weight gradient exists)
STATS = {"1x1_64_128": 2, "3x3_64_64": 2, "3x3_s2_128_128": 1}          # case -> operand magnitude that keeps every |z| a bf16 value


def _interpret(d: ce.Data) -> torch.Tensor:
    low = ce.lower(d, TorchPacker(), "cpu")
    c, op = d.case, low.op
    x = low.x
    if c.kind == "stem":               # what the layout launch leaves: NHWC4 in the activation dtype, channel 3 zero
        x4 = torch.zeros((c.B, c.H, c.width(d.dtype), 4))
        x4[..., :3] = x.permute(0, 2, 3, 1)
        x = x4.to(torch.bfloat16 if d.dtype == "bf16" else torch.float32)
    y = torch.full(low.out_shape, float("nan"), dtype=torch.float64)
    conv_desc_cpu(op.desc, x, op.w, op.scale, op.shift, low.res, y, c.B)
    assert not torch.isnan(y).any()
    return y


@pytest.mark.parametrize("case,dtype", PAIRS + [(c, "fp32") for c in TAP_SKIP], ids=lambda v: v if isinstance(v, str) else v.name)
def test_conditions_and_interpreter_equals_the_integer_reference(case, dtype):
    d = ce.make(case, dtype)
    print(case.name, dtype, ce.conditions(d))
    y = _interpret(d)
    want = d.stored()
    diff = y != want
    assert not bool(diff.any()), f"{int(diff.sum())} of {diff.numel()} differ, first at {tuple(diff.nonzero()[0].tolist())}"
    assert tuple(d.expected().shape) == tuple(y.shape) and d.expected().dtype == d.store_dtype


def test_the_case_table_reaches_every_kernel_family():
    """The coverage condition of the GPU module, decided by the library's own dispatch (eligibility tests and kernel names need no GPU)."""
    lib = _lib.lib()
    seen = set()
    try:
        for case, dtype in PAIRS + [(c, "fp32") for c in TAP_SKIP]:
            d = ce.make(case, dtype)
            low = ce.lower(d, TorchPacker(), "cpu")
            cands = ce.candidates(low, case)
            if case in TAP_SKIP:
                tile = tuple(int(v) for v in case.name.split("_")[-1].split("x"))
                cands = [(tile[0], tile[1], _lib.SP_CONV_KERNEL_IGEMM)]
            assert cands, case.name
            lib.sp_conv_set_tap_skip(1)
            fams = {ce.family(low, k, case.residual) for k in cands}
            if case in TAP_SKIP:
                assert fams == {("tapskip", cands[0][:2])}, fams
                lib.sp_conv_set_tap_skip(0)
                assert {ce.family(low, k, case.residual) for k in cands} == {("igemm", cands[0][:2], "fp32")}
            seen |= fams
    finally:
        lib.sp_conv_set_tap_skip(1)
    assert not ce.missing_families(seen), ce.missing_families(seen)
    assert ("direct", "head128") in seen          # the 128 -> 17 head kernel behind sp_conv3x3_direct takes part as well


@pytest.mark.parametrize("name", BACKWARD_LAYERS)
def test_backward_conditions(name):
    _, kind, I, O, k, s, p, H, W, B = next(c for c in LAYERS if c[0] == name)
    print(name, ce.backward_conditions(ce.backward_reference(kind, I, O, k, s, p, H, W, B, seed=1), acc_mag=4))


@pytest.mark.parametrize("C,groups,stride,B,H,W", GROUPED)
def test_grouped_backward_conditions(C, groups, stride, B, H, W):
    print(ce.backward_conditions(ce.backward_reference("conv", C, C, 3, stride, 1, H, W, B, seed=2, groups=groups), acc_mag=4))


def test_stem_wgrad_conditions():
    print(ce.backward_conditions(ce.backward_reference("conv", *STEM, seed=4)))


@pytest.mark.parametrize("name", sorted(STATS))
def test_statistics_conditions(name):
    _, I, O, k, s, p, H, W, B = next(c for c in STATS_CASES if c[0] == name)
    r = ce.backward_reference("conv", I, O, k, s, p, H, W, B, seed=3, mag=STATS[name])
    ce.backward_conditions(r)
    print(name, ce.stats_conditions(r["y"].permute(0, 2, 3, 1).reshape(-1, O), torch.bfloat16))


# ---- the method catches what it is for ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["one_product", "one_tap"])
def test_a_dropped_term_at_k4608_changes_the_bf16_result(what):
    """One product (one tap of one channel: 512 of them) of one output channel zeroed in the packed matrix: more than 90 % of the outputs that
    read it change in the bf16-rounded result - the error a tolerance of 6e-3 of the tensor's maximum lets through."""
    case = next(c for c in ce.FORWARD_CASES if c.name == "c3_512_128_k4608")
    d = ce.make(case, "bf16")
    low = ce.lower(d, TorchPacker(), "cpu")
    op, o, tap, ch = low.op, 37, 5, 301
    ty, tx = divmod(tap, 3)
    y = torch.empty(low.out_shape, dtype=torch.float64)
    conv_desc_cpu(op.desc, low.x, op.w, op.scale, op.shift, None, y, case.B)
    assert torch.equal(y.bfloat16(), d.expected())
    w = op.w.clone()
    assert w.shape[1] == 9 * 512
    k0, k1 = (tap * 512 + ch, tap * 512 + ch + 1) if what == "one_product" else (tap * 512, (tap + 1) * 512)
    assert bool((w[o, k0:k1] != 0).all())
    w[o, k0:k1] = 0
    conv_desc_cpu(op.desc, low.x, w, op.scale, op.shift, None, y, case.B)
    changed = y.bfloat16() != d.expected()
    assert not bool(changed[..., :o].any()) and not bool(changed[..., o + 1:].any())
    # the outputs whose tap (ty, tx) lies inside the image: the others never read the zeroed weights
    oy, ox = torch.arange(case.H).view(-1, 1), torch.arange(case.W).view(1, -1)
    reads = ((oy + ty - 1 >= 0) & (oy + ty - 1 < case.H) & (ox + tx - 1 >= 0) & (ox + tx - 1 < case.W)).expand(case.B, case.H, case.W)
    assert not bool(changed[..., o][~reads].any())
    share = changed[..., o][reads].double().mean().item()
    print(what, "changed", share, "of", int(reads.sum()))
    assert share > 0.90


@pytest.mark.parametrize("name", ["round_c3_128", "round_c3_128_relu"])
def test_a_truncating_store_fails_the_rounding_case(name):
    d = ce.make(next(c for c in ce.FORWARD_CASES if c.name == name), "bf16")
    assert torch.equal(d.expected(), d.stored().float().bfloat16())
    wrong = ce.truncate_to_bf16(d.stored())
    share = (wrong.view(torch.int16) != d.expected().view(torch.int16)).double().mean().item()
    print(name, "a truncating store differs on", share)
    assert share >= 0.10
