"""The exact-integer convolution cases (tests/conv_exact.py) without a GPU: every case's conditions hold on its reference, the descriptor
interpreter (tests/desc_interp.conv_desc_cpu on TorchPacker's layouts) reproduces the integer reference exactly - packing and geometry against an
independent float64 convolution - the case table reaches every kernel family the GPU module must run, and the method catches what it is for: one
dropped product at K = 4608, and a store that truncates.  The same for the fused launches (conv_exact.Fused): the tables of tests/test_gpu_fused_exact.py,
the float64 chain against the per-conv chain of the interpreter, and four mutated chains that must store other bits."""
import copy

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

# ---- the launches that run several convolutions at once (conv_exact.Fused): (B, H, W) per entry point, the smallest maps at which its tiling can go
# wrong - one pixel, below one tile, exactly one tile, ragged in both directions - and one ragged map with more tiles than the part has compute units
CUS = 256                                                               # MI355X; the GPU module asserts tiles > the device's own count


def _more_tiles_than_cus(family, H, W):
    return (CUS // ce.fused_tiles(ce.Fused(family, 1, H, W)) + 1, H, W)


FUSED_SHAPES = {
    "bneck64": [(1, 1, 1), (2, 5, 3), (1, 16, 8), (3, 19, 11), (2, 17, 9), (1, 24, 40), (70, 17, 9)],                 # 16x8 tiles, persistent
    "bb32": [(1, 1, 1), (2, 7, 5), (1, 8, 48), (3, 9, 50), (2, 23, 100), _more_tiles_than_cus("bb32", 9, 50)],        # 8x48 strips (8x16 tiles behind the knob)
    "bb64": [(1, 1, 1), (2, 3, 5), (1, 4, 24), (3, 5, 26), (2, 32, 24), _more_tiles_than_cus("bb64", 5, 26)],         # 4x24 strips
    "dual_bf16": [(1, 1, r) for r in (77, 128, 1000, 128 * 300 + 5)],                                                 # 128-row tiles
    "dual_f32": [(1, 1, r) for r in (50, 64 * 9, 1000, 64 * 700 + 3)],
    "pwchain64": [(1, 1, r) for r in (50, 64 * 9, 1000, 64 * 700 + 3)],
    "pwchain128": [(1, 1, r) for r in (50, 64 * 9, 1000, 64 * 700 + 3)],
    "htrans": [(1, 2, 2), (1, 8, 6), (3, 34, 18), (2, 32, 16), (1, 66, 34)],                                          # 32x16 tiles, h and w even
}
FUSED_CASES = [ce.Fused(f, *shape) for f, shapes in FUSED_SHAPES.items() for shape in shapes]
MANY_TILES = {f: ce.Fused(f, *FUSED_SHAPES[f][-1]) for f in ("bneck64", "bb32", "bb64")}
# the mutation checks run on one ragged case per family; which of the four exist for it (no 3x3 padding in a pointwise chain, no intermediate bf16 store
# in an fp32 one or in transition1, no residual in transition1)
MUTATIONS = {"bneck64": ((3, 19, 11), ("ring", "trunc", "drop", "shift_res")), "bb32": ((3, 9, 50), ("ring", "trunc", "drop", "shift_res")),
             "bb64": ((3, 5, 26), ("ring", "trunc", "drop", "shift_res")), "dual_bf16": ((1, 1, 1000), ("trunc", "drop", "shift_res")),
             "dual_f32": ((1, 1, 1000), ("drop", "shift_res")), "pwchain64": ((1, 1, 1000), ("drop", "shift_res")),
             "pwchain128": ((1, 1, 1000), ("drop", "shift_res")), "htrans": ((3, 34, 18), ("drop",))}


def _interpret(d: ce.Data, c0_shift: int = 0) -> torch.Tensor:
    """The lowered launch through the descriptor interpreter.  SP_CONV_HARDSWISH / SP_CONV_OUT_SLICE as include/simple_pose_hip.h documents them
    (detector_ref.run_yolo_program_cpu does the same for the whole network): the plain launch of c_out channels, then the activation in fp32 - one
    torch operation per IEEE operation, the divisor a tensor - then the residual, stored at channels [c0, c0 + c_out) of the out_c-channel
    tensor, whose other channels stay NaN.  `c0_shift`: MUTATION - the slice lands that many channels further on."""
    low = ce.lower(d, TorchPacker(), "cpu")
    c, op = d.case, low.op
    x = low.x
    if c.kind == "stem":               # what the layout launch leaves: NHWC4 in the activation dtype, channel 3 zero
        x4 = torch.zeros((c.B, c.H, c.width(d.dtype), 4))
        x4[..., :3] = x.permute(0, 2, 3, 1)
        x = x4.to(torch.bfloat16 if d.dtype == "bf16" else torch.float32)
    y = torch.full(low.out_shape, float("nan"), dtype=torch.float64)
    if op.desc.flags & (_lib.SP_CONV_HARDSWISH | _lib.SP_CONV_OUT_SLICE):
        dd = copy.copy(op.desc)
        dd.flags = op.desc.flags & ~(_lib.SP_CONV_HARDSWISH | _lib.SP_CONV_OUT_SLICE)
        dd.out_c = dd.c_out
        t = torch.full(low.out_shape[:3] + (dd.c_out,), float("nan"), dtype=torch.float64)
        conv_desc_cpu(dd, x, op.w, op.scale, op.shift, None, t, c.B)
        assert torch.equal(t.float().double(), t)
        if op.desc.flags & _lib.SP_CONV_HARDSWISH:
            v = t.float()
            t = ((v * torch.clamp(v + 3.0, 0.0, 6.0)) / torch.full_like(v, 6.0)).double()
        if low.res is not None:
            t = (t.float() + low.res).double()
        c0 = op.c0 + c0_shift
        y[..., c0:c0 + dd.c_out] = t
        return y
    conv_desc_cpu(op.desc, x, op.w, op.scale, op.shift, low.res, y, c.B)
    assert not torch.isnan(y).any()
    return y


def _full(d: ce.Data) -> torch.Tensor:
    """What the whole output tensor of the launch must hold (float64): d.stored(), for a slice launch inside NaN channels."""
    want = d.stored()
    if not d.case.slice_of:
        return want
    out_c, c0 = d.case.slice_of
    full = torch.full(tuple(want.shape[:3]) + (out_c,), float("nan"), dtype=torch.float64)
    full[..., c0:c0 + d.case.c_out] = want
    return full


def _same64(a, b):
    """Bit equality of two float64 tensors, NaN and the sign of zero included."""
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


@pytest.mark.parametrize("case,dtype", PAIRS + [(c, "fp32") for c in TAP_SKIP], ids=lambda v: v if isinstance(v, str) else v.name)
def test_conditions_and_interpreter_equals_the_integer_reference(case, dtype):
    d = ce.make(case, dtype)
    print(case.name, dtype, ce.conditions(d))
    y = _interpret(d)
    want = _full(d)
    if case.hardswish or case.slice_of:    # the sign of a zero and the untouched channels count: compare the bits
        diff = y.view(torch.int64) != want.view(torch.int64)
    else:
        diff = y != want
    assert not bool(diff.any()), f"{int(diff.sum())} of {diff.numel()} differ, first at {tuple(diff.nonzero()[0].tolist())}"
    assert tuple(d.expected().shape) == tuple(d.stored().shape) and d.expected().dtype == d.store_dtype
    assert tuple(y.shape[:-1]) == tuple(d.stored().shape[:-1]) or case.nchw


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
            for f in set(fams):
                fams |= ce.detector_families(case, f)
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


# ---- the detector's epilogues ---------------------------------------------------------------------------------------------------------------------
DETECTOR_3X3 = [c for c in ce.DETECTOR_CASES if c.k == 3]


@pytest.mark.parametrize("case", DETECTOR_3X3, ids=lambda c: c.name)
def test_detector_3x3_cases_resolve_to_the_tap_skipping_kernel_where_eligible(case):
    """With the knob on, a 3x3 detector case whose c_in fills whole K tiles runs the tap-skipping kernel on every tile that holds at most two
    images' worth of one position (batch >= tile_m / 2: the batch-70 cases on the 64- and 128-row tiles), every other launch - the Focus conv
    with c_in = 12 among them - the plain kernel; with the knob off all run the plain kernel.  The library's own dispatch decides; nothing is
    launched."""
    lib = _lib.lib()
    low = ce.lower(ce.make(case, "fp32"), TorchPacker(), "cpu")
    cands = ce.candidates(low, case)
    try:
        lib.sp_conv_set_tap_skip(1)
        on = {k: ce.family(low, k, case.residual)[0] for k in cands}
        lib.sp_conv_set_tap_skip(0)
        off = {ce.family(low, k, case.residual)[0] for k in cands}
    finally:
        lib.sp_conv_set_tap_skip(1)
    want = {k: "tapskip" if (case.c_in % 32 == 0 and case.B >= k[0] // 2) else "igemm" for k in cands}
    assert on == want and off == {"igemm"}, (case.name, on, off)
    if case.B == 70:
        assert "tapskip" in on.values() and "igemm" in on.values()          # (256-row tiles: 70 < 128)


@pytest.mark.parametrize("case", [c for c in ce.DETECTOR_CASES if c.hardswish], ids=lambda c: c.name)
def test_a_mutated_hardswish_epilogue_differs_from_the_reference(case):
    """The negative self-check for the detector's epilogue: the activation applied after the residual, a quotient whose last bit is cut off, and
    a slice that lands four channels further on each store other bits than the reference, on a share of the outputs that makes the
    comparison sensitive to it."""
    d = ce.make(case, "fp32")
    bits = lambda t: t.float().contiguous().view(torch.int32)
    m = ce.make(case, "fp32", mutation="trunc_div")
    share = (bits(m.ref) != bits(d.ref)).double().mean().item()
    print(case.name, "a truncated quotient moves", share)
    assert share >= (0.02 if case.residual else 0.05)            # (with a residual, the sum's rounding hides most cut bits)
    if case.residual:
        m = ce.make(case, "fp32", mutation="act_after_res")
        inside = (d.pre.abs() < 3)
        share = (bits(m.ref) != bits(d.ref))[inside].double().mean().item()
        print(case.name, "activation after the residual moves", share, "of the outputs with |v| < 3")
        assert share >= 0.90
    if case.slice_of:
        out_c, c0 = case.slice_of
        by = 4 if c0 + case.c_out + 4 <= out_c else -4                     # (towards the side that has room)
        y, moved = _interpret(d), _interpret(d, c0_shift=by)
        assert _same64(y, _full(d)) and not _same64(moved, _full(d))
        differ = (moved.view(torch.int64) != y.view(torch.int64)).any(0).any(0).any(0)
        lo, hi = min(c0, c0 + by), max(c0, c0 + by)                        # the four channels that change hands at either end of the slice
        assert bool(differ[lo:hi].all()) and bool(differ[lo + case.c_out:hi + case.c_out].all())


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


# ---- fused launches: conditions, the per-conv chain of the descriptor interpreter, the four mutations -------------------------------------------
def _interpret_chain(d: ce.FusedData) -> dict:
    """The per-conv program of the block, launch by launch through conv_desc_cpu on TorchPacker's layouts, every buffer in the activation dtype."""
    low = ce.lower_fused(d, TorchPacker(), "cpu", fused=False)
    bufs, B = dict(low.bufs), d.case.B
    for op in low.ops:
        y = torch.full((B, op.desc.out_h, op.desc.out_w, op.desc.out_c), float("nan"), dtype=d.store_dtype)
        conv_desc_cpu(op.desc, bufs[op.src], op.w, op.scale, op.shift, bufs[op.res] if op.res else None, y, B)
        assert not torch.isnan(y).any(), op.name
        bufs[op.dst] = y
    return {n: bufs[b] for n, b in low.outs.items()}


@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: c.name)
def test_fused_conditions_and_per_conv_chain_equals_the_chain_reference(case):
    """Every fused case: its conditions hold, the per-conv chain of tests/desc_interp.py (packing, geometry and the place of every bf16 store,
    independent of the float64 chain) stores the reference's bits, and the engine's builder lowers it to the one fused op the GPU module launches."""
    d = ce.make_fused(case)
    print(case.name, ce.fused_conditions(d))
    for name, y in _interpret_chain(d).items():
        want = d.expected(name)
        assert y.dtype == want.dtype and y.shape == want.shape, (name, y.shape, want.shape)
        diff = y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32) != want.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32)
        assert not bool(diff.any()), f"{name}: {int(diff.sum())} of {diff.numel()} differ, first at {tuple(diff.nonzero()[0].tolist())}"
    low = ce.lower_fused(d, TorchPacker(), "cpu")
    assert len(low.ops) == 1
    print(case.name, "->", ce.fused_kernel_name(low, case.family))


def test_the_many_tile_cases_have_more_tiles_than_compute_units():
    for fam, case in MANY_TILES.items():
        assert case in FUSED_CASES and ce.fused_tiles(case) > CUS and (case.H % ce.FUSED_TILES[fam][0] and case.W % ce.FUSED_TILES[fam][1]), case
    assert ce.fused_tiles(MANY_TILES["bb32"], (8, 16)) > 2 * CUS           # the 8x16 kernel behind SP_BB32_W8=0 runs two workgroups per unit


def _ring(t):
    """Mask of the outermost ring of pixels of t [B, C, H, W]."""
    m = torch.zeros(t.shape[-2:], dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m.expand_as(t)


def _moved(d, m, name):
    """Where the mutated reference `m` stores other bits than the true one."""
    return m.ref[name].to(d.store_dtype) != d.ref[name].to(d.store_dtype)


@pytest.mark.parametrize("family,mutation", [(f, m) for f, (_, ms) in MUTATIONS.items() for m in ms])
def test_a_mutated_chain_differs_from_the_reference(family, mutation):
    """The negative self-check, per chain family: a reference with one of the mistakes a fused kernel can make - the intermediate outside the image
    not zero, an intermediate store that truncates, one term of a product dropped, the residual of the neighbouring pixel - stores other bits, on
    at least the share of the outputs that makes the comparison sensitive to it.  Conditions on the inputs; no kernel runs here."""
    case = ce.Fused(family, *MUTATIONS[family][0])
    o = ce.fused_operands(case)
    d = ce.fused_eval(case, o)
    ce.fused_conditions(d)
    if mutation == "drop":
        term = (5, 3, 4 if o["w1" if family == "bneck64" else "w0"].shape[-1] == 3 else 0)
        m = ce.fused_eval(case, o, drop=term)
    else:
        m = ce.fused_eval(case, o, **{mutation: True})
    final = "y_hi" if family == "htrans" else "y"
    moved = _moved(d, m, final)
    if mutation == "ring":
        share = moved[_ring(moved)].double().mean().item()
        print(family, "padding bug moves", share, "of the border ring")
        assert share >= 0.30
    elif mutation == "trunc":
        share = moved.double().mean().item()
        print(family, "truncating intermediate stores move", share, "of all outputs")
        assert share >= 0.25
    elif mutation == "shift_res":
        pos = d.pre[final] > 0
        share = moved[pos].double().mean().item()
        print(family, "the neighbour's residual moves", share, "of the positive outputs,", moved.double().mean().item(), "of all")
        assert share >= 0.60
    else:
        ch = term[0]
        only = lambda t: not bool(t[:, :ch].any()) and not bool(t[:, ch + 1:].any())
        pix = lambda t: t[:, ch:ch + 1]                                    # [B, 1, H, W]: the pixels at which channel `ch` moved
        if family == "bneck64":                                            # one product of the 3x3: t2 moves in that channel, y only at those pixels
            src = m.inter["t2"] != d.inter["t2"]
            assert only(src) and not bool((moved & ~pix(src)).any())
        elif family in ("bb32", "bb64"):                                   # conv1: t moves in that channel, y only within one pixel of it
            src = m.inter["t"] != d.inter["t"]
            near = torch.nn.functional.max_pool2d(pix(src).double(), 3, 1, 1) > 0
            assert only(src) and not bool((moved & ~near).any())
        elif family.startswith("dual"):                                    # the shortcut's product: r and y move in that channel alone
            src = m.inter["r"] != d.inter["r"]
            assert only(src) and only(moved) and not bool((moved & ~src).any())
        elif family.startswith("pwchain"):                                 # conv3: y moves in that channel, t_next only in those rows
            assert only(moved)
            nxt = _moved(d, m, "t_next")
            assert bool(nxt.any()) and not bool((nxt & ~pix(moved)).any())
        else:                                                              # transition1.0: y_hi in that channel, y_lo not at all
            assert only(moved) and not bool(_moved(d, m, "y_lo").any())
        share = moved.double().mean().item()
        print(family, "one dropped term moves", share, "of all outputs,", int(moved.sum()), "elements")
        assert int(moved.sum()) >= 1
    assert not all(torch.equal(m.ref[n], d.ref[n]) for n in d.ref)


def test_a_truncating_store_fails_transition1():
    """transition1 has one store per output and no intermediate: a store that truncates must still change bits of both outputs."""
    case = ce.Fused("htrans", *MUTATIONS["htrans"][0])
    o = ce.fused_operands(case)
    d, m = ce.fused_eval(case, o), ce.fused_eval(case, o, trunc=True)
    for n in d.ref:
        share = _moved(d, m, n).double().mean().item()
        print(n, "a truncating store differs on", share)
        assert share > 0
