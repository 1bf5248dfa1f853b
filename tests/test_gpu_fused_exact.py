"""The launches that run several convolutions at once against exact integer chains, bit for bit (tests/conv_exact.py: Fused): sp_bottleneck_c64,
sp_basic_block_c32 / _c64, sp_dual_pw_bf16 / _f32, sp_pw_chain_f32 and sp_hrnet_transition1, each called directly through the C ABI on the maps where
its tiling can go wrong - one pixel, below one tile, exactly one tile, ragged in both directions, more tiles than compute units.  Small integer
operands, power-of-two scales and integer shifts make every fp32 partial sum of every stage exact in any order, so a float64 chain on the CPU that
rounds where the per-conv program stores predicts every stored bit - of transition1 too, whose reduction order differs from the two launches.
There is no tolerance in this module: every comparison is torch.equal on the stored bits.  tests/test_conv_exact_host.py holds the case tables, their
conditions, the proof of the chain reference against the descriptor interpreter and the mutations the comparison must catch (no GPU)."""
import os
import re
import subprocess
import sys

import pytest
import torch

from simple_pose_amd import _lib, engine
from tests import conv_exact as ce
from tests.test_conv_exact_host import FUSED_CASES, FUSED_SHAPES, MANY_TILES
from tests.test_gpu_conv_exact import DEV, _guarded, _same_bits, _take

pytestmark = pytest.mark.gpu

P = _lib.ptr
# the knobs are read once per process (csrc/conv_bneck.hip, csrc/conv_block.hip): what this process runs follows from its environment
_lead = re.match(r"\s*[+-]?\d+", os.environ.get("SP_BNECK_W8", "1"))             # (atoi)
BNECK_W8 = bool(_lead) and int(_lead.group()) != 0
BB32_W8 = not os.environ.get("SP_BB32_W8", "1").startswith("0")
EXPECTED_KERNEL = {"bneck64": "bottleneck_c64_w8_kernel" if BNECK_W8 else "bottleneck_c64_kernel",
                   "bb32": "basic_block_c32_w8_kernel" if BB32_W8 else "basic_block_c32_kernel", "bb64": "basic_block_c64_kernel"}
ENTRY = {"bneck64": "sp_bottleneck_c64", "bb32": "sp_basic_block_c32", "bb64": "sp_basic_block_c64", "dual_bf16": "sp_dual_pw_bf16",
         "dual_f32": "sp_dual_pw_f32", "pwchain64": "sp_pw_chain_f32", "pwchain128": "sp_pw_chain_f32", "htrans": "sp_hrnet_transition1"}
CHILD = "SP_FUSED_EXACT_CHILD"     # set in the environment of the child runs of test_kernels_behind_the_knobs_store_the_exact_bits
SEEN = {}        # family -> {kernel name: cases that stored exact bits in this process}


def _launch(lib, fam, op, bufs, outs, B, st):
    """The entry point of `fam` with the arguments engine.Program._launch gives it; `outs`: output name -> guarded flat tensor."""
    if fam in ("bb32", "bb64"):
        w2, scale2, shift2 = op.args
        fn = lib.sp_basic_block_c32 if fam == "bb32" else lib.sp_basic_block_c64
        return fn(op.desc, P(bufs[op.src]), P(op.w), P(op.scale), P(op.shift), P(w2), P(scale2), P(shift2), P(outs["y"]), st)
    if fam == "bneck64":
        w1, s1, h1, w3, s3, h3 = op.args
        return lib.sp_bottleneck_c64(op.desc, P(bufs[op.src]), P(w1), P(s1), P(h1), P(op.w), P(op.scale), P(op.shift), P(w3), P(s3), P(h3), P(outs["y"]), st)
    if fam in ("dual_bf16", "dual_f32"):
        w_s, s_s, h_s, rows_per_image, relu = op.args
        fn = lib.sp_dual_pw_bf16 if fam == "dual_bf16" else lib.sp_dual_pw_f32
        assert (op.w.element_size() == 2) == (fam == "dual_bf16")
        return fn(P(bufs[op.src]), P(op.w), P(op.scale), P(op.shift), P(bufs[op.res]), P(w_s), P(s_s), P(h_s), P(outs["y"]), B * rows_per_image, 64, 64, 256, relu, st)
    if fam in ("pwchain64", "pwchain128"):
        w1, s1, h1, rows_per_image, c_next, _ = op.args
        assert c_next == ce.FAMILIES[fam]["c_next"]
        return lib.sp_pw_chain_f32(P(bufs[op.src]), P(op.w), P(op.scale), P(op.shift), P(bufs[op.res]), P(outs["y"]), P(w1), P(s1), P(h1), P(outs["t_next"]),
                                   B * rows_per_image, 64, 256, c_next, st)
    assert fam == "htrans", fam
    h, w, k_pad, wb, sb, hb, _ = op.args
    return lib.sp_hrnet_transition1(P(bufs[op.src]), B, h, w, P(op.w), k_pad, P(op.scale), P(op.shift), P(wb), P(sb), P(hb), P(outs["y_hi"]), P(outs["y_lo"]), st)


def _run(case):
    """One fused case: lowered as the engine lowers it, launched once on NaN-prefilled outputs with guard elements behind them; every element
    written, nothing stored behind a tensor, the exact bits in every output, the inputs untouched.  Returns the kernel that ran."""
    lib, st, fam = _lib.lib(), _lib.current_stream(), case.family
    d = ce.make_fused(case)
    ce.fused_conditions(d)                         # a changed generator cannot silently empty the case
    low = ce.lower_fused(d, engine.HipPacker(), DEV)
    op = low.ops[0]
    name = ce.fused_kernel_name(low, fam)
    if fam in EXPECTED_KERNEL:
        assert name == EXPECTED_KERNEL[fam], (name, EXPECTED_KERNEL[fam])
    want = {n: d.expected(n) for n in d.ref}
    outs = {n: _guarded(w.numel(), d.store_dtype) for n, w in want.items()}
    before = {n: t.clone() for n, t in low.bufs.items()}
    _lib.check(_launch(lib, fam, op, low.bufs, outs, case.B, st), case.name)
    for n, w in want.items():
        what = f"{case.name} {n} ({name})"
        _same_bits(_take(outs[n], w.numel(), w.shape, what), w, what)
    for n, t in before.items():
        _same_bits(low.bufs[n], t, f"{case.name}: input {n} after the launch")
    SEEN.setdefault(fam, {}).setdefault(name, []).append(case.name)
    return name


def _cases(*families):
    return [c for c in FUSED_CASES if c.family in families]


def _more_tiles_than_units(case, tile=None, per_unit=1):
    """The case whose workgroups must take a second tile: on a part with more compute units it fails here instead of quietly covering nothing."""
    units = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = ce.fused_tiles(case, tile)
    assert tiles > per_unit * units, (case.name, tiles, units)


@pytest.mark.parametrize("case", _cases("bneck64"), ids=lambda c: c.name)
def test_bottleneck_c64_stores_the_exact_bits(case):
    if case == MANY_TILES["bneck64"]:
        _more_tiles_than_units(case)               # 280 tiles of 16x8 on 17x9 maps: second tiles cross an image boundary and are ragged
    print(case.name, "->", _run(case))


@pytest.mark.parametrize("case", _cases("bb32"), ids=lambda c: c.name)
def test_basic_block_c32_stores_the_exact_bits(case):
    if case == MANY_TILES["bb32"]:                 # (the 8x16 kernel behind SP_BB32_W8=0 runs two workgroups per unit)
        _more_tiles_than_units(case, None if BB32_W8 else (8, 16), 1 if BB32_W8 else 2)
    print(case.name, "->", _run(case))


@pytest.mark.parametrize("case", _cases("bb64"), ids=lambda c: c.name)
def test_basic_block_c64_stores_the_exact_bits(case):
    if case == MANY_TILES["bb64"]:
        _more_tiles_than_units(case)
    print(case.name, "->", _run(case))


@pytest.mark.parametrize("case", _cases("dual_bf16", "dual_f32"), ids=lambda c: c.name)
def test_dual_pointwise_tail_stores_the_exact_bits(case):
    """bf16: the shortcut value bn_d(x . Wd) is rounded to bf16 before it is added (include/simple_pose_hip.h); fp32: nothing is rounded."""
    print(case.name, "->", _run(case))


@pytest.mark.parametrize("case", _cases("pwchain64", "pwchain128"), ids=lambda c: c.name)
def test_pw_chain_stores_the_exact_bits_in_both_outputs(case):
    print(case.name, "->", _run(case))


@pytest.mark.parametrize("case", _cases("htrans"), ids=lambda c: c.name)
def test_hrnet_transition1_stores_the_exact_bits_in_both_outputs(case):
    """The reduction order (chunk, tap, channel) is not the two launches'; with exact partial sums the stored bits do not depend on it."""
    print(case.name, "->", _run(case))


def test_every_fused_entry_point_ran():
    """The coverage condition: every listed entry point stored exact bits in this process on every case of its table (cases that have not run yet run
    here), the Bottleneck and the 32-channel block through the kernel this process's knobs select - the eight-wave / strip kernel by default."""
    for case in FUSED_CASES:
        if case.name not in [n for names in SEEN.get(case.family, {}).values() for n in names]:
            _run(case)
    for fam, shapes in FUSED_SHAPES.items():
        ran = SEEN[fam]
        assert sum(len(v) for v in ran.values()) == len(shapes) and len(ran) == 1, (fam, ran)
        print(ENTRY[fam], {k: len(v) for k, v in ran.items()})
    assert set(ENTRY[f] for f in SEEN) == set(ENTRY.values())
    assert list(SEEN["bneck64"]) == [EXPECTED_KERNEL["bneck64"]] and list(SEEN["bb32"]) == [EXPECTED_KERNEL["bb32"]]
    if "SP_BNECK_W8" not in os.environ and "SP_BB32_W8" not in os.environ:
        assert list(SEEN["bneck64"]) == ["bottleneck_c64_w8_kernel"] and list(SEEN["bb32"]) == ["basic_block_c32_w8_kernel"]


@pytest.mark.parametrize("knob,selector,kernel", [("SP_BNECK_W8", "test_bottleneck_c64_stores_the_exact_bits", "bottleneck_c64_kernel"),
                                                  ("SP_BB32_W8", "test_basic_block_c32_stores_the_exact_bits", "basic_block_c32_kernel")],
                         ids=["four_wave_bottleneck", "8x16_basic_block"])          # (ids without the selector: `-k` matches ids too)
def test_kernels_behind_the_knobs_store_the_exact_bits(knob, selector, kernel):
    """The four-wave Bottleneck (SP_BNECK_W8=0) and the 8x16 BasicBlock kernel (SP_BB32_W8=0) stay in the library for same-box A/Bs; the knobs are
    read once per process, so a fresh interpreter runs this module's cases of that entry point on them.  Each case in the child asserts, through
    sp_conv2d_kernel_name, that the kernel its environment selects is the one that ran; the names it prints are read back here."""
    assert CHILD not in os.environ, "a child run must never select this test: it would start a child of its own"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **{knob: "0", CHILD: "1"})
    selector += " and not test_kernels_behind_the_knobs"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-m", "gpu", "-k", selector], env=env, capture_output=True,
                       text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    ran = [ln.split("-> ")[1].strip() for ln in r.stdout.splitlines() if "-> " in ln]
    assert len(ran) == len(FUSED_SHAPES["bneck64" if knob == "SP_BNECK_W8" else "bb32"]) and set(ran) == {kernel}, r.stdout[-2000:]
