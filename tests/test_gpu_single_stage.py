"""The single-stage form of the fp32 implicit GEMM at tile 128x128 (conv_igemm_single_kernel / conv_igemm_tapskip_single_kernel,
csrc/conv_igemm.hip): one LDS operand stage, two barriers per K tile, the NHWC transpose 32 accumulator rows at a time, three workgroups per CU.
Every kernel case runs one launch through the C ABI (sp_conv2d_fwd) with the form off and on in the same process (sp_conv_set_single_stage) into
NaN-prefilled buffers with guards on both sides and compares the raw bits; finite cases are also held against the CPU interpreter of the
descriptors (tests/desc_interp.conv_desc_cpu) at the bar its other users apply: 1e-4 of the largest reference magnitude."""
import ctypes

import pytest
import torch

from oracle import nets_oracle
from simple_pose_amd import _lib, conv_geometry, engine, synth
from simple_pose_amd.metrics import GaussTaylorKeyPointDecoder
from simple_pose_amd.nets import pose_resnet_dconv
from tests.desc_interp import conv_desc_cpu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 4096       # guard elements in front of and behind every output: a store outside the tensor would land here
TILE = (128, 128)
PLAIN = "conv_igemm_kernel<128, 128, 2, 2, true, false, false, false, false, false>"
TAPSKIP = "conv_igemm_tapskip_kernel<128, 128, 2, 2>"


@pytest.fixture(autouse=True)
def _knobs_back_on():
    yield
    _lib.lib().sp_conv_set_single_stage(1)
    _lib.lib().sp_conv_set_tap_skip(1)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch(d, x, w, scale, shift, res, n_out, single, inplace):
    lib = _lib.lib()
    _lib.check(lib.sp_conv_set_single_stage(int(single)), "sp_conv_set_single_stage")
    buf = torch.full((PAD + n_out + PAD,), float("nan"), dtype=torch.float32, device=DEV)
    guard = _bits(buf[:PAD]).clone()
    y = buf[PAD:PAD + n_out]
    if inplace:                                                   # the accumulate form: y holds the residual and is read before it is written
        y.copy_(res.reshape(-1))
        res = y
    p = lambda t: _lib.ptr(t) if t is not None else None
    _lib.check(lib.sp_conv2d_fwd(d, _lib.ptr(x), _lib.ptr(w), p(scale), p(shift), p(res), _lib.ptr(y), _lib.current_stream()), "sp_conv2d_fwd")
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf[:PAD]), guard) and torch.equal(_bits(buf[PAD + n_out:]), guard)       # nothing written outside the tensor
    return y


def _off_on(d, x, w, scale=None, shift=None, res=None, *, name=PLAIN, finite=True, inplace=False):
    """The launch with the single-stage form off and on: what the query says, the (unchanged) kernel name, the same bits, the interpreter."""
    lib = _lib.lib()
    B = d.batch
    assert (d.tile_m, d.tile_n) == TILE
    nchw = bool(d.flags & _lib.SP_CONV_OUT_NCHW)
    shape = (B, d.out_c, d.out_h, d.out_w) if nchw else (B, d.out_h, d.out_w, d.out_c)
    n_out = B * d.out_h * d.out_w * d.out_c
    has_res = res is not None
    lib.sp_conv_set_single_stage(0)
    assert _lib.conv_single_stage(d, has_res) is False and _lib.conv_kernel_name(d, has_res) == name
    lib.sp_conv_set_single_stage(1)
    assert _lib.conv_single_stage(d, has_res) is True and _lib.conv_kernel_name(d, has_res) == name
    off = _launch(d, x, w, scale, shift, res, n_out, False, inplace)
    on = _launch(d, x, w, scale, shift, res, n_out, True, inplace)
    diff = int((_bits(on) != _bits(off)).sum())
    assert diff == 0, f"{diff} of {n_out} elements differ between the single-stage and the double-buffered kernel"
    if finite:
        assert bool(torch.isfinite(on).all())
        ref = torch.empty(shape, dtype=torch.float32)
        c = lambda t: t.cpu() if t is not None else None
        conv_desc_cpu(d, x.cpu(), w.cpu(), c(scale), c(shift), c(res), ref, B)
        err, top = (on.view(shape).cpu() - ref).abs().max().item(), ref.abs().max().item()
        print(f"max |gpu - interpreter| {err:.3e}, largest reference magnitude {top:.3e}")
        assert top > 0 and err <= 1e-4 * top
    return on.view(shape)


def _conv(h, w, c_in, c_out, batch, k=1, stride=1, flags=0, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 131 * h + 17 * w + 7 * c_in + 3 * c_out + batch + k)
    wt = (torch.randn(c_out, c_in, k, k, generator=g) * 0.1).to(DEV)
    packed, _, _, _, k_pad = engine.HipPacker().conv(wt)
    d = conv_geometry.conv_fwd(h, w, c_in, c_out, packed.shape[0], k, k, k, k, k_pad, stride, k // 2, flags)
    d.batch, d.tile_m, d.tile_n, d.kernel = batch, TILE[0], TILE[1], _lib.SP_CONV_KERNEL_IGEMM
    x = torch.randn(batch, h, w, c_in, generator=g).to(DEV)
    return d, x, packed, g


@pytest.mark.parametrize("c_in", [32, 64, 96, 160], ids=lambda c: f"{c // 32}_k_tiles")
def test_1x1_k_loop_lengths(c_in):
    """32: one K tile - the loop body with both barriers never runs.  64: one such iteration; 96 / 160: odd counts."""
    d, x, packed, _ = _conv(1, 1, c_in, 128, 128)
    _off_on(d, x, packed)


@pytest.mark.parametrize("m", [50, 128, 129, 300])
def test_1x1_rows(m):
    """50: rows >= M masked inside the only tile.  128: one full tile.  129: a second tile with one row.  300: three tiles, the last ragged."""
    d, x, packed, _ = _conv(1, 1, 64, 128, m)
    _off_on(d, x, packed)


@pytest.mark.parametrize("c_out", [128, 256, 120])
def test_1x1_columns(c_out):
    """256: two N tiles.  120: packed to 128 rows - the lanes of the last two 16-byte chunks of a row are masked (col_ok false)."""
    d, x, packed, _ = _conv(1, 1, 64, c_out, 200)
    assert packed.shape[0] == (256 if c_out == 256 else 128)
    _off_on(d, x, packed)


def _epilogue_operands(d, g, m):
    scale = (torch.rand(d.c_out, generator=g) + 0.5).to(DEV)
    shift = torch.randn(d.c_out, generator=g).to(DEV)
    res = torch.randn(m, 1, 1, d.c_out, generator=g).to(DEV)
    return scale, shift, res


@pytest.mark.parametrize("inplace", [False, True], ids=["residual", "residual_in_place"])
def test_residual_and_relu_through_both_halves(inplace):
    """Scale, shift, residual and ReLU on three M tiles; in place: y aliases the residual (every residual load of a wave is requested before its
    first store).  Both 32-row halves of every wave's tile hold kept and clipped values."""
    d, x, packed, g = _conv(1, 1, 96, 256, 300, flags=_lib.SP_CONV_RELU, seed=1)
    scale, shift, res = _epilogue_operands(d, g, 300)
    y = _off_on(d, x, packed, scale, shift, res, inplace=inplace).view(300, 256)
    for r0 in (0, 32, 64, 96):
        half = y[r0:r0 + 32]
        assert bool((half == 0).any()) and bool((half > 0).any())


def test_no_scale_no_shift():
    d, x, packed, g = _conv(1, 1, 64, 128, 129, seed=2)
    res = torch.randn(129, 1, 1, 128, generator=g).to(DEV)
    _off_on(d, x, packed, None, None, res)


def test_non_finite_activations_in_both_halves_of_a_wave_tile():
    """Rows 5 / 40 are the first / second 32-row half of wave row 0, rows 70 / 100 those of wave row 1: an inf or a NaN activation reaches every
    channel of its own row and nothing else, with the bits of the double-buffered kernel."""
    d, x, packed, g = _conv(1, 1, 64, 128, 128, seed=3)
    scale, shift, res = _epilogue_operands(d, g, 128)
    rows = {5: float("inf"), 40: float("nan"), 70: float("nan"), 100: float("-inf")}
    for r, v in rows.items():
        x[r, 0, 0, (7 * r) % 64] = v
    y = _off_on(d, x, packed, scale, shift, res, finite=False).view(128, 128)
    bad = ~torch.isfinite(y)
    for r in rows:
        assert bool(bad[r].all())
        bad[r] = False
    assert not bool(bad.any())


@pytest.mark.parametrize("tap_skip", [1, 0], ids=["tap_skip_on", "tap_skip_off"])
@pytest.mark.parametrize("batch", [128, 64, 70, 1])
@pytest.mark.parametrize("h,w", [(3, 2), (1, 1)], ids=["3x2", "1x1"])
def test_3x3_pad1(h, w, batch, tap_skip):
    """128 / 64: whole / half tiles of one position; 70: ragged M, tiles that straddle positions; 1: tap-skip-ineligible - the plain single-stage
    kernel.  1x1 map: only the centre tap is inside the image (with tap skipping: one K tile, no loop iteration)."""
    _lib.lib().sp_conv_set_tap_skip(tap_skip)
    d, x, packed, _ = _conv(h, w, 32, 128, batch, k=3)
    _off_on(d, x, packed, name=TAPSKIP if (tap_skip and batch >= 64) else PLAIN)


@pytest.mark.parametrize("tap_skip", [1, 0], ids=["tap_skip_on", "tap_skip_off"])
@pytest.mark.parametrize("size", [5, 6], ids=["odd_5x5", "even_6x6"])
def test_3x3_stride2(size, tap_skip):
    _lib.lib().sp_conv_set_tap_skip(tap_skip)
    d, x, packed, g = _conv(size, size, 32, 128, 64, k=3, stride=2, flags=_lib.SP_CONV_RELU, seed=4)
    assert (d.grid_h, d.grid_w) == (3, 3)
    scale, shift, _ = _epilogue_operands(d, g, 1)
    res = torch.randn(64, 3, 3, 128, generator=g).to(DEV)
    _off_on(d, x, packed, scale, shift, res, name=TAPSKIP if tap_skip else PLAIN)


@pytest.mark.parametrize("tap_skip", [1, 0], ids=["tap_skip_on", "tap_skip_off"])
def test_deconv_k4s2p1_four_phases(tap_skip):
    """ConvTranspose2d(4, 2, 1) as its four 2x2-tap phases in one launch (blockIdx.y), input 2x3: each phase has its own border."""
    _lib.lib().sp_conv_set_tap_skip(tap_skip)
    g = torch.Generator().manual_seed(5)
    wt = (torch.randn(64, 128, 4, 4, generator=g) * 0.1).to(DEV)
    packed, n_pad = engine.HipPacker().deconv(wt)
    d = conv_geometry.deconv_k4s2p1_fwd(2, 3, 64, 128, n_pad)
    d.batch, d.tile_m, d.tile_n, d.kernel = 64, TILE[0], TILE[1], _lib.SP_CONV_KERNEL_IGEMM
    x = torch.randn(64, 2, 3, 64, generator=g).to(DEV)
    _off_on(d, x, packed, name=TAPSKIP if tap_skip else PLAIN)


def test_nchw_store_at_tile_n_128():
    """The NCHW store does not go through the transpose area; such a launch is tap-skip-ineligible, so it takes the plain single-stage kernel."""
    d, x, packed, g = _conv(4, 4, 32, 128, 20, k=3, flags=_lib.SP_CONV_OUT_NCHW | _lib.SP_CONV_RELU, seed=6)
    scale, shift, _ = _epilogue_operands(d, g, 1)
    y = _off_on(d, x, packed, scale, shift)
    assert tuple(y.shape) == (20, 128, 4, 4)


def test_three_workgroups_per_cu():
    """hipOccupancyMaxActiveBlocksPerMultiprocessor at the LDS size each launcher passes: the double-buffered 128x128 kernels hold two workgroups
    per CU, the single-stage ones at least three - the point of the change; a build that falls back to two fails here."""
    lib = _lib.lib()
    got = {}
    for which in range(4):
        n, lds = ctypes.c_int(-1), ctypes.c_int(-1)
        _lib.check(lib.sp_conv_igemm_resident_workgroups(which, ctypes.byref(n), ctypes.byref(lds)), "sp_conv_igemm_resident_workgroups")
        got[which] = (n.value, lds.value)
    print(got)
    assert got[0] == (2, 67584) and got[1] == (2, 67584)
    assert got[2][0] >= 3 and got[3][0] >= 3 and got[2][1] == got[3][1] == 34816


def _model():
    m = pose_resnet_dconv.resnet50(pretrained=False, num_classes=17)
    sd = synth.conditioned_state_dict(nets_oracle.state_dict_shapes_resnet50("dconv"), 6)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    m.autotune = False
    return m


def test_resnet50_dconv_program_bitwise_and_interleaved():
    """The ResNet50-DConv program, fp32, 64x64 input, batch 128, every implicit-GEMM launch that can be cut into 128x128 tiles pinned to them:
    heat maps with the single-stage form off and on bit for bit; then the same batches through InterleavedForward(depth=2) with the form on."""
    lib = _lib.lib()
    m = _model()
    dec = GaussTaylorKeyPointDecoder()
    xs = [torch.from_numpy(synth.input_images(128, 40 + i, h=64, w=64)).to(DEV) for i in range(2)]
    tinv = torch.from_numpy(synth.trans_inv_batch(128)).to(DEV)
    with torch.no_grad():
        prog = m.hip_program(xs[0])
        pinned = {op.name: (128, 128, _lib.SP_CONV_KERNEL_IGEMM) for op in prog.ops
                  if op.kind == "conv" and op.desc.n_pad % 128 == 0 and op.desc.c_in % 32 == 0 and not op.desc.c_in_group}
        prog.set_tiles(pinned, 128)
        taken = 0
        for op in prog.ops:
            if op.kind == "conv" and op.name in pinned:
                op.desc.batch = 128
                taken += _lib.conv_single_stage(op.desc, op.res is not None)
        assert taken == len(pinned) and taken >= 20, (taken, len(pinned))
        lib.sp_conv_set_single_stage(0)
        ref = [m(x).clone() for x in xs]
        ref_dec = [tuple(v.clone() for v in dec(r, tinv)) for r in ref]
        lib.sp_conv_set_single_stage(1)
        assert m.hip_program(xs[0]) is prog
        got = [m(x).clone() for x in xs]
        for a, b in zip(got, ref):
            assert torch.equal(_bits(a), _bits(b))
        inter = engine.InterleavedForward(prog, dec, depth=2)
        out = [inter(x, tinv) for x in xs]
        inter.sync()
        torch.cuda.synchronize()
    for (k, s), (rk, rs) in zip(out, ref_dec):
        assert torch.equal(k, rk) and torch.equal(s, rs)
    assert not torch.equal(ref[0], ref[1])
    inter.close()
