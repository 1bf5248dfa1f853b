"""Tap skipping of the fp32 implicit GEMM (conv_igemm_tapskip_kernel, csrc/conv_igemm.hip): rows ordered (output position, image) and the K tiles
of all-padding taps not multiplied.  Every kernel case runs one launch through the C ABI (sp_conv2d_fwd) with the path on and off in the same
process (sp_conv_set_tap_skip) and compares the raw bits; each is also held against the CPU interpreter of the descriptors
(tests/desc_interp.conv_desc_cpu) at the bar its other users apply: 1e-4 of the largest reference magnitude."""
import pytest
import torch

from oracle import nets_oracle
from simple_pose_amd import _lib, conv_geometry, engine, synth
from simple_pose_amd.metrics import GaussTaylorKeyPointDecoder
from simple_pose_amd.nets import pose_resnet_dconv
from tests.desc_interp import conv_desc_cpu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 4096       # guard elements behind every output: a store beyond the tensor would land here


@pytest.fixture(autouse=True)
def _knob_back_on():
    yield
    _lib.lib().sp_conv_set_tap_skip(1)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch(d, x, w, scale, shift, res, n_out, skip):
    lib = _lib.lib()
    _lib.check(lib.sp_conv_set_tap_skip(int(skip)), "sp_conv_set_tap_skip")
    y = torch.full((n_out + PAD,), float("nan"), dtype=torch.float32, device=DEV)
    p = lambda t: _lib.ptr(t) if t is not None else None
    _lib.check(lib.sp_conv2d_fwd(d, _lib.ptr(x), _lib.ptr(w), p(scale), p(shift), p(res), _lib.ptr(y), _lib.current_stream()), "sp_conv2d_fwd")
    torch.cuda.synchronize()
    assert torch.isnan(y[n_out:]).all()                         # nothing written behind the tensor
    return y[:n_out]


def _on_off(d, x, w, scale=None, shift=None, res=None, *, eligible=True, finite=True):
    """The launch with the path on and off: the kernel each resolves to, the same bits, and the interpreter.  Returns the output."""
    lib = _lib.lib()
    B = d.batch
    nchw = bool(d.flags & _lib.SP_CONV_OUT_NCHW)
    shape = (B, d.out_c, d.out_h, d.out_w) if nchw else (B, d.out_h, d.out_w, d.out_c)
    n_out = B * d.out_h * d.out_w * d.out_c
    lib.sp_conv_set_tap_skip(1)
    name_on = _lib.conv_kernel_name(d, res is not None)
    lib.sp_conv_set_tap_skip(0)
    name_off = _lib.conv_kernel_name(d, res is not None)
    assert name_off.startswith("conv_igemm_kernel<")
    assert name_on == (f"conv_igemm_tapskip_kernel<{d.tile_m}, {d.tile_n}, 2, 2>" if eligible else name_off), name_on
    on = _launch(d, x, w, scale, shift, res, n_out, True)
    off = _launch(d, x, w, scale, shift, res, n_out, False)
    diff = int((_bits(on) != _bits(off)).sum())
    assert diff == 0, f"{diff} of {n_out} elements differ between tap skipping on and off"
    if finite:
        assert bool(torch.isfinite(on).all())
        ref = torch.empty(shape, dtype=torch.float32)
        c = lambda t: t.cpu() if t is not None else None
        conv_desc_cpu(d, x.cpu(), w.cpu(), c(scale), c(shift), c(res), ref, B)
        err, top = (on.view(shape).cpu() - ref).abs().max().item(), ref.abs().max().item()
        print(f"max |gpu - interpreter| {err:.3e}, largest reference magnitude {top:.3e}")
        assert top > 0 and err <= 1e-4 * top
    return on.view(shape)


def _conv3x3(h, w, c_in, c_out, batch, tile, stride=1, flags=0, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 131 * h + 17 * w + c_in + batch)
    wt = (torch.randn(c_out, c_in, 3, 3, generator=g) * 0.1).to(DEV)
    packed, _, _, _, k_pad = engine.HipPacker().conv(wt)
    d = conv_geometry.conv_fwd(h, w, c_in, c_out, packed.shape[0], 3, 3, 3, 3, k_pad, stride, 1, flags)
    d.batch, d.tile_m, d.tile_n, d.kernel = batch, tile[0], tile[1], _lib.SP_CONV_KERNEL_IGEMM
    x = torch.randn(batch, h, w, c_in, generator=g).to(DEV)
    return d, x, packed, g


@pytest.mark.parametrize("c_in", [32, 64], ids=["one_k_tile_per_tap", "two_k_tiles_per_tap"])
@pytest.mark.parametrize("h,w", [(3, 2), (1, 1)], ids=["3x2_all_border", "1x1_centre_tap_only"])
def test_3x3_on_maps_without_interior(h, w, c_in):
    """3x2: every position lies on the border, the corners keep 4 of 9 taps.  1x1: only the centre tap is valid (one tap's K tiles run)."""
    d, x, packed, _ = _conv3x3(h, w, c_in, 64, 128, (64, 64))
    done, full = conv_geometry.tap_skip_k_tiles(d, 128, 64)
    assert done * 9 == full if (h, w) == (1, 1) else done < full
    _on_off(d, x, packed)


@pytest.mark.parametrize("batch", [128, 64, 70, 1])
@pytest.mark.parametrize("h,w", [(3, 2), (5, 4)], ids=["3x2", "5x4"])
def test_3x3_batches(h, w, batch):
    """128 / 64: whole tiles of one position.  70: ragged M and tiles that straddle positions (the union of their masks).  1: fewer than half a
    tile of images per position - the launch keeps the (image, position) kernel.  5x4 has interior, edge and corner positions."""
    d, x, packed, _ = _conv3x3(h, w, 64, 64, batch, (64, 64))
    _on_off(d, x, packed, eligible=batch >= 32)


@pytest.mark.parametrize("batch", [128, 70])
@pytest.mark.parametrize("tile", [(64, 64), (128, 64), (128, 128)], ids=lambda t: f"{t[0]}x{t[1]}")
def test_3x3_tiles(tile, batch):
    d, x, packed, _ = _conv3x3(5, 4, 64, 64 if tile[1] == 64 else 128, batch, tile)
    _on_off(d, x, packed)


def test_3x3_stride2_5x5_to_3x3():
    """Top and left taps fall outside at output row / column 0; on an odd map the last window also hangs one row / column over the far edge."""
    d, x, packed, _ = _conv3x3(5, 5, 64, 64, 64, (64, 64), stride=2)
    assert (d.grid_h, d.grid_w) == (3, 3)
    assert [conv_geometry.tap_mask(d, gy, gx) for gy, gx in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 2))] == [0b110110000, 0b111111000, 0b110110110, 0b111111111, 0b000011011]
    _on_off(d, x, packed)


def test_3x3_stride2_6x6_to_3x3():
    """An even map (what the network's stride-2 layers see): only the top and left taps fall outside."""
    d, x, packed, _ = _conv3x3(6, 6, 64, 64, 64, (64, 64), stride=2)
    assert (d.grid_h, d.grid_w) == (3, 3)
    assert [conv_geometry.tap_mask(d, gy, gx) for gy, gx in ((0, 0), (0, 2), (2, 0), (2, 2))] == [0b110110000, 0b111111000, 0b110110110, 0b111111111]
    _on_off(d, x, packed)


def test_deconv_k4s2p1_four_phases():
    """ConvTranspose2d(4, 2, 1) as its four 2x2-tap phases in one launch (blockIdx.y), input 2x3: each phase has its own border."""
    g = torch.Generator().manual_seed(5)
    wt = (torch.randn(64, 64, 4, 4, generator=g) * 0.1).to(DEV)
    packed, n_pad = engine.HipPacker().deconv(wt)
    d = conv_geometry.deconv_k4s2p1_fwd(2, 3, 64, 64, n_pad)
    d.batch, d.tile_m, d.tile_n, d.kernel = 64, 64, 64, _lib.SP_CONV_KERNEL_IGEMM
    x = torch.randn(64, 2, 3, 64, generator=g).to(DEV)
    done, full = conv_geometry.tap_skip_k_tiles(d, 64, 64)
    assert done < full
    _on_off(d, x, packed)


def test_residual_and_relu_through_the_permuted_rows():
    d, x, packed, g = _conv3x3(5, 4, 64, 64, 70, (64, 64), flags=_lib.SP_CONV_RELU, seed=2)
    scale = (torch.rand(64, generator=g) + 0.5).to(DEV)
    shift = torch.randn(64, generator=g).to(DEV)
    res = torch.randn(70, 5, 4, 64, generator=g).to(DEV)
    y = _on_off(d, x, packed, scale, shift, res)
    assert bool((y == 0).any()) and bool((y > 0).any())


@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_non_finite_activation_in_a_border_pixel(value):
    """An in-image value is never skipped: the inf / NaN reaches every output its taps cover, exactly as with the full K loop."""
    d, x, packed, _ = _conv3x3(5, 4, 64, 64, 64, (64, 64), seed=3)
    x[7, 0, 0, 5] = value
    x[9, 4, 3, 63] = value
    y = _on_off(d, x, packed, finite=False)
    bad = ~torch.isfinite(y)
    assert bool(bad[7, :2, :2].all()) and bool(bad[9, 3:, 2:].all())
    bad[7, :2, :2] = False
    bad[9, 3:, 2:] = False
    assert not bool(bad.any())


def test_nchw_store_is_not_eligible():
    d, x, packed, _ = _conv3x3(4, 4, 64, 64, 64, (64, 64), flags=_lib.SP_CONV_OUT_NCHW, seed=4)
    _on_off(d, x, packed, eligible=False)


def _model():
    m = pose_resnet_dconv.resnet50(pretrained=False, num_classes=17)
    sd = synth.conditioned_state_dict(nets_oracle.state_dict_shapes_resnet50("dconv"), 6)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    m.autotune = False
    return m


def test_resnet50_dconv_program_bitwise_and_interleaved():
    """The ResNet50-DConv program, fp32, 64x64 input, batch 128: heat maps with the path on and off bit for bit; then the same batches through
    InterleavedForward(depth=2) with the path on."""
    lib = _lib.lib()
    m = _model()
    dec = GaussTaylorKeyPointDecoder()
    xs = [torch.from_numpy(synth.input_images(128, 40 + i, h=64, w=64)).to(DEV) for i in range(2)]
    tinv = torch.from_numpy(synth.trans_inv_batch(128)).to(DEV)
    with torch.no_grad():
        lib.sp_conv_set_tap_skip(0)
        ref = [m(x).clone() for x in xs]
        ref_dec = [tuple(v.clone() for v in dec(r, tinv)) for r in ref]
        lib.sp_conv_set_tap_skip(1)
        prog = m.hip_program(xs[0])
        names = []
        for op in prog.ops:
            if op.kind == "conv" and not op.direct and op.desc.kernel == _lib.SP_CONV_KERNEL_IGEMM:
                op.desc.batch = 128
                names.append(_lib.conv_kernel_name(op.desc, op.res is not None))
        assert sum(n.startswith("conv_igemm_tapskip_kernel<") for n in names) >= 10, names
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
