"""sp_pw_chain_f32 (csrc/conv_pw.hip, round 7): conv3 (+ bn3 + residual + relu) of an identity Bottleneck with 64 mid channels and the next block's conv1
(+ bn1 + relu) as one launch - the kernel against the two sp_conv2d_fwd launches it replaces, the lowered programs with and without the fusion, and the
host-side rules of the switch.  The tests marked `gpu` need the MI355X; the others run anywhere."""
import ctypes

import pytest
import torch

from oracle import nets_oracle
from simple_pose_amd import _lib, engine, synth
from simple_pose_amd.metrics import GaussTaylorKeyPointDecoder
from simple_pose_amd.nets import pose_resnet_dconv, pose_resnet_duc
from tests.desc_interp import TorchPacker

DEV = "cuda:0"
PAD = 64         # guard rows behind every output: a store at or beyond `rows` would land here


def _chain_operands(rows, c_next, poison):
    t = torch.from_numpy(synth.tensor_normal(9, "chain/t", (rows, 64)))
    x = torch.from_numpy(synth.tensor_normal(9, "chain/x", (rows, 256)))
    if poison:
        t[123, 5] = float("inf")
        t[700, 17] = float("nan")
    w3 = torch.from_numpy(synth.tensor_normal(9, "chain/w3", (256, 64, 1, 1), std=0.2))
    w1 = torch.from_numpy(synth.tensor_normal(9, f"chain/w1_{c_next}", (c_next, 256, 1, 1), std=0.2))
    s3, h3 = (torch.from_numpy(synth.tensor_uniform(9, "chain/" + n, (256,), lo, hi)).float().to(DEV) for n, lo, hi in (("s3", 0.5, 1.5), ("h3", -0.3, 0.3)))
    s1, h1 = (torch.from_numpy(synth.tensor_uniform(9, f"chain/{n}_{c_next}", (c_next,), lo, hi)).float().to(DEV)
              for n, lo, hi in (("s1", 0.5, 1.5), ("h1", -0.3, 0.3)))
    return t, x, w3, w1, s3, h3, s1, h1


@pytest.mark.gpu
@pytest.mark.parametrize("c_next", [64, 128])
@pytest.mark.parametrize("rows,poison", [(50, False), (64 * 9, False), (1000, False), (64 * 700 + 3, False), (1000, True)],
                         ids=["below_one_tile", "whole_tiles", "ragged", "many_tiles_ragged", "ragged_inf_nan"])
def test_pw_chain_equals_the_two_launches_bitwise(rows, poison, c_next):
    """y and t_next of one sp_pw_chain_f32 launch against conv3 (scale, shift, residual, ReLU) followed by conv1 (scale, shift, ReLU) through
    sp_conv2d_fwd on the default tiled kernel: bit for bit, an inf and a NaN in `t` included (the chained product then runs on a row of y that
    holds infinities), and nothing written at or beyond `rows`."""
    lib = _lib.lib()
    t, x, w3, w1, s3, h3, s1, h1 = _chain_operands(rows, c_next, poison)
    b = engine.ProgramBuilder(1, rows, dtype="fp32")                     # a [1 x rows] "image"
    b.p.shapes["t"] = (1, rows, 64)
    b.p.shapes["x"] = (1, rows, 256)
    y = b.conv("t", w3.to(DEV), scale=s3, shift=h3, relu=True, res="x", name="c3")
    b.conv(y, w1.to(DEV), scale=s1, shift=h1, relu=True, name="c1")
    ops = {o.name: o for o in b.p.ops}
    assert ops["c3"].desc.kernel == _lib.SP_CONV_KERNEL_IGEMM and ops["c1"].desc.kernel == _lib.SP_CONV_KERNEL_IGEMM
    tg, xg = t.to(DEV), x.to(DEV)
    nan = lambda c: torch.full((rows + PAD, c), float("nan"), dtype=torch.float32, device=DEV)
    y2, t2, y1, t1 = nan(256), nan(c_next), nan(256), nan(c_next)
    for o, src, res, dst in ((ops["c3"], tg, xg, y2), (ops["c1"], y2, None, t2)):
        o.desc.batch = 1
        _lib.check(lib.sp_conv2d_fwd(o.desc, _lib.ptr(src), _lib.ptr(o.w), _lib.ptr(o.scale), _lib.ptr(o.shift), _lib.ptr(res) if res is not None else None,
                                     _lib.ptr(dst), _lib.current_stream()), o.name)
    assert lib.sp_pw_chain_f32_ok(rows, 64, 256, c_next) == 1
    _lib.check(lib.sp_pw_chain_f32(_lib.ptr(tg), _lib.ptr(ops["c3"].w), _lib.ptr(s3), _lib.ptr(h3), _lib.ptr(xg), _lib.ptr(y1), _lib.ptr(ops["c1"].w),
                                   _lib.ptr(s1), _lib.ptr(h1), _lib.ptr(t1), rows, 64, 256, c_next, _lib.current_stream()), "pw chain")
    torch.cuda.synchronize()
    for one, two in ((y1, y2), (t1, t2)):
        assert torch.isnan(one[rows:]).all() and torch.isnan(two[rows:]).all()           # no row at or beyond `rows` was written
        assert not torch.isnan(one[:rows]).any()                                         # every row below was (ReLU: `v > 0 ? v : 0` stores 0 for a NaN)
        assert torch.equal(one[:rows].view(torch.int32), two[:rows].view(torch.int32)), int((one[:rows].view(torch.int32) != two[:rows].view(torch.int32)).sum())
    if poison:
        assert torch.isinf(y1[123]).any() and not y1[700].any()           # the inf reaches y and the chained product; the NaN row is all zeros after ReLU
    else:
        ref = torch.relu((t.double() @ w3.double().view(256, 64).T) * s3.cpu().double() + h3.cpu().double() + x.double())
        assert float((y1[:rows].cpu().double() - ref).abs().max() / ref.abs().max()) < 2e-6          # (the bar of the dual-tail test)
        # t_next against float64, element by element: a 256-term fp32 dot product, one scale and one shift err by at most (256 + 3) * 2^-24 times
        # the sum of the magnitudes (Higham, gamma_n), plus what the error already in y contributes; ReLU does not increase a difference
        w1a, s1a, h1a = w1.double().view(c_next, 256).abs(), s1.cpu().double().abs(), h1.cpu().double().abs()
        ey = (y1[:rows].cpu().double() - ref).abs()
        ref1 = torch.relu((ref @ w1.double().view(c_next, 256).T) * s1.cpu().double() + h1.cpu().double())
        bound = 259 * 2.0 ** -24 * (((ref + ey) @ w1a.T) * s1a + h1a) + (ey @ w1a.T) * s1a
        assert bool(((t1[:rows].cpu().double() - ref1).abs() <= bound).all())


def _model(head, seed=6):
    m = {"dconv": pose_resnet_dconv, "duc": pose_resnet_duc}[head].resnet50(pretrained=False, num_classes=17)
    sd = synth.conditioned_state_dict(nets_oracle.state_dict_shapes_resnet50(head), seed)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    m.autotune = False
    return m


CHAIN_NAMES = ["layer1.1.conv3+layer1.2.conv1", "layer1.2.conv3+layer2.0.conv1"]


@pytest.mark.gpu
@pytest.mark.parametrize("fuse_bottlenecks", [False, True], ids=["per_conv", "dual_tail"])
@pytest.mark.parametrize("head,B,H,W", [("dconv", 3, 256, 192), ("duc", 1, 96, 160)])
def test_fp32_pw_chain_program_equals_the_unchained_program_bitwise(head, B, H, W, fuse_bottlenecks):
    """`fuse_chain` (the models' default) against the program without it, for both values of `fuse_bottlenecks`: the same heat maps bit for bit, exactly
    the two named `pwchain` ops, two ops fewer, the same algorithmic FLOPs."""
    m = _model(head)
    m.fuse_bottlenecks = fuse_bottlenecks
    x = torch.from_numpy(synth.input_images(B, 23, h=H, w=W)).to(DEV)
    assert type(m).fuse_chain is True
    with torch.no_grad():
        m.fuse_chain = False
        ref = m(x).clone()
        p0 = m.hip_program(x)
        n_ref, flops_ref = len(p0.ops), p0.flops_per_image
        assert not any(op.kind == "pwchain" for op in p0.ops)
        m.fuse_chain = True
        got = m(x)
        prog = m.hip_program(x)
    assert prog is not p0                                                # (the switch is part of the program cache key)
    assert [op.name for op in prog.ops if op.kind == "pwchain"] == CHAIN_NAMES and len(prog.ops) == n_ref - 2
    assert not any(op.name in ("layer1.1.conv3", "layer1.2.conv1", "layer1.2.conv3", "layer2.0.conv1") for op in prog.ops)
    assert prog.flops_per_image == flops_ref
    assert torch.equal(got, ref)


@pytest.mark.gpu
def test_fp32_pw_chain_program_through_interleaved_forward():
    """The chained program on two streams with their own activation pools (engine.InterleavedForward(depth=2), bench.py's default mode for the
    headline): key points and scores of four different batches equal the unchained program + decoder bit for bit."""
    m = _model("dconv")
    dec = GaussTaylorKeyPointDecoder()
    xs = [torch.from_numpy(synth.input_images(3, 60 + i)).to(DEV) for i in range(4)]
    tinv = torch.from_numpy(synth.trans_inv_batch(3)).to(DEV)
    with torch.no_grad():
        m.fuse_chain = False
        ref = [tuple(v.clone() for v in dec(m(x), tinv)) for x in xs]
        m.fuse_chain = True
        prog = m.hip_program(xs[0])
        assert sum(op.kind == "pwchain" for op in prog.ops) == 2
        inter = engine.InterleavedForward(prog, dec, depth=2)
        got = [inter(x, tinv) for x in xs]
        inter.sync()
        torch.cuda.synchronize()
    for (k, s), (rk, rs) in zip(got, ref):
        assert torch.equal(k, rk) and torch.equal(s, rs)
    assert not torch.equal(ref[0][0], ref[1][0])
    inter.close()


# ---------------------------------------------------------------------------------------------- host side (no GPU)
def _cpu_sd(head="dconv"):
    return {k: torch.from_numpy(v) for k, v in synth.conditioned_state_dict(nets_oracle.state_dict_shapes_resnet50(head), seed=3).items()}


def test_lowering_defaults_emit_no_pw_chain():
    """engine.resnet_program's own default is off (the CPU interpreter of the host tests lowers with it); bf16 programs never carry the op."""
    sd = _cpu_sd()
    prog = engine.resnet_program(sd, "dconv", in_h=64, in_w=64, packer=TorchPacker())
    assert not any(op.kind == "pwchain" for op in prog.ops)
    for fb in (False, True):
        p16 = engine.resnet_program(sd, "dconv", in_h=64, in_w=64, dtype="bf16", packer=TorchPacker(), fuse_bottlenecks=fb, fuse_chain=True)
        assert not any(op.kind == "pwchain" for op in p16.ops)
    assert pose_resnet_dconv.resnet50(pretrained=False, num_classes=17).fuse_chain is True


def test_pw_chain_rejects_bad_arguments_without_touching_the_gpu():
    lib = _lib.lib()
    ptrs = lambda: [ctypes.c_void_p(16 * (i + 1)) for i in range(10)]        # t, w3, scale3, shift3, residual, y, w1, scale1, shift1, t_next
    a = ptrs()
    a[9] = None
    assert lib.sp_pw_chain_f32(*a, 1000, 64, 256, 64, None) == -1 and b"null" in lib.sp_last_error()
    a = ptrs()
    a[0] = None
    assert lib.sp_pw_chain_f32(*a, 1000, 64, 256, 128, None) == -1 and b"null" in lib.sp_last_error()
    assert lib.sp_pw_chain_f32(*ptrs(), 1000, 64, 256, 96, None) == -1 and b"64 or 128" in lib.sp_last_error()
    assert lib.sp_pw_chain_f32(*ptrs(), 1000, 128, 256, 64, None) == -1 and lib.sp_pw_chain_f32(*ptrs(), 1000, 64, 512, 64, None) == -1
    a = ptrs()
    a[5] = a[4]                                                              # y on the residual
    assert lib.sp_pw_chain_f32(*a, 1000, 64, 256, 64, None) == -1 and b"alias" in lib.sp_last_error()
    a = ptrs()
    a[9] = a[5]                                                              # t_next on y
    assert lib.sp_pw_chain_f32(*a, 1000, 64, 256, 64, None) == -1 and b"alias" in lib.sp_last_error()
    assert [lib.sp_pw_chain_f32_ok(1000, 64, 256, n) for n in (64, 128, 96, 256)] == [1, 1, 0, 0]
    assert lib.sp_pw_chain_f32_ok(0, 64, 256, 64) == 0 and lib.sp_pw_chain_f32_ok(1 << 22, 64, 256, 64) == 0
