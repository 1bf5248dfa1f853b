"""TEST HELPER: convolutions whose every output bit is known in advance.

Operands are small non-zero integers: exact in bf16 and fp32, every product and every partial sum an integer below 2^24, so an fp32 accumulator
holds the exact result in any reduction order, on any tile, in any kernel.  The epilogue (a power-of-two scale, an integer shift and residual,
ReLU) stays exact; the one inexact step left is the final store, whose bits are unique: round-to-nearest-even of the exact value.  A float64
torch convolution therefore predicts every stored bit of every launch - one wrong, missing or doubled term in one element is a mismatch.

The launches that run several convolutions at once (Fused, below) are chains of such stages: each stage's pre-store value is exact, so its store
rounding is unique, and so is everything after it.

tests/test_conv_exact_host.py holds the case tables against the descriptor interpreter (no GPU), tests/test_gpu_conv_exact.py the kernels that run
one convolution, tests/test_gpu_fused_exact.py the fused ones.
"""
import zlib
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from simple_pose_amd import _lib, engine

LIMIT = float(2 ** 24)


def ints(shape, max_mag, generator):
    """Integer-valued float64 tensor with values in {-max_mag..-1, 1..max_mag}: never 0, so a dropped term moves the exact sum by at least 1."""
    mag = torch.randint(1, max_mag + 1, tuple(shape), generator=generator)
    sign = torch.randint(0, 2, tuple(shape), generator=generator) * 2 - 1
    return (mag * sign).double()


def generator(name: str, salt: int = 0) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) + salt)


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                          # "conv" | "deconv" (ConvTranspose2d k4 s2 p1) | "stem" (3 -> c_out on the NHWC4 image)
    B: int
    H: int
    W: int
    c_in: int
    c_out: int
    k: int = 1
    stride: int = 1
    pad: int = 0
    x_mag: int = 1
    w_mag: int = 1
    groups: int = 1
    scale: bool = True                 # per-channel power of two from {0.5, 1, 2}; False: no scale pointer at all
    shift: bool = True
    shift_bias: int = 0                # added to every channel's shift (integers in +-4): moves the share of outputs that ReLU keeps
    residual: bool = False
    relu: bool = False
    nchw: bool = False
    pshuf: bool = False
    out_f32: bool = False              # bf16 operands with SP_CONV_OUT_F32: exact with no store rounding at all
    inplace: bool = False              # residual == y: the accumulate form of the input-gradient launches (implicit GEMM only)
    role: str = "index"                # "index": sums below 256, a change of one term changes the stored bf16 | "rounding": ties and inexact sums
    dtypes: Tuple[str, ...] = ("fp32", "bf16")
    w_even_bf16: Optional[int] = None  # the bf16 stem reads pixel pairs: its image width must be even
    # ---- the detector's epilogues (fp32 only) ----
    hardswish: bool = False            # SP_CONV_HARDSWISH: y = hardswish(scale * conv + shift), the residual added AFTER the activation
    slice_of: Optional[Tuple[int, int]] = None     # SP_CONV_OUT_SLICE: (out_c, c0) - the launch writes channels [c0, c0 + c_out) of an out_c-channel tensor
    scales: Optional[Tuple[float, ...]] = None     # per-channel powers of two to draw from instead of {0.5, 1, 2}: a hardswish case needs small values
    head: Optional[Tuple[int, int]] = None         # (anchors, no): the detector's head conv - bias, no activation, every anchor's `no` rows padded
    #                                                to engine.yolo_anchor_stride(no) with zero rows (c_out = anchors * that stride)

    def width(self, dtype: str) -> int:
        return self.w_even_bf16 if (dtype == "bf16" and self.w_even_bf16) else self.W


_C3 = Case("c3_64_res_relu", "conv", 3, 13, 11, 64, 64, 3, 1, 1, 2, 2, residual=True, relu=True)
_C7 = Case("c3_512_128_k4608", "conv", 1, 8, 6, 512, 128, 3, 1, 1, 1, 1)

# Magnitudes per depth K (sum variance = K * E[x^2] * E[w^2]): the largest scaled sum stays a few hundred, so that at least 90 % of the outputs
# lie below 256, where bf16 holds every integer (conditions() asserts it on the reference of each case).
FORWARD_CASES = [
    Case("pw_64_256_res_relu", "conv", 3, 9, 7, 64, 256, x_mag=3, w_mag=3, residual=True, relu=True),     # M = 189 < one tile; fp32 streaming 1x1 kernel
    Case("pw_256_64", "conv", 2, 9, 7, 256, 64, x_mag=2, w_mag=2),
    _C3,                                                                                                  # direct (64) and ring
    Case("c3_32", "conv", 2, 8, 16, 32, 32, 3, 1, 1, 2, 2, relu=True),                                    # direct (32)
    Case("c3_128_res", "conv", 1, 7, 5, 128, 128, 3, 1, 1, 1, 1, residual=True),                          # direct (128)
    Case("c3s2_192_128", "conv", 5, 17, 9, 192, 128, 3, 2, 1, 1, 1, relu=True),                           # odd sizes, stride 2, c_in % 64 != 0
    Case("pw_s2_256_512", "conv", 2, 9, 7, 256, 512, 1, 2, 0, 2, 2),                                      # projection shortcut
    _C7,                                                                                                  # ragged M, deep K
    Case("pw_2048_512", "conv", 2, 4, 3, 2048, 512, x_mag=1, w_mag=1, relu=True),
    Case("pw_256_512_res", "conv", 2, 31, 23, 256, 512, x_mag=2, w_mag=2, residual=True, relu=True),      # K = 4 ring tiles: the ring wraps inside every tile
    Case("c3_128_17_nchw", "conv", 2, 6, 5, 128, 17, 3, 1, 1, 1, 1, nchw=True),                           # ragged N, the final-layer store
    Case("pw_64_17_nchw", "conv", 2, 6, 5, 64, 17, x_mag=3, w_mag=3, nchw=True),
    Case("pw_64_17_nhwc", "conv", 2, 6, 5, 64, 17, x_mag=3, w_mag=3, dtypes=("fp32",)),                   # (bf16 NHWC stores need c_out % 8 == 0)
    Case("c3_128_512_pshuf", "conv", 2, 6, 5, 128, 512, 3, 1, 1, 1, 1, relu=True, pshuf=True),            # scale / shift in row_perm order
    Case("deconv_256_256", "deconv", 3, 7, 5, 256, 256, 4, 2, 1, 1, 1, relu=True),                        # 4 phases
    Case("g32_128_s1", "conv", 3, 12, 10, 128, 128, 3, 1, 1, 3, 3, groups=32),
    Case("g32_128_s2", "conv", 3, 12, 10, 128, 128, 3, 2, 1, 3, 3, groups=32, relu=True),
    Case("stem7_3_64", "stem", 2, 33, 47, 3, 64, 7, 2, 3, 8, 1, relu=True, w_even_bf16=46),               # integer "pixels" up to 8
    replace(_C3, name="c3_64_f32out", out_f32=True, dtypes=("bf16",)),
    replace(_C7, name="c3_512_128_k4608_f32out", out_f32=True, dtypes=("bf16",)),
    replace(_C3, name="c3_64_inplace", inplace=True),
    Case("round_c3_128", "conv", 2, 9, 7, 128, 128, 3, 1, 1, 8, 8, scale=False, residual=True, role="rounding"),
    Case("round_c3_128_relu", "conv", 2, 9, 7, 128, 128, 3, 1, 1, 8, 8, scale=False, shift_bias=600, residual=True, relu=True, role="rounding"),
    # the rounding case again on every other store path a bf16 launch can take: the 64- and 32-channel direct kernels, the ring on a 1x1 layer,
    # the fused PixelShuffle store, the four phases of the transposed convolution, the pixel-pair stem
    Case("round_c3_64", "conv", 2, 9, 7, 64, 64, 3, 1, 1, 8, 8, scale=False, residual=True, role="rounding"),
    Case("round_c3_32", "conv", 2, 9, 7, 32, 32, 3, 1, 1, 12, 12, scale=False, residual=True, role="rounding"),
    Case("round_pw_256_512", "conv", 2, 9, 7, 256, 512, x_mag=12, w_mag=12, scale=False, residual=True, role="rounding"),
    Case("round_pshuf_128_512", "conv", 2, 6, 5, 128, 512, 3, 1, 1, 8, 8, scale=False, pshuf=True, role="rounding"),
    Case("round_deconv_256", "deconv", 1, 7, 5, 256, 256, 4, 2, 1, 8, 8, scale=False, role="rounding"),
    Case("round_stem7", "stem", 2, 33, 47, 3, 64, 7, 2, 3, 16, 8, scale=False, role="rounding", w_even_bf16=46),
]

# ---- the YOLOv5 detector's convolutions: hardswish (before the residual) and the channel-slice store, fp32 only ----------------------------------
# Magnitudes of 1 and scales of 1/8 .. 1/2 keep the pre-activation v (exact: a multiple of 1/8) within a few units of 0, where hardswish is not
# the identity; conditions() asserts the shares on the reference of each case.
_HS = dict(kind="conv", x_mag=1, w_mag=1, hardswish=True, scales=(0.125, 0.25, 0.5), dtypes=("fp32",))
_HS3 = dict(_HS, k=3, pad=1)
DETECTOR_CASES = [
    Case("hsw_pw_64_40", B=2, H=10, W=12, c_in=64, c_out=40, **_HS),                                      # M = 240 and N = 40 ragged against every tile
    Case("hsw_pw_64_40_res", B=2, H=10, W=12, c_in=64, c_out=40, residual=True, **_HS),                   # the activation before the add
    Case("hsw_slice_pw_64_40_of56_c8", B=2, H=10, W=12, c_in=64, c_out=40, slice_of=(56, 8), **_HS),
    Case("slice_pw_64_64_of128_c64", "conv", 2, 10, 12, 64, 64, x_mag=3, w_mag=3, slice_of=(128, 64), dtypes=("fp32",)),   # the last pixel's slice ends the extent
    Case("hsw_c3_12_32", B=2, H=9, W=7, c_in=12, c_out=32, **_HS3),                                       # Focus conv: c_in below a K tile
    Case("hsw_c3s2_32_64", B=3, H=13, W=11, c_in=32, c_out=64, stride=2, **_HS3),                         # the downsampling convs, odd map
    Case("hsw_c3_64_64_res", B=3, H=13, W=11, c_in=64, c_out=64, residual=True, **_HS3),                  # BottleNeck (batch 3: the plain kernel)
    Case("hsw_c3_64_64_res_b70", B=70, H=3, W=2, c_in=64, c_out=64, residual=True, **_HS3),               # the same in the tap-skipping kernel
    Case("hsw_slice_c3_64_64_of128_c64", B=70, H=3, W=2, c_in=64, c_out=64, slice_of=(128, 64), **_HS3),  # tiles straddle images; slice store
    Case("hsw_pw_384_128", B=2, H=9, W=7, c_in=384, c_out=128, **_HS),                                    # the concat widths: six K tiles
    # the 128-column tiles need n_pad % 128 == 0: the residual and the slice once more at 128 output channels
    Case("hsw_pw_64_128_res", B=2, H=9, W=7, c_in=64, c_out=128, residual=True, **_HS),
    Case("hsw_slice_pw_64_128_of192_c64", B=2, H=9, W=7, c_in=64, c_out=128, slice_of=(192, 64), **_HS),
    Case("hsw_slice_c3_64_128_of192_c64", B=70, H=3, W=2, c_in=64, c_out=128, slice_of=(192, 64), **_HS3),
    # the one detector conv without hardswish: 3 anchors x 6 columns at a stride of 8, bias, no scale
    Case("head_pw_128_a3_no6", "conv", 2, 5, 7, 128, 24, x_mag=2, w_mag=2, scale=False, head=(3, 6), dtypes=("fp32",)),
]
FORWARD_CASES += DETECTOR_CASES
FORWARD_IDS = [c.name for c in FORWARD_CASES]


def tap_skip_case(h: int, w: int, tile) -> Case:
    """3x3 64 -> 64 (128 columns for the 128-wide tile) at batch 70 on a map without / with interior: ragged M, tiles that straddle positions."""
    return Case(f"tapskip_{h}x{w}_{tile[0]}x{tile[1]}", "conv", 70, h, w, 64, 64 if tile[1] == 64 else 128, 3, 1, 1, 2, 2, residual=True, relu=True,
                dtypes=("fp32",))


@dataclass
class Data:
    """Operands (float64, reference layouts) and the exact result of one case at one dtype."""
    case: Case
    dtype: str
    x: torch.Tensor                    # [B, c_in, H, W]
    w: torch.Tensor                    # [O, I / groups, k, k]; deconv: [I, O, 4, 4]
    scale: Optional[torch.Tensor]
    shift: Optional[torch.Tensor]
    res: Optional[torch.Tensor]        # [B, c_out, oh, ow]
    pre: torch.Tensor                  # before ReLU, NCHW (after the pixel shuffle where flagged); hardswish: the pre-activation v (no residual)
    step: torch.Tensor                 # what one term of magnitude 1 more or less adds to each element of `pre`: its channel's scale
    ref: torch.Tensor                  # the exact result, NCHW
    bias: Optional[torch.Tensor] = None    # head cases: the bias per (anchor, column) before the padding (`shift` holds the padded vector)

    @property
    def store_dtype(self):
        c = self.case
        return torch.float32 if (self.dtype == "fp32" or c.nchw or c.out_f32) else torch.bfloat16

    def stored(self, t=None) -> torch.Tensor:
        """The exact result in the layout the launch writes (NHWC unless the NCHW store is flagged), float64."""
        t = self.ref if t is None else t
        return t.contiguous() if self.case.nchw else t.permute(0, 2, 3, 1).contiguous()

    def expected(self) -> torch.Tensor:
        """What the launch must store: torch's conversion rounds to nearest even."""
        return self.stored().to(self.store_dtype)


def _conv(c: Case, x, w):
    if c.kind == "deconv":
        return F.conv_transpose2d(x, w, stride=2, padding=1)
    return F.conv2d(x, w, stride=c.stride, padding=c.pad, groups=c.groups)


def hardswish_f32(v: torch.Tensor, res: Optional[torch.Tensor] = None, *, act_after_res: bool = False, trunc_div: bool = False) -> torch.Tensor:
    """The kernel's epilogue on an exact pre-activation `v` (float64 holding fp32 values), one IEEE fp32 operation at a time in the kernel's own
    order (numpy: each operation rounds once): h = (v * clamp(v + 3, 0, 6)) / 6, then h + residual.  With v + 3 and the product exact
    (conditions() asserts both) the division and the add round once each, so the bits are unique.  Returns float64 (-0.0 where v <= -3 and
    nothing is added: -|v| * 0).  MUTATIONS for the negative self-check: `act_after_res` - hardswish(v + residual); `trunc_div` - the
    quotient's last bit cleared."""
    f = np.float32
    a = v.numpy().astype(f)
    assert np.array_equal(a.astype(np.float64), v.numpy())
    r = None if res is None else res.numpy().astype(f)
    if act_after_res:
        a, r = a + r, None
    q = (a * np.minimum(np.maximum(a + f(3), f(0)), f(6))) / f(6)
    assert q.dtype == f
    if trunc_div:
        q = (q.view(np.int32) & ~np.int32(1)).view(f)
    if r is not None:
        q = q + r
    return torch.from_numpy(q.astype(np.float64))


def head_rows(t: torch.Tensor, anchors: int, no: int) -> torch.Tensor:
    """[anchors * no, ...] -> [anchors * a_stride, ...]: every anchor's `no` rows followed by zero rows up to engine.yolo_anchor_stride(no)."""
    a_stride = engine.yolo_anchor_stride(no)
    out = torch.zeros((anchors, a_stride) + tuple(t.shape[1:]), dtype=t.dtype)
    out[:, :no] = t.reshape((anchors, no) + tuple(t.shape[1:]))
    return out.reshape((anchors * a_stride,) + tuple(t.shape[1:]))


def make(c: Case, dtype: str, mutation: Optional[str] = None) -> Data:
    """`mutation` (hardswish cases; the negative self-check of tests/test_conv_exact_host.py): "act_after_res" | "trunc_div"."""
    g = generator(c.name)
    W = c.width(dtype)
    x = ints((c.B, c.c_in, c.H, W), c.x_mag, g)
    wshape = (c.c_in, c.c_out, 4, 4) if c.kind == "deconv" else (c.c_out, c.c_in // c.groups, c.k, c.k)
    if c.head:
        assert c.c_out == c.head[0] * engine.yolo_anchor_stride(c.head[1]) and not c.scale and c.k == 1
        wshape = (c.head[0] * c.head[1], c.c_in, 1, 1)
    w = ints(wshape, c.w_mag, g)
    z = _conv(c, x, head_rows(w, *c.head) if c.head else w)
    scale = shift = res = bias = None
    bc = lambda v: v.view(1, -1, 1, 1)
    step = torch.ones_like(z)
    if c.scale:
        scale = torch.tensor(c.scales or (0.5, 1.0, 2.0), dtype=torch.float64)[torch.randint(0, len(c.scales or (0, 0, 0)), (c.c_out,), generator=g)]
        z, step = z * bc(scale), step * bc(scale)
    if c.shift:
        if c.head:
            bias = ints((c.head[0] * c.head[1],), 4, g) + c.shift_bias
            shift = head_rows(bias, *c.head)
        else:
            shift = ints((c.c_out,), 4, g) + c.shift_bias
        z = z + bc(shift)
    v = z
    if c.residual:
        res = ints(tuple(z.shape), 4, g)
        z = z + res
    if c.hardswish:
        assert not c.relu and not c.pshuf
        ref = hardswish_f32(v, res, **({mutation: True} if mutation else {}))
        return Data(c, dtype, x, w, scale, shift, res, v, step, ref, bias)
    assert mutation is None
    pre, ref = z, (torch.relu(z) if c.relu else z)
    if c.pshuf:
        pre, ref, step = F.pixel_shuffle(pre, 2), F.pixel_shuffle(ref, 2), F.pixel_shuffle(step, 2)
    return Data(c, dtype, x, w, scale, shift, res, pre, step, ref + 0.0, bias)


def bf16_low_bits(t: torch.Tensor) -> torch.Tensor:
    """The 16 bits of an fp32 value that a bf16 store drops (the value must be exact in fp32)."""
    f = t.float()
    assert torch.equal(f.double(), t.double())
    return f.contiguous().view(torch.int32) & 0xFFFF


def conditions(d: Data) -> dict:
    """What makes the case worth running, computed on the reference alone; asserts and returns the figures."""
    c = d.case
    top = _conv(c, d.x.abs(), d.w.abs()).max().item() * (d.scale.abs().max().item() if d.scale is not None else 1.0)
    top += (d.shift.abs().max().item() if d.shift is not None else 0.0) + (d.res.abs().max().item() if d.res is not None else 0.0)
    out = {"bound": top}
    assert top < LIMIT, (c.name, top)                                     # exactness: every partial sum in every order is an integer below 2^24
    assert not bool((d.x == 0).any()) and not bool((d.w == 0).any())       # every product counts
    assert torch.equal(d.ref.float().double(), d.ref)                      # the exact result is an fp32 value
    if c.hardswish or c.slice_of or c.head:
        assert c.dtypes == ("fp32",) and not (c.slice_of and c.residual), c.name          # fp32-only epilogues; a slice takes no residual
    if c.slice_of:
        out_c, c0 = c.slice_of
        assert c0 % 4 == 0 and c.c_out % 4 == 0 and out_c % 4 == 0 and c0 + c.c_out <= out_c, c.name
    if c.hardswish:
        # v is exact (above: integer sums below 2^24 times a power of two, plus an integer), and so are v + 3 and the product: the division
        # and the residual add are the only roundings, once each
        v = d.pre
        assert torch.equal(v.float().double(), v)
        for t in (v + 3, v * (v + 3), v * torch.clamp(v + 3, 0, 6)):
            assert torch.equal(t.float().double(), t), c.name
        out["above_minus_3"] = (v > -3).double().mean().item()
        out["inside_pm_3"] = ((v > -3) & (v < 3)).double().mean().item()
        assert out["above_minus_3"] >= 0.40, (c.name, out)                 # the activation does not blank the comparison
        assert out["inside_pm_3"] >= 0.20, (c.name, out)                   # where the division is inexact and "residual first" differs
        q = v * torch.clamp(v + 3, 0, 6) / 6
        out["inexact_quotients"] = (q.float().double() != q).double().mean().item()
        assert out["inexact_quotients"] >= 0.10, (c.name, out)             # the division really rounds
        return out
    if c.role == "index":
        below = (d.pre.abs() < 256).double().mean().item()
        out["below_256"] = below
        assert below >= 0.90, (c.name, below)
        if d.store_dtype == torch.bfloat16:
            # one term more or less (the sum moves by 1, the output by its channel's scale) changes the stored bf16 of most outputs
            moved = ((d.pre + d.step).bfloat16() != d.pre.bfloat16()) & ((d.pre - d.step).bfloat16() != d.pre.bfloat16())
            out["moved_by_one_term"] = moved.double().mean().item()
            assert out["moved_by_one_term"] >= 0.90, (c.name, out)
        if c.relu:
            out["positive"] = (d.pre > 0).double().mean().item()
            assert out["positive"] >= 0.40, (c.name, out)                  # ReLU does not blank the comparison
    else:
        low = bf16_low_bits(d.ref)
        out["ties"] = (low == 0x8000).double().mean().item()
        out["inexact_non_ties"] = ((low != 0) & (low != 0x8000)).double().mean().item()
        assert out["ties"] >= 0.10 and out["inexact_non_ties"] >= 0.10, (c.name, out)
    return out


def truncate_to_bf16(t: torch.Tensor) -> torch.Tensor:
    """A wrong store: the dropped bits cut off instead of rounded (what the negative self-check must catch)."""
    f = t.float().contiguous()
    return (f.view(torch.int32) & ~0xFFFF).view(torch.float32).bfloat16()


@dataclass
class Lowered:
    """One case lowered through engine.ProgramBuilder: the launch descriptor, packed weights and operands in the launch's layouts."""
    op: engine.Op
    prog: engine.Program
    x: torch.Tensor                    # NHWC activation in the activation dtype; stem: the fp32 NCHW image (the layout launch comes first)
    res: Optional[torch.Tensor]
    out_shape: tuple


def lower(d: Data, packer, device) -> Lowered:
    c, bf = d.case, d.dtype == "bf16"
    adt = torch.bfloat16 if bf else torch.float32
    W = c.width(d.dtype)
    dev = lambda t: None if t is None else t.float().to(device)
    b = engine.ProgramBuilder(c.H, W, dtype=d.dtype, packer=packer)
    scale, shift = d.scale, d.shift
    if c.pshuf:                        # packed rows are sub-pixel-major: the epilogue vectors come in the same order
        from tests.desc_interp import TorchPacker
        perm = TorchPacker.row_perm(c.c_out, "cpu")
        scale, shift = (None if scale is None else scale[perm]), (None if shift is None else shift[perm])
    if c.kind == "stem":
        src = b.to_nhwc4("input")
        out = b.conv(src, dev(d.w), stride=c.stride, pad=c.pad, scale=dev(scale), shift=dev(shift), relu=c.relu, name=c.name)
        x = d.x.float().to(device)
    else:
        b.p.shapes["input"] = (c.H, W, c.c_in)
        x = d.x.permute(0, 2, 3, 1).contiguous().to(adt).to(device)
        if c.kind == "deconv":
            out = b.deconv_k4s2p1("input", dev(d.w), scale=dev(scale), shift=dev(shift), relu=c.relu, name=c.name)
        elif c.head:                   # as engine.yolov5_program lowers a head: the padded rows and bias of engine._head_conv, no scale
            wp, bp = engine._head_conv(dev(d.w), dev(d.bias), c.head[0], c.head[1], engine.yolo_head_columns(c.head[1], -1))
            out = b.conv("input", wp, shift=b.packer.bias(bp), name=c.name)
        else:
            if c.residual:
                b.p.shapes["res"] = tuple(d.res.shape[2:]) + (c.c_out,)
            out_slice = None
            if c.slice_of:             # the producers of a concat write their channel slices of one buffer (engine._cbr's `out`)
                out_slice = (b.buffer("cat", d.ref.shape[2], d.ref.shape[3], c.slice_of[0]), c.slice_of[1])
            out = b.conv("input", dev(d.w), stride=c.stride, pad=c.pad, scale=dev(scale), shift=dev(shift), relu=c.relu,
                         res="res" if c.residual else None, pixel_shuffle=c.pshuf, out_nchw=c.nchw, groups=c.groups, name=c.name,
                         hardswish=c.hardswish, out_slice=out_slice)
    op = b.p.ops[-1]
    op.desc.batch = c.B
    if c.out_f32:
        op.desc.flags |= _lib.SP_CONV_OUT_F32
        op.direct = False
    want_flags = (_lib.SP_CONV_HARDSWISH if c.hardswish else 0) | (_lib.SP_CONV_OUT_SLICE if c.slice_of else 0)
    assert op.desc.flags & (_lib.SP_CONV_HARDSWISH | _lib.SP_CONV_OUT_SLICE) == want_flags, (c.name, op.desc.flags)
    assert op.c0 == (c.slice_of[1] if c.slice_of else 0)
    res = None if d.res is None else d.res.permute(0, 2, 3, 1).contiguous().to(d.store_dtype).to(device)      # (read in the dtype of the store)
    oh, ow, oc = b.p.shapes[out]       # a slice launch: the whole buffer (oc = out_c); the launch writes [c0, c0 + c_out) of it
    assert oc == (c.slice_of[0] if c.slice_of else c.c_out if not c.pshuf else c.c_out // 4), (c.name, oc)
    return Lowered(op, b.p, x, res, (c.B, oc, oh, ow) if c.nchw else (c.B, oh, ow, oc))


def candidates(low: Lowered, case: Case):
    """Every (tile_m, tile_n, kernel) the launch can run as (engine.Program._candidates); the in-place form belongs to the implicit GEMM."""
    cands = low.prog._candidates(_lib.lib(), low.op)
    if case.hardswish or case.slice_of:
        # the library runs these flags on the implicit GEMM alone: the engine must not offer the tuner anything else
        assert cands and all(k[0] > 0 and k[2] == _lib.SP_CONV_KERNEL_IGEMM for k in cands), (case.name, cands)
    if case.inplace:
        cands = [k for k in cands if k[0] > 0 and k[2] == _lib.SP_CONV_KERNEL_IGEMM]
    return cands


def family(low: Lowered, cand, has_res: bool) -> tuple:
    """Which kernel a candidate resolves to, as the coverage condition counts them (the library's own dispatch names it; nothing is launched)."""
    d = low.op.desc
    bf = "bf16" if d.flags & _lib.SP_CONV_BF16 else "fp32"
    if cand[0] < 0:
        return ("direct", d.c_in if d.c_out == d.c_in else f"head{d.c_in}")
    keep = (d.tile_m, d.tile_n, d.kernel)
    d.tile_m, d.tile_n, d.kernel = cand
    try:
        name = _lib.conv_kernel_name(d, has_res)
    finally:
        d.tile_m, d.tile_n, d.kernel = keep
    if cand[2] == _lib.SP_CONV_KERNEL_IGEMM:
        if name.startswith("conv_igemm_tapskip_kernel<"):
            return ("tapskip", cand[:2])
        assert name.startswith("conv_igemm_kernel<"), name
        return ("igemm", cand[:2], bf)
    assert name.startswith({_lib.SP_CONV_KERNEL_PW: "conv_pw_kernel<"}.get(cand[2], "conv_ring_kernel<")), name
    return ({_lib.SP_CONV_KERNEL_RING: "ring", _lib.SP_CONV_KERNEL_RING_LW: "ring_lw", _lib.SP_CONV_KERNEL_RING_LW4: "ring_lw4",
             _lib.SP_CONV_KERNEL_PW: "pw"}[cand[2]],)


def detector_families(case: Case, fam: tuple) -> set:
    """What a launch of a detector case adds to the coverage condition besides its kernel family `fam`: per implicit-GEMM tile "hsw", "slice"
    (at c0 > 0) and "hsw_res"; for the tap-skipping kernel (at any tile) ("tapskip", "hsw") and ("tapskip", "slice")."""
    tags = (["hsw"] if case.hardswish else []) + (["slice"] if case.slice_of and case.slice_of[1] > 0 else []) + \
           (["hsw_res"] if case.hardswish and case.residual else [])
    if fam[0] == "tapskip":
        return {("tapskip", t) for t in tags if t != "hsw_res"}
    return {(t, fam[1]) for t in tags} if fam[0] == "igemm" else set()


def required_detector_families() -> set:
    return {(t, tile) for t in ("hsw", "slice", "hsw_res") for tile in _lib.CONV_TILES} | {("tapskip", "hsw"), ("tapskip", "slice")}


def required_families() -> set:
    need = {("igemm", t, dt) for t in _lib.CONV_TILES for dt in ("fp32", "bf16")}
    return need | {("ring",), ("ring_lw",), ("ring_lw4",), ("pw",), ("direct", 32), ("direct", 64), ("direct", 128)}


def missing_families(seen: set) -> set:
    """Families of the coverage condition that `seen` lacks (the tap-skip kernel counts at any tile)."""
    miss = (required_families() | required_detector_families()) - seen
    if not any(f[0] == "tapskip" and isinstance(f[1], tuple) for f in seen):
        miss.add(("tapskip",))
    return miss


# ---- backward: integer operands through train.ConvT --------------------------------------------------------------------------------------------
def backward_reference(kind, I, O, k, s, p, H, W, B, seed, groups=1, mag=2):
    """x, w, dz (magnitudes <= `mag`) and the exact y, dx, dW by float64 autograd; also the bounds sum |dz| |w| and sum |dz| |x| of the two
    gradients' partial sums.  Returns a dict of float64 tensors in the reference layouts."""
    g = generator(f"bwd/{kind}/{I}/{O}/{k}/{s}/{H}/{W}/{B}/{groups}", seed)
    x = ints((B, I, H, W), mag, g)
    w = ints((O, I // groups, k, k) if kind == "conv" else (I, O, k, k), mag, g)
    fwd = (lambda a, b: F.conv2d(a, b, stride=s, padding=p, groups=groups)) if kind == "conv" else (lambda a, b: F.conv_transpose2d(a, b, stride=2, padding=1))
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = fwd(xr, wr)
    dz = ints(tuple(y.shape), mag, g)
    y.backward(dz)
    xa, wa = x.abs().requires_grad_(True), w.abs().requires_grad_(True)
    ya = fwd(xa, wa)
    ya.backward(dz.abs())
    out = dict(x=x, w=w, dz=dz, y=y.detach(), dx=xr.grad, dw=wr.grad, y_bound=ya.detach().max().item(), dx_bound=xa.grad.max().item(),
               dw_bound=wa.grad.max().item())
    return out


def backward_conditions(r: dict, acc_mag: int = 0) -> dict:
    """Exactness of the three results of one layer: every partial sum, in any order and any split of the pixels, is an integer below 2^24."""
    assert r["y_bound"] < LIMIT and r["dx_bound"] + acc_mag < LIMIT and r["dw_bound"] < LIMIT, {k: v for k, v in r.items() if k.endswith("_bound")}
    for k in ("x", "w", "dz"):
        assert not bool((r[k] == 0).any())
    for k in ("y", "dx", "dw"):
        assert torch.equal(r[k].float().double(), r[k]), k
    return {k: v for k, v in r.items() if k.endswith("_bound")}


def stats_conditions(z: torch.Tensor, store_dtype) -> dict:
    """The statistics epilogue: z [rows, C] is stored exactly (so the sums of the stored tensor and of the accumulators are the same numbers), and
    a whole column's sum of squares - hence every tile's share of it, in any order - stays below 2^24."""
    assert torch.equal(z.to(store_dtype).double(), z)
    top = (z * z).sum(0).max().item()
    assert top < LIMIT and z.abs().sum(0).max().item() < LIMIT, top
    return {"column_sumsq_max": top}


# ---- fused launches: several convolutions in one launch -----------------------------------------------------------------------------------------
# A fused case is a chain of stages.  One stage: convolution (float64), times a per-channel power-of-two scale, plus an integer shift, plus an
# optional residual, optional ReLU, then the store rounding of THAT stage: bf16 where the per-conv program stores bf16, none where it stores fp32.
# The pre-store value of a stage is an fp32 value (asserted), so its round-to-nearest-even is unique - and with it every later stage.
def _p2(*exponents):
    return tuple(2.0 ** -e for e in exponents)


# family -> channels of x, operand magnitudes, and per stage the scale choices and what is added to every channel's shift (integers in +-4)
FAMILIES = {
    # t1 = bf16(relu(s1 (x.W1) + b1)), 0 outside the image; t2 = bf16(relu(s2 conv3x3(t1) + b2)); y = bf16(relu(s3 (t2.W3) + b3 + x))
    "bneck64": dict(c=256, x_mag=3, scales=(_p2(1, 0, -1), _p2(4, 3, 2), _p2(5, 4, 3)), bias=(4, 0, 0)),
    # t = bf16(relu(s1 conv3x3(x) + b1)), 0 outside the image; y = bf16(relu(s2 conv3x3(t) + b2 + x))
    "bb32": dict(c=32, x_mag=16, w_mag=(8, 1), scales=(_p2(1, 0, -1), _p2(9, 8, 7)), bias=(128, 0)),
    "bb64": dict(c=64, x_mag=16, w_mag=(8, 1), scales=(_p2(1, 0, -1), _p2(10, 9, 8)), bias=(128, 0)),
    # r = [bf16](sd (x.Wd) + hd); y = [bf16](relu(s3 (t.W3) + h3 + r)): the shortcut's shift lifts r to where a third of a bf16's bits are dropped
    "dual_bf16": dict(c=64, x_mag=4, w_mag=4, scales=(_p2(4, 3, 2), _p2(3, 2, 1)), bias=(160, -148)),
    "dual_f32": dict(c=64, x_mag=4, w_mag=4, scales=(_p2(4, 3, 2), _p2(3, 2, 1)), bias=(160, -148)),
    # y = relu(s3 (t.W3) + b3 + residual); t_next = relu(s1 (y.W1) + b1): fp32 stores, nothing rounded
    "pwchain64": dict(c=64, x_mag=3, scales=(_p2(2, 1, 0), _p2(3, 2, 1)), bias=(0, 0), c_next=64),
    "pwchain128": dict(c=64, x_mag=3, scales=(_p2(2, 1, 0), _p2(3, 2, 1)), bias=(0, 0), c_next=128),
    # y_hi = bf16(relu(sa conv3x3(x) + ha)), y_lo = bf16(relu(sb conv3x3_stride2(x) + hb)): two one-stage convolutions of the same x
    "htrans": dict(c=256, x_mag=3, scales=(_p2(4, 3, 2), _p2(4, 3, 2)), bias=(0, 0)),
}
POINTWISE = ("dual_bf16", "dual_f32", "pwchain64", "pwchain128")       # B = H = 1, W = rows
FUSED_TILES = {"bneck64": (16, 8), "bb32": (8, 48), "bb64": (4, 24), "htrans": (32, 16)}       # output tile of the default kernel (rows, columns)
KERNEL_VARIANT = {"bb32": 4, "bneck64": 5, "bb64": 6}                   # sp_conv2d_kernel_name's variant of the families the library names


@dataclass(frozen=True)
class Fused:
    family: str
    B: int
    H: int
    W: int

    @property
    def name(self) -> str:
        return f"{self.family}_{self.W}" if self.family in POINTWISE else f"{self.family}_{self.B}x{self.H}x{self.W}"


def fused_tiles(c: Fused, tile=None) -> int:
    th, tw = tile or FUSED_TILES[c.family]
    return c.B * (-(-c.H // th)) * (-(-c.W // tw))


def fused_operands(c: Fused) -> dict:
    """The operands of one fused case (float64, reference layouts: activations NCHW, weights [O, I, k, k], vectors [C])."""
    f, g = FAMILIES[c.family], generator(c.name)
    pick = lambda choices, n: torch.tensor(choices, dtype=torch.float64)[torch.randint(0, len(choices), (n,), generator=g)]
    wm = f.get("w_mag", 1)
    wm = wm if isinstance(wm, tuple) else (wm,) * 3
    o = {"x": ints((c.B, f["c"], c.H, c.W), f["x_mag"], g)}
    if c.family == "bneck64":
        shapes = ((64, 256, 1, 1), (64, 64, 3, 3), (256, 64, 1, 1))
    elif c.family in ("bb32", "bb64"):
        shapes = ((f["c"], f["c"], 3, 3),) * 2
    elif c.family.startswith("dual"):
        o["t"] = ints((c.B, 64, c.H, c.W), f["x_mag"], g)
        shapes = ((256, 64, 1, 1),) * 2                                    # the shortcut's Wd, then W3
    elif c.family.startswith("pwchain"):
        o["res"] = ints((c.B, 256, c.H, c.W), 4, g)
        shapes = ((256, 64, 1, 1), (f["c_next"], 256, 1, 1))               # W3, then the next block's W1
    else:
        shapes = ((32, 256, 3, 3), (64, 256, 3, 3))
    for i, (shape, choices, bias) in enumerate(zip(shapes, f["scales"], f["bias"])):
        o[f"w{i}"], o[f"s{i}"], o[f"b{i}"] = ints(shape, wm[i], g), pick(choices, shape[0]), ints((shape[0],), 4, g) + bias
    return o


@dataclass
class FusedData:
    """One fused case evaluated: the operands, what every stage saw, the intermediates and the exact outputs (float64, NCHW)."""
    case: Fused
    ops: dict
    stages: list                       # per stage: name, pre (before ReLU and store), relu, bound_units, unit
    inter: dict                        # intermediates as stored
    pre: dict                          # output name -> its stage's value before ReLU and store
    ref: dict                          # output name -> the exact stored value
    store_dtype: torch.dtype

    def expected(self, name: str) -> torch.Tensor:
        """What the launch must store in output `name` (NHWC): torch's conversion rounds to nearest even."""
        return self.ref[name].permute(0, 2, 3, 1).contiguous().to(self.store_dtype)


def _pad_with(t, fill):
    """t [B, C, H, W] with a one-pixel ring of the per-channel value `fill` around it."""
    B, C, H, W = t.shape
    out = fill.view(1, C, 1, 1).expand(B, C, H + 2, W + 2).clone()
    out[:, :, 1:-1, 1:-1] = t
    return out


def _stage(log, name, x, w, scale, shift, *, pad=0, stride=1, res=None, relu=True, store=None, unit_in=1.0, res_unit=1.0, ring=None, trunc=False):
    """One stage.  `unit_in` / `res_unit`: the finest bit of x / of the residual (weights, shifts are integers, scales powers of two, so every
    partial sum of the stage is a multiple of `unit`); `ring`: MUTATION - x outside the image holds this per-channel value instead of 0;
    `trunc`: MUTATION - a bf16 store that cuts the dropped bits off."""
    bc = lambda v: v.view(1, -1, 1, 1)
    xin = x
    if ring is not None:
        assert pad == 1
        xin, pad = _pad_with(x, ring), 0
    pre = F.conv2d(xin, w, stride=stride, padding=pad) * bc(scale) + bc(shift)
    top = F.conv2d(xin.abs(), w.abs(), stride=stride, padding=pad).max().item() * scale.max().item() + shift.abs().max().item()
    if res is not None:
        pre, top = pre + res, top + res.abs().max().item()
    unit = min(unit_in * scale.min().item(), res_unit, 1.0)
    out = torch.relu(pre) if relu else pre
    if store == "bf16":
        out = (truncate_to_bf16(out) if trunc else out.float().bfloat16()).double()
    log.append(dict(name=name, pre=pre, relu=relu, bound_units=top / unit, unit=unit))
    return out + 0.0, unit


def _drop(w, term):
    """MUTATION: one (output channel, input channel, tap) product left out."""
    if term is None:
        return w
    o, i, tap = term
    w = w.clone()
    assert w[o, i].reshape(-1)[tap] != 0
    w[o, i].view(-1)[tap] = 0
    return w


def fused_eval(c: Fused, o: dict, ring=False, trunc=False, drop=None, shift_res=False) -> FusedData:
    """The float64 chain of case `c` on operands `o`.  The keyword arguments are the four mutations of the negative self-check (each family takes
    those that exist for it): `ring` - the 3x3's input outside the image is bf16(relu(shift)) of the stage before, not 0; `trunc` - every
    intermediate bf16 store (transition1: its only store) truncates; `drop` - one term of the 3x3 (pointwise families: of the first product)
    left out; `shift_res` - the residual comes from the neighbouring pixel."""
    fam, log, inter = c.family, [], {}
    bf = None if fam in ("dual_f32", "pwchain64", "pwchain128") else "bf16"
    x = o["x"]
    side = lambda t: torch.roll(t, 1, dims=-1) if shift_res else t
    edge = lambda i: torch.relu(o[f"b{i}"]).float().bfloat16().double() if ring else None
    if fam == "bneck64":
        t1, u = _stage(log, "t1", x, o["w0"], o["s0"], o["b0"], store=bf, trunc=trunc)
        t2, u = _stage(log, "t2", t1, _drop(o["w1"], drop), o["s1"], o["b1"], pad=1, store=bf, unit_in=u, ring=edge(0), trunc=trunc)
        y, _ = _stage(log, "y", t2, o["w2"], o["s2"], o["b2"], res=side(x), store=bf, unit_in=u)
        inter, outs = {"t1": t1, "t2": t2}, {"y": y}
    elif fam in ("bb32", "bb64"):
        t, u = _stage(log, "t", x, _drop(o["w0"], drop), o["s0"], o["b0"], pad=1, store=bf, trunc=trunc)
        y, _ = _stage(log, "y", t, o["w1"], o["s1"], o["b1"], pad=1, res=side(x), store=bf, unit_in=u, ring=edge(0))
        inter, outs = {"t": t}, {"y": y}
    elif fam.startswith("dual"):
        r, u = _stage(log, "r", x, _drop(o["w0"], drop), o["s0"], o["b0"], relu=False, store=bf, trunc=trunc)
        y, _ = _stage(log, "y", o["t"], o["w1"], o["s1"], o["b1"], res=side(r), res_unit=u, store=bf)
        inter, outs = {"r": r}, {"y": y}
    elif fam.startswith("pwchain"):
        y, u = _stage(log, "y", x, _drop(o["w0"], drop), o["s0"], o["b0"], res=side(o["res"]))
        tn, _ = _stage(log, "t_next", y, o["w1"], o["s1"], o["b1"], unit_in=u)
        outs = {"y": y, "t_next": tn}
    else:
        assert fam == "htrans", fam
        hi, _ = _stage(log, "y_hi", x, _drop(o["w0"], drop), o["s0"], o["b0"], pad=1, store=bf, trunc=trunc)
        lo, _ = _stage(log, "y_lo", x, o["w1"], o["s1"], o["b1"], pad=1, stride=2, store=bf, trunc=trunc)
        outs = {"y_hi": hi, "y_lo": lo}
    pre = {s["name"]: s["pre"] for s in log if s["name"] in outs}
    return FusedData(c, o, log, inter, pre, outs, torch.bfloat16 if bf else torch.float32)


def make_fused(c: Fused) -> FusedData:
    return fused_eval(c, fused_operands(c))


def fused_conditions(d: FusedData) -> dict:
    """What makes a fused case exact and worth running, asserted on the reference alone; returns the figures."""
    out = {}
    for k, v in d.ops.items():
        assert torch.equal(v, v.round()) or k[0] == "s", k
        if k[0] in "xtw":
            assert not bool((v == 0).any()), k                              # every product counts
        if k[0] == "s":
            assert torch.equal(torch.log2(v), torch.log2(v).round()), k     # powers of two
    for s in d.stages:
        n = s["name"]
        out[n + "_bound_units"] = s["bound_units"]
        assert s["bound_units"] < LIMIT, (d.case.name, n, s["bound_units"])   # every partial sum, in any order, is below 2^24 of the stage's finest bit
        assert torch.equal(s["pre"].float().double(), s["pre"]), (d.case.name, n)
        if s["relu"]:
            out[n + "_positive"] = (s["pre"] > 0).double().mean().item()
            assert out[n + "_positive"] >= 0.40, (d.case.name, out)         # ReLU does not blank what follows
    for n, p in d.pre.items():
        out[n + "_below_256"] = (p.abs() < 256).double().mean().item()
        assert out[n + "_below_256"] >= 0.90, (d.case.name, out)
    return out


@dataclass
class LoweredFused:
    """One fused case lowered through engine.ProgramBuilder: the program's ops (one fused op, or the per-conv launches it replaces), the
    operands in the launch's layouts under their buffer names, and the buffer of every output."""
    ops: list
    bufs: dict
    outs: dict
    shapes: dict


def lower_fused(d: FusedData, packer, device, fused: bool = True) -> LoweredFused:
    """`fused`: through the builder methods the engine itself uses (bottleneck_c64, basic_block_c32, dual_pointwise_tail, the `pwchain` / `htrans`
    lowerings); else the per-conv program of the same block.  Scale and shift are the exact fp32 vectors of the case."""
    c, o, fam = d.case, d.ops, d.case.family
    bf = d.store_dtype == torch.bfloat16
    adt = d.store_dtype
    dev = lambda t: t.float().to(device)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(adt).to(device)
    b = engine.ProgramBuilder(c.H, c.W, dtype="bf16" if bf else "fp32", packer=packer)
    b.fuse_bottlenecks = b.fuse_blocks = b.fuse_blocks64 = b.fuse_tail = b.fuse_chain = b.fuse_transition = fused
    b.p.shapes["input"] = (c.H, c.W, FAMILIES[fam]["c"])
    bufs = {"input": nhwc(o["x"])}
    W, S, Hh = ([dev(o[f"{k}{i}"]) for i in range(3) if f"{k}{i}" in o] for k in "wsb")
    if fam == "bneck64":
        y = b.bottleneck_c64("input", W[0], S[0], Hh[0], W[1], S[1], Hh[1], W[2], S[2], Hh[2], name="blk")
        if not fused:
            assert y is None
            t1 = b.conv("input", W[0], scale=S[0], shift=Hh[0], relu=True, name="blk.conv1")
            t2 = b.conv(t1, W[1], pad=1, scale=S[1], shift=Hh[1], relu=True, name="blk.conv2")
            y = b.conv(t2, W[2], scale=S[2], shift=Hh[2], relu=True, res="input", name="blk.conv3")
        outs = {"y": y}
    elif fam in ("bb32", "bb64"):
        y = b.basic_block_c32("input", W[0], S[0], Hh[0], W[1], S[1], Hh[1], name="blk")
        if not fused:
            assert y is None
            t = b.conv("input", W[0], pad=1, scale=S[0], shift=Hh[0], relu=True, name="blk.conv1")
            y = b.conv(t, W[1], pad=1, scale=S[1], shift=Hh[1], relu=True, res="input", name="blk.conv2")
        outs = {"y": y}
    elif fam.startswith("dual"):
        b.p.shapes["t"] = (c.H, c.W, 64)
        bufs["t"] = nhwc(o["t"])
        y = b.dual_pointwise_tail("t", W[1], S[1], Hh[1], "input", W[0], S[0], Hh[0], name="blk")
        if not fused:
            assert y is None
            r = b.conv("input", W[0], scale=S[0], shift=Hh[0], name="blk.downsample")
            y = b.conv("t", W[1], scale=S[1], shift=Hh[1], relu=True, res=r, name="blk.conv3")
        outs = {"y": y}
    elif fam.startswith("pwchain"):
        b.p.shapes["res"] = (c.H, c.W, 256)
        bufs["res"] = nhwc(o["res"])
        y = b.conv("input", W[0], scale=S[0], shift=Hh[0], relu=True, res="res", name="blk.conv3")
        tn = b.conv(y, W[1], scale=S[1], shift=Hh[1], relu=True, name="next.conv1")
        engine._fuse_pw_chains(b, {})
        outs = {"y": y, "t_next": tn}
    else:
        hi = b.conv("input", W[0], pad=1, scale=S[0], shift=Hh[0], relu=True, name="transition1.0")
        lo = b.conv("input", W[1], stride=2, pad=1, scale=S[1], shift=Hh[1], relu=True, name="transition1.1")
        engine._fuse_transition1(b)
        outs = {"y_hi": hi, "y_lo": lo}
    assert all(v is not None for v in outs.values()), (c.name, outs)
    kinds = [op.kind for op in b.p.ops]
    want = {"bneck64": "bneck64", "bb32": "bb32", "bb64": "bb64", "dual_bf16": "dual1x1", "dual_f32": "dual1x1", "pwchain64": "pwchain",
            "pwchain128": "pwchain", "htrans": "htrans"}[fam]
    assert (kinds == [want]) if fused else (set(kinds) == {"conv"}), (c.name, kinds)
    for op in b.p.ops:
        if op.desc is not None:
            op.desc.batch = c.B
    return LoweredFused(b.p.ops, bufs, outs, b.p.shapes)


def fused_kernel_name(low: LoweredFused, family: str) -> str:
    """The instantiation the fused launch resolves to where the library names it (variants 4, 5, 6), else the entry point."""
    if family in KERNEL_VARIANT:
        return _lib.conv_kernel_name(low.ops[0].desc, False, KERNEL_VARIANT[family])
    return {"dual_bf16": "sp_dual_pw_bf16", "dual_f32": "sp_dual_pw_f32", "pwchain64": "sp_pw_chain_f32<64>", "pwchain128": "sp_pw_chain_f32<128>",
            "htrans": "sp_hrnet_transition1"}[family]
