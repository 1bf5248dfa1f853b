"""TEST HELPER: convolutions whose every output bit is known in advance.

Operands are small non-zero integers: exact in bf16 and fp32, every product and every partial sum an integer below 2^24, so an fp32 accumulator
holds the exact result in any reduction order, on any tile, in any kernel.  The epilogue (a power-of-two scale, an integer shift and residual,
ReLU) stays exact; the one inexact step left is the final store, whose bits are unique: round-to-nearest-even of the exact value.  A float64
torch convolution therefore predicts every stored bit of every launch - one wrong, missing or doubled term in one element is a mismatch.

tests/test_conv_exact_host.py holds the case table against the descriptor interpreter (no GPU), tests/test_gpu_conv_exact.py the kernels.
"""
import zlib
from dataclasses import dataclass, replace
from typing import Optional, Tuple

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
    pre: torch.Tensor                  # before ReLU, NCHW (after the pixel shuffle where flagged)
    step: torch.Tensor                 # what one term of magnitude 1 more or less adds to each element of `pre`: its channel's scale
    ref: torch.Tensor                  # the exact result, NCHW

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


def make(c: Case, dtype: str) -> Data:
    g = generator(c.name)
    W = c.width(dtype)
    x = ints((c.B, c.c_in, c.H, W), c.x_mag, g)
    wshape = (c.c_in, c.c_out, 4, 4) if c.kind == "deconv" else (c.c_out, c.c_in // c.groups, c.k, c.k)
    w = ints(wshape, c.w_mag, g)
    z = _conv(c, x, w)
    scale = shift = res = None
    bc = lambda v: v.view(1, -1, 1, 1)
    step = torch.ones_like(z)
    if c.scale:
        scale = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (c.c_out,), generator=g)]
        z, step = z * bc(scale), step * bc(scale)
    if c.shift:
        shift = ints((c.c_out,), 4, g) + c.shift_bias
        z = z + bc(shift)
    if c.residual:
        res = ints(tuple(z.shape), 4, g)
        z = z + res
    pre, ref = z, (torch.relu(z) if c.relu else z)
    if c.pshuf:
        pre, ref, step = F.pixel_shuffle(pre, 2), F.pixel_shuffle(ref, 2), F.pixel_shuffle(step, 2)
    return Data(c, dtype, x, w, scale, shift, res, pre, step, ref + 0.0)


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
        else:
            if c.residual:
                b.p.shapes["res"] = tuple(d.res.shape[2:]) + (c.c_out,)
            out = b.conv("input", dev(d.w), stride=c.stride, pad=c.pad, scale=dev(scale), shift=dev(shift), relu=c.relu,
                         res="res" if c.residual else None, pixel_shuffle=c.pshuf, out_nchw=c.nchw, groups=c.groups, name=c.name)
    op = b.p.ops[-1]
    op.desc.batch = c.B
    if c.out_f32:
        op.desc.flags |= _lib.SP_CONV_OUT_F32
        op.direct = False
    res = None if d.res is None else d.res.permute(0, 2, 3, 1).contiguous().to(d.store_dtype).to(device)      # (read in the dtype of the store)
    oh, ow, oc = b.p.shapes[out]
    return Lowered(op, b.p, x, res, (c.B, oc, oh, ow) if c.nchw else (c.B, oh, ow, oc))


def candidates(low: Lowered, case: Case):
    """Every (tile_m, tile_n, kernel) the launch can run as (engine.Program._candidates); the in-place form belongs to the implicit GEMM."""
    cands = low.prog._candidates(_lib.lib(), low.op)
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


def required_families() -> set:
    need = {("igemm", t, dt) for t in _lib.CONV_TILES for dt in ("fp32", "bf16")}
    return need | {("ring",), ("ring_lw",), ("ring_lw4",), ("pw",), ("direct", 32), ("direct", 64), ("direct", 128)}


def missing_families(seen: set) -> set:
    """Families of the coverage condition that `seen` lacks (the tap-skip kernel counts at any tile)."""
    miss = required_families() - seen
    if not any(f[0] == "tapskip" for f in seen):
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
