"""The kernel chain nn.SyncBatchNorm maps to (include/simple_pose_hip.h: "nn.SyncBatchNorm = the same three steps with a cross-rank SUM between
the halves"), entry point by entry point:

  forward : sp_bn_train_partial_nhwc | sp_bn_sums_from_conv -> SUM -> sp_bn_train_finalize + sp_bn_apply_nhwc | sp_bn_apply_sums_nhwc
  backward: sp_bn_train_bwd_reduce_nhwc | sp_bn_bwd_sums_from_conv2 -> SUM -> sp_bn_train_bwd_apply_nhwc(total_rows > rows)
  and sp_channel_sum_nhwc, which runs the same reduction kernel.

The whole-net multi-rank tests of test_gpu_train.py compare one run of the net with another at chaos-limited bars; an error every rank makes
alike cancels there.  Here the W ranks are emulated on ONE device - every shard's launches one after the other on the current stream, the
all-reduce a torch sum of the shard buffers in rank order (float64 forward message, float32 backward message, as comm.hip sends them) - and
compared (a) bit for bit where the header promises an identity, (b) bit for bit on integer operands whose every sum is exact, (c) against
tests/syncbn_ref.py (float64; proved against torch.nn.BatchNorm2d in tests/test_syncbn_ref_host.py) at the bars of the local passes.

Shards: rows (37, 64, 5) for W = 3, (300, 1) for W = 2, one shard of 6144; C in {4 (smallest legal), 24 (no multiple of the 16-channel fold slab),
64, 256, 2048 (two trips through the channel loop of the reduction)}.  The 6144-row shard runs at C = 2048 only where a test is about that size
(the integer sums): 50 MB of float64 reference per tensor buys nothing elsewhere.  Every output is NaN-prefilled with guard elements behind it.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from simple_pose_amd import _lib  # noqa: E402
from tests import conv_exact as ce  # noqa: E402
from tests import syncbn_ref as ref  # noqa: E402
from tests.test_conv_exact_host import STATS  # noqa: E402
from tests.test_gpu_backward_kernels import BN_BAR, STATS_CASES, _nhwc, _OneLayer, _rel, _rel_bf16  # noqa: E402
from tests.test_gpu_conv_exact import _guarded, _same_bits, _take  # noqa: E402

DEV = "cuda:0"
P = _lib.ptr
EPS, MOM = 1e-5, 0.1
SHARDS = [(37, 64, 5), (300, 1), (6144,)]
SHARD_IDS = ["37x64x5", "300x1", "6144"]
WIDTHS = [4, 24, 64, 256, 2048]
DTYPES = pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
Y_BAR = {False: 2e-6, True: 4e-3}        # test_batchnorm_train_backward_vs_float64's bars on y (_rel / _rel_bf16)
# (C, shards) of the tests on random operands: the 6144-row shard up to C = 256
SHAPES = [(C, s) for C in WIDTHS for s in SHARDS if not (C == 2048 and s == (6144,))]
SHAPE_IDS = [f"c{C}-{'x'.join(map(str, s))}" for C, s in SHAPES]
SHARDED = [(C, s) for C, s in SHAPES if len(s) > 1]
SHARDED_IDS = [f"c{C}-{'x'.join(map(str, s))}" for C, s in SHARDED]


@pytest.fixture(scope="module")
def ws():
    return torch.empty(4 << 20, dtype=torch.uint8, device=DEV)          # SP_REDUCE_WORKSPACE_BYTES


def _adt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _randn(shape, g):
    return torch.randn(shape, generator=g, dtype=torch.float64)


def _random_shards(rows, C, g, dtype):
    """Well-conditioned activations as in test_batchnorm_train_backward_vs_float64, one distribution for every shard; float64 of the STORED values."""
    scale, shift = 0.5 + torch.rand(C, generator=g, dtype=torch.float64), _randn(C, g)
    return [(_randn((n, C), g) * scale + shift).to(dtype).double() for n in rows]


def _affine(C, g):
    gamma = (0.75 + 0.5 * torch.rand(C, generator=g, dtype=torch.float64)).float().double()
    beta = (0.1 * _randn(C, g)).float().double()
    rm0 = _randn(C, g).float().double()                                   # running statistics start from non-trivial values
    rv0 = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)).float().double()
    return gamma, beta, rm0, rv0


def _dev(t, dtype=torch.float32):
    return None if t is None else t.to(dtype).to(DEV).contiguous()


def _started(start):
    """A guarded buffer that holds the start values of a running statistic (the kernels update it in place)."""
    buf = _guarded(start.numel(), torch.float32)
    buf[:start.numel()] = start.float().to(DEV)
    return buf


def _call(rc, what):
    _lib.check(rc, what)


# ---- one wrapper per entry point: guarded outputs in, checked views out ---------------------------------------------------------------------------
def _partial(z, bf16, ws, what="partial"):
    rows, C = z.shape
    buf = _guarded(2 * C, torch.float64)
    _call(_lib.lib().sp_bn_train_partial_nhwc(P(z), int(bf16), rows, C, P(buf), P(ws), _lib.current_stream()), what)
    return _take(buf, 2 * C, (C, 2), what)


def _stats_out(C, rm0, rv0):
    return _guarded(C, torch.float32), _guarded(C, torch.float32), _started(rm0), _started(rv0)


def _stats_take(bufs, C, what):
    return {k: _take(b, C, (C,), f"{what}.{k}") for k, b in zip(("mean", "invstd", "running_mean", "running_var"), bufs)}


def _finalize(sums, total_rows, C, rm0, rv0, what="finalize"):
    bufs = _stats_out(C, rm0, rv0)
    _call(_lib.lib().sp_bn_train_finalize(P(sums), total_rows, C, EPS, MOM, *(P(b) for b in bufs), _lib.current_stream()), what)
    return _stats_take(bufs, C, what)


def _stats_nhwc(z, bf16, rm0, rv0, ws, what="stats"):
    rows, C = z.shape
    bufs = _stats_out(C, rm0, rv0)
    _call(_lib.lib().sp_bn_train_stats_nhwc(P(z), int(bf16), rows, C, EPS, MOM, *(P(b) for b in bufs), P(ws), _lib.current_stream()), what)
    return _stats_take(bufs, C, what)


def _apply(z, bf16, st, gamma, beta, res, relu, mask=None, what="apply"):
    rows, C = z.shape
    y = _guarded(rows * C, z.dtype)
    _call(_lib.lib().sp_bn_apply_nhwc(P(z), int(bf16), P(st["mean"]), P(st["invstd"]), P(gamma), P(beta), P(res), P(y), rows, C, int(relu), P(mask),
                                      _lib.current_stream()), what)
    return _take(y, rows * C, (rows, C), what)


def _apply_sums(z, bf16, sums, total_rows, gamma, beta, res, relu, rm0, rv0, what="apply_sums"):
    rows, C = z.shape
    y = _guarded(rows * C, z.dtype)
    bufs = _stats_out(C, rm0, rv0)
    _call(_lib.lib().sp_bn_apply_sums_nhwc(P(z), int(bf16), P(sums), total_rows, EPS, MOM, P(gamma), P(beta), P(res), P(y), rows, C, int(relu),
                                           *(P(b) for b in bufs), _lib.current_stream()), what)
    out = _stats_take(bufs, C, what)
    out["y"] = _take(y, rows * C, (rows, C), what)
    return out


def _same_stats(a, b, what):
    for k in ("mean", "invstd", "running_mean", "running_var"):
        _same_bits(a[k], b[k], f"{what}: {k}")


# ---- a. identities the header states ---------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("C", WIDTHS)
def test_a1_partial_then_finalize_has_the_bits_of_the_one_call_statistics(C, bf16, ws):
    """W = 1: sp_bn_train_stats_nhwc "is exactly these halves back to back with total_rows = rows"."""
    g = torch.Generator().manual_seed(100 + C)
    _, _, rm0, rv0 = _affine(C, g)
    for rows in sorted({n for s in SHARDS for n in s}):
        if C == 2048 and rows == 6144:
            continue
        z = _dev(_random_shards((rows,), C, g, _adt(bf16))[0], _adt(bf16))
        one = _stats_nhwc(z, bf16, rm0, rv0, ws)
        two = _finalize(_partial(z, bf16, ws), rows, C, rm0, rv0)
        _same_stats(two, one, f"rows={rows}")


@DTYPES
@pytest.mark.parametrize("relu,res_on", [(False, False), (True, False), (False, True), (True, True)], ids=["plain", "relu", "res", "res_relu"])
@pytest.mark.parametrize("C", WIDTHS)
def test_a2_apply_from_sums_has_the_bits_of_finalize_then_apply(C, relu, res_on, bf16, ws):
    """sp_bn_apply_sums_nhwc = sp_bn_train_finalize + sp_bn_apply_nhwc on the same all-reduced sums, for a shard of a larger batch.
    The fused kernel keeps a thread's four channels and finalises again when the thread's next element lies in another channel chunk: the grid is
    capped at 2048 workgroups of 256 threads (sp_grid_for), a stride of 524288 = 2 (mod 6), so with C = 24 (C/4 = 6) every tensor of more than
    524288 / 6 = 87382 rows makes threads see a second chunk: 90001 rows (8.6 MB in fp32) run that path."""
    g = torch.Generator().manual_seed(200 + C)
    gamma64, beta64, rm0, rv0 = _affine(C, g)
    gamma, beta = _dev(gamma64), _dev(beta64)
    adt = _adt(bf16)
    for rows in (37, 300) + ((6144,) if C <= 256 else ()) + ((90001,) if C == 24 else ()):
        mine, other = _random_shards((rows, 123), C, g, adt)
        z, zo = _dev(mine, adt), _dev(other, adt)
        res = _dev(_randn((rows, C), g), adt) if res_on else None
        sums = (_partial(z, bf16, ws) + _partial(zo, bf16, ws)).contiguous()          # rank order, float64
        total = rows + 123
        st = _finalize(sums, total, C, rm0, rv0)
        y = _apply(z, bf16, st, gamma, beta, res, relu)
        fused = _apply_sums(z, bf16, sums, total, gamma, beta, res, relu, rm0, rv0)
        _same_stats(fused, st, f"rows={rows}")
        _same_bits(fused["y"], y, f"rows={rows}: y")


def _random_conv(name, bf16, offset=0.0):
    """One STATS_CASES layer on random operands through ConvT.forward_bn_stats: (layer, z [rows, C] as stored, partial sums [2, prow, n_pad], prow)."""
    _, I, O, k, s, p, H, W, B = next(c for c in STATS_CASES if c[0] == name)
    g = torch.Generator().manual_seed(5 + I + O)
    x = _randn((B, I, H, W), g) + offset
    w = (_randn((O, I, k, k), g) / (I * k * k) ** 0.5).float()
    one = _OneLayer("conv", w, H, W, bf16, stride=s, pad=p)
    z, part, prow = one.layer.forward_bn_stats(_nhwc(x, dtype=_adt(bf16)), B)
    torch.cuda.synchronize()
    assert part.shape[1] == prow and prow > 0 and part.shape[2] >= O
    return one, z.reshape(-1, O), part, prow


def _sums_from_conv(part, prow, C, buf=None, what="sums_from_conv"):
    own = buf is None
    if own:
        buf = _guarded(2 * C, torch.float64)
    _call(_lib.lib().sp_bn_sums_from_conv(P(part[0]), P(part[1]), prow, part.shape[2], C, P(buf), _lib.current_stream()), what)
    return _take(buf, 2 * C, (C, 2), what) if own else None


@DTYPES
def test_a3_sums_from_conv_then_finalize_has_the_bits_of_stats_from_conv(bf16):
    """On the partial rows of ConvT.forward_bn_stats (3x3_64_64: ragged last M tile; 1x1_wide_m: 48-96 partial rows), and the conv1 / downsample
    pair of the header: two layers folded into consecutive slices of ONE float64 buffer leave each other's slice and the guard alone."""
    lib, st = _lib.lib(), _lib.current_stream()
    g = torch.Generator().manual_seed(31)
    alone = []
    for name in ("3x3_64_64", "1x1_wide_m"):
        one, z, part, prow = _random_conv(name, bf16)
        rows, C = z.shape
        _, _, rm0, rv0 = _affine(C, g)
        bufs = _stats_out(C, rm0, rv0)
        _call(lib.sp_bn_train_stats_from_conv(P(part[0]), P(part[1]), prow, part.shape[2], rows, C, EPS, MOM, *(P(b) for b in bufs), st), name)
        fold = _stats_take(bufs, C, name)
        sums = _sums_from_conv(part, prow, C)
        _same_stats(_finalize(sums, rows, C, rm0, rv0), fold, name)
        alone.append((one, part, prow, C, sums.clone()))
    (_, part1, prow1, C1, s1), (_, part2, prow2, C2, s2) = alone
    n = 2 * (C1 + C2)
    buf = _guarded(n, torch.float64)
    _sums_from_conv(part1, prow1, C1, buf=buf[:2 * C1])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[2 * C1:]).all()), "the first layer's fold wrote outside its slice"
    _sums_from_conv(part2, prow2, C2, buf=buf[2 * C1:])
    both = _take(buf, n, (n,), "two layers, one buffer")
    _same_bits(both[:2 * C1].view(C1, 2), s1, "first slice")
    _same_bits(both[2 * C1:].view(C2, 2), s2, "second slice")


@pytest.mark.parametrize("flag", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["3x3_64_64", "1x1_256_1024"])
def test_a4_bwd_sums_from_conv2_has_the_bits_of_the_plain_fold_and_copies_them(name, flag):
    """On the partial rows a ConvT.dgrad(..., bn_src=...) launch leaves: dgamma / dbeta of sp_bn_bwd_sums_from_conv2 = sp_bn_bwd_sums_from_conv's, and the
    message copies are the same values.  The same rows folded with c = 24 (no multiple of the 16-channel slab) and stride = n_pad > c: every output
    holds its first 24 channels and nothing behind them."""
    from simple_pose_amd.train import Act
    _, I, O, k, s, p, H, W, B = next(c for c in STATS_CASES if c[0] == name)
    bf16 = bool(flag & 1)
    adt = _adt(bf16)
    g = torch.Generator().manual_seed(9 + I + O)
    w = (_randn((O, I, k, k), g) / (I * k * k) ** 0.5).float()
    one = _OneLayer("conv", w, H, W, bf16, stride=s, pad=p)
    L = one.layer
    rows, C = B * H * W, I
    zb = _random_shards((rows,), C, g, adt)[0]
    mean, invstd = _dev(zb.mean(0)), _dev(1 / torch.sqrt(zb.var(0, unbiased=False) + EPS))
    yb = torch.relu((zb - zb.mean(0)) * invstd.double().cpu() + 0.1 * _randn(C, g)).to(adt)
    zd, yd = _dev(zb, adt).reshape(B, H, W, C), yb.to(DEV).reshape(B, H, W, C)
    dzn = _randn((B, L.oh, L.ow, L.c_out_buf), g).to(adt).to(DEV)
    src = Act(yd, H, W, C)
    src.bn = (zd, mean, invstd)
    L.dgrad(dzn, B, None, bn_src=src)
    part, prow = src.bstats
    torch.cuda.synchronize()
    stride = part.shape[2]
    assert stride >= C and prow > 0
    lib, st = _lib.lib(), _lib.current_stream()

    def fold(c):
        a = [_guarded(c, torch.float32) for _ in range(2)]
        _call(lib.sp_bn_bwd_sums_from_conv(P(part[0]), P(part[1]), prow, stride, c, P(a[0]), P(a[1]), st), "fold")
        b = [_guarded(c, torch.float32) for _ in range(4)]
        _call(lib.sp_bn_bwd_sums_from_conv2(P(part[0]), P(part[1]), prow, stride, c, *(P(t) for t in b), st), "fold2")
        a = [_take(t, c, (c,), f"fold c={c}") for t in a]
        b = [_take(t, c, (c,), f"fold2 c={c}") for t in b]           # (_take: nothing at index >= c written, everything below it written)
        for nm, x, y in (("dgamma", b[0], a[0]), ("dbeta", b[1], a[1]), ("dgamma_copy", b[2], b[0]), ("dbeta_copy", b[3], b[1])):
            _same_bits(x, y, f"c={c}: {nm}")
        return b

    full = fold(C)
    assert stride > 24
    part24 = fold(24)
    for x, y in zip(part24, full):
        _same_bits(x, y[:24].contiguous(), "a channel's sums do not depend on the layer's width")
    # the sums are the layer's: float64 on the stored dy (the dgrad launch's own output is checked in test_gpu_backward_kernels.py)
    assert float(full[0].abs().max()) > 0 and float(full[1].abs().max()) > 0


# ---- b. exact integer operands ---------------------------------------------------------------------------------------------------------------------
def _int_sums(z):
    return torch.stack((z.sum(0), (z * z).sum(0)), dim=1)


@DTYPES
@pytest.mark.parametrize("rows", SHARDS, ids=SHARD_IDS)
@pytest.mark.parametrize("C", WIDTHS)
def test_b1_b2_partial_sums_of_integer_shards_are_exact_and_add_up_to_the_concatenated_call(C, rows, bf16, ws):
    g = ce.generator(f"syncbn/b1/{C}/{rows}")
    zs = [ce.ints((n, C), 8, g) for n in rows]
    assert all(torch.equal(z.to(_adt(bf16)).double(), z) for z in zs)                        # stored exactly
    assert float(sum((z * z).sum(0).max() for z in zs)) < 2.0 ** 53                          # every sum in any order is an exact double
    got = [_partial(_dev(z, _adt(bf16)), bf16, ws, f"shard {i}") for i, z in enumerate(zs)]
    for i, (p, z) in enumerate(zip(got, zs)):
        assert torch.equal(p.cpu(), _int_sums(z)), f"shard {i}: not the integer column sums"
    total = got[0].clone()
    for p in got[1:]:
        total += p                                                                           # rank order
    whole = _partial(_dev(torch.cat(zs), _adt(bf16)), bf16, ws, "concatenated")
    assert torch.equal(total, whole) and torch.equal(whole.cpu(), _int_sums(torch.cat(zs)))


@DTYPES
@pytest.mark.parametrize("name", sorted(STATS))
def test_b3_sums_from_conv_of_the_exact_conv_cases_are_the_integer_column_sums(name, bf16):
    """The rows of test_statistics_epilogue_sums_are_the_integer_column_sums, through the fold the SyncBatchNorm path uses."""
    _, I, O, k, s, p, H, W, B = next(c for c in STATS_CASES if c[0] == name)
    r = ce.backward_reference("conv", I, O, k, s, p, H, W, B, seed=3, mag=STATS[name])
    ce.backward_conditions(r)
    adt = _adt(bf16)
    cols = r["y"].permute(0, 2, 3, 1).reshape(-1, O)
    ce.stats_conditions(cols, adt)
    one = _OneLayer("conv", r["w"].float(), H, W, bf16, stride=s, pad=p)
    z, part, prow = one.layer.forward_bn_stats(_nhwc(r["x"], dtype=adt), B)
    torch.cuda.synchronize()
    _same_bits(z.reshape(-1, O), cols.to(adt), f"{name} z")
    assert torch.equal(_sums_from_conv(part, prow, O).cpu(), _int_sums(cols))


def test_b4_channel_sum_nhwc_of_integers_is_exact(ws):
    """sp_channel_sum_nhwc accumulates in fp64 and rounds once: small integers come out exactly."""
    lib, st = _lib.lib(), _lib.current_stream()
    for rows in (1, 60, 6144):
        for C in (4, 24, 2048):
            a = ce.ints((rows, C), 8, ce.generator(f"syncbn/b4/{rows}/{C}"))
            assert float(a.abs().sum(0).max()) < ce.LIMIT
            out, ad = _guarded(C, torch.float32), _dev(a)
            _call(lib.sp_channel_sum_nhwc(P(ad), rows, C, P(out), P(ws), st), f"rows={rows} c={C}")
            got = _take(out, C, (C,), f"rows={rows} c={C}")
            assert torch.equal(got.double().cpu(), a.sum(0)), f"rows={rows} c={C}"


@pytest.mark.parametrize("flag", [0, 1, 3], ids=["fp32", "bf16", "bf16_grads"])
@pytest.mark.parametrize("rows", SHARDS, ids=SHARD_IDS)
@pytest.mark.parametrize("C", WIDTHS)
def test_b5_backward_reduction_of_integer_operands_is_exact(C, rows, flag, ws):
    """mean = 0, invstd = 1: xhat = z, so dbeta = sum g and dgamma = sum g z are integers; the ReLU source has both signs."""
    if C == 2048 and rows == (6144,):
        rows = (613,)                                   # (the two-trip width at a size of a few MB; the 6144-row reduction runs at every other width)
    lib, st = _lib.lib(), _lib.current_stream()
    adt, gdt = _adt(flag & 1), _adt(flag & 2)
    g = ce.generator(f"syncbn/b5/{C}/{rows}")
    mean, invstd = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    srcs = []
    for n in rows:
        dy, z, src = ce.ints((n, C), 4, g), ce.ints((n, C), 8, g), ce.ints((n, C), 2, g)
        srcs.append(src)
        gg = dy * (src > 0)
        assert float((gg * z).abs().sum(0).max()) < ce.LIMIT                       # |dy z| rows < 2^24: the final cast to fp32 is exact
        dg, db = _guarded(C, torch.float32), _guarded(C, torch.float32)
        dyd, srcd, zd = _dev(dy, gdt), _dev(src, adt), _dev(z, adt)
        _call(lib.sp_bn_train_bwd_reduce_nhwc(P(dyd), flag, P(srcd), P(zd), P(mean), P(invstd), n, C, P(dg), P(db), P(ws), st), f"rows={n}")
        assert torch.equal(_take(db, C, (C,), "dbeta").double().cpu(), gg.sum(0)), f"rows={n}: dbeta"
        assert torch.equal(_take(dg, C, (C,), "dgamma").double().cpu(), (gg * z).sum(0)), f"rows={n}: dgamma"
    allsrc = torch.cat(srcs)
    assert bool((allsrc > 0).any()) and bool((allsrc < 0).any())


# ---- c. the sharded chain against float64 -----------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("relu,res_on", [(False, False), (True, False), (True, True)], ids=["plain", "relu", "res_relu"])
@pytest.mark.parametrize("C,rows", SHARDED, ids=SHARDED_IDS)
def test_c1_sharded_forward_vs_float64(C, rows, relu, res_on, bf16, ws, measured):
    """Per-shard partial sums, their float64 sum in rank order, then both finishing routes per shard (every emulated rank owns its running
    statistics, started from the same non-trivial values): statistics, running statistics and every shard's y against tests/syncbn_ref.py."""
    g = torch.Generator().manual_seed(300 + C + sum(rows))
    adt = _adt(bf16)
    zs = _random_shards(rows, C, g, adt)
    ress = [_randn((n, C), g).to(adt).double() for n in rows] if res_on else None
    gamma64, beta64, rm0, rv0 = _affine(C, g)
    want = ref.forward(zs, gamma64, beta64, EPS, MOM, rm0, rv0, residuals=ress, relu=relu)
    gamma, beta = _dev(gamma64), _dev(beta64)
    zd = [_dev(z, adt) for z in zs]
    sums = None
    for i, z in enumerate(zd):
        p = _partial(z, bf16, ws, f"shard {i}")
        sums = p.clone() if sums is None else sums + p                     # the all-reduce: rank order, float64
    total = sum(rows)
    worst = dict(mean=0.0, invstd=0.0, running_mean=0.0, running_var=0.0, y=0.0)
    first = None
    for i, z in enumerate(zd):
        res = _dev(ress[i], adt) if res_on else None
        st = _finalize(sums, total, C, rm0, rv0, f"shard {i} finalize")
        st["y"] = _apply(z, bf16, st, gamma, beta, res, relu, what=f"shard {i} apply")
        fused = _apply_sums(z, bf16, sums, total, gamma, beta, res, relu, rm0, rv0, f"shard {i} apply_sums")
        for route in (st, fused):
            for k in ("mean", "invstd", "running_mean", "running_var"):
                worst[k] = max(worst[k], _rel(route[k], want[k]))
            worst["y"] = max(worst["y"], (_rel_bf16 if bf16 else _rel)(route["y"].float(), want["y"][i]))
            first = first or route
            _same_bits(route["mean"], first["mean"], f"shard {i}: every rank publishes the same mean")
            _same_bits(route["invstd"], first["invstd"], f"shard {i}: every rank publishes the same invstd")
    bars = dict(mean=BN_BAR[bf16]["stats"], invstd=BN_BAR[bf16]["stats"], running_mean=BN_BAR[bf16]["stats"], running_var=BN_BAR[bf16]["stats"],
                y=Y_BAR[bf16])
    for k, v in worst.items():
        measured(f"{k}_rel", v, bars[k])
    for k, v in worst.items():
        assert v <= bars[k], (k, v, bars[k])


# the backward flag word: 0 fp32, 1 bf16 activations, 3 + bf16 gradients, 7 + the ReLU source of the apply pass is the forward pass's bit mask (c % 8 == 0)
C2_CASES = [(C, rows, flag, relu) for C, rows in SHARDED for flag in (0, 1, 3, 7) for relu in (True, False)
            if not (flag == 7 and (C % 8 or not relu)) and not (not relu and flag in (1, 3))]
C2_IDS = [f"c{C}-{'x'.join(map(str, r))}-{ {0: 'fp32', 1: 'bf16', 3: 'bf16_grads', 7: 'bf16_grads_relu_mask'}[f]}-{'res_relu' if relu else 'plain'}"
          for C, r, f, relu in C2_CASES]


@pytest.mark.parametrize("C,rows,flag,relu", C2_CASES, ids=C2_IDS)
def test_c2_sharded_backward_vs_float64(C, rows, flag, relu, ws, measured):
    """sp_bn_train_bwd_reduce_nhwc per shard (LOCAL sums: the parameter gradients), their float32 sum in rank order, then
    sp_bn_train_bwd_apply_nhwc(total_rows = all rows, rows = this shard's) per shard.  `relu` cases carry a residual too; the ReLU mask of the
    reference is the kernel's own y (a pre-activation within rounding of 0 has no defined sign).  The last block is a mutation check: dz formed
    with total_rows = rows_i (the local BatchNorm) misses the bar by more than 25x."""
    lib, stream = _lib.lib(), _lib.current_stream()
    bf16, g16, masked = bool(flag & 1), bool(flag & 2), bool(flag & 4)
    adt, gdt = _adt(bf16), _adt(g16)
    g = torch.Generator().manual_seed(400 + C + sum(rows) + flag)
    zs = _random_shards(rows, C, g, adt)
    ress = [_randn((n, C), g).to(adt).double() for n in rows] if relu else None
    dys = [_randn((n, C), g).to(gdt).double() for n in rows]
    gamma64, beta64, rm0, rv0 = _affine(C, g)
    gamma, beta = _dev(gamma64), _dev(beta64)
    total = sum(rows)
    # forward on the device: global statistics, every shard's y (and its bit mask)
    zd = [_dev(z, adt) for z in zs]
    sums = None
    for z in zd:
        p = _partial(z, bf16, ws)
        sums = p.clone() if sums is None else sums + p
    st = _finalize(sums, total, C, rm0, rv0)
    yd, mk = [], []
    for i, z in enumerate(zd):
        m = torch.zeros(rows[i] * C // 8, dtype=torch.uint8, device=DEV) if masked else None
        yd.append(_apply(z, bf16, st, gamma, beta, _dev(ress[i], adt) if relu else None, relu, mask=m))
        mk.append(m)
    fwd = ref.forward(zs, gamma64, beta64, EPS, MOM)
    masks = [(y.double().cpu() > 0).double() for y in yd] if relu else None
    want = ref.backward(zs, dys, fwd["mean"], fwd["invstd"], gamma64, masks)
    bar = BN_BAR[bf16]
    dyd = [_dev(dy, gdt) for dy in dys]
    # local sums
    local, worst = [], dict(local_dgamma=0.0, local_dbeta=0.0)
    for i, n in enumerate(rows):
        dg, db = _guarded(C, torch.float32), _guarded(C, torch.float32)
        _call(lib.sp_bn_train_bwd_reduce_nhwc(P(dyd[i]), flag & 3, P(yd[i]) if relu else None, P(zd[i]), P(st["mean"]), P(st["invstd"]), n, C, P(dg),
                                              P(db), P(ws), stream), f"shard {i} reduce")
        dg, db = _take(dg, C, (C,), f"shard {i} dgamma"), _take(db, C, (C,), f"shard {i} dbeta")
        local.append((dg, db))
        worst["local_dgamma"] = max(worst["local_dgamma"], _rel(dg, want["local_dgamma"][i]))
        worst["local_dbeta"] = max(worst["local_dbeta"], _rel(db, want["local_dbeta"][i]))
    tg, tb = local[0][0].clone(), local[0][1].clone()
    for dg, db in local[1:]:
        tg, tb = tg + dg, tb + db                                        # the all-reduce: rank order, float32
    worst["dgamma"], worst["dbeta"] = _rel(tg, want["dgamma"]), _rel(tb, want["dbeta"])
    bars = dict(local_dgamma=bar["sums"], local_dbeta=bar["sums"], dgamma=bar["sums"], dbeta=bar["sums"], dz=bar["dz"],
                dres=4e-3 if g16 else bar["dres"], dres_accumulate=4e-3 if g16 else bar["dres"])
    worst.update(dz=0.0, dres=0.0, dres_accumulate=0.0)

    def apply(i, total_rows, acc, base=None):
        n = rows[i]
        dz = _guarded(n * C, adt)
        dres = None
        if relu:
            dres = _guarded(n * C, gdt)
            if acc:
                dres[:n * C] = base.reshape(-1)
        _call(lib.sp_bn_train_bwd_apply_nhwc(P(dyd[i]), flag, (P(mk[i]) if masked else P(yd[i])) if relu else None, P(zd[i]), P(st["mean"]),
                                             P(st["invstd"]), P(gamma), P(tg), P(tb), total_rows, n, C, P(dz), P(dres), acc, stream), f"shard {i} apply")
        return _take(dz, n * C, (n, C), f"shard {i} dz"), (_take(dres, n * C, (n, C), f"shard {i} dres") if relu else None)

    rel_dz = _rel_bf16 if bf16 else _rel
    for i, n in enumerate(rows):
        dz, dres = apply(i, total, 0)
        worst["dz"] = max(worst["dz"], rel_dz(dz.float(), want["dz"][i]))
        if relu:
            base = torch.randn(n, C, generator=torch.Generator().manual_seed(1)).to(gdt).to(DEV)
            dz1, dres1 = apply(i, total, 1, base)
            _same_bits(dz1, dz, f"shard {i}: dz does not depend on the accumulate flag")
            if g16:
                worst["dres"] = max(worst["dres"], _rel_bf16(dres.float(), want["dres"][i]))
                worst["dres_accumulate"] = max(worst["dres_accumulate"], _rel_bf16(dres1.float(), base.double().cpu() + want["dres"][i]))
            else:
                worst["dres"] = max(worst["dres"], _rel(dres, want["dres"][i]))
                worst["dres_accumulate"] = max(worst["dres_accumulate"], _rel(dres1 - base, want["dres"][i]))
    for k, v in worst.items():
        measured(f"{k}_rel", v, bars[k])
    for k, v in worst.items():
        assert v <= bars[k], (k, v, bars[k])
    # mutation: the smallest shard's dz with total_rows = its own rows
    i = min(range(len(rows)), key=lambda j: rows[j])
    wrong, _ = apply(i, rows[i], 0)
    e = rel_dz(wrong.float(), want["dz"][i])
    measured("dz_rel_with_total_rows_of_the_shard_alone", e)
    assert e > 25 * bars["dz"], (e, bars["dz"])


@DTYPES
def test_c3_ill_conditioned_channels_through_the_conv_epilogue_route(bf16, measured):
    """1x1_64_128 on an input with a constant offset: output channels with |mean| / std up to about 16.  The epilogue's partial rows are fp32 sums
    over at most tile_m rows, so the variance is off by at most (tile_m - 1) 2^-24 (mean^2 + var) and invstd by half of that relative to var + eps;
    the mean by at most (tile_m - 1) 2^-24 mean|z| plus its own rounding.  No channel reaches the var < 0 -> 0 clamp."""
    one, z, part, prow = _random_conv("1x1_64_128", bf16, offset=6.0)
    rows, C = z.shape
    d = one.layer.d_fwd
    tm, tn = ctypes.c_int(d.tile_m), ctypes.c_int(d.tile_n)
    if tm.value == 0:
        _call(_lib.lib().sp_conv2d_default_tile(d, ctypes.byref(tm), ctypes.byref(tn)), "default tile")
    tile_m = tm.value
    assert tile_m > 0 and prow == -(-rows // tile_m)                       # one partial row per M tile of the launch
    z64 = z.double().cpu()
    mean, var = z64.mean(0), z64.var(0, unbiased=False)
    invstd = 1 / torch.sqrt(var + EPS)
    assert float((mean.abs() / var.sqrt()).max()) >= 12.0                  # the case is what it claims to be
    g = torch.Generator().manual_seed(7)
    _, _, rm0, rv0 = _affine(C, g)
    st = _finalize(_sums_from_conv(part, prow, C), rows, C, rm0, rv0)
    u = 2.0 ** -24
    bound_is = 0.5 * (tile_m - 1) * u * (mean * mean + var) / (var + EPS)
    ratio_is = float((((st["invstd"].double().cpu() - invstd).abs() / invstd) / bound_is).max())
    bound_mu = (tile_m - 1) * u * z64.abs().mean(0) + u * mean.abs()
    ratio_mu = float(((st["mean"].double().cpu() - mean).abs() / bound_mu).max())
    measured("invstd_error_over_derived_bound", ratio_is, 1.0)
    measured("mean_error_over_derived_bound", ratio_mu, 1.0)
    assert ratio_is <= 1.0 and ratio_mu <= 1.0
    assert float(st["invstd"].max()) < EPS ** -0.5


# ---- the width condition of the reduction kernel ----------------------------------------------------------------------------------------------------
def test_every_entry_point_of_the_reduction_refuses_c_1536_and_takes_1024_and_2048(ws):
    """channel_reduce_kernel (and the stem's sibling of the same structure) has a workgroup barrier inside its loop over c/4 channel quads, 256 at a
    time: at c = 1536 half the threads would make one trip more than the others.  Every entry point that launches it answers SP_EINVAL with its
    own name and the same words - checked on the return code alone, nothing of that width is ever launched - and still runs c = 1024 and 2048."""
    lib, st = _lib.lib(), _lib.current_stream()
    B, H, W = 2, 2, 2
    rows = B * H * W
    for C in (1536, 1024, 2048):
        z = _dev(ce.ints((rows, C), 8, ce.generator(f"syncbn/width/{C}")))
        dy = _dev(ce.ints((rows, C), 4, ce.generator(f"syncbn/width/dy/{C}")))
        dyp = dy[:B].contiguous()                                          # the 2x2 maps pool to 1x1
        idx = torch.full((B, 1, 1, C), 4, dtype=torch.uint8, device=DEV)     # the window's centre tap: pixel (0, 0)
        mean, invstd, gamma, beta = (torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.ones(C, device=DEV), torch.zeros(C, device=DEV))
        o = [_guarded(C, torch.float32) for _ in range(9)]
        sums, dz, dz2 = _guarded(2 * C, torch.float64), _guarded(rows * C, torch.float32), _guarded(rows * C, torch.float32)
        calls = {
            "sp_bn_train_stats_nhwc": lambda: lib.sp_bn_train_stats_nhwc(P(z), 0, rows, C, EPS, MOM, P(o[0]), P(o[1]), None, None, P(ws), st),
            "sp_bn_train_partial_nhwc": lambda: lib.sp_bn_train_partial_nhwc(P(z), 0, rows, C, P(sums), P(ws), st),
            "sp_bn_train_bwd_reduce_nhwc": lambda: lib.sp_bn_train_bwd_reduce_nhwc(P(dy), 0, P(z), P(z), P(mean), P(invstd), rows, C, P(o[2]), P(o[3]), P(ws), st),
            "sp_bn_train_bwd_nhwc": lambda: lib.sp_bn_train_bwd_nhwc(P(dy), 0, P(z), P(z), P(mean), P(invstd), P(gamma), rows, C, P(dz), P(o[4]), P(o[5]),
                                                                     None, 0, P(ws), st),
            "sp_channel_sum_nhwc": lambda: lib.sp_channel_sum_nhwc(P(z), rows, C, P(o[6]), P(ws), st),
            "sp_bn_maxpool_bwd_nhwc": lambda: lib.sp_bn_maxpool_bwd_nhwc(P(dyp), 0, P(idx), P(z), P(mean), P(invstd), P(gamma), P(beta), B, H, W, C, P(o[7]),
                                                                         P(o[8]), P(dz2), P(ws), st),
        }
        for name, call in calls.items():
            rc = call()
            if C == 1536:
                msg = lib.sp_last_error().decode()
                assert rc != 0, f"{name} accepted c = 1536"
                assert msg.startswith(f"{name}: bad shape") and msg.endswith("c=1536 (c % 4 == 0; c/4 must be <= 256 or a multiple of 256)"), msg
            else:
                _call(rc, f"{name} c={C}")
        torch.cuda.synchronize()
        if C == 1536:
            assert all(bool(torch.isnan(t).all()) for t in o + [sums, dz, dz2]), "a refused call wrote something"
            continue
        zc = z.double().cpu()
        assert torch.equal(_take(sums, 2 * C, (C, 2), "partial").cpu(), _int_sums(zc))
        assert torch.equal(_take(o[6], C, (C,), "channel sum").double().cpu(), zc.sum(0))
        gg = dy.double().cpu() * (zc > 0)
        assert torch.equal(_take(o[3], C, (C,), "dbeta").double().cpu(), gg.sum(0))
        assert torch.equal(_take(o[2], C, (C,), "dgamma").double().cpu(), (gg * zc).sum(0))
        assert torch.equal(_take(o[0], C, (C,), "mean").double().cpu(), zc.mean(0).float().double())
    # the reduction reads the ReLU source as a tensor: the flag bit of the bit mask is refused, not misread
    C = 64
    t = torch.ones(rows, C, dtype=torch.bfloat16, device=DEV)
    v, dg, db = (torch.ones(C, device=DEV) for _ in range(3))
    assert lib.sp_bn_train_bwd_reduce_nhwc(P(t), 7, P(t), P(t), P(v), P(v), rows, C, P(dg), P(db), P(ws), st) != 0
    assert "bit mask" in lib.sp_last_error().decode()
