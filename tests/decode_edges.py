"""What the decoder edge tests share (tests/test_decode_edges_host.py on the CPU, tests/test_gpu_decode_edges.py on the MI355X): the cases of
tests/golden/g4b_decode_shapes.npz (the real reference's decoders at eleven (map size, kernel size) pairs on hand-built maps,
oracle/gen_golden.py gen_decode_shapes), a NaN-aware comparison, and the reference's two refinement guards restated in numpy."""
import numpy as np

from simple_pose_amd import synth

FIXTURE = "g4b_decode_shapes.npz"
# (H, W, kernel_size): the first three need more than 64 KiB of LDS on the ks = 11 template path (66,656 / 65,696 / 113,184 B), the fourth on
# the generic path at MAX_KS (69,888 B); 17x13 takes the scalar staging loop (W not a multiple of 4 or 12); in 5x4 and 3x50 the GaussTaylor
# guard can never hold; 32x24 at ks = 1 has no padding and blurs with the identity
SHAPES = ((96, 72, 11), (72, 96, 11), (128, 96, 11), (96, 72, 15), (80, 56, 13), (32, 24, 1), (17, 13, 3), (40, 52, 7), (5, 4, 3), (3, 50, 5),
          (1, 1, 1))
B, J = 2, 3
IDS = [f"{h}x{w}_ks{k}" for h, w, k in SHAPES]


def trans_sets():
    return (("ident4", synth.trans_inv_batch(B)), ("rand", synth.trans_inv_batch(B, seed=21)))


def scale_of(tinv):
    """px per unit of |trans_inv|, as tests/test_gpu_parity.py scales its decoder bars."""
    return max(np.abs(tinv[:, :, :2]).sum(-1).max(), 1.0)


def groups(g, H, W, ks):
    """Yields (group index, maps [B,J,H,W], expected {key: array}) of one (size, kernel size)."""
    maps = g[f"{H}x{W}/maps"]
    assert maps.shape[1:] == (B, J, H, W) and maps.dtype == np.float32
    pre = f"{H}x{W}/ks{ks}/"
    for n in range(maps.shape[0]):
        yield n, maps[n], {k[len(pre) + len(str(n)) + 1:]: g[k] for k in g.files if k.startswith(f"{pre}{n}/")}


def names(g, H, W):
    """Name of every map of a size in storage order (the padding repeats the first)."""
    nm = [str(s) for s in g[f"{H}x{W}/names"]]
    total = g[f"{H}x{W}/maps"].shape[0] * B * J
    return nm + [nm[0]] * (total - len(nm))


def max_err(a, b):
    """max |a - b| where both are finite or equal infinities; NaN must stand in the same places, infinities must be equal."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN in different places"
    inf = np.isinf(a) | np.isinf(b)
    assert np.array_equal(a[inf], b[inf]), "infinities differ"
    ok = ~(np.isnan(a) | inf)
    return float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0


def same_bits(a, b):
    """Bit equality of two fp32 arrays, except that any NaN equals any NaN (the payload of a propagated NaN is not the reference's)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


def guards(maps):
    """The guards of pose_metrics.py:39 and :78 on the arg-max of every map: (basic_ok, gauss_taylor_ok) as [B,J] booleans, restated
    with numpy alone (np.argmax: first index of the maximum, NaN wins, as torch.max)."""
    Bn, Jn, H, W = maps.shape
    flat = maps.reshape(Bn, Jn, -1)
    idx = flat.argmax(-1)
    mx = np.take_along_axis(flat, idx[..., None], -1)[..., 0]
    keep = mx > 0
    xi, yi = (idx % W) * keep, (idx // W) * keep
    basic = (xi > 1) & (xi < W - 1) & (yi > 1) & (yi < H - 1)
    gt = (xi > 1) & (xi < W - 2) & (yi > 1) & (yi < H - 2)
    return basic, gt, xi, yi


def affine(coords, tinv):
    """einsum("bcd,bad->bca", [x, y, 1], trans_inv) in float64, rounded once."""
    c = np.concatenate([coords.astype(np.float64), np.ones(coords.shape[:-1] + (1,))], -1)
    return np.einsum("bcd,bad->bca", c, tinv.astype(np.float64)).astype(np.float32)
