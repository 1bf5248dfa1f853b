"""Device decoding of progressive JPEG files (csrc/jpeg_prog.hip: sp_jpeg_progressive_entropy feeding the IDCT and colour kernels of
csrc/jpeg.hip; datasets.jpeg.JpegDecoder) against the fixture g17_jpeg_prog.npz - PIL's (libjpeg-turbo's) pixels - and
tests/jpeg_prog_ref.py, mixed with the baseline files of g15_jpeg.npz.  Every comparison is bitwise; every image is at most 96x96."""
import ctypes
import types

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib
from simple_pose_amd.datasets.coco import GpuAugmentLoader
from simple_pose_amd.datasets.jpeg import JpegDecoder
from tests import jpeg_prog_ref

pytestmark = pytest.mark.gpu

COEF_POISON, BYTE_POISON = 0x5A5A, 0xA5


def _load(golden, name):
    z = golden(name)
    out = []
    for i, n in enumerate(bytes(z["names"]).decode().split("\n")):
        if z["code"][i]:
            continue
        data = bytes(z["bytes"][z["offsets"][i]:z["offsets"][i + 1]])
        px = z["pixels"][z["pixel_offsets"][i]:z["pixel_offsets"][i + 1]].reshape(int(z["shapes"][i, 0]), int(z["shapes"][i, 1]), 3)
        out.append(types.SimpleNamespace(name=n, data=data, pixels=px))
    return out


@pytest.fixture(scope="module")
def prog(golden):
    return _load(golden, "g17_jpeg_prog.npz")


@pytest.fixture(scope="module")
def base(golden):
    return _load(golden, "g15_jpeg.npz")


@pytest.fixture(scope="module")
def ref_coef(prog):
    """The restatement's coefficient arena of every progressive case (MCU padding included), computed once."""
    out = {}
    for c in prog:
        coef, status = jpeg_prog_ref.decode_coefficients(jpeg_prog_ref.parse_scans(c.data), c.data)
        assert status == 0, c.name
        out[c.name] = coef
    return out


def _raw_decode(files, slack=0, entropy_only=False):
    """The C ABI with arenas laid out here: tight, `slack` extra elements between images (8 * slack bytes between planes), everything
    poisoned first.  Files are placed in the caller's order; the descriptors are [baseline..., progressive...], and the launch order is
    the decoder's: entropy of the baseline files, entropy of the progressive files, IDCT + colour of all.  Checks that nothing was
    written between two regions.  -> (images, status, coefficient arena, descriptors), all in the caller's order."""
    lib = _lib.lib()
    n = len(files)
    parsed, blob = [], bytearray()
    at = dict(coef=0, plane=0, out=0)
    for data in files:
        d = _lib.JpegDesc()
        cap = (ctypes.c_int32 * 4096)()
        scans = None
        rc = lib.sp_jpeg_parse(data, len(data), ctypes.byref(d), cap, 4096)
        if rc == _lib.SP_JPEG_EPROGRESSIVE:
            scans, count = (_lib.JpegScan * 64)(), ctypes.c_int32(0)
            rc = lib.sp_jpeg_parse_scans(data, len(data), ctypes.byref(d), scans, 64, ctypes.byref(count), cap, 4096)
            assert count.value <= 64
            scans = list(scans[:count.value])
        _lib.check(rc, "parse")
        assert d.segments <= 4096
        d.file_offset, d.coef_offset, d.plane_offset, d.out_offset = len(blob), at["coef"], at["plane"], at["out"]
        parsed.append((d, list(cap[:d.segments]), scans))
        blob += data + b"\xff" * slack
        at["coef"] += d.coef_count + slack
        at["plane"] += d.plane_bytes + 8 * slack
        at["out"] += d.out_bytes + slack
    order = [i for i in range(n) if parsed[i][2] is None] + [i for i in range(n) if parsed[i][2] is not None]
    nb = sum(p[2] is None for p in parsed)
    descs = (_lib.JpegDesc * n)()
    segs, all_scans, ranges = [], [], [0]
    for k, i in enumerate(order):
        d, s, scans = parsed[i]
        d.seg_index = len(segs)
        descs[k] = d
        segs += s
        if scans is not None:
            all_scans += scans
            ranges.append(len(all_scans))
    scans_host = (_lib.JpegScan * max(1, len(all_scans)))(*all_scans)
    ranges_host = (ctypes.c_int32 * len(ranges))(*ranges)
    dev = "cuda"
    up = lambda a: torch.from_numpy(np.frombuffer(a, np.uint8).copy()).to(dev)
    descs_dev, scans_dev, ranges_dev, bytes_dev = up(descs), up(scans_host), up(ranges_host), up(bytes(blob))
    segs_dev = torch.tensor(segs, dtype=torch.int32, device=dev)
    coef = torch.full((max(1, at["coef"]),), COEF_POISON, dtype=torch.int16, device=dev)
    planes = torch.full((max(1, at["plane"]),), BYTE_POISON, dtype=torch.uint8, device=dev)
    out = torch.full((max(1, at["out"]),), BYTE_POISON, dtype=torch.uint8, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    size = ctypes.sizeof(_lib.JpegDesc)

    def batch(first, count, stages):
        _lib.check(lib.sp_jpeg_decode_batch(ctypes.addressof(descs) + first * size, descs_dev.data_ptr() + first * size, count, _lib.ptr(bytes_dev),
                                            bytes_dev.numel(), _lib.ptr(segs_dev), segs_dev.numel(), _lib.ptr(coef), coef.numel(), _lib.ptr(planes),
                                            planes.numel(), _lib.ptr(out), out.numel(), status.data_ptr() + 4 * first, stages, _lib.current_stream()),
                   "sp_jpeg_decode_batch")

    if nb:
        batch(0, nb, _lib.SP_JPEG_STAGE_ENTROPY)
    if n - nb:
        _lib.check(lib.sp_jpeg_progressive_entropy(ctypes.addressof(descs) + nb * size, descs_dev.data_ptr() + nb * size, n - nb, scans_host,
                                                   _lib.ptr(scans_dev), ranges_host, _lib.ptr(ranges_dev), len(all_scans), _lib.ptr(bytes_dev),
                                                   bytes_dev.numel(), _lib.ptr(segs_dev), segs_dev.numel(), _lib.ptr(coef), coef.numel(),
                                                   status.data_ptr() + 4 * nb, _lib.current_stream()), "sp_jpeg_progressive_entropy")
    if not entropy_only:
        batch(0, n, _lib.SP_JPEG_STAGE_IDCT | _lib.SP_JPEG_STAGE_COLOR)
    torch.cuda.synchronize()
    o, cf, pl, st = out.cpu().numpy(), coef.cpu().numpy(), planes.cpu().numpy(), status.cpu().numpy()
    where = np.empty(n, np.int64)
    where[order] = np.arange(n)
    by_file = [parsed[i][0] for i in range(n)]
    if slack:                                                      # nothing was written between the regions
        for d in by_file:
            assert (cf[d.coef_offset + d.coef_count:d.coef_offset + d.coef_count + slack] == COEF_POISON).all()
            if not entropy_only:
                assert (o[d.out_offset + d.out_bytes:d.out_offset + d.out_bytes + slack] == BYTE_POISON).all()
                assert (pl[d.plane_offset + d.plane_bytes:d.plane_offset + d.plane_bytes + 8 * slack] == BYTE_POISON).all()
    imgs = [o[d.out_offset:d.out_offset + d.out_bytes].reshape(d.height, d.width, 3) for d in by_file]
    return imgs, st[where], cf, by_file


def _assert_all_equal(cases, imgs, what):
    for c, got in zip(cases, imgs):
        assert got.shape == c.pixels.shape, (what, c.name)
        assert np.array_equal(got, c.pixels), f"{what}: {c.name}: {int((got != c.pixels).sum())} differing bytes"


def _interleaved(prog, base):
    out = []
    for i in range(max(len(prog), len(base))):
        out += prog[i:i + 1] + base[i:i + 1]
    return out


def test_one_mixed_batch_of_both_fixtures_equals_libjpeg_bit_for_bit(prog, base):
    cases = _interleaved(prog, base)
    assert len(cases) == len(prog) + len(base)
    imgs, status, _, _ = _raw_decode([c.data for c in cases], slack=3)
    assert (status == 0).all(), dict(zip([c.name for c in cases], status))
    _assert_all_equal(cases, imgs, "mixed batch")


def test_one_file_per_call_and_reversed_order_give_the_same_bytes(prog, base):
    for c in prog:
        imgs, status, _, _ = _raw_decode([c.data])
        assert status[0] == 0, c.name
        _assert_all_equal([c], imgs, "single")
    rev = _interleaved(prog, base)[::-1]
    imgs, status, _, _ = _raw_decode([c.data for c in rev])
    assert (status == 0).all()
    _assert_all_equal(rev, imgs, "reversed")


def test_coefficient_arena_after_the_entropy_entry_equals_the_reference(prog, ref_coef):
    _, status, coef, descs = _raw_decode([c.data for c in prog], slack=5, entropy_only=True)
    assert (status == 0).all(), dict(zip([c.name for c in prog], status))
    for c, d in zip(prog, descs):
        flat = np.concatenate([w.reshape(-1) for w in ref_coef[c.name]])
        assert flat.size == d.coef_count, c.name
        assert np.array_equal(coef[d.coef_offset:d.coef_offset + d.coef_count], flat), c.name
    # the MCU padding of p_17x9_420: luma is 3 blocks wide in its own scans and 4 in the arena; the fourth column got its DC from the
    # interleaved DC scans and nothing from the luma AC scans
    i = [c.name for c in prog].index("p_17x9_420")
    d = descs[i]
    luma = coef[d.coef_offset:d.coef_offset + d.mcus_x * 2 * d.mcus_y * 2 * 64].reshape(d.mcus_y * 2, d.mcus_x * 2, 64)
    assert luma.shape[:2] == (2, 4) and (luma[:, 3, 0] != 0).all() and not luma[:, 3, 1:].any() and luma[:, :3, 1:].any()


def test_decoder_returns_the_callers_order_is_repeatable_and_reuses_its_arenas(prog, base):
    cases = _interleaved(prog, base)
    files = [c.data for c in cases]
    dec = JpegDecoder("cuda")
    first = [t.clone() for t in dec.decode(files)]
    arena = dec._out.data_ptr()
    assert (dec.status.cpu().numpy() == 0).all() and dec.status.numel() == len(files)
    second = dec.decode(files)
    assert dec._out.data_ptr() == arena
    for c, a, b in zip(cases, first, second):
        assert a.is_cuda and a.dtype == torch.uint8 and tuple(a.shape) == c.pixels.shape
        assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), c.pixels), c.name
    # a baseline-only batch and a progressive-only one through the same object, in the same arenas
    only = dec.decode([c.data for c in base[:3]], check=False)
    assert dec._out.data_ptr() == arena and (dec.status.cpu().numpy() == 0).all()
    _assert_all_equal(base[:3], [t.cpu().numpy() for t in only], "baseline only")
    only = dec.decode([c.data for c in prog[:3]])
    assert dec._out.data_ptr() == arena
    _assert_all_equal(prog[:3], [t.cpu().numpy() for t in only], "progressive only")


def test_decode_into_fills_a_batch_tensor_from_the_three_37x53_files(prog):
    by = {c.name: c for c in prog}
    three = [by["p_37x53_444"], by["p_37x53_422"], by["p_37x53_420"]]
    dec = JpegDecoder("cuda")
    out = torch.full((3, 53, 37, 3), 0xA5, dtype=torch.uint8, device="cuda")
    assert dec.decode_into([c.data for c in three], out) is out
    got = out.cpu().numpy()
    for b, c in enumerate(three):
        assert np.array_equal(got[b], c.pixels), c.name


def test_relaunch_of_the_entropy_stage_reproduces_the_coefficients(prog, base, ref_coef):
    cases = [base[4], prog[1], prog[5], base[0], prog[11]]
    dec = JpegDecoder("cuda")
    want = [t.clone() for t in dec.decode([c.data for c in cases])]
    coef, offsets, counts = dec.coefficients
    before = coef.clone()
    coef.fill_(0x1234)
    dec.relaunch(_lib.SP_JPEG_STAGE_ENTROPY)
    assert (dec.status.cpu().numpy() == 0).all()
    for c, o, n in zip(cases, offsets, counts):
        assert torch.equal(coef[o:o + n], before[o:o + n]), c.name
        if c.name in ref_coef:
            assert np.array_equal(coef[o:o + n].cpu().numpy(), np.concatenate([w.reshape(-1) for w in ref_coef[c.name]])), c.name
    dec._out.fill_(0)
    dec.relaunch(_lib.SP_JPEG_STAGE_IDCT | _lib.SP_JPEG_STAGE_COLOR)
    for c, w, g in zip(cases, want, dec.decode([c.data for c in cases])):
        assert torch.equal(w, g), c.name


def test_a_damaged_progressive_file_ends_in_its_status_and_leaves_its_neighbours_exact(prog, base):
    """p_r2_33x17_420 with the second half of the first restart segment of its fifth scan cut out: the file still parses (every scan is
    there), the segment runs out of bits."""
    by = {c.name: c for c in prog}
    victim = by["p_r2_33x17_420"]
    s = jpeg_prog_ref.parse_scans(victim.data).scans[4]
    a, b = s.seg_offsets[0], s.seg_offsets[1] - 2
    cut = victim.data[:a + (b - a) // 2] + victim.data[b:]
    info = jpeg_prog_ref.parse_scans(cut)
    assert len(info.scans) == 10 and jpeg_prog_ref.decode_coefficients(info, cut)[1] != 0
    batch = [by["p_37x53_422"], types.SimpleNamespace(name="cut", data=cut, pixels=victim.pixels), base[3], by["c_split_dc_40x40_420"]]
    imgs, status, _, _ = _raw_decode([c.data for c in batch], slack=3)
    assert status[1] != 0 and status[0] == 0 and status[2] == 0 and status[3] == 0, status
    _assert_all_equal([batch[0], batch[2], batch[3]], [imgs[0], imgs[2], imgs[3]], "neighbours of a damaged file")
    dec = JpegDecoder("cuda")
    with pytest.raises(_lib.HipLibraryError, match=r"files\[1\] is damaged"):
        dec.decode([c.data for c in batch])
    out = dec.decode([c.data for c in batch], check=False)
    assert dec.status.cpu().numpy().tolist() == status.tolist()
    for k in (0, 2, 3):
        assert np.array_equal(out[k].cpu().numpy(), batch[k].pixels), batch[k].name
    with pytest.raises(_lib.HipLibraryError, match=r"files\[2\]: .*progression ends"):
        dec.decode([victim.data, base[0].data, victim.data[:s.ecs_offset] + b"\xff\xd9"])


def test_loader_with_progressive_jpeg_samples_equals_the_loader_fed_decoded_images(prog):
    use = [c for c in prog if c.pixels.shape[0] >= 16 and c.pixels.shape[1] >= 16][:8]
    assert len(use) == 8

    def epoch(kind):
        samples = []
        for i, c in enumerate(use):
            H, W = c.pixels.shape[:2]
            r = np.random.default_rng(300 + i)
            x1, y1 = r.uniform(0, W * 0.3), r.uniform(0, H * 0.3)
            x2, y2 = r.uniform(W * 0.6, W - 1), r.uniform(H * 0.6, H - 1)
            j = np.stack([r.uniform(x1, x2, 17), r.uniform(y1, y2, 17), (r.random(17) > 0.2).astype(np.float64)], 1).astype(np.float32)
            s = types.SimpleNamespace(box=[float(x1), float(y1), float(x2), float(y2)], joints=j, shape=(W, H), img_id=700 + i)
            if kind == "jpeg":
                s.jpeg = c.data
            else:
                s.img = torch.from_numpy(np.ascontiguousarray(c.pixels)).cuda()
            samples.append(s)
        return [([t.clone() for t in b[:4]], b[4]) for b in GpuAugmentLoader(samples, 4, 0, 1, seed=11)]

    want, got = epoch("img"), epoch("jpeg")
    assert len(want) == len(got) == 2
    for (ta, ia), (tb, ib) in zip(want, got):
        assert ia == ib and all(torch.equal(p, q) for p, q in zip(ta, tb))
