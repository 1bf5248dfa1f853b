"""Device JPEG decoder (csrc/jpeg.hip: sp_jpeg_decode_batch, datasets.jpeg.JpegDecoder, GpuAugmentLoader with .jpeg samples) against
the fixture g15_jpeg.npz - PIL's (libjpeg-turbo's) pixels - and tests/jpeg_ref.py.  Every comparison is bitwise.

decode_into: the fixture's 37x53 files are 37 wide and 53 high, so four of them fill a [4, 53, 37, 3] tensor ([B, H, W, 3])."""
import ctypes
import types

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib
from simple_pose_amd.datasets.coco import GpuAugmentLoader
from simple_pose_amd.datasets.jpeg import JpegDecoder
from tests import jpeg_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(golden):
    z = golden("g15_jpeg.npz")
    names = bytes(z["names"]).decode().split("\n")
    out = []
    for i, name in enumerate(names):
        if z["code"][i]:
            continue
        data = bytes(z["bytes"][z["offsets"][i]:z["offsets"][i + 1]])
        px = z["pixels"][z["pixel_offsets"][i]:z["pixel_offsets"][i + 1]].reshape(int(z["shapes"][i, 0]), int(z["shapes"][i, 1]), 3)
        out.append(types.SimpleNamespace(name=name, data=data, pixels=px))
    return out


def _raw_decode(files, stages=_lib.SP_JPEG_STAGE_ALL, slack=0):
    """sp_jpeg_decode_batch through the C ABI with arenas laid out here (tight, `slack` extra bytes between images, all poisoned with
    0xA5 first).  -> (list of uint8 [H,W,3] arrays, status int32 [n], coefficient arena int16, descriptors)."""
    lib = _lib.lib()
    n = len(files)
    descs = (_lib.JpegDesc * n)()
    segs, blob = [], bytearray()
    at = dict(coef=0, plane=0, out=0)
    for i, data in enumerate(files):
        cap = (ctypes.c_int32 * 4096)()
        _lib.check(lib.sp_jpeg_parse(data, len(data), ctypes.byref(descs[i]), cap, 4096), "sp_jpeg_parse")
        d = descs[i]
        assert d.segments <= 4096
        d.seg_index, d.file_offset, d.coef_offset, d.plane_offset, d.out_offset = len(segs), len(blob), at["coef"], at["plane"], at["out"]
        segs += list(cap[:d.segments])
        blob += data + b"\xff" * slack
        at["coef"] += d.coef_count + slack
        at["plane"] += d.plane_bytes + 8 * slack
        at["out"] += d.out_bytes + slack
    dev = "cuda"
    descs_dev = torch.from_numpy(np.frombuffer(descs, np.uint8).copy()).to(dev)
    bytes_dev = torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).to(dev)
    segs_dev = torch.tensor(segs, dtype=torch.int32, device=dev)
    coef = torch.full((max(1, at["coef"]),), 0x5A5A, dtype=torch.int16, device=dev)
    planes = torch.full((max(1, at["plane"]),), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((max(1, at["out"]),), 0xA5, dtype=torch.uint8, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    _lib.check(lib.sp_jpeg_decode_batch(descs, _lib.ptr(descs_dev), n, _lib.ptr(bytes_dev), bytes_dev.numel(), _lib.ptr(segs_dev), segs_dev.numel(),
                                        _lib.ptr(coef), coef.numel(), _lib.ptr(planes), planes.numel(), _lib.ptr(out), out.numel(), _lib.ptr(status),
                                        stages, _lib.current_stream()), "sp_jpeg_decode_batch")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    imgs = [o[d.out_offset:d.out_offset + d.out_bytes].reshape(d.height, d.width, 3) for d in descs]
    if slack and stages == _lib.SP_JPEG_STAGE_ALL:                     # nothing was written between the images
        for d in descs:
            assert (o[d.out_offset + d.out_bytes:d.out_offset + d.out_bytes + slack] == 0xA5).all()
    return imgs, status.cpu().numpy(), coef.cpu().numpy(), descs


def _assert_all_equal(cases, imgs, what):
    for c, got in zip(cases, imgs):
        assert got.shape == c.pixels.shape, (what, c.name)
        assert np.array_equal(got, c.pixels), f"{what}: {c.name}: {int((got != c.pixels).sum())} differing bytes"


def test_whole_fixture_as_one_mixed_batch_equals_libjpeg_bit_for_bit(cases):
    imgs, status, _, _ = _raw_decode([c.data for c in cases], slack=3)
    assert (status == 0).all(), dict(zip([c.name for c in cases], status))
    _assert_all_equal(cases, imgs, "mixed batch")


def test_one_file_per_call_and_reversed_order_give_the_same_bytes(cases):
    for c in cases:
        imgs, status, _, _ = _raw_decode([c.data])
        assert status[0] == 0, c.name
        _assert_all_equal([c], imgs, "single")
    rev = cases[::-1]
    imgs, status, _, _ = _raw_decode([c.data for c in rev])
    assert (status == 0).all()
    _assert_all_equal(rev, imgs, "reversed")


def test_decoder_is_repeatable_and_reuses_its_arenas(cases):
    dec = JpegDecoder("cuda")
    files = [c.data for c in cases]
    first = [t.clone() for t in dec.decode(files)]
    arena = dec._out.data_ptr()
    second = dec.decode(files)
    assert dec._out.data_ptr() == arena
    for c, a, b in zip(cases, first, second):
        assert a.is_cuda and a.dtype == torch.uint8 and tuple(a.shape) == c.pixels.shape
        assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), c.pixels), c.name
    small = dec.decode(files[:2], check=False)                        # a smaller batch in the same arenas, no synchronisation
    assert isinstance(dec.status, torch.Tensor) and dec.status.is_cuda and dec._out.data_ptr() == arena
    assert (dec.status.cpu().numpy() == 0).all() and np.array_equal(small[1].cpu().numpy(), cases[1].pixels)
    assert dec.decode([]) == []
    with pytest.raises(TypeError):
        dec.decode([torch.zeros(4, dtype=torch.uint8)])
    with pytest.raises(TypeError):
        dec.decode(files[0])
    with pytest.raises(_lib.HipLibraryError):
        dec.decode_into(files[:1], torch.zeros((1,) + cases[0].pixels.shape, dtype=torch.uint8))      # CPU tensor


def test_decode_into_fills_a_batch_tensor(cases):
    c = next(c for c in cases if c.name == "m_37x53_420")
    dec = JpegDecoder("cuda")
    out = torch.full((4, 53, 37, 3), 0xA5, dtype=torch.uint8, device="cuda")
    assert dec.decode_into([c.data] * 4, out) is out
    got = out.cpu().numpy()
    for b in range(4):
        assert np.array_equal(got[b], c.pixels)
    with pytest.raises(_lib.HipLibraryError, match="frames"):
        dec.decode_into([c.data, cases[0].data], out[:2])


def test_coefficient_arena_equals_the_reference_for_multi_segment_files(cases):
    multi = [c for c in cases if len(jpeg_ref.parse(c.data).seg_offsets) > 1]
    assert {c.name for c in multi} >= {"rr_17x16_422", "rb2_33x17_420", "r1_40x40_420", "r1_72x64_444"}
    _, status, coef, descs = _raw_decode([c.data for c in multi], stages=_lib.SP_JPEG_STAGE_ENTROPY, slack=5)
    assert (status == 0).all()
    for c, d in zip(multi, descs):
        want, st = jpeg_ref.decode_coefficients(jpeg_ref.parse(c.data), c.data)
        assert st == 0
        flat = np.concatenate([w.reshape(-1) for w in want])
        assert np.array_equal(coef[d.coef_offset:d.coef_offset + d.coef_count], flat), c.name
        assert (coef[d.coef_offset + d.coef_count:d.coef_offset + d.coef_count + 5] == 0x5A5A).all(), c.name      # nothing past the image's region


def test_a_damaged_file_ends_in_its_status_and_leaves_its_neighbours_exact(cases):
    by = {c.name: c for c in cases}
    victim = by["rb2_33x17_420"]
    info = jpeg_ref.parse(victim.data)
    cut = victim.data[:info.ecs_offset + (info.ecs_end - info.ecs_offset) // 2]
    assert jpeg_ref.decode_coefficients(jpeg_ref.parse(cut), cut)[1] != 0
    batch = [by["m_37x53_422"], types.SimpleNamespace(name="cut", data=cut, pixels=victim.pixels), by["r1_40x40_420"]]
    imgs, status, _, _ = _raw_decode([c.data for c in batch], slack=3)
    assert status[0] == 0 and status[2] == 0 and status[1] != 0
    _assert_all_equal([batch[0], batch[2]], [imgs[0], imgs[2]], "neighbours of a damaged file")
    dec = JpegDecoder("cuda")
    with pytest.raises(_lib.HipLibraryError, match=r"files\[1\]"):
        dec.decode([c.data for c in batch])
    out = dec.decode([c.data for c in batch], check=False)
    assert dec.status.cpu().numpy().tolist() == status.tolist()
    assert np.array_equal(out[0].cpu().numpy(), batch[0].pixels) and np.array_equal(out[2].cpu().numpy(), batch[2].pixels)


def test_loader_with_jpeg_samples_equals_the_loader_fed_decoded_images(cases):
    use = [c for c in cases if c.pixels.shape[0] >= 16 and c.pixels.shape[1] >= 16][:8]
    assert len(use) == 8
    def samples(kind):
        out = []
        for i, c in enumerate(use):
            H, W = c.pixels.shape[:2]
            r = np.random.default_rng(100 + i)
            x1, y1 = r.uniform(0, W * 0.3), r.uniform(0, H * 0.3)
            x2, y2 = r.uniform(W * 0.6, W - 1), r.uniform(H * 0.6, H - 1)
            j = np.stack([r.uniform(x1, x2, 17), r.uniform(y1, y2, 17), (r.random(17) > 0.2).astype(np.float64)], 1).astype(np.float32)
            s = types.SimpleNamespace(box=[float(x1), float(y1), float(x2), float(y2)], joints=j, shape=(W, H), img_id=500 + i)
            if kind == "jpeg" or (kind == "mixed" and i % 2 == 0):
                s.jpeg = c.data
            else:
                s.img = torch.from_numpy(np.ascontiguousarray(c.pixels)).cuda()
            out.append(s)
        return out

    def epoch(kind):
        loader = GpuAugmentLoader(samples(kind), 4, 0, 1, seed=9)
        return [([t.clone() for t in b[:4]], b[4]) for b in loader]

    want = epoch("img")
    assert len(want) == 2
    for kind in ("jpeg", "mixed"):
        got = epoch(kind)
        assert len(got) == 2
        for (ta, ia), (tb, ib) in zip(want, got):
            assert ia == ib and all(torch.equal(p, q) for p, q in zip(ta, tb)), kind
