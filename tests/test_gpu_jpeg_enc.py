"""Device JPEG encoder (csrc/jpeg_enc.hip: sp_jpeg_encode_batch, datasets.jpeg.JpegEncoder) against the fixture g16_jpeg_enc.npz - the
files Pillow / libjpeg-turbo wrote - and tests/jpeg_enc_ref.py, which tests/test_jpeg_enc_host.py pins to the same files.  Every
comparison is of whole files, byte for byte."""
import types

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib
from simple_pose_amd.datasets.jpeg import JpegDecoder, JpegEncoder
from tests import jpeg_enc_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SUB = {444: "4:4:4", 422: "4:2:2", 420: "4:2:0"}


@pytest.fixture(scope="module")
def cases(golden):
    z = golden("g16_jpeg_enc.npz")
    names = bytes(z["image_names"]).decode().split("\n")
    out = []
    for c, (i, sub, q, r) in enumerate(z["cases"].tolist()):
        h, w = z["image_shapes"][i].tolist()
        img = z["images"][z["image_offsets"][i]:z["image_offsets"][i + 1]].reshape(h, w, 3)
        out.append(types.SimpleNamespace(name=names[i], image=img, sub=sub, q=q, r=r, data=bytes(z["bytes"][z["offsets"][c]:z["offsets"][c + 1]])))
    return out


def _gpu(img):
    return torch.from_numpy(np.ascontiguousarray(img)).to(DEV)


def _pick(cases, name, sub, q, r):
    return next(c for c in cases if (c.name, c.sub, c.q, c.r) == (name, sub, q, r))


def test_every_golden_case_in_mixed_size_batches(cases):
    """One batch per (sampling, quality, interval): the seven sizes (three with restart markers) side by side in one call."""
    groups = {}
    for c in cases:
        groups.setdefault((c.sub, c.q, c.r), []).append(c)
    assert len(groups) == 38 and max(len(g) for g in groups.values()) == 7
    for (sub, q, r), g in groups.items():
        enc = JpegEncoder(DEV, quality=q, subsampling=SUB[sub], restart_interval=r)
        files = enc.encode([_gpu(c.image) for c in g])
        assert enc.status.cpu().tolist() == [0] * len(g)
        for c, f in zip(g, files):
            assert f == c.data, (c.name, sub, q, r, len(f), len(c.data))


def test_one_tensor_batch_and_empty_batch(cases):
    c = _pick(cases, "smooth_33x16", 422, 75, 0)
    enc = JpegEncoder(DEV, quality=75, subsampling="4:2:2")
    assert enc.encode(_gpu(np.stack([c.image, c.image[::-1], c.image])))[0::2] == [c.data, c.data]
    assert enc.encode([]) == [] and enc.encode(torch.empty(0, 8, 8, 3, dtype=torch.uint8, device=DEV)) == []


def test_encode_device_stage_by_stage_and_the_coefficients(cases):
    g = [_pick(cases, n, 420, 75, 3) for n in ("smooth_17x23", "smooth_9x41", "smooth_64x50")]
    enc = JpegEncoder(DEV, quality=75, subsampling="4:2:0", restart_interval=3)
    frames = [_gpu(c.image) for c in g]
    files = enc.encode(frames)
    arena, offsets, lengths = enc.encode_device(frames)
    assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.cpu().tolist() == [len(c.data) for c in g]
    host = arena.cpu().numpy()
    for c, f, o in zip(g, files, offsets):
        assert f == c.data and host[o:o + len(f)].tobytes() == f
    # the same batch again, one stage per call, after everything the stages leave has been overwritten
    coef, coef_at, coef_n = enc.coefficients
    enc._ws.fill_(0xA5)
    arena.fill_(0xA5)
    lengths.fill_(-1)
    enc.status.fill_(-1)
    enc.relaunch(_lib.SP_JPEG_ENC_STAGE_COEF)
    zz, real = ref.coefficients(g[0].image, 420, 75)
    got = coef[coef_at[0]:coef_at[0] + coef_n[0]].cpu().numpy().reshape(-1, 64)
    assert not real.all() and np.array_equal(got, zz)             # 17x23 at 4:2:0 has dummy blocks on both edges: they are zero
    for stage in (_lib.SP_JPEG_ENC_STAGE_SCAN, _lib.SP_JPEG_ENC_STAGE_EMIT, _lib.SP_JPEG_ENC_STAGE_STUFF):
        enc.relaunch(stage)
    assert lengths.cpu().tolist() == [len(c.data) for c in g] and enc.status.cpu().tolist() == [0, 0, 0]
    host = arena.cpu().numpy()
    for c, o in zip(g, offsets):
        assert host[o:o + len(c.data)].tobytes() == c.data
    enc.relaunch()
    assert arena.cpu().numpy()[offsets[2]:offsets[2] + len(g[2].data)].tobytes() == g[2].data


@pytest.mark.parametrize("sub, r", [(444, 0), (444, 7), (422, 0), (422, 7), (420, 0), (420, 7), (444, 1)])
def test_frame_larger_than_one_workgroup_share(sub, r):
    """136x200 noise at quality 95.  The three prefix sums work in chunks of 256 elements (one workgroup each): this frame has 1275 /
    900 / 702 blocks (4:4:4 / 4:2:2 / 4:2:0), so the bit offsets cross two chunk boundaries at least; its file is 33 KB and more, so
    the stuffed-byte counts cross the 4096-byte chunks of the third sum many times, and the emit / coefficient launches take several
    workgroups.  r = 1 at 4:4:4 gives 425 restart segments: the sum over segments crosses a chunk as well."""
    img = np.random.RandomState(136200).randint(0, 256, (200, 136, 3)).astype(np.uint8)
    want = ref.encode(img, sub, 95, r)
    assert len(want) > 8 * 4096
    enc = JpegEncoder(DEV, quality=95, subsampling=SUB[sub], restart_interval=r)
    assert enc.descs is None and enc._plan_for(136, 200).blocks > 2 * 256
    got = enc.encode([_gpu(img)])[0]
    assert got == want, (len(got), len(want))


@pytest.mark.parametrize("amp, q, r", [(96, 75, 0), (3, 25, 128)])
def test_more_chunks_than_one_pass_of_the_chunk_scan(amp, q, r):
    """1024x1408 at 4:4:4 has 67584 blocks = 264 chunks: the workgroup that scans an image's chunk sums 256 at a time takes a second
    pass with a carry.  With noise of amplitude 96 at quality 75 the file has 1.49 MB = 365 chunks of 4096 stream bytes, so the third sum
    takes a second pass too; the smooth variant (few non-zero coefficients) does the same with a restart interval of one MCU row."""
    yy, xx = np.mgrid[0:1408, 0:1024]
    img = np.stack([(xx * 3 + yy * 2) >> 4, (xx + yy * 5) >> 5, 255 - ((xx * 2 + yy) >> 4)], -1) + np.random.RandomState(7).randint(0, amp, (1408, 1024, 3))
    img = (img & 255).astype(np.uint8)
    want = ref.encode(img, 444, q, r)
    assert amp < 96 or len(want) > 256 * 4096
    enc = JpegEncoder(DEV, quality=q, subsampling="4:4:4", restart_interval=r)
    assert enc._plan_for(1024, 1408).blocks == 67584 > 256 * 256
    assert enc.encode(_gpu(img)[None])[0] == want


def test_round_trip_through_the_device_decoder(cases):
    dec = JpegDecoder(DEV)
    for name, sub, q, r in [("noise_64x50", 420, 95, 1), ("noise_64x50", 444, 95, 7), ("smooth_9x41", 422, 25, 3), ("noise_17x23", 420, 95, 0),
                            ("smooth_1x1", 420, 75, 0), ("noise_17x23", 420, 100, 0)]:
        c = _pick(cases, name, sub, q, r)
        enc = JpegEncoder(DEV, quality=q, subsampling=SUB[sub], restart_interval=r)
        mine = dec.decode(enc.encode([_gpu(c.image)]))[0].cpu().numpy()
        assert dec.status.cpu().tolist() == [0]
        theirs = dec.decode([c.data])[0].cpu().numpy()
        assert np.array_equal(mine, theirs) and mine.shape == c.image.shape


def test_overflow_is_a_status_and_writes_nothing(cases):
    big, small = _pick(cases, "noise_17x23", 420, 95, 0), _pick(cases, "noise_8x8", 420, 95, 0)
    assert len(small.data) < len(big.data) - 1
    enc = JpegEncoder(DEV, quality=95, subsampling="4:2:0")
    frames = [_gpu(big.image), _gpu(small.image)]
    assert enc.encode(frames) == [big.data, small.data]                      # sizes the arenas
    for cap in (len(big.data) - 1, len(small.data), 700, 0):                 # 700: the header fits, the first byte of data does not
        enc._out.fill_(0xA5)
        arena, offsets, lengths = enc.encode_device(frames, capacity=cap)
        assert arena.data_ptr() == enc._out.data_ptr()
        fits = cap >= len(small.data)
        assert enc.status.cpu().tolist() == [_lib.SP_JPEG_ENC_STATUS_OVERFLOW, 0 if fits else _lib.SP_JPEG_ENC_STATUS_OVERFLOW]
        assert lengths.cpu().tolist() == [0, len(small.data) if fits else 0]
        host = arena.cpu().numpy().copy()
        if fits:
            o = offsets[1]
            assert host[o:o + len(small.data)].tobytes() == small.data
            host[o:o + len(small.data)] = 0xA5
        assert (host == 0xA5).all()                                          # guard bytes and the refused file's region: untouched
        with pytest.raises(_lib.HipLibraryError, match=r"frames\[0\] does not fit"):
            enc.encode(frames, capacity=cap)
    assert enc.encode(frames, capacity=len(big.data)) == [big.data, small.data]


def test_input_may_be_overwritten_right_after_the_call(cases):
    g = [_pick(cases, n, 420, 75, 0) for n in ("smooth_64x50", "smooth_33x16")]
    enc = JpegEncoder(DEV, quality=75, subsampling="4:2:0")
    frames = [_gpu(c.image) for c in g]
    arena, offsets, lengths = enc.encode_device(frames)
    for f in frames:
        f.fill_(255)                                                          # same stream: ordered after the encoder's reads
    host, n = arena.cpu().numpy(), lengths.cpu().tolist()
    for c, o, k in zip(g, offsets, n):
        assert host[o:o + k].tobytes() == c.data


def test_encoder_on_a_side_stream(cases):
    c = _pick(cases, "noise_64x50", 444, 95, 3)
    enc = JpegEncoder(DEV, quality=95, subsampling="4:4:4", restart_interval=3)
    x = _gpu(c.image)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        assert enc.encode([x]) == [c.data]
