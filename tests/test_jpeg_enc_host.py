"""The JPEG encoder's host half, on a machine without a GPU: the numpy restatement (tests/jpeg_enc_ref.py) against the files Pillow /
libjpeg-turbo wrote (tests/golden/g16_jpeg_enc.npz, byte for byte), sp_jpeg_enc_plan's header, tables and refusals, sp_jpeg_parse on
every fixture file, and JpegEncoder's argument errors, none of which makes a GPU call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from simple_pose_amd import _lib
from simple_pose_amd.datasets import jpeg
from tests import jpeg_enc_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(ref.GOLDEN, allow_pickle=False)
NAMES = bytes(Z["image_names"]).decode().split("\n")
CASES = [tuple(c) for c in Z["cases"].tolist()]


def image(i):
    h, w = Z["image_shapes"][i].tolist()
    return Z["images"][Z["image_offsets"][i]:Z["image_offsets"][i + 1]].reshape(h, w, 3)


def golden(c):
    return bytes(Z["bytes"][Z["offsets"][c]:Z["offsets"][c + 1]])


def plan(w, h, sub, q, r):
    d = _lib.JpegEncDesc()
    rc = _lib.lib().sp_jpeg_enc_plan(w, h, sub, q, r, ctypes.byref(d))
    return rc, d


def test_fixture_holds_the_cases_the_encoder_is_specified_by():
    sizes = {(1, 1), (8, 8), (16, 16), (17, 23), (9, 41), (33, 16), (64, 50)}
    assert {tuple(s[::-1]) for s in Z["image_shapes"].tolist()} == sizes and len(NAMES) == 14
    have = {(NAMES[i].split("_")[1], sub, q, r) for i, sub, q, r in CASES}
    for w, h in sizes:
        for sub in (444, 422, 420):
            for q in (25, 75, 95):
                assert (f"{w}x{h}", sub, q, 0) in have
                for r in (1, 3, 7):
                    assert ((f"{w}x{h}", sub, q, r) in have) == ((w, h) in {(17, 23), (9, 41), (64, 50)})
    assert {q for _, _, q, _ in CASES} == {1, 25, 75, 95, 100}
    assert os.path.getsize(ref.GOLDEN) < 400 * 1024


def test_restatement_equals_libjpeg_turbo_on_every_case():
    stats = {}
    for c, (i, sub, q, r) in enumerate(CASES):
        assert ref.encode(image(i), sub, q, r, stats) == golden(c), (NAMES[i], sub, q, r)
    assert stats["stuffed"] > 0 and stats["zrl"] > 0 and stats["c63"] > 0, stats


def test_plan_header_equals_the_golden_header_on_every_case():
    for c, (i, sub, q, r) in enumerate(CASES):
        h, w = image(i).shape[:2]
        rc, d = plan(w, h, sub, q, r)
        assert rc == 0
        g = golden(c)
        sos = g.index(b"\xff\xda")
        n = sos + 2 + ((g[sos + 2] << 8) | g[sos + 3])
        assert d.header_bytes == n <= _lib.SP_JPEG_ENC_HEADER_MAX and bytes(d.header[:n]) == g[:n], (NAMES[i], sub, q, r)
        assert d.header_bytes == len(ref.header(w, h, sub, q, r))


@pytest.mark.parametrize("q", [1, 25, 50, 75, 100])
def test_scaled_tables_and_huffman_codes(q):
    rc, d = plan(16, 16, 420, q, 0)
    assert rc == 0
    assert np.array_equal(np.ctypeslib.as_array(d.quant), ref.quant_tables(q))
    if q == 50:
        assert np.array_equal(np.ctypeslib.as_array(d.quant), Z["std_quant"])
    for t in range(4):
        code, length = ref.huff_codes(t)
        assert np.array_equal(np.ctypeslib.as_array(d.hcode)[t], code) and np.array_equal(np.ctypeslib.as_array(d.hlen)[t], length)


def test_plan_geometry_and_workspace_layout():
    for w, h, sub in [(17, 23, 420), (17, 23, 422), (17, 23, 444), (64, 50, 420), (1, 1, 420), (1920, 1080, 420), (16384, 16384, 444)]:
        rc, d = plan(w, h, sub, 75, 7)
        assert rc == 0
        g = ref.geometry(w, h, sub)
        assert (d.h_samp, d.v_samp, d.mcus_x, d.mcus_y) == (g["hs"], g["vs"], g["mcus_x"], g["mcus_y"])
        assert list(d.wb) == g["wb"] and list(d.hb) == g["hb"]
        mcus = g["mcus_x"] * g["mcus_y"]
        assert d.blocks_per_mcu == g["hs"] * g["vs"] + 2 and d.blocks == mcus * d.blocks_per_mcu and d.segments == -(-mcus // 7)
        at = [64, d.ws_coef, d.ws_bits, d.ws_pos, d.ws_seg, d.ws_chunk, d.ws_bytes]
        need = [0, d.blocks * 128, d.blocks * 2, (d.blocks + 1) * 8, (d.segments + 1) * 8, (-(-max(d.blocks, d.segments) // 256) + 1) * 8]
        assert at[1] == 64 and all(a % 64 == 0 for a in at) and all(at[k + 1] - at[k] >= need[k] for k in range(1, 6))
        assert (d.src, d.ws_offset, d.out_offset, d.out_capacity) == (0, 0, 0, 0)
    assert _lib.jpeg_enc_stream_ws(0) == 128 and _lib.jpeg_enc_stream_ws(4096) == 64 + 4096 + 64


@pytest.mark.parametrize("args, code", [((0, 8, 420, 75, 0), _lib.SP_JPEG_ESIZE), ((8, 0, 420, 75, 0), _lib.SP_JPEG_ESIZE),
                                        ((16385, 8, 420, 75, 0), _lib.SP_JPEG_ESIZE), ((8, 16385, 420, 75, 0), _lib.SP_JPEG_ESIZE),
                                        ((8, 8, 411, 75, 0), _lib.SP_JPEG_ESAMPLING), ((8, 8, 0, 75, 0), _lib.SP_JPEG_ESAMPLING),
                                        ((8, 8, 420, 0, 0), -1), ((8, 8, 420, 101, 0), -1), ((8, 8, 420, 75, -1), -1), ((8, 8, 420, 75, 65536), -1)])
def test_plan_refusals(args, code):
    rc, _ = plan(*args)
    assert rc == code
    msg = _lib.lib().sp_last_error().decode()
    assert msg.startswith("sp_jpeg_enc_plan:") and len(msg) > 20
    assert _lib.lib().sp_jpeg_enc_plan(8, 8, 420, 75, 0, None) == -1


def test_parser_accepts_every_golden_file_and_agrees_with_the_plan():
    for c, (i, sub, q, r) in enumerate(CASES):
        h, w = image(i).shape[:2]
        info = jpeg.parse(golden(c))
        rc, d = plan(w, h, sub, q, r)
        assert rc == 0
        assert (info.width, info.height, info.components, info.restart_interval) == (w, h, 3, r)
        assert info.mcus == (d.mcus_x, d.mcus_y) and info.sampling == ((d.h_samp, d.v_samp), (1, 1), (1, 1))
        assert len(info.seg_offsets) == d.segments and info.ecs_offset == d.header_bytes
        assert np.array_equal(info.quant[0][ref.ZIGZAG], np.ctypeslib.as_array(d.quant)[0])


def test_header_declares_and_library_exports_the_encoder_entries():
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", hdr))
    handle = _lib.lib()
    for name in ("sp_jpeg_enc_plan", "sp_jpeg_encode_batch"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(handle, name), name
    for name, value in re.findall(r"#define (SP_JPEG_ENC_[A-Z_]+) (\d+)", hdr):
        assert getattr(_lib, name) == int(value), name
    assert ctypes.sizeof(_lib.JpegEncDesc) % 8 == 0 and _lib.JpegEncDesc.src.offset % 8 == 0
    # the batch entry checks the host descriptors before it touches a device pointer: a descriptor that is not the planner's is refused
    rc, d = plan(16, 16, 420, 75, 0)
    d.blocks += 1
    assert handle.sp_jpeg_encode_batch(ctypes.byref(d), None, 1, None, 0, None, 0, None, None, 15, None) == -1
    assert "sp_jpeg_enc_plan" in handle.sp_last_error().decode()
    rc, d = plan(16, 16, 420, 75, 0)
    d.src, d.out_capacity = 64, 1024
    assert handle.sp_jpeg_encode_batch(ctypes.byref(d), None, 1, None, 0, None, 1024, None, None, 15, None) == -1
    assert "workspace" in handle.sp_last_error().decode()
    assert handle.sp_jpeg_encode_batch(ctypes.byref(d), None, 1, None, 1 << 30, None, 1023, None, None, 15, None) == -1
    assert "output" in handle.sp_last_error().decode()
    assert handle.sp_jpeg_encode_batch(ctypes.byref(d), None, 1, None, 1 << 30, None, 1024, None, None, 16, None) == -1
    assert handle.sp_jpeg_encode_batch(ctypes.byref(d), None, 1, None, 1 << 30, None, 1024, None, None, 15, None) == -1
    assert "null pointer" in handle.sp_last_error().decode()
    assert handle.sp_jpeg_encode_batch(None, None, 0, None, 0, None, 0, None, None, 15, None) == 0


def test_encoder_argument_errors_come_before_any_gpu_call():
    with pytest.raises(_lib.HipLibraryError, match="subsampling"):
        jpeg.JpegEncoder("cuda:0", subsampling="4:1:1")
    with pytest.raises(_lib.HipLibraryError, match="quality 0"):
        jpeg.JpegEncoder("cuda:0", quality=0)
    with pytest.raises(_lib.HipLibraryError, match="quality 101"):
        jpeg.JpegEncoder("cuda:0", quality=101)
    with pytest.raises(_lib.HipLibraryError, match="restart interval 65536"):
        jpeg.JpegEncoder("cuda:0", restart_interval=65536)
    with pytest.raises(TypeError, match="quality"):
        jpeg.JpegEncoder("cuda:0", quality=75.0)
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        jpeg.JpegEncoder("cpu")
    enc = jpeg.JpegEncoder("cuda:0", quality=90, subsampling="4:2:2", restart_interval=3)
    assert (enc.quality, enc.subsampling, enc.restart_interval) == (90, 422, 3)
    assert enc.default_capacity(17, 23) == (629 + 17 * 23 * 3 + 63) // 64 * 64
    with pytest.raises(TypeError, match="frames"):
        enc.encode_device(np.zeros((1, 8, 8, 3), np.uint8))
    with pytest.raises(TypeError, match=r"frames\[0\]"):
        enc.encode_device([b"x"])
    with pytest.raises(TypeError, match="uint8"):
        enc.encode_device(torch.zeros(1, 8, 8, 3))
    with pytest.raises(_lib.HipLibraryError, match="is on cpu"):
        enc.encode_device(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(_lib.HipLibraryError, match="shape"):
        enc.encode_device(torch.zeros(8, 8, 3, dtype=torch.uint8))


def test_estimator_takes_an_encoder_or_nothing():
    from simple_pose_amd.detector.yolov5_detector import YOLOv5Detector
    from simple_pose_amd.pipeline import PoseResult, TopDownPoseEstimator

    class _Model:
        training = False

        def hip_program(self, x):
            raise AssertionError("not called")

    det = object.__new__(YOLOv5Detector)
    det.device = "cuda:0"
    with pytest.raises(TypeError, match="encoder"):
        TopDownPoseEstimator(det, _Model(), encoder=object())
    enc = jpeg.JpegEncoder("cuda:0")
    assert TopDownPoseEstimator(det, _Model(), encoder=enc).encoder is enc and TopDownPoseEstimator(det, _Model()).encoder is None
    with pytest.raises(_lib.HipLibraryError, match="encoder"):
        TopDownPoseEstimator(det, _Model(), encoder=jpeg.JpegEncoder("cuda:1"))
    assert PoseResult(np.zeros((1, 17, 3)), np.zeros(1), np.zeros((1, 5), np.float32)).jpeg is None
