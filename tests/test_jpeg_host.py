"""JPEG decoder, host side (no GPU): the numpy restatement tests/jpeg_ref.py reproduces the fixture (PIL / libjpeg-turbo) bit for bit;
sp_jpeg_parse through ctypes finds what jpeg_ref's parser finds and refuses every unsupported file with its own code and reason, and a
file cut anywhere in its headers without reading past the buffer; the symbols are declared, exported and bound without an ABI bump."""
import ctypes
import io
import os
import re
import types

import numpy as np
import pytest

from simple_pose_amd import _lib
from simple_pose_amd.build import LIB_PATH
from simple_pose_amd.datasets import jpeg as spjpeg
from simple_pose_amd.datasets.coco import GpuAugmentLoader
from tests import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sp_jpeg_parse", "sp_jpeg_decode_batch")


@pytest.fixture(scope="module")
def cases(golden):
    z = golden("g15_jpeg.npz")
    names = bytes(z["names"]).decode().split("\n")
    out = []
    for i, name in enumerate(names):
        data = bytes(z["bytes"][z["offsets"][i]:z["offsets"][i + 1]])
        px = z["pixels"][z["pixel_offsets"][i]:z["pixel_offsets"][i + 1]].reshape(int(z["shapes"][i, 0]), int(z["shapes"][i, 1]), 3)
        out.append(types.SimpleNamespace(name=name, data=data, pixels=px, code=int(z["code"][i])))
    return out


def test_fixture_holds_the_cases_the_decoder_has_to_reach(cases):
    by = {c.name: c for c in cases}
    good = [c for c in cases if c.code == 0]
    assert len(good) >= 15 and all(c.pixels.shape[0] * c.pixels.shape[1] <= 72 * 64 for c in good)
    info = {c.name: jpeg_ref.parse(c.data) for c in good}
    assert {(i.h[0], i.v[0]) for i in info.values() if i.components == 3} == {(1, 1), (2, 1), (2, 2)}
    assert info["gray_40x24"].components == 1
    assert len(info["r1_72x64_444"].seg_offsets) >= 65 and len(info["r1_40x40_420"].seg_offsets) == 9
    assert info["rr_17x16_422"].restart_interval == 2 and info["rb2_33x17_420"].restart_interval == 2
    assert max(l + 1 for l in range(16) for t in info["opt_48x64_420"].ac.values() if t[0][l]) > 9          # codes longer than the lookahead
    assert by["app1_com_16x8_420"].data[2:4] == b"\xff\xe1" and b"\xff\xfe" in by["app1_com_16x8_420"].data[:80]
    assert sorted(c.code for c in cases if c.code) == sorted([jpeg_ref.E_PROGRESSIVE, jpeg_ref.E_PRECISION, jpeg_ref.E_COMPONENTS, jpeg_ref.E_NO_TABLE])


def test_numpy_reference_equals_every_fixture_image_bit_for_bit(cases):
    for c in cases:
        if c.code == 0:
            got = jpeg_ref.decode(c.data)
            assert got.shape == c.pixels.shape and got.dtype == np.uint8, c.name
            assert np.array_equal(got, c.pixels), f"{c.name}: {int((got != c.pixels).sum())} differing bytes"
        else:
            with pytest.raises(jpeg_ref.JpegError) as e:
                jpeg_ref.decode(c.data)
            assert e.value.code == c.code, c.name


def test_numpy_reference_equals_a_fresh_pil_decode(cases):
    Image = pytest.importorskip("PIL.Image")
    for c in cases:
        if c.code == 0:
            im = Image.open(io.BytesIO(c.data))
            pil = np.asarray(im.convert("RGB"))[:, :, ::-1]
            assert np.array_equal(jpeg_ref.decode(c.data), pil), c.name


def _parse(data, capacity=4096):
    d = _lib.JpegDesc()
    segs = (ctypes.c_int32 * max(1, capacity))()
    rc = _lib.lib().sp_jpeg_parse(data, len(data), ctypes.byref(d), segs if capacity else None, capacity)
    return rc, d, list(segs[:min(capacity, d.segments)]) if rc == 0 else []


def test_parse_returns_the_fields_the_reference_parser_finds(cases):
    for c in cases:
        if c.code:
            continue
        ref = jpeg_ref.parse(c.data)
        rc, d, segs = _parse(c.data)
        assert rc == 0, (c.name, _lib.lib().sp_last_error())
        n = ref.components
        assert (d.width, d.height, d.components) == (ref.width, ref.height, n), c.name
        assert list(d.h_samp[:n]) == ref.h and list(d.v_samp[:n]) == ref.v and list(d.quant_sel[:n]) == ref.tq, c.name
        assert list(d.dc_sel[:n]) == ref.td and list(d.ac_sel[:n]) == ref.ta, c.name
        assert (d.restart_interval, d.mcus_x, d.mcus_y) == (ref.restart_interval, ref.mcus_x, ref.mcus_y), c.name
        assert (d.ecs_offset, d.ecs_end, d.file_bytes) == (ref.ecs_offset, ref.ecs_end, len(c.data)), c.name
        assert d.segments == len(ref.seg_offsets) and segs == ref.seg_offsets, c.name
        blocks = sum(ref.mcus_x * ref.h[k] * ref.mcus_y * ref.v[k] for k in range(n))
        assert (d.coef_count, d.plane_bytes, d.out_bytes) == (64 * blocks, 64 * blocks, ref.width * ref.height * 3), c.name
        quant = np.ctypeslib.as_array(d.quant)
        counts, values = np.ctypeslib.as_array(d.huff_counts), np.ctypeslib.as_array(d.huff_values)
        for t, q in ref.quant.items():
            assert np.array_equal(quant[t], q), c.name
        for cls, tabs in ((0, ref.dc), (1, ref.ac)):
            for t, (cn, vals) in tabs.items():
                assert list(counts[4 * cls + t]) == cn and list(values[4 * cls + t][:len(vals)]) == vals, c.name
        # the Python wrapper reports the same
        info = spjpeg.parse(c.data)
        assert (info.width, info.height, info.components, info.seg_offsets) == (ref.width, ref.height, n, tuple(ref.seg_offsets))
        assert info.sampling == tuple(zip(ref.h, ref.v)) and info.mcus == (ref.mcus_x, ref.mcus_y)


def test_parse_reports_the_segment_count_when_the_array_is_too_small(cases):
    c = next(c for c in cases if c.name == "r1_72x64_444")
    want = jpeg_ref.parse(c.data).seg_offsets
    rc, d, segs = _parse(c.data, capacity=5)
    assert rc == 0 and d.segments == len(want) and segs == want[:5]
    rc, d, _ = _parse(c.data, capacity=0)
    assert rc == 0 and d.segments == len(want)


def _edited(cases, name="s_16x16_420"):
    data = bytearray(next(c for c in cases if c.name == name).data)
    pos, at = 2, {}
    while data[pos + 1] != 0xDA:
        at.setdefault(data[pos + 1], pos)
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    at[0xDA] = pos
    return data, at


def test_every_rejection_has_its_own_code_and_reason(cases):
    lib = _lib.lib()
    seen = {}

    def refused(data, code, *words):
        rc, _, _ = _parse(bytes(data))
        msg = lib.sp_last_error().decode()
        assert rc == code, (rc, code, msg)
        for w in words:
            assert w in msg, (w, msg)
        seen[code] = msg

    for c in cases:                                   # the fixture's rejection files
        if c.code:
            refused(c.data, c.code)
    by = {c.name: c for c in cases}
    refused(by["x_progressive"].data, _lib.SP_JPEG_EPROGRESSIVE, "progressive", "byte")
    refused(by["x_precision12"].data, _lib.SP_JPEG_EPRECISION, "12-bit")
    refused(by["x_4components"].data, _lib.SP_JPEG_ECOMPONENTS, "4 components")
    refused(by["x_no_dht"].data, _lib.SP_JPEG_ENO_TABLE, "Huffman table 2")
    data, at = _edited(cases)
    sof, sos = at[0xC0], at[0xDA]
    d = bytearray(data); d[sof + 1] = 0xC1
    refused(d, _lib.SP_JPEG_EEXTENDED, "SOF1", f"byte {sof}")
    d = bytearray(data); d[sof + 1] = 0xC9
    refused(d, _lib.SP_JPEG_EARITHMETIC, "arithmetic", f"byte {sof}")
    d = bytearray(data); d[sof + 11] = 0x12                              # luma 1x2: 4:4:0
    refused(d, _lib.SP_JPEG_ESAMPLING, "1x2")
    d = bytearray(data); d[sof + 11] = 0x41                              # luma 4x1: 4:1:1
    refused(d, _lib.SP_JPEG_ESAMPLING, "4x1")
    d = bytearray(data); d[sof + 12] = 3                                 # luma quantisation table 3: not defined
    refused(d, _lib.SP_JPEG_ENO_TABLE, "quantisation table 3")
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"        # APP14, transform 0 (RGB)
    refused(data[:2] + adobe + data[2:], _lib.SP_JPEG_EADOBE, "transform 0")
    assert _parse(bytes(data[:2] + adobe[:-1] + b"\x01" + data[2:]))[0] == 0          # transform 1 (YCbCr) is fine
    d = bytearray(data); d[sos + 4] = 1; d[sos + 3] = 8; del d[sos + 7:sos + 11]     # a scan of one of the three components
    refused(d, _lib.SP_JPEG_ESCANS, "scan of 1 of 3")
    d = bytes(data[:-2]) + bytes(data[sos:])                            # a second SOS after the entropy data
    refused(d, _lib.SP_JPEG_ESCANS, "multiple scans", "byte")
    refused(b"\x89PNG\r\n\x1a\n" + bytes(16), _lib.SP_JPEG_ENOT_JPEG, "SOI")
    d = bytearray(data); d[sof + 5:sof + 7] = b"\x00\x00"
    refused(d, _lib.SP_JPEG_ESIZE, "size")
    d = bytearray(data); d[at[0xDB] + 4] = 0x10                          # 16-bit quantisation table
    refused(d, _lib.SP_JPEG_EBAD_TABLE, "DQT")
    d = bytearray(data); d[at[0xC4] + 5:at[0xC4] + 7] = b"\x03\x00"     # three codes of length 1: no prefix code
    refused(d, _lib.SP_JPEG_EBAD_TABLE, "DHT")
    refused(data[:at[0xDA] + 3], _lib.SP_JPEG_ETRUNCATED, "past the end", "byte")
    assert len(set(seen)) == 13 and len(set(seen.values())) == 13      # every code of the header, each with its own text
    with pytest.raises(_lib.HipLibraryError, match="progressive"):
        spjpeg.parse(by["x_progressive"].data)
    with pytest.raises(TypeError):
        spjpeg.parse(np.zeros(4, np.uint8))


def test_a_file_cut_at_every_header_byte_is_refused_without_reading_past_the_buffer(cases):
    """The cut file sits at the very end of an allocation followed by bytes that would parse as a continuation if they were read: the
    result must not depend on them."""
    c = next(c for c in cases if c.name == "s_8x8_420")
    ecs = jpeg_ref.parse(c.data).ecs_offset
    lib = _lib.lib()
    for cut in range(0, ecs):
        for tail in (c.data[cut:], b"\xff" * 64, bytes(64)):
            buf = ctypes.create_string_buffer(c.data[:cut] + tail, cut + len(tail))
            d = _lib.JpegDesc()
            rc = lib.sp_jpeg_parse(buf, cut, ctypes.byref(d), None, 0)
            assert rc < 0, (cut, rc)
            assert rc in (_lib.SP_JPEG_ETRUNCATED, _lib.SP_JPEG_ENOT_JPEG, _lib.SP_JPEG_EBAD_TABLE), (cut, rc, lib.sp_last_error())
        with pytest.raises(jpeg_ref.JpegError):
            jpeg_ref.parse(c.data[:cut])
    # cut inside the entropy data: the parser accepts (the decoder reports a status for the image)
    assert lib.sp_jpeg_parse(c.data, ecs + 3, ctypes.byref(_lib.JpegDesc()), None, 0) == 0


def test_new_symbols_declared_exported_bound_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(sp_\w+)\s*\(", hdr, flags=re.M))
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(handle, name), name
    assert re.search(r"#define SP_ABI_VERSION 36\b", hdr)
    assert _lib.ABI_VERSION == 36 and _lib.lib().sp_abi_version() == 36
    assert "typedef struct sp_jpeg_desc" in hdr and ctypes.sizeof(_lib.JpegDesc) == 2840
    for name in ("ETRUNCATED", "ENOT_JPEG", "EPROGRESSIVE", "EEXTENDED", "EARITHMETIC", "EPRECISION", "ECOMPONENTS", "ESAMPLING", "EADOBE", "ESCANS",
                 "ENO_TABLE", "EBAD_TABLE", "ESIZE"):
        assert int(re.search(r"#define SP_JPEG_%s \((-\d+)\)" % name, hdr).group(1)) == getattr(_lib, "SP_JPEG_" + name)
    assert os.path.isfile(os.path.join(ROOT, "simple_pose_amd", "csrc", "jpeg.hip"))
    core = open(os.path.join(ROOT, "simple_pose_amd", "csrc", "sp_jpeg.h")).read()
    assert "hip_runtime" not in core                  # the core compiles as plain C++


def test_decode_batch_refuses_bad_sizes_before_it_looks_at_a_device_pointer(cases):
    """Every device pointer is NULL in every call, and the entry point checks the host descriptors against the arena sizes first and the
    device pointers last: a size check that stopped refusing would end in "null pointer", never in a launch."""
    lib = _lib.lib()
    rc, d, _ = _parse(next(c for c in cases if c.name == "s_8x8_420").data)
    assert rc == 0
    descs = (_lib.JpegDesc * 1)(d)

    def call(count=1, nbytes=1 << 16, nseg=16, ncoef=1 << 16, nplane=1 << 16, nout=1 << 16, stages=7, host=descs):
        return lib.sp_jpeg_decode_batch(host, None, count, None, nbytes, None, nseg, None, ncoef, None, nplane, None, nout, None, stages, None)

    assert call(count=0) == 0
    assert call(host=None) == -1 and b"descs_host" in lib.sp_last_error()
    assert call(nbytes=d.file_bytes - 1) == -1 and b"file bytes" in lib.sp_last_error()
    assert call(ncoef=d.coef_count - 1) == -1 and b"coefficients" in lib.sp_last_error()
    assert call(nplane=d.plane_bytes - 1) == -1 and b"planes" in lib.sp_last_error()
    assert call(nout=d.out_bytes - 1) == -1 and b"output" in lib.sp_last_error()
    assert call(nseg=0) == -1 and b"segments" in lib.sp_last_error()
    assert call(stages=8) == -1 and b"stages" in lib.sp_last_error()
    descs[0].restart_interval = 65536
    assert call() == -1 and b"restart interval" in lib.sp_last_error()
    descs[0].restart_interval = 0
    descs[0].width = 9                                # sizes no longer follow from the geometry
    assert call() == -1 and b"do not follow" in lib.sp_last_error()
    descs[0].width, descs[0].h_samp[0] = 8, 4
    assert call() == -1 and b"sampling" in lib.sp_last_error()
    descs[0].h_samp[0] = d.h_samp[0]
    assert call() == -1 and b"null pointer" in lib.sp_last_error()      # a valid descriptor: the device pointers are what is refused


def test_status_bits_are_the_same_in_the_header_and_the_binding():
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    bits = {int(v) for v in re.findall(r"#define SP_JPEG_STATUS_\w+ (\d+)", hdr)}
    assert bits == set(_lib.SP_JPEG_STATUS) == {1, 2, 4, 8, 16}
    core = open(os.path.join(ROOT, "simple_pose_amd", "csrc", "sp_jpeg.h")).read()
    assert {int(v) for v in re.findall(r"#define SP_JPEG_ST_\w+ (\d+)", core)} == bits      # (jpeg.hip static_asserts them name by name)


def test_loader_rejects_a_sample_with_neither_img_nor_jpeg():
    s = types.SimpleNamespace(box=[1.0, 2.0, 30.0, 40.0], joints=np.ones((17, 3), np.float32), shape=(64, 48), img_id=7)
    loader = GpuAugmentLoader([s], 1, 0, 1, seed=0)
    with pytest.raises(_lib.HipLibraryError, match="neither .img"):
        next(iter(loader))
    s.jpeg = 12345                                    # not bytes either
    with pytest.raises(_lib.HipLibraryError, match="neither .img"):
        next(iter(loader))


def test_decoder_refuses_cpu_devices_and_non_bytes_inputs():
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        spjpeg.JpegDecoder("cpu")
