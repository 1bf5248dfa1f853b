"""Progressive JPEG decoder, host side (no GPU): the restatement tests/jpeg_prog_ref.py reproduces the fixture g17_jpeg_prog.npz (PIL /
libjpeg-turbo) bit for bit; sp_jpeg_parse_scans through ctypes finds the scans, segments, restart intervals and tables the restatement
finds, refuses every unsupported file with its own code and a byte offset, honours its capacities and never reads past the buffer;
sp_jpeg_parse still refuses progressive files; sp_jpeg_progressive_entropy refuses bad ranges before it looks at a device pointer."""
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
from tests import jpeg_prog_ref, jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sp_jpeg_parse_scans", "sp_jpeg_progressive_entropy")
COLOUR_SCRIPT = [(7, 0, 0, 0, 1), (1, 1, 5, 0, 2), (4, 1, 63, 0, 1), (2, 1, 63, 0, 1), (1, 6, 63, 0, 2), (1, 1, 63, 2, 1), (7, 0, 0, 1, 0), (4, 1, 63, 1, 0),
                 (2, 1, 63, 1, 0), (1, 1, 63, 1, 0)]          # (component mask, Ss, Se, Ah, Al): libjpeg-turbo's script for colour files


@pytest.fixture(scope="module")
def cases(golden):
    z = golden("g17_jpeg_prog.npz")
    names = bytes(z["names"]).decode().split("\n")
    out = []
    for i, name in enumerate(names):
        data = bytes(z["bytes"][z["offsets"][i]:z["offsets"][i + 1]])
        px = z["pixels"][z["pixel_offsets"][i]:z["pixel_offsets"][i + 1]].reshape(int(z["shapes"][i, 0]), int(z["shapes"][i, 1]), 3)
        script = [tuple(int(v) for v in r) for r in z["scripts"][z["script_offsets"][i]:z["script_offsets"][i + 1]]]
        out.append(types.SimpleNamespace(name=name, data=data, pixels=px, code=int(z["code"][i]), script=script))
    return out


@pytest.fixture(scope="module")
def decoded(cases):
    """The restatement's parse and coefficients of every accepted case, computed once."""
    out = {}
    for c in cases:
        if c.code == 0:
            info = jpeg_prog_ref.parse_scans(c.data)
            coef, status = jpeg_prog_ref.decode_coefficients(info, c.data)
            out[c.name] = (info, coef, status)
    return out


def test_fixture_holds_the_cases_the_decoder_has_to_reach(cases, decoded):
    by = {c.name: c for c in cases}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g17_jpeg_prog.npz")) < 150 * 1024
    good = [c for c in cases if c.code == 0]
    assert len(good) == 14 and all(c.pixels.shape[0] <= 96 and c.pixels.shape[1] <= 96 for c in good)
    for c in good:
        if c.name.startswith("p_") and "gray" not in c.name:
            assert [s[:5] for s in c.script] == COLOUR_SCRIPT, c.name
    assert len(by["p_gray_40x24"].script) == 6
    info = {n: d[0] for n, d in decoded.items()}
    assert {(info[n].h[0], info[n].v[0]) for n in ("p_37x53_444", "p_37x53_422", "p_37x53_420")} == {(1, 1), (2, 1), (2, 2)}
    # the non-interleaved geometry: luma 3 blocks wide in its own scans, 4 in the MCU grid
    i = info["p_17x9_420"]
    assert jpeg_prog_ref.scan_grid(i, i.scans[1])[0] == 3 and i.mcus_x * i.h[0] == 4
    # restart segments that count MCUs in the DC scans and blocks in the AC scans
    i = info["p_r2_33x17_420"]
    assert all(s.restart_interval == 2 for s in i.scans) and len(i.scans[0].seg_offsets) == 3 and len(i.scans[1].seg_offsets) == 8
    assert len(i.scans[2].seg_offsets) == 3                       # chroma: 3 x 2 blocks of its own
    assert all(len(s.seg_offsets) == 72 for s in info["p_r1_72x64_444"].scans)           # a lane takes a second segment
    assert by["p_app1_com_16x8_420"].data[2:4] == b"\xff\xe1" and b"\xff\xfe" in by["p_app1_com_16x8_420"].data[:80]
    assert [s[0] for s in by["c_split_dc_40x40_420"].script[:2]] == [1, 6]              # Y DC alone, then Cb + Cr interleaved
    assert [s[1:5] for s in by["c_dc_sa_24x16_444"].script[:6]] == [(0, 0, 0, 1)] * 3 + [(0, 0, 1, 0)] * 3
    assert (1, 10, 63, 0, 1) in [s[:5] for s in by["c_partial_hf_16x16_420"].script]    # sent at Al 1 and never refined
    assert sorted(c.code for c in cases if c.code) == sorted([-24, -24, -23, -23, -23, jpeg_ref.E_NO_TABLE, jpeg_ref.E_SCANS])


def test_reference_equals_every_fixture_image_bit_for_bit(cases, decoded):
    for c in cases:
        if c.code == 0:
            info, coef, status = decoded[c.name]
            assert status == 0, c.name
            got = jpeg_ref.color(info, jpeg_ref.planes(info, coef))
            assert got.shape == c.pixels.shape and got.dtype == np.uint8, c.name
            assert np.array_equal(got, c.pixels), f"{c.name}: {int((got != c.pixels).sum())} differing bytes"
        else:
            with pytest.raises(jpeg_ref.JpegError) as e:
                jpeg_prog_ref.parse_scans(c.data)
            assert e.value.code == c.code, c.name


def test_reference_equals_a_fresh_pil_decode(cases, decoded):
    Image = pytest.importorskip("PIL.Image")
    for c in cases:
        if c.code == 0:
            info, coef, _ = decoded[c.name]
            pil = np.asarray(Image.open(io.BytesIO(c.data)).convert("RGB"))[:, :, ::-1]
            assert np.array_equal(jpeg_ref.color(info, jpeg_ref.planes(info, coef)), pil), c.name


def _parse(data, scan_capacity=64, seg_capacity=4096):
    d = _lib.JpegDesc()
    scans = (_lib.JpegScan * (scan_capacity + 1))()              # one more than the capacity: it has to stay untouched
    segs = (ctypes.c_int32 * (seg_capacity + 1))(*([-77] * (seg_capacity + 1)))
    ctypes.memset(scans, 0xA5, ctypes.sizeof(scans))
    count = ctypes.c_int32(-1)
    rc = _lib.lib().sp_jpeg_parse_scans(data, len(data), ctypes.byref(d), scans if scan_capacity else None, scan_capacity, ctypes.byref(count),
                                        segs if seg_capacity else None, seg_capacity)
    assert segs[seg_capacity] == -77 and bytes(scans[scan_capacity]) == b"\xa5" * ctypes.sizeof(_lib.JpegScan)
    return rc, d, scans, count.value, segs


def test_parse_scans_returns_what_the_reference_finds(cases, decoded):
    for c in cases:
        if c.code:
            continue
        ref = decoded[c.name][0]
        rc, d, scans, count, segs = _parse(c.data)
        assert rc == 0, (c.name, _lib.lib().sp_last_error())
        n = ref.components
        assert (d.width, d.height, d.components) == (ref.width, ref.height, n), c.name
        assert list(d.h_samp[:n]) == ref.h and list(d.v_samp[:n]) == ref.v and list(d.quant_sel[:n]) == ref.tq, c.name
        assert list(d.dc_sel) == [0] * 3 and list(d.ac_sel) == [0] * 3, c.name
        assert not np.ctypeslib.as_array(d.huff_counts).any() and not np.ctypeslib.as_array(d.huff_values).any(), c.name
        assert (d.restart_interval, d.mcus_x, d.mcus_y) == (ref.restart_interval, ref.mcus_x, ref.mcus_y), c.name
        assert (d.ecs_offset, d.ecs_end, d.file_bytes) == (ref.scans[0].ecs_offset, ref.scans[-1].ecs_end, len(c.data)), c.name
        blocks = sum(ref.mcus_x * ref.h[k] * ref.mcus_y * ref.v[k] for k in range(n))
        assert (d.coef_count, d.plane_bytes, d.out_bytes) == (64 * blocks, 64 * blocks, ref.width * ref.height * 3), c.name
        for t, q in ref.quant.items():
            assert np.array_equal(np.ctypeslib.as_array(d.quant)[t], q), c.name
        assert count == len(ref.scans) == len(c.script) and d.segments == len(ref.seg_offsets), c.name
        assert list(segs[:d.segments]) == ref.seg_offsets, c.name
        at = 0
        for k, (s, r) in enumerate(zip(scans, ref.scans)):
            what = (c.name, k)
            assert (s.components, list(s.comp[:s.components])) == (len(r.comps), r.comps), what
            assert (s.ss, s.se, s.ah, s.al, s.restart_interval) == (r.ss, r.se, r.ah, r.al, r.restart_interval), what
            assert (sum(1 << x for x in r.comps), r.ss, r.se, r.ah, r.al, r.restart_interval) == c.script[k], what
            assert (s.ecs_offset, s.ecs_end, s.seg_index, s.segments) == (r.ecs_offset, r.ecs_end, at, len(r.seg_offsets)), what
            at += s.segments
            counts, values = np.ctypeslib.as_array(s.huff_counts), np.ctypeslib.as_array(s.huff_values)
            for j in range(3):
                if j < len(r.tables):
                    assert list(counts[j]) == r.tables[j][0] and list(values[j][:len(r.tables[j][1])]) == r.tables[j][1], what
                    assert not values[j][len(r.tables[j][1]):].any(), what
                else:
                    assert not counts[j].any() and not values[j].any(), what
        # the Python wrapper reports the same
        info, listed = spjpeg.parse_scans(c.data)
        assert (info.width, info.height, info.components, info.seg_offsets) == (ref.width, ref.height, n, tuple(ref.seg_offsets))
        assert [(s.components, s.ss, s.se, s.ah, s.al, s.restart_interval, s.segments) for s in listed] == \
            [(tuple(r.comps), r.ss, r.se, r.ah, r.al, r.restart_interval, len(r.seg_offsets)) for r in ref.scans]


def test_every_rejection_has_its_code_and_names_a_byte_offset(cases):
    lib = _lib.lib()
    by = {c.name: c for c in cases}

    def refused(data, code, *words):
        rc = _parse(bytes(data))[0]
        msg = lib.sp_last_error().decode()
        assert rc == code, (rc, code, msg)
        assert re.search(r"byte \d+", msg), msg
        for w in words:
            assert w in msg, (w, msg)

    for c in cases:
        if c.code:
            refused(c.data, c.code)
    refused(by["x_cut_after_dc"].data, _lib.SP_JPEG_EINCOMPLETE, "stops at bit 1")
    refused(by["x_cut_before_last"].data, _lib.SP_JPEG_EINCOMPLETE, "component 0 coefficient 1")
    refused(by["x_ac_two_components"].data, _lib.SP_JPEG_EBAD_SCAN, "3 components")
    refused(by["x_bad_refine_ah"].data, _lib.SP_JPEG_EBAD_SCAN, "Ah 3")
    refused(by["x_ss_gt_se"].data, _lib.SP_JPEG_EBAD_SCAN, "Ss 6, Se 5")
    refused(by["x_no_dht_scan3"].data, _lib.SP_JPEG_ENO_TABLE, "AC Huffman table 3")
    refused(by["x_baseline_two_scans"].data, _lib.SP_JPEG_ESCANS, "SOF0")
    # more scan headers libjpeg rejects or warns about, edited into the 16x8 file (scan positions from the restatement)
    data = by["p_app1_com_16x8_420"].data
    ref = jpeg_prog_ref.parse_scans(data)
    sos = [s.ecs_offset - (8 + 2 * len(s.comps)) for s in ref.scans]
    d = bytearray(data); d[sos[1] + 9] = 0x0E                           # Al 14
    refused(d, _lib.SP_JPEG_EBAD_SCAN, "Al 14")
    d = bytearray(data); d[sos[1] + 9] = 0x31                           # a first pass over coefficients with Ah != 0 (and Al != Ah - 1)
    refused(d, _lib.SP_JPEG_EBAD_SCAN)
    d = bytearray(data); d[sos[1] + 9] = 0x10                           # Ah 1, Al 0 for coefficients that had no first pass
    refused(d, _lib.SP_JPEG_EBAD_SCAN, "no first pass")
    d = bytearray(data); d[sos[0] + 5], d[sos[0] + 7] = d[sos[0] + 7], d[sos[0] + 5]      # components out of order
    refused(d, _lib.SP_JPEG_EBAD_SCAN, "out of order")
    d = bytearray(data); d[sos[0] + 7] = d[sos[0] + 5]                  # a component twice
    refused(d, _lib.SP_JPEG_EBAD_SCAN, "twice")
    d = bytearray(data); d[sos[1] + 8] = 64                             # Se 64
    refused(d, _lib.SP_JPEG_EBAD_SCAN, "Se 64")
    d = bytearray(data); d[sos[0] + 12] = 3                             # Ss 0 with Se 3
    refused(d, _lib.SP_JPEG_EBAD_SCAN, "Se 3")
    d = bytes(data[:sos[0]]) + bytes(data[sos[1]:])                    # no DC scan: the AC scan of Y comes first
    refused(d, _lib.SP_JPEG_EBAD_SCAN, "before its DC scan")
    dqt = data.index(b"\xff\xdb")
    L = 2 + ((data[dqt + 2] << 8) | data[dqt + 3])
    d = bytes(data[:sos[1]]) + bytes(data[dqt:dqt + L]) + bytes(data[sos[1]:])           # a DQT after the first SOS
    refused(d, _lib.SP_JPEG_EBAD_TABLE, "after the first scan")
    refused(data[:sos[3] + 3], _lib.SP_JPEG_ETRUNCATED, "past the end")
    with pytest.raises(_lib.HipLibraryError, match="progression ends"):
        spjpeg.parse_scans(by["x_cut_after_dc"].data)
    with pytest.raises(TypeError):
        spjpeg.parse_scans(np.zeros(4, np.uint8))


def test_high_bands_that_are_never_sent_or_refined_are_accepted(cases):
    """Zigzag positions 10..63 may stay unsent: libjpeg decodes such a file through its ordinary path.  The file: c_partial_hf without its
    last scan (Cr 10..63)."""
    c = next(c for c in cases if c.name == "c_partial_hf_16x16_420")
    ref = jpeg_prog_ref.parse_scans(c.data)
    cut = c.data[:ref.scans[-1].ecs_offset - 10 - 2 - 17 - len(ref.scans[-1].tables[0][1]) - 2] + b"\xff\xd9"      # before the last DHT + SOS
    rc, d, scans, count, _ = _parse(cut)
    assert rc == 0 and count == len(ref.scans) - 1, _lib.lib().sp_last_error()
    assert len(jpeg_prog_ref.parse_scans(cut).scans) == count


def test_capacities_one_too_few_report_the_needed_count_and_write_nothing_past_them(cases, decoded):
    for name in ("p_r2_33x17_420", "c_split_dc_40x40_420"):
        c = next(c for c in cases if c.name == name)
        ref = decoded[name][0]
        ns, ng = len(ref.scans), len(ref.seg_offsets)
        rc, d, scans, count, segs = _parse(c.data, scan_capacity=ns - 1, seg_capacity=ng - 1)      # _parse checks the element past each capacity
        assert rc == 0 and count == ns and d.segments == ng
        assert list(segs[:ng - 1]) == ref.seg_offsets[:-1] and scans[ns - 2].se == ref.scans[ns - 2].se
        rc, d, _, count, _ = _parse(c.data, scan_capacity=0, seg_capacity=0)
        assert rc == 0 and count == ns and d.segments == ng


def test_every_truncation_of_the_header_region_is_refused_without_reading_past_the_buffer(cases, decoded):
    """Every prefix up to the last SOS header.  The prefix sits at the very end of an allocation followed by bytes that would parse as
    a continuation if they were read: the result must not depend on them."""
    c = next(c for c in cases if c.name == "p_17x9_420")
    last = decoded[c.name][0].scans[-1].ecs_offset
    lib = _lib.lib()
    allowed = (_lib.SP_JPEG_ETRUNCATED, _lib.SP_JPEG_ENOT_JPEG, _lib.SP_JPEG_EBAD_TABLE, _lib.SP_JPEG_EINCOMPLETE)
    for cut in range(0, last):
        got = set()
        for tail in (c.data[cut:], b"\xff" * 64, bytes(64)):
            buf = ctypes.create_string_buffer(c.data[:cut] + tail, cut + len(tail))
            d, count = _lib.JpegDesc(), ctypes.c_int32(0)
            rc = lib.sp_jpeg_parse_scans(buf, cut, ctypes.byref(d), None, 0, ctypes.byref(count), None, 0)
            assert rc in allowed, (cut, rc, lib.sp_last_error())
            got.add(rc)
        assert len(got) == 1, (cut, got)
        with pytest.raises(jpeg_ref.JpegError):
            jpeg_prog_ref.parse_scans(c.data[:cut])
    # cut inside the last scan's entropy data: the parser accepts (the decoder reports a status for the image)
    assert lib.sp_jpeg_parse_scans(c.data, last + 1, ctypes.byref(_lib.JpegDesc()), None, 0, ctypes.byref(ctypes.c_int32(0)), None, 0) == 0


def test_the_baseline_parser_still_refuses_every_fixture_file(cases):
    lib = _lib.lib()
    for c in cases:
        rc = lib.sp_jpeg_parse(c.data, len(c.data), ctypes.byref(_lib.JpegDesc()), None, 0)
        msg = lib.sp_last_error().decode()
        if c.name == "x_baseline_two_scans":                  # the one SOF0 file
            assert rc == _lib.SP_JPEG_ESCANS and "multiple scans" in msg, (c.name, rc, msg)
        else:
            assert rc == _lib.SP_JPEG_EPROGRESSIVE and "progressive SOF2 at byte" in msg, (c.name, rc, msg)
        with pytest.raises(_lib.HipLibraryError):
            spjpeg.parse(c.data)


def test_progressive_entropy_refuses_bad_ranges_before_it_looks_at_a_device_pointer(cases):
    """Every device pointer is NULL in every call: a range check that stopped refusing would end in "null pointer", never in a launch."""
    lib = _lib.lib()
    c = next(c for c in cases if c.name == "p_r2_33x17_420")
    rc, d, scans, count, _ = _parse(c.data)
    assert rc == 0
    descs = (_lib.JpegDesc * 1)(d)
    ranges = (ctypes.c_int32 * 2)(0, count)

    def call(n=1, nscan=None, nbytes=1 << 16, nseg=1 << 10, ncoef=1 << 16, host=descs, host_scans=scans, host_ranges=ranges):
        return lib.sp_jpeg_progressive_entropy(host, None, n, host_scans, None, host_ranges, None, count if nscan is None else nscan, None, nbytes,
                                               None, nseg, None, ncoef, None, None)

    def refused(words, **kw):
        assert call(**kw) == -1 and words in lib.sp_last_error(), lib.sp_last_error()

    assert call(n=0) == 0 and call(n=0, host=None, host_scans=None, host_ranges=None) == 0
    refused(b"null pointer (descs_host", host=None)
    refused(b"null pointer (descs_host", host_scans=None)
    refused(b"file bytes", nbytes=d.file_bytes - 1)
    refused(b"coefficients", ncoef=d.coef_count - 1)
    refused(b"segments", nseg=d.segments - 1)
    refused(b"scan range", nscan=count - 1)
    ranges[1] = 0
    refused(b"0 scans")
    ranges[1] = 257
    refused(b"257 scans", nscan=300)
    ranges[0], ranges[1] = 2, 1
    refused(b"scan range")
    ranges[0], ranges[1] = 0, count
    for field, bad, words in (("ecs_end", d.file_bytes + 1, b"entropy data"), ("ecs_offset", -1, b"entropy data"), ("segments", 0, b"segments"),
                              ("seg_index", d.segments, b"segments"), ("se", 64, b"Se 64"), ("al", 14, b"Al 14"), ("components", 4, b"component list"),
                              ("restart_interval", 65536, b"restart interval")):
        keep = getattr(scans[3], field)
        setattr(scans[3], field, bad)
        refused(words)
        setattr(scans[3], field, keep)
    scans[0].comp[1] = 0                                  # a component twice
    refused(b"component list")
    scans[0].comp[1] = 1
    scans[1].components, scans[1].comp[1] = 2, 1         # an AC scan of two components
    refused(b"2 components")
    scans[1].components, scans[1].comp[1] = 1, 0
    descs[0].coef_count -= 64                             # no longer follows from the size
    refused(b"coef_count")
    descs[0].coef_count += 64
    descs[0].h_samp[0] = 4
    refused(b"sampling")
    descs[0].h_samp[0] = 2
    refused(b"null pointer")                              # everything valid: the device pointers are what is refused


def test_new_symbols_declared_exported_bound_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "simple_pose_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(sp_\w+)\s*\(", hdr, flags=re.M))
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(handle, name), name
    assert re.search(r"#define SP_ABI_VERSION 36\b", hdr) and _lib.ABI_VERSION == 36 and _lib.lib().sp_abi_version() == 36
    assert "typedef struct sp_jpeg_scan" in hdr and ctypes.sizeof(_lib.JpegScan) == 56 + 3 * 16 + 3 * 256
    assert ctypes.sizeof(_lib.JpegDesc) == 2840           # sp_jpeg_desc keeps its layout
    for name, value in (("EBAD_SCAN", -23), ("EINCOMPLETE", -24)):
        assert int(re.search(r"#define SP_JPEG_%s \((-\d+)\)" % name, hdr).group(1)) == getattr(_lib, "SP_JPEG_" + name) == value
    assert (jpeg_prog_ref.E_BAD_SCAN, jpeg_prog_ref.E_INCOMPLETE) == (_lib.SP_JPEG_EBAD_SCAN, _lib.SP_JPEG_EINCOMPLETE)
    for name in ("jpeg_prog.hip", "sp_jpeg_prog.h", "sp_jpeg_parse_scans.h"):
        src = open(os.path.join(ROOT, "simple_pose_amd", "csrc", name)).read()
        assert ("hip_runtime" not in src and "sp_common.h" not in src) == name.endswith(".h"), name      # the headers compile as plain C++
    core = open(os.path.join(ROOT, "simple_pose_amd", "csrc", "sp_jpeg_prog.h")).read()
    assert not re.search(r"#define SP_JPEG_ST_", core)    # no new status bit
