"""tools/gen_golden_jpeg_prog.py - TEST INFRASTRUCTURE.  Needs PIL (libjpeg-turbo); run where it is installed:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_jpeg_prog.py [--check]

g17_jpeg_prog.npz: small progressive (SOF2) JPEG files and PIL's own decode of each as BGR - the pixels the device decoder has to
reproduce bit for bit.  The arrays of g15_jpeg.npz (tools/gen_golden_jpeg.py), uint8 / int32 only (allow_pickle=False):

    names, bytes, offsets, pixels, pixel_offsets, shapes, code       as there (code: what sp_jpeg_parse_scans has to return)
    scripts   int32 [scans, 6]  every accepted file's scan list: (component bit mask, Ss, Se, Ah, Al, restart interval)
    script_offsets int32 [n+1]  (a rejection case has no rows)

p_* files are PIL's progressive saves (libjpeg-turbo's 10-scan script for colour, 6 scans for gray; a new DHT before almost every scan).
c_* files come from the small progressive writer below, which re-codes the quantised coefficients of a PIL baseline file under a scan
script libjpeg-turbo's writer never uses: DC scans of one and of two components, DC refinement per component, AC bands that are never
refined.  It writes DC first / DC refinement / AC first passes with EOB runs, and one Huffman table per scan that gives every used
symbol an 8-bit code.  The expected pixels are PIL's decode of the written file.  x_* files are rejections made by editing bytes.
"""
from __future__ import annotations

import io
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import jpeg_prog_ref, jpeg_ref  # noqa: E402
from tools.gen_golden_jpeg import find_marker, image, pil_bgr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g17_jpeg_prog.npz")
SEED = 17

# name, (W, H), mode, PIL save options (progressive=True is added)
CASES = [
    ("p_1x1_420", (1, 1), "RGB", dict(quality=90, subsampling=2)),
    ("p_17x9_420", (17, 9), "RGB", dict(quality=85, subsampling=2)),
    ("p_37x53_444", (37, 53), "RGB", dict(quality=80, subsampling=0)),
    ("p_37x53_422", (37, 53), "RGB", dict(quality=80, subsampling=1)),
    ("p_37x53_420", (37, 53), "RGB", dict(quality=80, subsampling=2)),
    ("p_r2_33x17_420", (33, 17), "RGB", dict(quality=85, subsampling=2, restart_marker_blocks=2)),
    ("p_r1_72x64_444", (72, 64), "RGB", dict(quality=50, subsampling=0, restart_marker_blocks=1)),
    ("p_q100_24x24_420", (24, 24), "RGB", dict(quality=100, subsampling=2)),
    ("p_flat_96x96_444", (96, 96), "RGB", dict(quality=90, subsampling=0)),
    ("p_gray_40x24", (40, 24), "L", dict(quality=90)),
    ("p_app1_com_16x8_420", (16, 8), "RGB", dict(quality=90, subsampling=2)),
]
Y, CB, CR = 0, 1, 2
# name, (W, H), PIL options of the baseline source, script: (components, Ss, Se, Ah, Al)
CUSTOM = [
    ("c_split_dc_40x40_420", (40, 40), dict(quality=85, subsampling=2),
     [((Y,), 0, 0, 0, 0), ((CB, CR), 0, 0, 0, 0)] + [((c,), a, b, 0, 0) for c in (Y, CB, CR) for a, b in ((1, 2), (3, 9), (10, 63))]),
    ("c_dc_sa_24x16_444", (24, 16), dict(quality=85, subsampling=0),
     [((c,), 0, 0, 0, 1) for c in (Y, CB, CR)] + [((c,), 0, 0, 1, 0) for c in (Y, CB, CR)] + [((c,), 1, 63, 0, 0) for c in (Y, CB, CR)]),
    ("c_partial_hf_16x16_420", (16, 16), dict(quality=90, subsampling=2),
     [((Y, CB, CR), 0, 0, 0, 0)] + [((c,), a, b, 0, al) for c in (Y, CB, CR) for a, b, al in ((1, 9, 0), (10, 63, 1))]),
]
REJECT = [("x_cut_after_dc", jpeg_prog_ref.E_INCOMPLETE), ("x_cut_before_last", jpeg_prog_ref.E_INCOMPLETE), ("x_ac_two_components", jpeg_prog_ref.E_BAD_SCAN),
          ("x_bad_refine_ah", jpeg_prog_ref.E_BAD_SCAN), ("x_ss_gt_se", jpeg_prog_ref.E_BAD_SCAN), ("x_no_dht_scan3", jpeg_ref.E_NO_TABLE),
          ("x_baseline_two_scans", jpeg_ref.E_SCANS)]


def scan_positions(data):
    """[(offset of the SOS marker, offset of the marker that ends the scan's entropy data)] of every scan."""
    out, pos = [], 2
    while data[pos + 1] != 0xD9:
        L = (data[pos + 2] << 8) | data[pos + 3]
        if data[pos + 1] != 0xDA:
            pos += 2 + L
            continue
        p = pos + 2 + L
        while True:
            p = data.index(b"\xff", p)
            if data[p + 1] == 0 or 0xD0 <= data[p + 1] <= 0xD7:
                p += 2
                continue
            break
        out.append((pos, p))
        pos = p
    return out


# ---- a small progressive writer ---------------------------------------------------------------------------------------------------------------
def _pack(items):
    """[(8-bit code or None, extra bits, their count)] -> entropy bytes: FF is stuffed, the last byte padded with ones."""
    acc = nacc = 0
    out = bytearray()
    for code, bits, nbits in items:
        if code is not None:
            acc, nacc = (acc << 8) | code, nacc + 8
        acc, nacc = (acc << nbits) | (bits & ((1 << nbits) - 1)), nacc + nbits
        while nacc >= 8:
            out.append((acc >> (nacc - 8)) & 0xFF)
            if out[-1] == 0xFF:
                out.append(0)
            nacc -= 8
        acc &= (1 << nacc) - 1
    if nacc:
        out.append(((acc << (8 - nacc)) | ((1 << (8 - nacc)) - 1)) & 0xFF)
        if out[-1] == 0xFF:
            out.append(0)
    return bytes(out)


def _magnitude(v):
    """-> (size, the `size` low bits T.81 F.1.2.1 sends for v)."""
    size = abs(v).bit_length()
    return size, v if v >= 0 else v + (1 << size) - 1


def write_progressive(baseline: bytes, script) -> bytes:
    """The quantised coefficients of a PIL baseline file, coded again under `script`: [(components, Ss, Se, Ah, Al)] with Ah != 0 for DC
    scans only.  One DHT per table in front of every scan; every used symbol gets the 8-bit code that is its rank in its table."""
    info = jpeg_ref.parse(baseline)
    coef, status = jpeg_ref.decode_coefficients(info, baseline)
    assert status == 0 and info.restart_interval == 0
    dqt, sof = find_marker(baseline, 0xDB), find_marker(baseline, 0xC0)
    sof_len = (baseline[sof + 2] << 8) | baseline[sof + 3]
    out = bytearray(baseline[:2] + baseline[dqt:sof] + b"\xff\xc2" + baseline[sof + 2:sof + 2 + sof_len])      # SOI, the DQT segments, SOF2
    assert all(m == 0xDB for m in _markers(baseline[dqt:sof]))

    def own_grid(c):                                                               # the blocks a one-component scan covers
        cw, ch = -(-info.width * info.h[c] // info.h[0]), -(-info.height * info.v[c] // info.v[0])
        return [(by, bx) for by in range(-(-ch // 8)) for bx in range(-(-cw // 8))]

    for comps, ss, se, ah, al in script:
        items = []                                                                 # (table, symbol or None, extra bits, their count)
        if ss == 0:
            if len(comps) == 1:
                order = [(0, comps[0], by, bx) for by, bx in own_grid(comps[0])]
            else:
                order = [(j, c, my * info.v[c] + vy, mx * info.h[c] + hx) for my in range(info.mcus_y) for mx in range(info.mcus_x)
                         for j, c in enumerate(comps) for vy in range(info.v[c]) for hx in range(info.h[c])]
            pred = [0] * len(comps)
            for j, c, by, bx in order:
                v = int(coef[c][by, bx, 0]) >> al
                if ah:
                    items.append((j, None, v & 1, 1))
                else:
                    size, bits = _magnitude(v - pred[j])
                    pred[j] = v
                    items.append((j, size, bits, size))
        else:
            assert len(comps) == 1 and ah == 0
            eobrun = 0

            def flush():
                nonlocal eobrun
                if eobrun:
                    nb = eobrun.bit_length() - 1
                    items.append((0, nb << 4, eobrun - (1 << nb), nb))
                    eobrun = 0
            for by, bx in own_grid(comps[0]):
                r = 0
                for k in range(ss, se + 1):
                    v = int(coef[comps[0]][by, bx, jpeg_ref.ZIGZAG[k]])
                    t = abs(v) >> al
                    if t == 0:
                        r += 1
                        continue
                    flush()
                    while r > 15:
                        items.append((0, 0xF0, 0, 0))
                        r -= 16
                    size, bits = _magnitude(t if v > 0 else -t)
                    items.append((0, (r << 4) | size, bits, size))
                    r = 0
                if r:
                    eobrun += 1
                    if eobrun == 0x7FFF:
                        flush()
            flush()
        tables = {}
        for t, sym, _, _ in items:
            if sym is not None:
                tables.setdefault(t, set()).add(sym)
        tables = {t: sorted(v) for t, v in tables.items()}
        cls = 1 if ss else 0
        for t, values in sorted(tables.items()):
            assert len(values) <= 255
            body = bytes([(cls << 4) | (1 if ss else t)]) + bytes([0] * 7 + [len(values)] + [0] * 8) + bytes(values)
            out += b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body
        sos = bytes([len(comps)]) + b"".join(bytes([info.comp_id[c], 0x01 if ss else j << 4]) for j, c in enumerate(comps)) + bytes([ss, se, (ah << 4) | al])
        out += b"\xff\xda" + (len(sos) + 2).to_bytes(2, "big") + sos
        out += _pack([(None if sym is None else tables[t].index(sym), bits, nbits) for t, sym, bits, nbits in items])
    return bytes(out + b"\xff\xd9")


def _markers(segments):
    pos = 0
    while pos < len(segments):
        yield segments[pos + 1]
        pos += 2 + ((segments[pos + 2] << 8) | segments[pos + 3])


def script_of(data):
    info = jpeg_prog_ref.parse_scans(data)
    return [(sum(1 << c for c in s.comps), s.ss, s.se, s.ah, s.al, s.restart_interval) for s in info.scans]


def build():
    from PIL import Image
    rng = np.random.RandomState(SEED)
    files, pix, codes, names, scripts = [], [], [], [], []

    def accept(name, data):
        want = pil_bgr(data)                                                       # PIL decodes it ...
        got = jpeg_prog_ref.decode(data)                                           # ... and the restatement gives the same pixels
        assert np.array_equal(got, want), name
        files.append(data); names.append(name); pix.append(want); codes.append(0); scripts.append(script_of(data))

    for name, (w, h), mode, opts in CASES:
        src = image(rng, w, h, mode)
        if name.startswith("p_flat"):
            src = np.full((h, w, 3), 120, np.uint8)
            src[41:49, 43:51] = 200                                                # one bright 8x8 square, off the block grid: four blocks have AC
        buf = io.BytesIO()
        Image.fromarray(src, mode).save(buf, "JPEG", progressive=True, **opts)
        data = buf.getvalue()
        if name.startswith("p_app1_com"):
            exif = b"Exif\0\0" + bytes(range(40))
            com = b"simple_pose_amd fixture"
            data = (data[:2] + b"\xff\xe1" + (len(exif) + 2).to_bytes(2, "big") + exif + b"\xff\xfe" + (len(com) + 2).to_bytes(2, "big") + com
                    + data[2:])
        accept(name, data)
        if mode == "RGB":
            assert [s[:5] for s in scripts[-1]] == [(7, 0, 0, 0, 1), (1, 1, 5, 0, 2), (4, 1, 63, 0, 1), (2, 1, 63, 0, 1), (1, 6, 63, 0, 2), (1, 1, 63, 2, 1),
                                                    (7, 0, 0, 1, 0), (4, 1, 63, 1, 0), (2, 1, 63, 1, 0), (1, 1, 63, 1, 0)], (name, scripts[-1])
        else:
            assert len(scripts[-1]) == 6
    for name, (w, h), opts, script in CUSTOM:
        buf = io.BytesIO()
        Image.fromarray(image(rng, w, h, "RGB"), "RGB").save(buf, "JPEG", **opts)
        data = write_progressive(buf.getvalue(), script)
        accept(name, data)
        assert [s[:5] for s in scripts[-1]] == [(sum(1 << c for c in comps), ss, se, ah, al) for comps, ss, se, ah, al in script], name
    src = image(rng, 16, 16, "RGB")
    prog, base = io.BytesIO(), io.BytesIO()
    Image.fromarray(src, "RGB").save(prog, "JPEG", quality=90, subsampling=2, progressive=True)
    Image.fromarray(src, "RGB").save(base, "JPEG", quality=90, subsampling=2)
    prog, base = prog.getvalue(), base.getvalue()
    sp = scan_positions(prog)
    assert len(sp) == 10
    eoi = b"\xff\xd9"
    two, refine, ssse, nodht = bytearray(prog), bytearray(prog), bytearray(prog), bytearray(prog)
    two[sp[0][0] + 11:sp[0][0] + 13] = bytes([1, 5])          # the interleaved DC scan made an AC scan of three components
    assert refine[sp[5][0] + 9] == 0x21
    refine[sp[5][0] + 9] = 0x32                                # Y refinement 2 -> 1 made 3 -> 2: Ah is not the Al it was sent with
    ssse[sp[1][0] + 7:sp[1][0] + 9] = bytes([6, 5])           # Ss > Se
    nodht[sp[2][0] + 6] = 0x03                                 # the third scan selects AC table 3, which no DHT defines
    reject = (prog[:sp[0][1]] + eoi, prog[:sp[8][1]] + eoi, bytes(two), bytes(refine), bytes(ssse), bytes(nodht), base[:-2] + base[find_marker(base, 0xDA):])
    for (name, code), data in zip(REJECT, reject):
        try:
            jpeg_prog_ref.parse_scans(data)
            raise AssertionError(f"{name}: the restatement accepts it")
        except jpeg_ref.JpegError as e:
            assert e.code == code, (name, e.code, str(e))
        files.append(bytes(data)); names.append(name); pix.append(np.zeros((0, 0, 3), np.uint8)); codes.append(code); scripts.append([])
    return {
        "names": np.frombuffer("\n".join(names).encode(), np.uint8),
        "bytes": np.frombuffer(b"".join(files), np.uint8),
        "offsets": np.cumsum([0] + [len(f) for f in files]).astype(np.int32),
        "pixels": np.concatenate([p.reshape(-1) for p in pix]),
        "pixel_offsets": np.cumsum([0] + [p.size for p in pix]).astype(np.int32),
        "shapes": np.array([p.shape[:2] for p in pix], np.int32),
        "code": np.array(codes, np.int32),
        "scripts": np.array([r for s in scripts for r in s], np.int32).reshape(-1, 6),
        "script_offsets": np.cumsum([0] + [len(s) for s in scripts]).astype(np.int32),
    }


def main():
    new = build()
    if "--check" in sys.argv:
        old = np.load(OUT, allow_pickle=False)
        bad = [k for k in new if not np.array_equal(old[k], new[k])]
        print("g17_jpeg_prog.npz:", "identical" if not bad else f"DIFFERS in {bad}")
        return 1 if bad else 0
    np.savez_compressed(OUT, **new)
    print(f"wrote {OUT}: {len(new['offsets']) - 1} files, {new['bytes'].size} file bytes, {os.path.getsize(OUT)} bytes on disk")
    return 0


if __name__ == "__main__":
    sys.exit(main())
