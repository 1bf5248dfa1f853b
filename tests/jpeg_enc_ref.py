"""TEST INFRASTRUCTURE: libjpeg's default baseline compressor restated in numpy (the rules of simple_pose_amd/csrc/sp_jpeg_enc.h), the
yardstick of the encoder tests.  tests/test_jpeg_enc_host.py pins it byte for byte to the files Pillow / libjpeg-turbo wrote
(tests/golden/g16_jpeg_enc.npz); the GPU tests then use it for frames that are not in the fixture.  The Annex K quantisation and Huffman
tables are not typed here: they are read from the fixture, where tools/gen_golden_jpeg_enc.py stored them out of Pillow-written files.

    data = encode(bgr, 420, 75, 0)                 # uint8 [H,W,3] BGR -> the file's bytes
    zz, real = coefficients(bgr, 420, 75)          # int16 [blocks,64] zigzag order, scan order, absolute DC; dummy blocks all zero
"""
from __future__ import annotations

import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g16_jpeg_enc.npz")
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
                   57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
SAMPLING = {444: (1, 1), 422: (2, 1), 420: (2, 2)}
_tables = None


def set_tables(std_quant, dht_counts, dht_values):
    """std_quant uint8 [2,64] (zigzag order, as in a DQT payload); dht_counts uint8 [4,16], dht_values uint8 [4,256]: DC0, AC0, DC1, AC1."""
    global _tables
    _tables = (np.asarray(std_quant, np.int64), np.asarray(dht_counts, np.int64), np.asarray(dht_values, np.int64))


def tables():
    if _tables is None:
        z = np.load(GOLDEN, allow_pickle=False)
        set_tables(z["std_quant"], z["dht_counts"], z["dht_values"])
    return _tables


def _fix(x):
    return int(x * 65536 + 0.5)


def _cdiv(a, b):
    return -(-a // b)


def quant_tables(quality):
    """-> int64 [2,64] in zigzag order."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((tables()[0] * scale + 50) // 100, 1, 255)


def huff_codes(t):
    """Table t (0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma) -> (code int64 [256], length int64 [256])."""
    counts, values = tables()[1][t], tables()[2][t]
    code = np.zeros(256, np.int64)
    length = np.zeros(256, np.int64)
    c = k = 0
    for l in range(1, 17):
        for _ in range(int(counts[l - 1])):
            code[values[k]], length[values[k]] = c, l
            c += 1
            k += 1
        c <<= 1
    return code, length


def geometry(W, H, sub):
    hs, vs = SAMPLING[sub]
    g = dict(hs=hs, vs=vs, mcus_x=_cdiv(W, 8 * hs), mcus_y=_cdiv(H, 8 * vs), samp=[(hs, vs), (1, 1), (1, 1)])
    g["wb"] = [_cdiv(_cdiv(W * h, hs), 8) for h, _ in g["samp"]]
    g["hb"] = [_cdiv(_cdiv(H * v, vs), 8) for _, v in g["samp"]]
    return g


def header(W, H, sub, quality, restart):
    hs, vs = SAMPLING[sub]
    q = quant_tables(quality)
    counts, values = tables()[1], tables()[2]
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2):
        out += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(int(v) for v in q[t])
    out += b"\xff\xc0\x00\x11\x08" + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, hs * 16 + vs, 0, 2, 0x11, 1, 3, 0x11, 1])
    for t, tc_th in enumerate((0x00, 0x10, 0x01, 0x11)):
        n = int(counts[t].sum())
        out += b"\xff\xc4" + (19 + n).to_bytes(2, "big") + bytes([tc_th]) + bytes(int(v) for v in counts[t]) + bytes(int(v) for v in values[t][:n])
    if restart:
        out += b"\xff\xdd\x00\x04" + restart.to_bytes(2, "big")
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    return bytes(out)


def planes(bgr, sub):
    """-> three int64 planes of hb*8 x wb*8 samples each (the real blocks only)."""
    H, W = bgr.shape[:2]
    g = geometry(W, H, sub)
    b, gr, r = (bgr[..., i].astype(np.int64) for i in range(3))
    y = (_fix(.299) * r + _fix(.587) * gr + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * gr + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * gr - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    out = []
    for c, p in enumerate((y, cb, cr)):
        fx, fy = g["hs"] // g["samp"][c][0], g["vs"] // g["samp"][c][1]
        wide = g["wb"][c] * 8 * fx
        p = np.pad(p, ((0, 0), (0, wide - W)), mode="edge")
        if fy == 2:
            p = np.pad(p, ((0, (-H) % 2), (0, 0)), mode="edge")
            bias = 1 + (np.arange(wide // 2) & 1)
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        elif fx == 2:
            p = (p[:, 0::2] + p[:, 1::2] + (np.arange(wide // 2) & 1)) >> 1
        out.append(np.pad(p, ((0, g["hb"][c] * 8 - p.shape[0]), (0, 0)), mode="edge"))
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """d: [..., 8] along the last axis."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def fdct_quant(plane, qzz):
    """plane [hb*8, wb*8] -> int64 [hb, wb, 64] quantised coefficients in zigzag order."""
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    blk = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3) - 128          # [hb, wb, row, col]
    blk = _fdct_pass(blk, True)                                             # along the columns of each row
    blk = _fdct_pass(blk.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)
    zz = blk.reshape(hb, wb, 64)[..., ZIGZAG]
    qv = 8 * qzz
    mag = (np.abs(zz) + (qv >> 1)) // qv
    return np.where(zz < 0, -mag, mag)


def scan_blocks(bgr, sub, quality):
    """-> (zz int64 [blocks,64], real bool [blocks], comp int64 [blocks], mcu int64 [blocks]) in scan order; dummy blocks are all zero."""
    H, W = bgr.shape[:2]
    g = geometry(W, H, sub)
    q = quant_tables(quality)
    pl = planes(bgr, sub)
    mx, my = g["mcus_x"], g["mcus_y"]
    per = []
    for c in range(3):
        h, v = g["samp"][c]
        co = np.zeros((my * v, mx * h, 64), np.int64)
        re = np.zeros((my * v, mx * h), bool)
        co[:g["hb"][c], :g["wb"][c]] = fdct_quant(pl[c], q[min(c, 1)])
        re[:g["hb"][c], :g["wb"][c]] = True
        # [my, v, mx, h] -> [my, mx, v, h]
        per.append((co.reshape(my, v, mx, h, 64).transpose(0, 2, 1, 3, 4).reshape(my * mx, v * h, 64),
                    re.reshape(my, v, mx, h).transpose(0, 2, 1, 3).reshape(my * mx, v * h), np.full((my * mx, v * h), c)))
    zz = np.concatenate([p[0] for p in per], 1).reshape(-1, 64)
    real = np.concatenate([p[1] for p in per], 1).reshape(-1)
    comp = np.concatenate([p[2] for p in per], 1).reshape(-1)
    bpm = g["hs"] * g["vs"] + 2
    return zz, real, comp, np.arange(zz.shape[0]) // bpm


def coefficients(bgr, sub, quality):
    zz, real, _, _ = scan_blocks(bgr, sub, quality)
    return zz.astype(np.int16), real


def _nbits(v):
    v = np.abs(v)
    n = np.zeros(v.shape, np.int64)
    for k in range(12):
        n += (v >> k) > 0
    return n


def entropy(zz, real, comp, mcu, restart, stats=None):
    """-> list of the restart segments' bytes, unstuffed and padded with 1-bits (one segment when restart == 0)."""
    nblk = zz.shape[0]
    seg = mcu // restart if restart else np.zeros(nblk, np.int64)
    nseg = int(seg[-1]) + 1
    # DC differences: per component in scan order, dummies repeat the last coded DC, the prediction restarts with every segment
    diff = np.zeros(nblk, np.int64)
    for c in range(3):
        idx = np.nonzero(comp == c)[0]
        r = real[idx]
        src = np.maximum.accumulate(np.where(r, np.arange(idx.size), 0))
        dc = zz[idx[src], 0]
        prev = np.concatenate([[0], dc[:-1]])
        first = np.concatenate([[True], seg[idx][1:] != seg[idx][:-1]])
        prev[first] = 0
        diff[idx] = dc - prev
    codes = [huff_codes(t) for t in range(4)]
    tb, tk, tc, tl = [], [], [], []             # tokens: block, order key, code, length

    def add(b, k, c, l):
        tb.append(b); tk.append(k); tc.append(c); tl.append(l)

    blocks = np.arange(nblk)
    chroma = comp > 0
    cat = _nbits(diff)
    for ch in (False, True):
        m = chroma == ch
        code, length = codes[2 if ch else 0]
        add(blocks[m], np.full(m.sum(), 3), code[cat[m]], length[cat[m]])
    add(blocks, np.full(nblk, 4), np.where(diff < 0, diff - 1, diff) & ((1 << cat) - 1), cat)
    ac = zz.copy()
    ac[:, 0] = 0
    bi, ki = np.nonzero(ac)
    val = ac[bi, ki]
    prev = np.concatenate([[0], ki[:-1]])
    prev[np.concatenate([[True], bi[1:] != bi[:-1]])] = 0
    run = ki - prev - 1
    size = _nbits(val)
    sym = ((run & 15) << 4) | size
    for ch in (False, True):
        m = chroma[bi] == ch
        code, length = codes[3 if ch else 1]
        for j in range(3):
            z = m & ((run >> 4) > j)
            add(bi[z], ki[z] * 6 + j, np.full(z.sum(), code[0xF0]), np.full(z.sum(), length[0xF0]))
        add(bi[m], ki[m] * 6 + 3, code[sym[m]], length[sym[m]])
        last = np.zeros(nblk, np.int64)
        np.maximum.at(last, bi, ki)
        e = (chroma == ch) & (last < 63)
        add(blocks[e], np.full(e.sum(), 64 * 6), np.full(e.sum(), code[0]), np.full(e.sum(), length[0]))
    add(bi, ki * 6 + 4, np.where(val < 0, val - 1, val) & ((1 << size) - 1), size)
    if stats is not None:
        stats["zrl"] = stats.get("zrl", 0) + int((run >> 4).sum())
        stats["c63"] = stats.get("c63", 0) + int((ki == 63).sum())
    tb, tk, tc, tl = (np.concatenate(a).astype(np.int64) for a in (tb, tk, tc, tl))
    segbits = np.bincount(seg[tb], weights=tl, minlength=nseg).astype(np.int64)
    pad = (-segbits) % 8
    lastblk = np.concatenate([np.nonzero(seg[1:] != seg[:-1])[0], [nblk - 1]])
    tb, tk = np.concatenate([tb, lastblk]), np.concatenate([tk, np.full(nseg, 65 * 6)])
    tc, tl = np.concatenate([tc, (1 << pad) - 1]), np.concatenate([tl, pad])
    order = np.argsort(tb * 512 + tk, kind="stable")
    tc, tl = tc[order], tl[order]
    start = np.cumsum(tl) - tl
    total = int(tl.sum())
    rep = np.repeat(np.arange(tl.size), tl)
    j = np.arange(total) - start[rep]
    bits = ((tc[rep] >> (tl[rep] - 1 - j)) & 1).astype(np.uint8)
    data = np.packbits(bits).tobytes()
    ends = np.cumsum(segbits + pad) // 8
    return [data[(int(ends[s - 1]) if s else 0):int(ends[s])] for s in range(nseg)]


def encode(bgr, sub, quality, restart=0, stats=None):
    """uint8 [H,W,3] BGR -> the bytes of the baseline JPEG file libjpeg writes with its defaults (islow, standard Huffman tables)."""
    bgr = np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3
    H, W = bgr.shape[:2]
    segs = entropy(*scan_blocks(bgr, sub, quality), restart, stats)
    out = [header(W, H, sub, quality, restart)]
    for s, d in enumerate(segs):
        if s:
            out.append(bytes([0xFF, 0xD0 + ((s - 1) & 7)]))
        if stats is not None:
            stats["stuffed"] = stats.get("stuffed", 0) + d.count(b"\xff")
        out.append(d.replace(b"\xff", b"\xff\x00"))
    out.append(b"\xff\xd9")
    return b"".join(out)
