"""TEST HELPER: baseline JPEG decoding restated in numpy / plain Python, written for this project from the algorithm description in
include/simple_pose_hip.h (sp_jpeg_parse, sp_jpeg_decode_batch): header parse, canonical Huffman decode, the "islow" integer IDCT, "fancy"
chroma upsampling and the 16.16 fixed-point YCbCr -> BGR conversion.  It reproduces libjpeg-turbo (PIL) bit for bit on the fixture
tests/golden/g15_jpeg.npz and is what the host parser, the sanitized core program and the device kernels are compared with.  Never
imported by the product."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
                   57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# the error codes of include/simple_pose_hip.h
E_TRUNCATED, E_NOT_JPEG, E_PROGRESSIVE, E_EXTENDED, E_ARITHMETIC, E_PRECISION, E_COMPONENTS, E_SAMPLING, E_ADOBE, E_SCANS, E_NO_TABLE, \
    E_BAD_TABLE, E_SIZE = range(-10, -23, -1)
ST_TRUNCATED, ST_BAD_CODE, ST_BAD_RUN, ST_SEGMENTS = 1, 2, 4, 8


class JpegError(ValueError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class Info:
    pass


def parse(data: bytes) -> Info:
    d = bytes(data)
    n = len(d)

    def need(pos, k, what):
        if pos + k > n:
            raise JpegError(E_TRUNCATED, f"{what} runs past the end of the file at byte {pos}")

    if n < 2 or d[0] != 0xFF or d[1] != 0xD8:
        raise JpegError(E_NOT_JPEG, "no SOI marker at byte 0")
    o = Info()
    o.quant, o.dc, o.ac = {}, {}, {}
    o.restart_interval = 0
    o.width = 0
    pos = 2
    while True:
        need(pos, 2, "marker")
        if d[pos] != 0xFF:
            raise JpegError(E_NOT_JPEG, f"expected a marker at byte {pos}")
        m = d[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        pos += 2
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise JpegError(E_SCANS, f"EOI at byte {pos - 2} before any scan")
        need(pos, 2, "segment length")
        L = (d[pos] << 8) | d[pos + 1]
        if L < 2:
            raise JpegError(E_TRUNCATED, f"segment length {L} at byte {pos}")
        need(pos, L, f"segment FF{m:02X}")
        body = d[pos + 2:pos + L]
        if m == 0xC0:
            if o.width:
                raise JpegError(E_SCANS, f"second SOF at byte {pos - 2}")
            if len(body) < 6:
                raise JpegError(E_TRUNCATED, f"SOF0 too short at byte {pos}")
            if body[0] != 8:
                raise JpegError(E_PRECISION, f"{body[0]}-bit samples")
            o.height, o.width, o.components = (body[1] << 8) | body[2], (body[3] << 8) | body[4], body[5]
            if o.components not in (1, 3):
                raise JpegError(E_COMPONENTS, f"{o.components} components")
            if len(body) != 6 + 3 * o.components:
                raise JpegError(E_TRUNCATED, f"SOF0 length at byte {pos}")
            if not (1 <= o.width <= 16384 and 1 <= o.height <= 16384):
                raise JpegError(E_SIZE, f"size {o.width}x{o.height}")
            o.comp_id = [body[6 + 3 * c] for c in range(o.components)]
            o.h = [body[7 + 3 * c] >> 4 for c in range(o.components)]
            o.v = [body[7 + 3 * c] & 15 for c in range(o.components)]
            o.tq = [body[8 + 3 * c] for c in range(o.components)]
            if o.components == 1:
                o.h, o.v = [1], [1]
            elif not ((o.h[0], o.v[0]) in ((1, 1), (2, 1), (2, 2)) and o.h[1:] == [1, 1] and o.v[1:] == [1, 1]):
                raise JpegError(E_SAMPLING, "sampling factors " + " ".join(f"{a}x{b}" for a, b in zip(o.h, o.v)))
            if any(t > 3 for t in o.tq):
                raise JpegError(E_BAD_TABLE, "quantisation table selector")
        elif m in (0xC1, 0xC3, 0xC5, 0xC6, 0xC7):
            raise JpegError(E_EXTENDED, f"SOF{m - 0xC0} at byte {pos - 2}")
        elif m == 0xC2:
            raise JpegError(E_PROGRESSIVE, f"progressive SOF2 at byte {pos - 2}")
        elif m in (0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF, 0xCC):
            raise JpegError(E_ARITHMETIC, f"arithmetic coding (FF{m:02X}) at byte {pos - 2}")
        elif m == 0xDB:
            q = 0
            while q < len(body):
                pq, tq = body[q] >> 4, body[q] & 15
                if pq != 0 or tq > 3 or q + 65 > len(body):
                    raise JpegError(E_BAD_TABLE, f"DQT at byte {pos + 2 + q}")
                t = np.zeros(64, np.int32)
                t[ZIGZAG] = np.frombuffer(body[q + 1:q + 65], np.uint8)
                o.quant[tq] = t
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(body):
                if q + 17 > len(body):
                    raise JpegError(E_BAD_TABLE, f"DHT at byte {pos + 2 + q}")
                tc, th = body[q] >> 4, body[q] & 15
                counts = list(body[q + 1:q + 17])
                nv = sum(counts)
                if tc > 1 or th > 3 or nv > 256 or q + 17 + nv > len(body):
                    raise JpegError(E_BAD_TABLE, f"DHT at byte {pos + 2 + q}")
                code = 0
                for l in range(16):
                    code += counts[l]
                    if code > (1 << (l + 1)):
                        raise JpegError(E_BAD_TABLE, f"DHT at byte {pos + 2 + q}")
                    code <<= 1
                (o.ac if tc else o.dc)[th] = (counts, list(body[q + 17:q + 17 + nv]))
                q += 17 + nv
        elif m == 0xDD:
            if L != 4:
                raise JpegError(E_TRUNCATED, f"DRI length at byte {pos}")
            o.restart_interval = (body[0] << 8) | body[1]
        elif m == 0xEE:
            if len(body) >= 12 and body[:5] == b"Adobe":
                o.adobe_transform = body[11]
        elif m == 0xDA:
            if not o.width:
                raise JpegError(E_SCANS, f"SOS at byte {pos - 2} before SOF0")
            if len(body) < 1 or len(body) != 4 + 2 * body[0]:
                raise JpegError(E_TRUNCATED, f"SOS length at byte {pos}")
            if body[0] != o.components:
                raise JpegError(E_SCANS, f"scan of {body[0]} of {o.components} components at byte {pos - 2}")
            o.td, o.ta = [], []
            for c in range(o.components):
                if body[1 + 2 * c] != o.comp_id[c]:
                    raise JpegError(E_SCANS, f"scan component order at byte {pos - 2}")
                o.td.append(body[2 + 2 * c] >> 4)
                o.ta.append(body[2 + 2 * c] & 15)
            if getattr(o, "adobe_transform", 1) != 1 and o.components == 3:
                raise JpegError(E_ADOBE, f"Adobe APP14 transform {o.adobe_transform}")
            for c in range(o.components):
                if o.tq[c] not in o.quant:
                    raise JpegError(E_NO_TABLE, f"component {c}: no quantisation table {o.tq[c]}")
                if o.td[c] > 3 or o.td[c] not in o.dc:
                    raise JpegError(E_NO_TABLE, f"component {c}: no DC Huffman table {o.td[c]}")
                if o.ta[c] > 3 or o.ta[c] not in o.ac:
                    raise JpegError(E_NO_TABLE, f"component {c}: no AC Huffman table {o.ta[c]}")
            pos += L
            break
        pos += L
    o.ecs_offset = pos
    segs = [pos]
    end = n
    while pos < n:
        if d[pos] != 0xFF:
            pos += 1
            continue
        if pos + 1 >= n:
            end = pos
            break
        m = d[pos + 1]
        if m == 0x00:
            pos += 2
        elif m == 0xFF:
            pos += 1
        elif 0xD0 <= m <= 0xD7:
            pos += 2
            segs.append(pos)
        elif m == 0xD9:
            end = pos
            break
        else:
            raise JpegError(E_SCANS, f"marker FF{m:02X} at byte {pos} after the first scan (multiple scans)")
    o.ecs_end = end
    o.seg_offsets = segs
    hmax, vmax = max(o.h), max(o.v)
    o.mcus_x, o.mcus_y = -(-o.width // (8 * hmax)), -(-o.height // (8 * vmax))
    return o


class _Bits:
    def __init__(self, d, begin, end):
        self.d, self.p, self.end, self.acc, self.n, self.real, self.status = d, begin, end, 0, 0, 0, 0

    def fill(self):
        while self.n <= 24:
            b, real = 0, 0
            if self.p < self.end:
                b = self.d[self.p]
                if b != 0xFF:
                    self.p += 1
                    real = 8
                elif self.p + 1 < self.end and self.d[self.p + 1] == 0:
                    self.p += 2
                    real = 8
                else:
                    b = 0
            self.acc = ((self.acc << 8) | b) & 0xFFFFFFFF
            self.n += 8
            self.real += real                     # once a byte is missing every later one is: real bits are the leading ones

    def peek(self, k):
        return (self.acc >> (self.n - k)) & ((1 << k) - 1)

    def skip(self, k):
        self.n -= k
        self.real -= k
        if self.real < 0:
            self.real = 0
            self.status |= ST_TRUNCATED

    def get(self, k):
        if k == 0:
            return 0
        self.fill()
        v = self.peek(k)
        self.skip(k)
        return v


class _Huff:
    def __init__(self, counts, values):
        self.values = values
        self.maxcode, self.valoff = [-1] * 18, [0] * 18
        code = k = 0
        for l in range(1, 17):
            self.valoff[l] = k - code
            k += counts[l - 1]
            code += counts[l - 1]
            self.maxcode[l] = code - 1 if counts[l - 1] else -1
            code <<= 1

    def decode(self, br):
        br.fill()
        v = br.peek(16)
        for l in range(1, 17):
            code = v >> (16 - l)
            if code <= self.maxcode[l]:
                i = self.valoff[l] + code
                if not 0 <= i < len(self.values):
                    break
                br.skip(l)
                return self.values[i]
        br.status |= ST_BAD_CODE
        return 0


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def decode_coefficients(info, data):
    """-> ([per component int16 [blocks_y, blocks_x, 64], natural order], status)."""
    d = bytes(data)
    nc = info.components
    bw = [info.mcus_x * info.h[c] for c in range(nc)]
    bh = [info.mcus_y * info.v[c] for c in range(nc)]
    coef = [np.zeros((bh[c], bw[c], 64), np.int16) for c in range(nc)]
    dc = [_Huff(*info.dc[info.td[c]]) for c in range(nc)]
    ac = [_Huff(*info.ac[info.ta[c]]) for c in range(nc)]
    mcus = info.mcus_x * info.mcus_y
    ri = info.restart_interval or mcus
    status = 0
    if len(info.seg_offsets) != -(-mcus // ri):
        status |= ST_SEGMENTS
    for s, begin in enumerate(info.seg_offsets):
        if s * ri >= mcus:
            break
        end = info.seg_offsets[s + 1] - 2 if s + 1 < len(info.seg_offsets) else info.ecs_end
        br = _Bits(d, begin, end)
        pred = [0] * nc
        for mcu in range(s * ri, min(mcus, (s + 1) * ri)):
            my, mx = divmod(mcu, info.mcus_x)
            for c in range(nc):
                for vy in range(info.v[c]):
                    for hx in range(info.h[c]):
                        blk = coef[c][my * info.v[c] + vy, mx * info.h[c] + hx]
                        t = dc[c].decode(br)
                        if t > 15:
                            br.status |= ST_BAD_CODE
                            t = 0
                        pred[c] += _extend(br.get(t), t)
                        blk[0] = np.int16(((pred[c] + 32768) & 0xFFFF) - 32768)
                        k = 1
                        while k < 64:
                            rs = ac[c].decode(br)
                            r, sz = rs >> 4, rs & 15
                            if sz == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                br.status |= ST_BAD_RUN
                                break
                            blk[ZIGZAG[k]] = _extend(br.get(sz), sz)
                            k += 1
                        if br.status:
                            break
                    if br.status:
                        break
                if br.status:
                    break
            if br.status:
                break
        status |= br.status
    return coef, status


def _fix(x):
    return int(x * 8192 + 0.5)


def idct_islow(blocks):
    """blocks: int32 [..., 64] dequantised, natural order -> uint8 [..., 8, 8] (jidctint.c, CONST_BITS 13, PASS1_BITS 2)."""
    x = blocks.astype(np.int64).reshape(blocks.shape[:-1] + (8, 8))

    def one_d(i0, i1, i2, i3, i4, i5, i6, i7, shift):
        z2, z3 = i2, i6
        z1 = (z2 + z3) * 4433
        tmp2 = z1 + z3 * -15137
        tmp3 = z1 + z2 * 6270
        tmp0 = (i0 + i4) << 13
        tmp1 = (i0 - i4) << 13
        tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
        t0, t1, t2, t3 = i7, i5, i3, i1
        z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
        z5 = (z3 + z4) * 9633
        t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
        r = 1 << (shift - 1)
        return [(a + r) >> shift for a in (tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3)]

    ws = np.stack(one_d(*[x[..., r, :] for r in range(8)], 11), axis=-2)          # columns: rows r combine
    out = np.stack(one_d(*[ws[..., :, c] for c in range(8)], 18), axis=-1)        # rows: columns c combine
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def planes(info, coef):
    """IDCT of every block -> per component uint8 plane [blocks_y*8, blocks_x*8] (MCU padding included)."""
    out = []
    for c in range(info.components):
        px = idct_islow(coef[c].astype(np.int32) * info.quant[info.tq[c]])
        bh, bw = px.shape[:2]
        out.append(px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return out


def _up_h2v1(p):
    """p: int [rows, cw] -> [rows, 2*cw]; replication when cw <= 2 (libjpeg runs the fancy filter only for wider planes)."""
    p = p.astype(np.int32)
    cw = p.shape[1]
    out = np.empty((p.shape[0], 2 * cw), np.int32)
    if cw <= 2:
        out[:, 0::2], out[:, 1::2] = p, p
        return out
    left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def _up_h2v2(p):
    p = p.astype(np.int32)
    ch, cw = p.shape
    out = np.empty((2 * ch, 2 * cw), np.int32)
    if cw <= 2:
        for dy in (0, 1):
            for dx in (0, 1):
                out[dy::2, dx::2] = p
        return out
    up, down = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
    for dy, nb in ((0, up), (1, down)):
        s = 3 * p + nb
        left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
        ev, od = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
        ev[:, 0], od[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
        out[dy::2, 0::2], out[dy::2, 1::2] = ev, od
    return out


def color(info, pl):
    """Component planes -> uint8 BGR [H, W, 3]."""
    W, H = info.width, info.height
    y = pl[0][:H, :W].astype(np.int32)
    if info.components == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    hmax, vmax = info.h[0], info.v[0]
    cw, ch = -(-W // hmax), -(-H // vmax)
    up = []
    for c in (1, 2):
        p = pl[c][:ch, :cw]
        if hmax == 2 and vmax == 2:
            p = _up_h2v2(p)
        elif hmax == 2:
            p = _up_h2v1(p)
        up.append(p[:H, :W].astype(np.int32) - 128)
    cb, cr = up
    fix = lambda v: int(v * 65536 + 0.5)
    r = y + ((fix(1.402) * cr + 32768) >> 16)
    b = y + ((fix(1.772) * cb + 32768) >> 16)
    g = y + ((-fix(0.34414) * cb + 32768 - fix(0.71414) * cr) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def decode(data):
    """bytes of one baseline JPEG file -> uint8 BGR [H, W, 3]; raises JpegError on an unsupported or damaged file."""
    info = parse(data)
    coef, status = decode_coefficients(info, data)
    if status:
        raise JpegError(status, f"entropy data: status {status}")
    return color(info, planes(info, coef))
