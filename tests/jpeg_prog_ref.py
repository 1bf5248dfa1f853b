"""TEST HELPER: progressive (SOF2) JPEG decoding restated in plain Python, written for this project from the algorithm description in
include/simple_pose_hip.h (sp_jpeg_parse_scans, sp_jpeg_progressive_entropy) and T.81 G.1.2 / G.2: the scan parser with the rules a
progression has to satisfy, and the four block procedures (DC / AC, first pass / refinement) with the EOBRUN state and the correction
bits.  It writes the MCU-padded coefficient layout of tests/jpeg_ref.py, whose bit reader, IDCT, planes and colour conversion finish the
image.  It reproduces libjpeg-turbo (PIL) bit for bit on tests/golden/g17_jpeg_prog.npz.  Never imported by the product."""
import numpy as np

from tests import jpeg_ref
from tests.jpeg_ref import (E_ADOBE, E_ARITHMETIC, E_BAD_TABLE, E_COMPONENTS, E_EXTENDED, E_NO_TABLE, E_NOT_JPEG, E_PRECISION, E_SAMPLING, E_SCANS, E_SIZE,
                            E_TRUNCATED, ST_BAD_CODE, ST_BAD_RUN, ST_SEGMENTS, ZIGZAG, JpegError, _Bits, _Huff, _extend)

E_BAD_SCAN, E_INCOMPLETE = -23, -24


class Scan:
    pass


def parse_scans(data: bytes):
    """-> Info (the fields of jpeg_ref.parse that describe the frame, plus .scans, .seg_offsets = every scan's, .restart_interval = the first
    scan's).  Scan: comps, ss, se, ah, al, restart_interval, ecs_offset, ecs_end, seg_offsets (file offsets), tables = [(counts, values)]
    as the scan uses them (first DC scan: one per component; AC scan: one; DC refinement: none)."""
    d = bytes(data)
    n = len(d)

    def need(pos, k, what):
        if pos + k > n:
            raise JpegError(E_TRUNCATED, f"{what} runs past the end of the file at byte {pos}")

    if n < 2 or d[0] != 0xFF or d[1] != 0xD8:
        raise JpegError(E_NOT_JPEG, "no SOI marker at byte 0")
    o = jpeg_ref.Info()
    o.quant, o.scans, o.width = {}, [], 0
    dc, ac = {}, {}
    ri = 0
    sent = None
    pos = 2
    end_of_scans = n
    while True:
        if o.scans and pos >= n:
            break
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
            if not o.scans:
                raise JpegError(E_SCANS, f"EOI at byte {pos - 2} before any scan")
            break
        need(pos, 2, "segment length")
        L = (d[pos] << 8) | d[pos + 1]
        if L < 2:
            raise JpegError(E_TRUNCATED, f"segment length {L} at byte {pos}")
        need(pos, L, f"segment FF{m:02X}")
        body = d[pos + 2:pos + L]
        if m == 0xC0:
            raise JpegError(E_SCANS, f"baseline SOF0 at byte {pos - 2}")
        elif m == 0xC2:
            if o.width:
                raise JpegError(E_SCANS, f"second SOF at byte {pos - 2}")
            if len(body) < 6:
                raise JpegError(E_TRUNCATED, f"SOF2 too short at byte {pos}")
            if body[0] != 8:
                raise JpegError(E_PRECISION, f"{body[0]}-bit samples")
            o.height, o.width, o.components = (body[1] << 8) | body[2], (body[3] << 8) | body[4], body[5]
            if o.components not in (1, 3):
                raise JpegError(E_COMPONENTS, f"{o.components} components")
            if len(body) != 6 + 3 * o.components:
                raise JpegError(E_TRUNCATED, f"SOF2 length at byte {pos}")
            if not (1 <= o.width <= 16384 and 1 <= o.height <= 16384):
                raise JpegError(E_SIZE, f"size {o.width}x{o.height}")
            o.comp_id = [body[6 + 3 * c] for c in range(o.components)]
            o.h = [body[7 + 3 * c] >> 4 for c in range(o.components)]
            o.v = [body[7 + 3 * c] & 15 for c in range(o.components)]
            o.tq = [body[8 + 3 * c] for c in range(o.components)]
            if any(t > 3 for t in o.tq):
                raise JpegError(E_BAD_TABLE, "quantisation table selector")
            if o.components == 1:
                o.h, o.v = [1], [1]
            elif not ((o.h[0], o.v[0]) in ((1, 1), (2, 1), (2, 2)) and o.h[1:] == [1, 1] and o.v[1:] == [1, 1]):
                raise JpegError(E_SAMPLING, "sampling factors " + " ".join(f"{a}x{b}" for a, b in zip(o.h, o.v)))
            sent = [[-1] * 64 for _ in range(o.components)]
        elif m in (0xC1, 0xC3, 0xC5, 0xC6, 0xC7):
            raise JpegError(E_EXTENDED, f"SOF{m - 0xC0} at byte {pos - 2}")
        elif 0xC9 <= m <= 0xCF:
            raise JpegError(E_ARITHMETIC, f"arithmetic coding (FF{m:02X}) at byte {pos - 2}")
        elif m == 0xDB:
            if o.scans:
                raise JpegError(E_BAD_TABLE, f"DQT at byte {pos - 2} after the first scan")
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
                (ac if tc else dc)[th] = (counts, list(body[q + 17:q + 17 + nv]))
                q += 17 + nv
        elif m == 0xDD:
            if L != 4:
                raise JpegError(E_TRUNCATED, f"DRI length at byte {pos}")
            ri = (body[0] << 8) | body[1]
        elif m == 0xEE:
            if len(body) >= 12 and body[:5] == b"Adobe":
                o.adobe_transform = body[11]
        elif m == 0xDA:
            at = pos - 2
            if not o.width:
                raise JpegError(E_SCANS, f"SOS at byte {at} before SOF2")
            if len(body) < 1 or len(body) != 4 + 2 * body[0]:
                raise JpegError(E_TRUNCATED, f"SOS length at byte {pos}")
            ns = body[0]
            if not 1 <= ns <= o.components:
                raise JpegError(E_BAD_SCAN, f"scan of {ns} of {o.components} components at byte {at}")
            if getattr(o, "adobe_transform", 1) != 1 and o.components == 3:
                raise JpegError(E_ADOBE, f"Adobe APP14 transform {o.adobe_transform}")
            s = Scan()
            s.comps, td, ta = [], [], []
            for j in range(ns):
                if body[1 + 2 * j] not in o.comp_id:
                    raise JpegError(E_BAD_SCAN, f"scan at byte {at}: unknown component")
                c = o.comp_id.index(body[1 + 2 * j])
                if s.comps and c <= s.comps[-1]:
                    raise JpegError(E_BAD_SCAN, f"scan at byte {at}: component twice or out of order")
                s.comps.append(c)
                td.append(body[2 + 2 * j] >> 4)
                ta.append(body[2 + 2 * j] & 15)
            s.ss, s.se, s.ah, s.al = body[1 + 2 * ns], body[2 + 2 * ns], body[3 + 2 * ns] >> 4, body[3 + 2 * ns] & 15
            if s.ss > s.se or s.se > 63 or (s.ss == 0 and s.se != 0) or (s.ss > 0 and ns != 1):
                raise JpegError(E_BAD_SCAN, f"scan at byte {at}: Ss {s.ss}, Se {s.se}")
            if s.al > 13 or (s.ah != 0 and s.al != s.ah - 1):
                raise JpegError(E_BAD_SCAN, f"scan at byte {at}: Ah {s.ah}, Al {s.al}")
            for j, c in enumerate(s.comps):
                if s.ss > 0 and sent[c][0] < 0:
                    raise JpegError(E_BAD_SCAN, f"AC scan at byte {at} of component {c} before its DC scan")
                for k in range(s.ss, s.se + 1):
                    last = sent[c][k]
                    if (s.ah != 0) if last < 0 else (s.ah != last or s.ah == 0):
                        raise JpegError(E_BAD_SCAN, f"scan at byte {at}: component {c} coefficient {k} with Ah {s.ah} after {last}")
                if o.tq[c] not in o.quant:
                    raise JpegError(E_NO_TABLE, f"component {c}: no quantisation table {o.tq[c]}")
                if s.ss == 0 and s.ah == 0 and td[j] not in dc:
                    raise JpegError(E_NO_TABLE, f"component {c}: no DC Huffman table {td[j]}")
                if s.ss > 0 and ta[j] not in ac:
                    raise JpegError(E_NO_TABLE, f"component {c}: no AC Huffman table {ta[j]}")
            for c in s.comps:
                for k in range(s.ss, s.se + 1):
                    sent[c][k] = s.al
            s.tables = [ac[ta[0]]] if s.ss > 0 else ([dc[t] for t in td] if s.ah == 0 else [])
            s.restart_interval = ri
            pos += L
            s.ecs_offset = pos
            s.seg_offsets = [pos]
            end = n
            while pos < n:
                if d[pos] != 0xFF:
                    pos += 1
                    continue
                if pos + 1 >= n:
                    end = pos
                    break
                mm = d[pos + 1]
                if mm == 0x00:
                    pos += 2
                elif mm == 0xFF:
                    pos += 1
                elif 0xD0 <= mm <= 0xD7:
                    pos += 2
                    s.seg_offsets.append(pos)
                else:
                    end = pos
                    break
            s.ecs_end = end_of_scans = end
            o.scans.append(s)
            pos = n if end + 1 >= n else end
            continue
        pos += L
    for c in range(o.components):
        for k in range(10):
            if sent[c][k] != 0:
                raise JpegError(E_INCOMPLETE, f"the progression ends at byte {end_of_scans}: component {c} coefficient {k}: {sent[c][k]}")
    o.ecs_offset, o.ecs_end = o.scans[0].ecs_offset, end_of_scans
    o.restart_interval = o.scans[0].restart_interval
    o.seg_offsets = [x for s in o.scans for x in s.seg_offsets]
    o.mcus_x, o.mcus_y = -(-o.width // (8 * o.h[0])), -(-o.height // (8 * o.v[0]))
    return o


def _bit_correct(br, p1, blk, z):
    if br.get(1) and (int(blk[z]) & p1) == 0:
        blk[z] = int(blk[z]) + (p1 if blk[z] >= 0 else -p1)


def _i16(v):
    return ((int(v) + 32768) & 0xFFFF) - 32768


def scan_grid(info, s):
    """-> (MCUs per row, MCUs) of the scan: the frame's MCU grid when interleaved, the component's own ceil(w / 8) x ceil(h / 8) blocks
    when the scan has one component."""
    if len(s.comps) > 1:
        return info.mcus_x, info.mcus_x * info.mcus_y
    c = s.comps[0]
    cw, ch = -(-info.width * info.h[c] // info.h[0]), -(-info.height * info.v[c] // info.v[0])
    return -(-cw // 8), -(-cw // 8) * -(-ch // 8)


def decode_coefficients(info, data):
    """-> ([per component int16 [blocks_y, blocks_x, 64], natural order, MCU padding included], status)."""
    d = bytes(data)
    nc = info.components
    coef = [np.zeros((info.mcus_y * info.v[c], info.mcus_x * info.h[c], 64), np.int16) for c in range(nc)]
    status = 0
    for s in info.scans:
        tabs = [_Huff(*t) for t in s.tables]
        grid_w, mcus = scan_grid(info, s)
        ri = s.restart_interval or mcus
        if len(s.seg_offsets) != -(-mcus // ri):
            status |= ST_SEGMENTS
        p1 = 1 << s.al
        single = len(s.comps) == 1
        for sg, begin in enumerate(s.seg_offsets):
            if sg * ri >= mcus:
                break
            end = s.seg_offsets[sg + 1] - 2 if sg + 1 < len(s.seg_offsets) else s.ecs_end
            br = _Bits(d, begin, end)
            pred = [0] * 3
            eobrun = 0
            for mcu in range(sg * ri, min(mcus, (sg + 1) * ri)):
                my, mx = divmod(mcu, grid_w)
                if s.ss == 0:
                    for j, c in enumerate(s.comps):
                        h, v = (1, 1) if single else (info.h[c], info.v[c])
                        for vy in range(v):
                            for hx in range(h):
                                blk = coef[c][my * v + vy, mx * h + hx]
                                if s.ah == 0:
                                    t = tabs[j].decode(br)
                                    if t > 15:
                                        br.status |= ST_BAD_CODE
                                        t = 0
                                    pred[j] += _extend(br.get(t), t)
                                    blk[0] = _i16(pred[j] << s.al)
                                elif br.get(1):
                                    blk[0] = _i16(int(blk[0]) | p1)
                                if br.status:
                                    break
                            if br.status:
                                break
                        if br.status:
                            break
                else:
                    blk = coef[s.comps[0]][my, mx]
                    if s.ah == 0:
                        if eobrun > 0:
                            eobrun -= 1
                        else:
                            k = s.ss
                            while k <= s.se and not br.status:
                                rs = tabs[0].decode(br)
                                r, sz = rs >> 4, rs & 15
                                if sz == 0:
                                    if r == 15:
                                        k += 16
                                        continue
                                    eobrun = (1 << r) + br.get(r) - 1
                                    break
                                k += r
                                if k > s.se:
                                    br.status |= ST_BAD_RUN
                                    break
                                blk[ZIGZAG[k]] = _i16(_extend(br.get(sz), sz) << s.al)
                                k += 1
                    else:
                        k = s.ss
                        if eobrun == 0:
                            while k <= s.se and not br.status:
                                rs = tabs[0].decode(br)
                                r, sz = rs >> 4, rs & 15
                                value = 0
                                if sz:
                                    if sz != 1:
                                        br.status |= ST_BAD_CODE
                                        break
                                    value = p1 if br.get(1) else -p1
                                elif r != 15:
                                    eobrun = (1 << r) + br.get(r)
                                    break
                                while k <= s.se:
                                    z = ZIGZAG[k]
                                    if blk[z] != 0:
                                        _bit_correct(br, p1, blk, z)
                                    else:
                                        r -= 1
                                        if r < 0:
                                            break
                                    k += 1
                                if value:
                                    if k > s.se:
                                        br.status |= ST_BAD_RUN
                                        break
                                    blk[ZIGZAG[k]] = value
                                k += 1
                        if eobrun > 0 and not (br.status & (ST_BAD_CODE | ST_BAD_RUN)):
                            while k <= s.se and not br.status:
                                z = ZIGZAG[k]
                                if blk[z] != 0:
                                    _bit_correct(br, p1, blk, z)
                                k += 1
                            eobrun -= 1
                if br.status:
                    break
            status |= br.status
    return coef, status


def decode(data):
    """bytes of one progressive JPEG file -> uint8 BGR [H, W, 3]; raises JpegError on an unsupported or damaged file."""
    info = parse_scans(data)
    coef, status = decode_coefficients(info, data)
    if status:
        raise JpegError(status, f"entropy data: status {status}")
    return jpeg_ref.color(info, jpeg_ref.planes(info, coef))
