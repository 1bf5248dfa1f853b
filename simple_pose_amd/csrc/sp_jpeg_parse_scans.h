// sp_jpeg_parse_scans.h - the host parser behind sp_jpeg_parse_scans (simple_pose_hip.h): the headers of one progressive (SOF2) JPEG
// file -> sp_jpeg_desc + one sp_jpeg_scan per scan + the restart segments of every scan.  Plain C++, no HIP: jpeg_prog.hip wraps it, and
// tests/jpeg_prog_core_main.cpp compiles it into a stand-alone program that runs under the sanitizers.  Every read is preceded by a
// check of the marker / segment length against the buffer; the message names the reason and the byte offset.
// What a progression has to satisfy is libjpeg's rule (jdphuff start_pass / jdcoefct smoothing_ok), restated:
//   - a scan header it rejects or warns about is refused (SP_JPEG_EBAD_SCAN); stricter in one point: a coefficient is never sent with
//     Ah == 0 twice;
//   - at the end every component needs its DC and zigzag coefficients 1..9 down to bit 0 (SP_JPEG_EINCOMPLETE): otherwise
//     libjpeg-turbo switches to its block-smoothing output, whose pixels the ordinary IDCT does not give.
#pragma once
#include "sp_jpeg_parse.h"

inline int sp_jpeg_parse_scans_impl(const uint8_t* d, int64_t n, sp_jpeg_desc* o, sp_jpeg_scan* scans, int32_t scan_capacity, int32_t* scan_count,
                                    int32_t* seg_offsets, int32_t seg_capacity, char* err, int err_len) {
    if (!d || !o || !scan_count || n < 0 || scan_capacity < 0 || seg_capacity < 0 || (scan_capacity > 0 && !scans) || (seg_capacity > 0 && !seg_offsets))
        SP_JPEG_FAIL(SP_EINVAL, "sp_jpeg_parse_scans: null pointer or negative size");
    if (n >= (1ll << 31)) SP_JPEG_FAIL(SP_JPEG_ESIZE, "sp_jpeg_parse_scans: file of %lld bytes (2 GiB and more)", (long long)n);
    memset(o, 0, sizeof(*o));
    *scan_count = 0;
    if (n < 2 || d[0] != 0xFF || d[1] != 0xD8) SP_JPEG_FAIL(SP_JPEG_ENOT_JPEG, "sp_jpeg_parse_scans: no SOI marker at byte 0");
    unsigned quant_seen = 0, huff_seen = 0;
    uint8_t huff_counts[8][16], huff_values[8][256];     // the slots as the DHT segments so far left them: [4 * class + index]
    memset(huff_counts, 0, sizeof(huff_counts));
    memset(huff_values, 0, sizeof(huff_values));
    int adobe_transform = -1, comp_id[3] = {0, 0, 0}, restart_interval = 0;
    int8_t sent_al[3][64];                               // the Al each coefficient of each component was last sent with, -1 = never
    memset(sent_al, -1, sizeof(sent_al));
    bool have_sof = false;
    int32_t nscans = 0, segs = 0;
    int64_t pos = 2, end_of_scans = n;
    for (;;) {
        if (nscans > 0 && pos >= n) break;               // the file ends after a scan without an EOI: what there is gets judged below
        if (pos + 2 > n) SP_JPEG_FAIL(SP_JPEG_ETRUNCATED, "sp_jpeg_parse_scans: marker runs past the end of the file at byte %lld", (long long)pos);
        if (d[pos] != 0xFF) SP_JPEG_FAIL(SP_JPEG_ENOT_JPEG, "sp_jpeg_parse_scans: expected a marker at byte %lld", (long long)pos);
        const int m = d[pos + 1];
        if (m == 0xFF) { pos += 1; continue; }
        pos += 2;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD9) {
            if (nscans == 0) SP_JPEG_FAIL(SP_JPEG_ESCANS, "sp_jpeg_parse_scans: EOI at byte %lld before any scan", (long long)pos - 2);
            break;
        }
        if (pos + 2 > n) SP_JPEG_FAIL(SP_JPEG_ETRUNCATED, "sp_jpeg_parse_scans: segment length runs past the end of the file at byte %lld", (long long)pos);
        const int L = (d[pos] << 8) | d[pos + 1];
        if (L < 2) SP_JPEG_FAIL(SP_JPEG_ETRUNCATED, "sp_jpeg_parse_scans: segment length %d at byte %lld", L, (long long)pos);
        if (pos + L > n) SP_JPEG_FAIL(SP_JPEG_ETRUNCATED, "sp_jpeg_parse_scans: segment FF%02X runs past the end of the file at byte %lld", m, (long long)pos);
        const uint8_t* body = d + pos + 2;
        const int bl = L - 2;
        if (m == 0xC0) {
            SP_JPEG_FAIL(SP_JPEG_ESCANS, "sp_jpeg_parse_scans: baseline SOF0 at byte %lld (sp_jpeg_parse takes single-scan baseline files; multi-scan SOF0 is not decoded)",
                         (long long)pos - 2);
        } else if (m == 0xC2) {
            if (have_sof) SP_JPEG_FAIL(SP_JPEG_ESCANS, "sp_jpeg_parse_scans: second SOF at byte %lld", (long long)pos - 2);
            if (bl < 6) SP_JPEG_FAIL(SP_JPEG_ETRUNCATED, "sp_jpeg_parse_scans: SOF2 too short at byte %lld", (long long)pos);
            if (body[0] != 8) SP_JPEG_FAIL(SP_JPEG_EPRECISION, "sp_jpeg_parse_scans: %d-bit samples (8-bit only)", body[0]);
            o->height = (body[1] << 8) | body[2];
            o->width = (body[3] << 8) | body[4];
            o->components = body[5];
            if (o->components != 1 && o->components != 3) SP_JPEG_FAIL(SP_JPEG_ECOMPONENTS, "sp_jpeg_parse_scans: %d components (1 or 3)", o->components);
            if (bl != 6 + 3 * o->components) SP_JPEG_FAIL(SP_JPEG_ETRUNCATED, "sp_jpeg_parse_scans: SOF2 length at byte %lld", (long long)pos);
            if (o->width < 1 || o->width > 16384 || o->height < 1 || o->height > 16384)
                SP_JPEG_FAIL(SP_JPEG_ESIZE, "sp_jpeg_parse_scans: size %dx%d (1..16384)", o->width, o->height);
            for (int c = 0; c < o->components; ++c) {
                comp_id[c] = body[6 + 3 * c];
                o->h_samp[c] = body[7 + 3 * c] >> 4;
                o->v_samp[c] = body[7 + 3 * c] & 15;
                o->quant_sel[c] = body[8 + 3 * c];
                if (o->quant_sel[c] > 3)
                    SP_JPEG_FAIL(SP_JPEG_EBAD_TABLE, "sp_jpeg_parse_scans: quantisation table selector %d at byte %lld", o->quant_sel[c], (long long)pos);
            }
            if (o->components == 1) {
                o->h_samp[0] = o->v_samp[0] = 1;
            } else {
                const int h = o->h_samp[0], v = o->v_samp[0];
                const bool luma = (h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2);
                if (!luma || o->h_samp[1] != 1 || o->v_samp[1] != 1 || o->h_samp[2] != 1 || o->v_samp[2] != 1)
                    SP_JPEG_FAIL(SP_JPEG_ESAMPLING, "sp_jpeg_parse_scans: sampling factors %dx%d %dx%d %dx%d (luma 1x1, 2x1 or 2x2 with 1x1 chroma)", h, v,
                                 o->h_samp[1], o->v_samp[1], o->h_samp[2], o->v_samp[2]);
            }
            have_sof = true;
        } else if (m == 0xC1 || m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7) {
            SP_JPEG_FAIL(SP_JPEG_EEXTENDED, "sp_jpeg_parse_scans: SOF%d at byte %lld (progressive SOF2 only)", m - 0xC0, (long long)pos - 2);
        } else if (m >= 0xC9 && m <= 0xCF) {
            SP_JPEG_FAIL(SP_JPEG_EARITHMETIC, "sp_jpeg_parse_scans: arithmetic coding (FF%02X) at byte %lld", m, (long long)pos - 2);
        } else if (m == 0xDB) {
            // libjpeg latches a component's table at its first scan; no writer in use sends one later, and it is not worth the state
            if (nscans > 0) SP_JPEG_FAIL(SP_JPEG_EBAD_TABLE, "sp_jpeg_parse_scans: DQT at byte %lld after the first scan", (long long)pos - 2);
            for (int q = 0; q < bl; q += 65) {
                const int pq = body[q] >> 4, tq = body[q] & 15;
                if (pq != 0 || tq > 3 || q + 65 > bl) SP_JPEG_FAIL(SP_JPEG_EBAD_TABLE, "sp_jpeg_parse_scans: DQT at byte %lld (8-bit tables 0..3)", (long long)pos + 2 + q);
                for (int k = 0; k < 64; ++k) o->quant[tq][sp_jpeg_natural(k)] = body[q + 1 + k];
                quant_seen |= 1u << tq;
            }
        } else if (m == 0xC4) {
            for (int q = 0; q < bl;) {
                if (q + 17 > bl) SP_JPEG_FAIL(SP_JPEG_EBAD_TABLE, "sp_jpeg_parse_scans: DHT at byte %lld", (long long)pos + 2 + q);
                const int tc = body[q] >> 4, th = body[q] & 15;
                int nv = 0;
                for (int l = 0; l < 16; ++l) nv += body[q + 1 + l];
                if (tc > 1 || th > 3 || nv > 256 || q + 17 + nv > bl) SP_JPEG_FAIL(SP_JPEG_EBAD_TABLE, "sp_jpeg_parse_scans: DHT at byte %lld", (long long)pos + 2 + q);
                const int t = 4 * tc + th;
                memcpy(huff_counts[t], body + q + 1, 16);
                memset(huff_values[t], 0, 256);
                memcpy(huff_values[t], body + q + 17, (size_t)nv);
                sp_jpeg_huff probe;
                if (sp_jpeg_huff_build(probe, huff_counts[t], huff_values[t], 256))
                    SP_JPEG_FAIL(SP_JPEG_EBAD_TABLE, "sp_jpeg_parse_scans: DHT at byte %lld: the counts are no prefix code", (long long)pos + 2 + q);
                huff_seen |= 1u << t;
                q += 17 + nv;
            }
        } else if (m == 0xDD) {
            if (L != 4) SP_JPEG_FAIL(SP_JPEG_ETRUNCATED, "sp_jpeg_parse_scans: DRI length at byte %lld", (long long)pos);
            restart_interval = (body[0] << 8) | body[1];
        } else if (m == 0xEE) {
            if (bl >= 12 && memcmp(body, "Adobe", 5) == 0) adobe_transform = body[11];
        } else if (m == 0xDA) {
            const long long at = (long long)pos - 2;
            if (!have_sof) SP_JPEG_FAIL(SP_JPEG_ESCANS, "sp_jpeg_parse_scans: SOS at byte %lld before SOF2", at);
            if (bl < 1 || bl != 4 + 2 * body[0]) SP_JPEG_FAIL(SP_JPEG_ETRUNCATED, "sp_jpeg_parse_scans: SOS length at byte %lld", (long long)pos);
            const int ns = body[0];
            if (ns < 1 || ns > o->components) SP_JPEG_FAIL(SP_JPEG_EBAD_SCAN, "sp_jpeg_parse_scans: scan of %d of %d components at byte %lld", ns, o->components, at);
            if (adobe_transform >= 0 && adobe_transform != 1 && o->components == 3)
                SP_JPEG_FAIL(SP_JPEG_EADOBE, "sp_jpeg_parse_scans: Adobe APP14 transform %d (YCbCr only)", adobe_transform);
            int comp[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
            for (int j = 0; j < ns; ++j) {
                int c = 0;
                while (c < o->components && comp_id[c] != body[1 + 2 * j]) ++c;
                if (c == o->components) SP_JPEG_FAIL(SP_JPEG_EBAD_SCAN, "sp_jpeg_parse_scans: scan at byte %lld names component id %d, which the frame does not have", at, body[1 + 2 * j]);
                if (j > 0 && c <= comp[j - 1])
                    SP_JPEG_FAIL(SP_JPEG_EBAD_SCAN, "sp_jpeg_parse_scans: scan at byte %lld lists a component twice or out of order", at);
                comp[j] = c;
                td[j] = body[2 + 2 * j] >> 4;
                ta[j] = body[2 + 2 * j] & 15;
            }
            const int ss = body[1 + 2 * ns], se = body[2 + 2 * ns], ah = body[3 + 2 * ns] >> 4, al = body[3 + 2 * ns] & 15;
            if (ss > se || se > 63 || (ss == 0 && se != 0) || (ss > 0 && ns != 1))
                SP_JPEG_FAIL(SP_JPEG_EBAD_SCAN, "sp_jpeg_parse_scans: scan at byte %lld: Ss %d, Se %d with %d components (DC scans are 0..0, AC scans 1..63 of one component)", at,
                             ss, se, ns);
            if (al > 13 || (ah != 0 && al != ah - 1))
                SP_JPEG_FAIL(SP_JPEG_EBAD_SCAN, "sp_jpeg_parse_scans: scan at byte %lld: Ah %d, Al %d (Al <= 13, a refinement lowers the bit by one)", at, ah, al);
            for (int j = 0; j < ns; ++j) {
                const int c = comp[j];
                if (ss > 0 && sent_al[c][0] < 0) SP_JPEG_FAIL(SP_JPEG_EBAD_SCAN, "sp_jpeg_parse_scans: AC scan at byte %lld of component %d before its DC scan", at, c);
                for (int k = ss; k <= se; ++k) {
                    const int last = sent_al[c][k];
                    if (last < 0 ? ah != 0 : (ah != last || ah == 0))
                        SP_JPEG_FAIL(SP_JPEG_EBAD_SCAN, "sp_jpeg_parse_scans: scan at byte %lld: component %d coefficient %d with Ah %d after %s%d", at, c, k, ah,
                                     last < 0 ? "no first pass, Al " : "Al ", last);
                }
                if (!(quant_seen >> o->quant_sel[c] & 1u))
                    SP_JPEG_FAIL(SP_JPEG_ENO_TABLE, "sp_jpeg_parse_scans: scan at byte %lld: component %d: no quantisation table %d", at, c, o->quant_sel[c]);
                if (ss == 0 && ah == 0 && (td[j] > 3 || !(huff_seen >> td[j] & 1u)))
                    SP_JPEG_FAIL(SP_JPEG_ENO_TABLE, "sp_jpeg_parse_scans: scan at byte %lld: component %d: no DC Huffman table %d", at, c, td[j]);
                if (ss > 0 && (ta[j] > 3 || !(huff_seen >> (4 + ta[j]) & 1u)))
                    SP_JPEG_FAIL(SP_JPEG_ENO_TABLE, "sp_jpeg_parse_scans: scan at byte %lld: component %d: no AC Huffman table %d", at, c, ta[j]);
            }
            for (int j = 0; j < ns; ++j)
                for (int k = ss; k <= se; ++k) sent_al[comp[j]][k] = (int8_t)al;
            pos += L;
            // this scan's restart segments: the FF D0..D7 search of the baseline parser, up to the next marker of another kind
            const int64_t ecs = pos;
            const int32_t seg0 = segs;
            if (segs < seg_capacity) seg_offsets[segs] = (int32_t)pos;
            segs += 1;
            int64_t end = n;
            while (pos < n) {
                const uint8_t* f = (const uint8_t*)memchr(d + pos, 0xFF, (size_t)(n - pos));
                if (!f) break;
                pos = f - d;
                if (pos + 1 >= n) { end = pos; break; }
                const int mm = d[pos + 1];
                if (mm == 0x00) pos += 2;
                else if (mm == 0xFF) pos += 1;
                else if (mm >= 0xD0 && mm <= 0xD7) {
                    pos += 2;
                    if (segs < seg_capacity) seg_offsets[segs] = (int32_t)pos;
                    segs += 1;
                } else { end = pos; break; }
            }
            if (nscans < scan_capacity) {
                sp_jpeg_scan& s = scans[nscans];
                memset(&s, 0, sizeof(s));
                s.components = ns;
                for (int j = 0; j < ns; ++j) s.comp[j] = comp[j];
                s.ss = ss; s.se = se; s.ah = ah; s.al = al;
                s.restart_interval = restart_interval;
                s.ecs_offset = (int32_t)ecs; s.ecs_end = (int32_t)end;
                s.seg_index = seg0; s.segments = segs - seg0;
                if (ss > 0) {
                    memcpy(s.huff_counts[0], huff_counts[4 + ta[0]], 16);
                    memcpy(s.huff_values[0], huff_values[4 + ta[0]], 256);
                } else if (ah == 0) {
                    for (int j = 0; j < ns; ++j) {
                        memcpy(s.huff_counts[j], huff_counts[td[j]], 16);
                        memcpy(s.huff_values[j], huff_values[td[j]], 256);
                    }
                }
            }
            if (nscans == 0) { o->ecs_offset = (int32_t)ecs; o->restart_interval = restart_interval; }
            nscans += 1;
            end_of_scans = end;
            pos = end < n && end + 1 >= n ? n : end;     // a lone FF as the file's last byte is the end of the file
            continue;
        }
        pos += L;
    }
    *scan_count = nscans;
    for (int c = 0; c < o->components; ++c) {
        if (sent_al[c][0] < 0) SP_JPEG_FAIL(SP_JPEG_EINCOMPLETE, "sp_jpeg_parse_scans: the progression ends at byte %lld without a DC scan of component %d", (long long)end_of_scans, c);
        for (int k = 0; k <= 9; ++k) {
            if (sent_al[c][k] < 0)
                SP_JPEG_FAIL(SP_JPEG_EINCOMPLETE, "sp_jpeg_parse_scans: the progression ends at byte %lld: component %d coefficient %d was never sent", (long long)end_of_scans,
                             c, k);
            if (sent_al[c][k] != 0)
                SP_JPEG_FAIL(SP_JPEG_EINCOMPLETE, "sp_jpeg_parse_scans: the progression ends at byte %lld: component %d coefficient %d stops at bit %d", (long long)end_of_scans,
                             c, k, sent_al[c][k]);
        }
    }
    o->ecs_end = (int32_t)end_of_scans;
    o->segments = segs;
    o->file_bytes = (int32_t)n;
    o->mcus_x = (o->width + 8 * o->h_samp[0] - 1) / (8 * o->h_samp[0]);
    o->mcus_y = (o->height + 8 * o->v_samp[0] - 1) / (8 * o->v_samp[0]);
    int32_t bw[3], bh[3];
    int64_t blocks = 0;
    if (!sp_jpeg_geometry(*o, bw, bh, blocks)) SP_JPEG_FAIL(SP_JPEG_ESIZE, "sp_jpeg_parse_scans: size %dx%d", o->width, o->height);
    o->coef_count = (int32_t)(blocks * 64);
    o->plane_bytes = (int32_t)(blocks * 64);
    o->out_bytes = o->height * o->width * 3;
    return SP_OK;
}
