// sp_jpeg_parse.h - the host parser behind sp_jpeg_parse (simple_pose_hip.h): JPEG headers of one file -> sp_jpeg_desc.  Plain C++, no
// HIP: jpeg.hip wraps it, and tests/jpeg_core_main.cpp compiles it into a stand-alone program that runs under the sanitizers.
// Every read goes through `at(pos)` / a checked segment length; the message names the reason and the byte offset.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "simple_pose_hip.h"
#include "sp_jpeg.h"

#define SP_JPEG_FAIL(code, ...)                  \
    do {                                         \
        snprintf(err, (size_t)err_len, __VA_ARGS__); \
        return code;                             \
    } while (0)

// sizes that follow from width / height / sampling: blocks per component, coef_count, plane_bytes, out_bytes.  false when the
// geometry is not one the decoder accepts (the same test sp_jpeg_decode_batch applies to a hand-made descriptor).
inline bool sp_jpeg_geometry(const sp_jpeg_desc& d, int32_t blocks_w[3], int32_t blocks_h[3], int64_t& blocks) {
    if (!(d.components == 1 || d.components == 3)) return false;
    if (d.width < 1 || d.width > 16384 || d.height < 1 || d.height > 16384) return false;
    if (d.components == 1) {
        if (d.h_samp[0] != 1 || d.v_samp[0] != 1) return false;
    } else {
        const bool luma = (d.h_samp[0] == 1 && d.v_samp[0] == 1) || (d.h_samp[0] == 2 && d.v_samp[0] == 1) || (d.h_samp[0] == 2 && d.v_samp[0] == 2);
        if (!luma || d.h_samp[1] != 1 || d.v_samp[1] != 1 || d.h_samp[2] != 1 || d.v_samp[2] != 1) return false;
    }
    if (d.mcus_x != (d.width + 8 * d.h_samp[0] - 1) / (8 * d.h_samp[0]) || d.mcus_y != (d.height + 8 * d.v_samp[0] - 1) / (8 * d.v_samp[0])) return false;
    blocks = 0;
    for (int c = 0; c < d.components; ++c) {
        blocks_w[c] = d.mcus_x * d.h_samp[c];
        blocks_h[c] = d.mcus_y * d.v_samp[c];
        blocks += (int64_t)blocks_w[c] * blocks_h[c];
    }
    return blocks * 64 < (1ll << 31);
}

inline int sp_jpeg_parse_impl(const uint8_t* d, int64_t n, sp_jpeg_desc* o, int32_t* seg_offsets, int32_t seg_capacity, char* err, int err_len) {
    if (!d || !o || n < 0 || seg_capacity < 0 || (seg_capacity > 0 && !seg_offsets)) SP_JPEG_FAIL(SP_EINVAL, "sp_jpeg_parse: null pointer or negative size");
    if (n >= (1ll << 31)) SP_JPEG_FAIL(SP_JPEG_ESIZE, "sp_jpeg_parse: file of %lld bytes (2 GiB and more)", (long long)n);
    memset(o, 0, sizeof(*o));
    if (n < 2 || d[0] != 0xFF || d[1] != 0xD8) SP_JPEG_FAIL(SP_JPEG_ENOT_JPEG, "sp_jpeg_parse: no SOI marker at byte 0");
    unsigned quant_seen = 0, huff_seen = 0;
    int adobe_transform = -1, comp_id[3] = {0, 0, 0};
    bool have_sof = false;
    int64_t pos = 2;
    for (;;) {
        if (pos + 2 > n) SP_JPEG_FAIL(SP_JPEG_ETRUNCATED, "sp_jpeg_parse: marker runs past the end of the file at byte %lld", (long long)pos);
        if (d[pos] != 0xFF) SP_JPEG_FAIL(SP_JPEG_ENOT_JPEG, "sp_jpeg_parse: expected a marker at byte %lld", (long long)pos);
        const int m = d[pos + 1];
        if (m == 0xFF) { pos += 1; continue; }
        pos += 2;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD9) SP_JPEG_FAIL(SP_JPEG_ESCANS, "sp_jpeg_parse: EOI at byte %lld before any scan", (long long)pos - 2);
        if (pos + 2 > n) SP_JPEG_FAIL(SP_JPEG_ETRUNCATED, "sp_jpeg_parse: segment length runs past the end of the file at byte %lld", (long long)pos);
        const int L = (d[pos] << 8) | d[pos + 1];
        if (L < 2) SP_JPEG_FAIL(SP_JPEG_ETRUNCATED, "sp_jpeg_parse: segment length %d at byte %lld", L, (long long)pos);
        if (pos + L > n) SP_JPEG_FAIL(SP_JPEG_ETRUNCATED, "sp_jpeg_parse: segment FF%02X runs past the end of the file at byte %lld", m, (long long)pos);
        const uint8_t* body = d + pos + 2;
        const int bl = L - 2;
        if (m == 0xC0) {
            if (have_sof) SP_JPEG_FAIL(SP_JPEG_ESCANS, "sp_jpeg_parse: second SOF at byte %lld", (long long)pos - 2);
            if (bl < 6) SP_JPEG_FAIL(SP_JPEG_ETRUNCATED, "sp_jpeg_parse: SOF0 too short at byte %lld", (long long)pos);
            if (body[0] != 8) SP_JPEG_FAIL(SP_JPEG_EPRECISION, "sp_jpeg_parse: %d-bit samples (8-bit only)", body[0]);
            o->height = (body[1] << 8) | body[2];
            o->width = (body[3] << 8) | body[4];
            o->components = body[5];
            if (o->components != 1 && o->components != 3) SP_JPEG_FAIL(SP_JPEG_ECOMPONENTS, "sp_jpeg_parse: %d components (1 or 3)", o->components);
            if (bl != 6 + 3 * o->components) SP_JPEG_FAIL(SP_JPEG_ETRUNCATED, "sp_jpeg_parse: SOF0 length at byte %lld", (long long)pos);
            if (o->width < 1 || o->width > 16384 || o->height < 1 || o->height > 16384)
                SP_JPEG_FAIL(SP_JPEG_ESIZE, "sp_jpeg_parse: size %dx%d (1..16384)", o->width, o->height);
            for (int c = 0; c < o->components; ++c) {
                comp_id[c] = body[6 + 3 * c];
                o->h_samp[c] = body[7 + 3 * c] >> 4;
                o->v_samp[c] = body[7 + 3 * c] & 15;
                o->quant_sel[c] = body[8 + 3 * c];
                if (o->quant_sel[c] > 3) SP_JPEG_FAIL(SP_JPEG_EBAD_TABLE, "sp_jpeg_parse: quantisation table selector %d at byte %lld", o->quant_sel[c], (long long)pos);
            }
            if (o->components == 1) {
                o->h_samp[0] = o->v_samp[0] = 1;
            } else {
                const int h = o->h_samp[0], v = o->v_samp[0];
                const bool luma = (h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2);
                if (!luma || o->h_samp[1] != 1 || o->v_samp[1] != 1 || o->h_samp[2] != 1 || o->v_samp[2] != 1)
                    SP_JPEG_FAIL(SP_JPEG_ESAMPLING, "sp_jpeg_parse: sampling factors %dx%d %dx%d %dx%d (luma 1x1, 2x1 or 2x2 with 1x1 chroma)", h, v,
                                 o->h_samp[1], o->v_samp[1], o->h_samp[2], o->v_samp[2]);
            }
            have_sof = true;
        } else if (m == 0xC1 || m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7) {
            SP_JPEG_FAIL(SP_JPEG_EEXTENDED, "sp_jpeg_parse: SOF%d at byte %lld (baseline SOF0 only)", m - 0xC0, (long long)pos - 2);
        } else if (m == 0xC2) {
            SP_JPEG_FAIL(SP_JPEG_EPROGRESSIVE, "sp_jpeg_parse: progressive SOF2 at byte %lld", (long long)pos - 2);
        } else if (m >= 0xC9 && m <= 0xCF) {
            SP_JPEG_FAIL(SP_JPEG_EARITHMETIC, "sp_jpeg_parse: arithmetic coding (FF%02X) at byte %lld", m, (long long)pos - 2);
        } else if (m == 0xDB) {
            for (int q = 0; q < bl; q += 65) {
                const int pq = body[q] >> 4, tq = body[q] & 15;
                if (pq != 0 || tq > 3 || q + 65 > bl) SP_JPEG_FAIL(SP_JPEG_EBAD_TABLE, "sp_jpeg_parse: DQT at byte %lld (8-bit tables 0..3)", (long long)pos + 2 + q);
                for (int k = 0; k < 64; ++k) o->quant[tq][sp_jpeg_natural(k)] = body[q + 1 + k];
                quant_seen |= 1u << tq;
            }
        } else if (m == 0xC4) {
            for (int q = 0; q < bl;) {
                if (q + 17 > bl) SP_JPEG_FAIL(SP_JPEG_EBAD_TABLE, "sp_jpeg_parse: DHT at byte %lld", (long long)pos + 2 + q);
                const int tc = body[q] >> 4, th = body[q] & 15;
                int nv = 0;
                for (int l = 0; l < 16; ++l) nv += body[q + 1 + l];
                if (tc > 1 || th > 3 || nv > 256 || q + 17 + nv > bl) SP_JPEG_FAIL(SP_JPEG_EBAD_TABLE, "sp_jpeg_parse: DHT at byte %lld", (long long)pos + 2 + q);
                const int t = 4 * tc + th;
                memcpy(o->huff_counts[t], body + q + 1, 16);
                memset(o->huff_values[t], 0, 256);
                memcpy(o->huff_values[t], body + q + 17, (size_t)nv);
                sp_jpeg_huff probe;
                if (sp_jpeg_huff_build(probe, o->huff_counts[t], o->huff_values[t], 256))
                    SP_JPEG_FAIL(SP_JPEG_EBAD_TABLE, "sp_jpeg_parse: DHT at byte %lld: the counts are no prefix code", (long long)pos + 2 + q);
                huff_seen |= 1u << t;
                q += 17 + nv;
            }
        } else if (m == 0xDD) {
            if (L != 4) SP_JPEG_FAIL(SP_JPEG_ETRUNCATED, "sp_jpeg_parse: DRI length at byte %lld", (long long)pos);
            o->restart_interval = (body[0] << 8) | body[1];
        } else if (m == 0xEE) {
            if (bl >= 12 && memcmp(body, "Adobe", 5) == 0) adobe_transform = body[11];
        } else if (m == 0xDA) {
            if (!have_sof) SP_JPEG_FAIL(SP_JPEG_ESCANS, "sp_jpeg_parse: SOS at byte %lld before SOF0", (long long)pos - 2);
            if (bl < 1 || bl != 4 + 2 * body[0]) SP_JPEG_FAIL(SP_JPEG_ETRUNCATED, "sp_jpeg_parse: SOS length at byte %lld", (long long)pos);
            if (body[0] != o->components)
                SP_JPEG_FAIL(SP_JPEG_ESCANS, "sp_jpeg_parse: scan of %d of %d components at byte %lld (one interleaved scan only)", body[0], o->components,
                             (long long)pos - 2);
            for (int c = 0; c < o->components; ++c) {
                if (body[1 + 2 * c] != comp_id[c]) SP_JPEG_FAIL(SP_JPEG_ESCANS, "sp_jpeg_parse: scan component order at byte %lld", (long long)pos - 2);
                o->dc_sel[c] = body[2 + 2 * c] >> 4;
                o->ac_sel[c] = body[2 + 2 * c] & 15;
            }
            if (adobe_transform >= 0 && adobe_transform != 1 && o->components == 3)
                SP_JPEG_FAIL(SP_JPEG_EADOBE, "sp_jpeg_parse: Adobe APP14 transform %d (YCbCr only)", adobe_transform);
            for (int c = 0; c < o->components; ++c) {
                if (!(quant_seen >> o->quant_sel[c] & 1u)) SP_JPEG_FAIL(SP_JPEG_ENO_TABLE, "sp_jpeg_parse: component %d: no quantisation table %d", c, o->quant_sel[c]);
                if (o->dc_sel[c] > 3 || !(huff_seen >> o->dc_sel[c] & 1u)) SP_JPEG_FAIL(SP_JPEG_ENO_TABLE, "sp_jpeg_parse: component %d: no DC Huffman table %d", c, o->dc_sel[c]);
                if (o->ac_sel[c] > 3 || !(huff_seen >> (4 + o->ac_sel[c]) & 1u)) SP_JPEG_FAIL(SP_JPEG_ENO_TABLE, "sp_jpeg_parse: component %d: no AC Huffman table %d", c, o->ac_sel[c]);
            }
            pos += L;
            break;
        }
        pos += L;
    }
    o->ecs_offset = (int32_t)pos;
    int32_t segs = 0;
    if (segs < seg_capacity) seg_offsets[segs] = (int32_t)pos;
    segs += 1;
    int64_t end = n;
    while (pos < n) {
        const uint8_t* f = (const uint8_t*)memchr(d + pos, 0xFF, (size_t)(n - pos));
        if (!f) break;
        pos = f - d;
        if (pos + 1 >= n) { end = pos; break; }
        const int m = d[pos + 1];
        if (m == 0x00) pos += 2;
        else if (m == 0xFF) pos += 1;
        else if (m >= 0xD0 && m <= 0xD7) {
            pos += 2;
            if (segs < seg_capacity) seg_offsets[segs] = (int32_t)pos;
            segs += 1;
        } else if (m == 0xD9) { end = pos; break; }
        else SP_JPEG_FAIL(SP_JPEG_ESCANS, "sp_jpeg_parse: marker FF%02X at byte %lld after the first scan (multiple scans)", m, (long long)pos);
    }
    o->ecs_end = (int32_t)end;
    o->segments = segs;
    o->file_bytes = (int32_t)n;
    o->mcus_x = (o->width + 8 * o->h_samp[0] - 1) / (8 * o->h_samp[0]);
    o->mcus_y = (o->height + 8 * o->v_samp[0] - 1) / (8 * o->v_samp[0]);
    int32_t bw[3], bh[3];
    int64_t blocks = 0;
    if (!sp_jpeg_geometry(*o, bw, bh, blocks)) SP_JPEG_FAIL(SP_JPEG_ESIZE, "sp_jpeg_parse: size %dx%d", o->width, o->height);
    o->coef_count = (int32_t)(blocks * 64);
    o->plane_bytes = (int32_t)(blocks * 64);
    o->out_bytes = o->height * o->width * 3;
    return SP_OK;
}
