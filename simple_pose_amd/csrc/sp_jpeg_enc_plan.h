// sp_jpeg_enc_plan.h - the host half of the JPEG encoder: sp_jpeg_enc_plan's body (geometry, scaled tables, Huffman code tables, the
// complete header bytes, the workspace layout).  Plain C++, no HIP header, no GPU call: jpeg_enc.hip wraps it in the C entry point and
// tests/jpeg_enc_core_main.cpp calls it directly under the sanitizers.
#pragma once
#include <stdio.h>
#include <string.h>

#include "sp_jpeg_enc.h"

#define SP_JPEG_ENC_CHUNK 256        // elements per chunk of the three prefix sums (one per lane of a 256-thread workgroup)
#define SP_JPEG_ENC_LANE_BYTES 16    // stream bytes per lane of the stuffing stage: one element of the third prefix sum

SP_JPEG_HD int64_t sp_jpeg_enc_round64(int64_t v) { return (v + 63) / 64 * 64; }

// code and length of every symbol of standard table t
static inline void sp_jpeg_enc_build_codes(int t, uint16_t* code, uint8_t* len) {
    memset(code, 0, 256 * sizeof(uint16_t));
    memset(len, 0, 256);
    int c = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < sp_jpeg_enc_std_count(t, l - 1); ++i, ++k, ++c) {
            const int v = sp_jpeg_enc_std_value(t, k);
            code[v] = (uint16_t)c;
            len[v] = (uint8_t)l;
        }
        c <<= 1;
    }
}

static inline int sp_jpeg_enc_plan_impl(int width, int height, int subsampling, int quality, int restart_interval, sp_jpeg_enc_desc* desc, char* err,
                                        int err_size) {
    if (err_size > 0) err[0] = 0;
    if (!desc) {
        snprintf(err, err_size, "sp_jpeg_enc_plan: null pointer (desc)");
        return SP_EINVAL;
    }
    if (width < 1 || height < 1 || width > 16384 || height > 16384) {
        snprintf(err, err_size, "sp_jpeg_enc_plan: size %dx%d (1..16384 each way)", width, height);
        return SP_JPEG_ESIZE;
    }
    if (subsampling != 444 && subsampling != 422 && subsampling != 420) {
        snprintf(err, err_size, "sp_jpeg_enc_plan: subsampling %d (444, 422 or 420)", subsampling);
        return SP_JPEG_ESAMPLING;
    }
    if (quality < 1 || quality > 100) {
        snprintf(err, err_size, "sp_jpeg_enc_plan: quality %d (1..100)", quality);
        return SP_EINVAL;
    }
    if (restart_interval < 0 || restart_interval > 65535) {
        snprintf(err, err_size, "sp_jpeg_enc_plan: restart interval %d (0..65535)", restart_interval);
        return SP_EINVAL;
    }
    sp_jpeg_enc_desc& d = *desc;
    memset(&d, 0, sizeof(d));
    d.width = width; d.height = height; d.subsampling = subsampling; d.quality = quality; d.restart_interval = restart_interval;
    d.h_samp = subsampling == 444 ? 1 : 2;
    d.v_samp = subsampling == 420 ? 2 : 1;
    d.mcus_x = (width + 8 * d.h_samp - 1) / (8 * d.h_samp);
    d.mcus_y = (height + 8 * d.v_samp - 1) / (8 * d.v_samp);
    for (int c = 0; c < 3; ++c) {
        const int cw = c ? (width + d.h_samp - 1) / d.h_samp : width, ch = c ? (height + d.v_samp - 1) / d.v_samp : height;
        d.wb[c] = (cw + 7) / 8;
        d.hb[c] = (ch + 7) / 8;
    }
    d.blocks_per_mcu = d.h_samp * d.v_samp + 2;
    const int mcus = d.mcus_x * d.mcus_y;                                  // <= 2048 * 2048
    d.blocks = mcus * d.blocks_per_mcu;                                    // <= 3 * 2^22
    d.segments = restart_interval ? (mcus + restart_interval - 1) / restart_interval : 1;

    // tables: (base * scale + 50) / 100 clamped to 1..255 (baseline)
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) {
            const int v = (sp_jpeg_enc_std_quant(t, k) * scale + 50) / 100;
            d.quant[t][k] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
    for (int t = 0; t < 4; ++t) sp_jpeg_enc_build_codes(t, d.hcode[t], d.hlen[t]);

    // header: SOI, APP0 (JFIF 1.01, no units, 1x1, no thumbnail), DQT x 2, SOF0, DHT x 4, [DRI], SOS
    uint8_t* h = d.header;
    int n = 0;
    auto put = [&](int v) { h[n++] = (uint8_t)v; };
    auto put16 = [&](int v) { put(v >> 8); put(v & 255); };
    const uint8_t app0[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (uint8_t v : app0) put(v);
    for (int t = 0; t < 2; ++t) {
        put(0xFF); put(0xDB); put16(67); put(t);
        for (int k = 0; k < 64; ++k) put(d.quant[t][k]);
    }
    put(0xFF); put(0xC0); put16(17); put(8); put16(height); put16(width); put(3);
    put(1); put(d.h_samp * 16 + d.v_samp); put(0);
    put(2); put(0x11); put(1);
    put(3); put(0x11); put(1);
    for (int t = 0; t < 4; ++t) {
        const int nv = sp_jpeg_enc_std_nvalues(t);
        put(0xFF); put(0xC4); put16(19 + nv); put(((t & 1) << 4) | (t >> 1));
        for (int l = 0; l < 16; ++l) put(sp_jpeg_enc_std_count(t, l));
        for (int i = 0; i < nv; ++i) put(sp_jpeg_enc_std_value(t, i));
    }
    if (restart_interval) { put(0xFF); put(0xDD); put16(4); put16(restart_interval); }
    const uint8_t sos[] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    for (uint8_t v : sos) put(v);
    d.header_bytes = n;                                                    // 623 / 629 <= SP_JPEG_ENC_HEADER_MAX

    // workspace: [totals | coefficients | bits | positions | segment starts | chunk sums]
    int64_t at = 64;
    d.ws_coef = at; at += (int64_t)d.blocks * 128;
    d.ws_bits = at; at += sp_jpeg_enc_round64((int64_t)d.blocks * 2);
    d.ws_pos = at; at += sp_jpeg_enc_round64(((int64_t)d.blocks + 1) * 8);
    d.ws_seg = at; at += sp_jpeg_enc_round64(((int64_t)d.segments + 1) * 8);
    const int64_t chunks = ((d.blocks > d.segments ? d.blocks : d.segments) + SP_JPEG_ENC_CHUNK - 1) / SP_JPEG_ENC_CHUNK;
    d.ws_chunk = at; at += sp_jpeg_enc_round64((chunks + 1) * 8);
    d.ws_bytes = at;
    return SP_OK;
}

// the stream part of an image's workspace (from ws_offset + ws_bytes): the third scan's chunk sums, then the unstuffed stream
SP_JPEG_HD int64_t sp_jpeg_enc_stream_chunk_bytes(int64_t cap) { return sp_jpeg_enc_round64((cap / (SP_JPEG_ENC_CHUNK * SP_JPEG_ENC_LANE_BYTES) + 2) * 8); }
SP_JPEG_HD int64_t sp_jpeg_enc_stream_bytes(int64_t cap) { return (cap + 127) / 64 * 64; }
// the most unstuffed bytes a file of `cap` bytes can hold
SP_JPEG_HD int64_t sp_jpeg_enc_stream_cap(const sp_jpeg_enc_desc& d, int64_t cap) {
    const int64_t v = cap - d.header_bytes - 2 - 2 * ((int64_t)d.segments - 1);
    return v > 0 ? v : 0;
}
