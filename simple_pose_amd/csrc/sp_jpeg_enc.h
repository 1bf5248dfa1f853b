// sp_jpeg_enc.h - the integer core of the baseline JPEG encoder: everything that defines a byte of the file, as inline functions shared
// by the kernels of jpeg_enc.hip (device), the host planner (sp_jpeg_enc_plan.h) and a stand-alone CPU program that runs the whole
// encode under the sanitizers (tests/jpeg_enc_core_main.cpp).  Plain C++: no HIP header, SP_JPEG_HD is empty outside hipcc.
// The arithmetic is libjpeg's default compressor (jccolor / jcsample without smoothing / jfdctint "islow" / jcdctmgr / jchuff with the
// Annex K tables), restated from its published description so that the file equals libjpeg-turbo's byte for byte.  Rules of this file:
//   - a source pixel is read at coordinates clamped into the image: edge replication is the clamp, nothing outside [0,W) x [0,H) is read;
//   - the bit writer ORs into 32-bit words below `nwords` only; what would land past them is dropped (the caller has refused the image
//     by then: SP_JPEG_ENC_STATUS_OVERFLOW);
//   - a block's place in the stream is a pure function of the descriptor and the per-block bit counts, so any lane can code any block.
#pragma once
#include <stdint.h>

#include "simple_pose_hip.h"
#include "sp_jpeg.h"

// ---- the Annex K tables, copied out of a file libjpeg-turbo wrote (tools/gen_golden_jpeg_enc.py stores the same bytes as std_quant /
// dht_counts / dht_values in tests/golden/g16_jpeg_enc.npz, and tests/test_jpeg_enc_host.py compares) -------------------------------------------
// unscaled quantisation table t (0 luma, 1 chroma) at zigzag position k
SP_JPEG_HD int sp_jpeg_enc_std_quant(int t, int k) {
    const uint8_t q[2][64] = {
        {16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18,  17,  16, 19, 24,  40,  26,  24,  22,  22, 24,  49, 35,  37,  29,  40, 58,  51, 61,  60, 57,  51,
         56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55,  56,  80, 109, 81,  87,  95,  98,  103, 104, 103, 62, 77,  113, 121, 112, 100, 120, 92,  101, 103, 99},
        {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
    return q[t & 1][k & 63];
}

// Huffman table t (0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma): the number of codes of length l + 1
SP_JPEG_HD int sp_jpeg_enc_std_count(int t, int l) {
    const uint8_t c[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                              {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                              {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                              {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
    return c[t & 3][l & 15];
}

SP_JPEG_HD int sp_jpeg_enc_std_nvalues(int t) { return (t & 1) ? 162 : 12; }

// ... and its i-th symbol in code order
SP_JPEG_HD int sp_jpeg_enc_std_value(int t, int i) {
    const uint8_t ac0[162] = {
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
        0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
        0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
        0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
        0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
        0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
        0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
    const uint8_t ac1[162] = {
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
        0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
        0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
        0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
        0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
        0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
        0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
    if (!(t & 1)) return i & 15;                     // both DC tables: the categories 0 .. 11 in order
    return (t & 2) ? ac1[i < 162 ? i : 0] : ac0[i < 162 ? i : 0];
}

// ---- colour: BGR -> YCbCr, 16.16 fixed point (FIX(x) = int(x * 65536 + 0.5)) -----------------------------------------------------------------
SP_JPEG_HD int sp_jpeg_enc_ycc(int b, int g, int r, int comp) {
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;                          // FIX(.299), FIX(.587), FIX(.114)
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;            // FIX(.16874), FIX(.33126), FIX(.5)
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;                           // FIX(.5), FIX(.41869), FIX(.08131)
}

// component `comp` of the source pixel (x, y), coordinates clamped into the image
SP_JPEG_HD int sp_jpeg_enc_px(const uint8_t* src, int W, int H, int x, int y, int comp) {
    x = sp_jpeg_clampi(x, 0, W - 1);
    y = sp_jpeg_clampi(y, 0, H - 1);
    const uint8_t* p = src + ((size_t)y * (size_t)W + (size_t)x) * 3;
    return sp_jpeg_enc_ycc(p[0], p[1], p[2], comp);
}

// sample (x, y) of component `comp`'s plane.  Chroma under 2x1 / 2x2 luma: the full-resolution plane is widened by repeating its last
// pixel and (2x2) lengthened to an even number of rows by repeating its last row, THEN averaged (bias 0,1 / 1,2 alternating by output
// column); the averaged plane of ceil(H / 2) rows is then lengthened by repeating ITS last row.
SP_JPEG_HD int sp_jpeg_enc_sample(const uint8_t* src, const sp_jpeg_enc_desc& d, int comp, int x, int y) {
    const int W = d.width, H = d.height;
    if (comp == 0 || d.h_samp == 1) return sp_jpeg_enc_px(src, W, H, x, y, comp);
    if (d.v_samp == 2) {
        y = sp_jpeg_clampi(y, 0, (H + 1) / 2 - 1);
        const int s = sp_jpeg_enc_px(src, W, H, 2 * x, 2 * y, comp) + sp_jpeg_enc_px(src, W, H, 2 * x + 1, 2 * y, comp) +
                      sp_jpeg_enc_px(src, W, H, 2 * x, 2 * y + 1, comp) + sp_jpeg_enc_px(src, W, H, 2 * x + 1, 2 * y + 1, comp);
        return (s + 1 + (x & 1)) >> 2;
    }
    return (sp_jpeg_enc_px(src, W, H, 2 * x, y, comp) + sp_jpeg_enc_px(src, W, H, 2 * x + 1, y, comp) + (x & 1)) >> 1;
}

// ---- geometry: block b of the scan (MCU after MCU; in an MCU the luma blocks row-major, then Cb, then Cr) -------------------------------------
struct sp_jpeg_enc_blk {
    int comp, bx, by;     // component and block coordinates in its plane
    int mcu, k;           // MCU and index within it
    bool real;            // false: a dummy block of the MCU grid beyond the component's ceil(samples / 8) blocks
};

SP_JPEG_HD sp_jpeg_enc_blk sp_jpeg_enc_locate(const sp_jpeg_enc_desc& d, int b) {
    sp_jpeg_enc_blk r;
    const int bpm = d.blocks_per_mcu, nl = bpm - 2;
    r.mcu = b / bpm;
    r.k = b - r.mcu * bpm;
    const int my = r.mcu / d.mcus_x, mx = r.mcu - my * d.mcus_x;
    if (r.k < nl) {
        const int vy = r.k / d.h_samp;
        r.comp = 0; r.bx = mx * d.h_samp + (r.k - vy * d.h_samp); r.by = my * d.v_samp + vy;
    } else {
        r.comp = r.k - nl + 1; r.bx = mx; r.by = my;
    }
    r.real = r.bx < d.wb[r.comp] && r.by < d.hb[r.comp];
    return r;
}

// first block of the restart segment block b lies in, and one past its last
SP_JPEG_HD void sp_jpeg_enc_segment(const sp_jpeg_enc_desc& d, int b, int& seg, int& first, int& end) {
    const int per = d.restart_interval > 0 ? d.restart_interval * d.blocks_per_mcu : d.blocks;        // <= 65535 * 6
    seg = b / per;
    first = seg * per;
    end = d.blocks - first > per ? first + per : d.blocks;
}

// ---- forward DCT: jfdctint "islow", CONST_BITS 13, PASS1_BITS 2; 8 points at p[0], p[stride], ... in place ---------------------------------
SP_JPEG_HD int32_t sp_jpeg_enc_descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }

SP_JPEG_HD void sp_jpeg_enc_fdct_1d(int32_t* p, int stride, bool first) {
    const int32_t d0 = p[0], d1 = p[stride], d2 = p[2 * stride], d3 = p[3 * stride], d4 = p[4 * stride], d5 = p[5 * stride], d6 = p[6 * stride],
                  d7 = p[7 * stride];
    const int32_t t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int n = first ? 11 : 15;
    p[0] = first ? (t10 + t11) * 4 : sp_jpeg_enc_descale(t10 + t11, 2);
    p[4 * stride] = first ? (t10 - t11) * 4 : sp_jpeg_enc_descale(t10 - t11, 2);
    int32_t z1 = (t12 + t13) * 4433;
    p[2 * stride] = sp_jpeg_enc_descale(z1 + t13 * 6270, n);
    p[6 * stride] = sp_jpeg_enc_descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int32_t z5 = (z3 + z4) * 9633;
    const int32_t a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    p[7 * stride] = sp_jpeg_enc_descale(a4 + z1 + z3, n);
    p[5 * stride] = sp_jpeg_enc_descale(a5 + z2 + z4, n);
    p[3 * stride] = sp_jpeg_enc_descale(a6 + z2 + z3, n);
    p[stride] = sp_jpeg_enc_descale(a7 + z1 + z4, n);
}

// coefficient c (8x the true DCT) by table value q: round half away from zero of c / (8 q)
SP_JPEG_HD int sp_jpeg_enc_quantise(int32_t c, int q) {
    const int32_t qv = 8 * q, m = ((c < 0 ? -c : c) + (qv >> 1)) / qv;
    return c < 0 ? -m : m;
}

// One block: samples - 128, rows then columns, quantise (d.quant: the scaled tables in zigzag order) -> zz[64] in zigzag order, DC
// absolute.  A dummy block is 64 zeros.
SP_JPEG_HD void sp_jpeg_enc_block(const uint8_t* src, const sp_jpeg_enc_desc& d, const sp_jpeg_enc_blk& k, int16_t* zz) {
    if (!k.real) {
        for (int i = 0; i < 64; ++i) zz[i] = 0;
        return;
    }
    int32_t ws[64];
    for (int y = 0; y < 8; ++y) {
        for (int x = 0; x < 8; ++x) ws[y * 8 + x] = sp_jpeg_enc_sample(src, d, k.comp, k.bx * 8 + x, k.by * 8 + y) - 128;
        sp_jpeg_enc_fdct_1d(ws + y * 8, 1, true);
    }
    for (int x = 0; x < 8; ++x) sp_jpeg_enc_fdct_1d(ws + x, 8, false);
    const uint16_t* q = d.quant[k.comp ? 1 : 0];
    for (int i = 0; i < 64; ++i) zz[i] = (int16_t)sp_jpeg_enc_quantise(ws[sp_jpeg_natural(i)], q[i]);
}

// ---- entropy coding ---------------------------------------------------------------------------------------------------------------------------
SP_JPEG_HD int sp_jpeg_enc_nbits(int v) {          // the category of v: bits of |v|
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// bits of a block's AC part: run/size symbols + value bits, ZRL for runs above 15, EOB unless coefficient 63 is non-zero
SP_JPEG_HD int sp_jpeg_enc_ac_bits(const int16_t* zz, const uint8_t* len) {
    int bits = 0, run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (!v) { ++run; continue; }
        bits += (run >> 4) * len[0xF0];
        const int s = sp_jpeg_enc_nbits(v);
        bits += len[((run & 15) << 4) | s] + s;
        run = 0;
    }
    return run ? bits + len[0] : bits;
}

// The DC a block's difference is taken against: the last CODED DC of its component in the segment (dummy blocks repeat it, so they are
// walked over; the first block of an MCU is never a dummy and chroma never has one), 0 at the start of a restart segment.
// coef: the image's coefficients, 64 per block in scan order.
SP_JPEG_HD int sp_jpeg_enc_dc_pred(const int16_t* coef, const sp_jpeg_enc_desc& d, int b, const sp_jpeg_enc_blk& k) {
    if (k.comp > 0 || k.k == 0) {
        if (k.mcu == 0 || (d.restart_interval > 0 && k.mcu % d.restart_interval == 0)) return 0;
        if (k.comp > 0) return coef[(size_t)(b - d.blocks_per_mcu) * 64];
    }
    int pb = k.k == 0 ? b - 3 : b - 1;               // the last luma block of the previous MCU, or the luma block before this one
    while (!sp_jpeg_enc_locate(d, pb).real) --pb;
    return coef[(size_t)pb * 64];
}

SP_JPEG_HD int sp_jpeg_enc_dc_diff(const int16_t* coef, const sp_jpeg_enc_desc& d, int b, const sp_jpeg_enc_blk& k) {
    return k.real ? coef[(size_t)b * 64] - sp_jpeg_enc_dc_pred(coef, d, b, k) : 0;
}

SP_JPEG_HD int sp_jpeg_enc_dc_bits(int diff, const uint8_t* len) {
    const int s = sp_jpeg_enc_nbits(diff);
    return len[s] + s;
}

// Bit writer into big-endian bit order over 32-bit words in memory order: stream bit i is bit 7 - (i & 7) of byte i >> 3.  Words are
// merged with `Or` (a plain |= on the host, an atomic OR on the device: neighbouring blocks share their first and last word), so the
// words have to be zero before the first writer.
struct sp_jpeg_enc_writer {
    uint32_t* words;
    uint64_t nwords;
    uint64_t word;      // index of the word the accumulator ends in
    uint64_t acc;       // the low `n` bits: the bits of that word so far (leading ones zero when the block starts inside the word)
    int n;
};

SP_JPEG_HD void sp_jpeg_enc_writer_init(sp_jpeg_enc_writer& w, uint32_t* words, uint64_t nwords, uint64_t bitpos) {
    w.words = words; w.nwords = nwords; w.word = bitpos >> 5; w.acc = 0; w.n = (int)(bitpos & 31);
}

template <class OrFn>
SP_JPEG_HD void sp_jpeg_enc_put(sp_jpeg_enc_writer& w, uint32_t code, int len, OrFn Or) {      // 0 <= len <= 16, code < 2^len
    w.acc = (w.acc << len) | code;
    w.n += len;
    if (w.n >= 32) {
        const uint32_t v = (uint32_t)(w.acc >> (w.n - 32));
        if (w.word < w.nwords && v) Or(w.words + w.word, __builtin_bswap32(v));
        w.word += 1;
        w.n -= 32;
        w.acc &= (1ull << w.n) - 1ull;
    }
}

template <class OrFn>
SP_JPEG_HD void sp_jpeg_enc_flush(sp_jpeg_enc_writer& w, OrFn Or) {
    if (w.n > 0) {
        const uint32_t v = (uint32_t)(w.acc << (32 - w.n));
        if (w.word < w.nwords && v) Or(w.words + w.word, __builtin_bswap32(v));
    }
}

// One block into the writer: DC category + value bits, the AC symbols.  `pad`: fill up to the next byte with 1-bits afterwards (the
// last block of a restart segment).  hcode / hlen: the DC and the AC table of the block's component.
template <class OrFn>
SP_JPEG_HD void sp_jpeg_enc_emit_block(sp_jpeg_enc_writer& w, const int16_t* zz, int diff, const uint16_t* dc_code, const uint8_t* dc_len,
                                       const uint16_t* ac_code, const uint8_t* ac_len, bool pad, OrFn Or) {
    int s = sp_jpeg_enc_nbits(diff);
    sp_jpeg_enc_put(w, dc_code[s], dc_len[s], Or);
    sp_jpeg_enc_put(w, (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u), s, Or);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (!v) { ++run; continue; }
        for (; run > 15; run -= 16) sp_jpeg_enc_put(w, ac_code[0xF0], ac_len[0xF0], Or);
        s = sp_jpeg_enc_nbits(v);
        const int sym = (run << 4) | s;
        sp_jpeg_enc_put(w, ac_code[sym], ac_len[sym], Or);
        sp_jpeg_enc_put(w, (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u), s, Or);
        run = 0;
    }
    if (run) sp_jpeg_enc_put(w, ac_code[0], ac_len[0], Or);
    if (pad) {
        const int p = (8 - (w.n & 7)) & 7;
        sp_jpeg_enc_put(w, (1u << p) - 1u, p, Or);
    }
    sp_jpeg_enc_flush(w, Or);
}

// ---- the file around the entropy data ---------------------------------------------------------------------------------------------------------
// One byte u of the unstuffed stream (segment s, `ff` bytes of value FF before it) goes to out[header + u + ff + 2 s], followed by a
// 00 when it is FF itself, by FF D0+(s&7) when it is the last byte of a segment that is not the last one, and by FF D9 when it is the
// last byte of all.  Returns 1 when the byte was FF.  `out`: the file's first byte; the caller has checked the final length.
SP_JPEG_HD int sp_jpeg_enc_place_byte(uint8_t* out, int header, uint64_t u, uint64_t ff, int s, int nseg, uint64_t seg_end, uint8_t byte) {
    uint8_t* o = out + (uint64_t)header + u + ff + 2ull * (uint64_t)s;
    *o++ = byte;
    const int isff = byte == 0xFF;
    if (isff) *o++ = 0;
    if (u + 1 == seg_end) {
        o[0] = 0xFF;
        o[1] = s + 1 < nseg ? (uint8_t)(0xD0 + (s & 7)) : (uint8_t)0xD9;
    }
    return isff;
}

// the file's length once the unstuffed stream has `ubytes` bytes, `ff` of them FF
SP_JPEG_HD uint64_t sp_jpeg_enc_file_bytes(const sp_jpeg_enc_desc& d, uint64_t ubytes, uint64_t ff) {
    return (uint64_t)d.header_bytes + ubytes + ff + 2ull * (uint64_t)(d.segments - 1) + 2ull;
}
