// sp_jpeg.h - the integer core of the baseline JPEG decoder: everything that touches untrusted bytes or defines a pixel value, as
// inline functions shared by the kernels of jpeg.hip (device), the host parser's table check and a stand-alone CPU program that runs
// them under the sanitizers (tests/jpeg_core_main.cpp).  Plain C++: no HIP header, SP_JPEG_HD is empty outside hipcc.
// The arithmetic is libjpeg's (jdhuff / jidctint "islow" / jdsample "fancy" / jdcolor), restated from its published description so that
// the pixels equal libjpeg-turbo's bit for bit.  Rules of this file:
//   - a reader never dereferences a byte at or past `end`; missing bits read as zeros and set a status bit;
//   - every table index is checked against the table's own count before the access;
//   - arithmetic that damaged data can push past 32 bits is done in uint32_t (wraps; valid streams never get there).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SP_JPEG_HD __host__ __device__ inline
#else
#define SP_JPEG_HD inline
#endif

// status bits of one image (sp_jpeg_decode_batch's `status`); 0 = decoded
#define SP_JPEG_ST_TRUNCATED 1   // a segment's entropy data ended (or hit a marker) before its last block
#define SP_JPEG_ST_BAD_CODE 2    // a bit pattern that is no Huffman code, or a DC category above 15
#define SP_JPEG_ST_BAD_RUN 4     // an AC run past coefficient 63
#define SP_JPEG_ST_SEGMENTS 8    // the number of restart segments is not ceil(MCUs / restart interval)
#define SP_JPEG_ST_BAD_TABLE 16  // a Huffman table whose counts are no prefix code

#define SP_JPEG_LOOKAHEAD 9

// natural (row-major) index of zigzag position k
SP_JPEG_HD int sp_jpeg_natural(int k) {
    const uint8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return z[k & 63];
}

// ---- bit reader over [p, end) with FF 00 unstuffing ---------------------------------------------------------------------------------------
struct sp_jpeg_bits {
    const uint8_t* p;
    const uint8_t* end;
    uint32_t acc;   // the low `n` bits are unread, most significant first
    int n;          // bits in acc (real + zero padding)
    int real;       // how many of them (the leading ones) came from the stream
    int status;
};

SP_JPEG_HD void sp_jpeg_bits_init(sp_jpeg_bits& b, const uint8_t* begin, const uint8_t* end) {
    b.p = begin; b.end = end < begin ? begin : end; b.acc = 0; b.n = 0; b.real = 0; b.status = 0;
}

// at least 25 bits in acc afterwards; a marker (FF followed by anything but 00) or the end of the data feeds zeros from there on
SP_JPEG_HD void sp_jpeg_bits_fill(sp_jpeg_bits& b) {
    while (b.n <= 24) {
        uint32_t byte = 0;
        if (b.p < b.end) {
            const uint32_t v = *b.p;
            if (v != 0xFF) { byte = v; b.p += 1; b.real += 8; }
            else if (b.end - b.p >= 2 && b.p[1] == 0) { byte = 0xFF; b.p += 2; b.real += 8; }
        }
        b.acc = (b.acc << 8) | byte;
        b.n += 8;
    }
}

SP_JPEG_HD uint32_t sp_jpeg_bits_peek(const sp_jpeg_bits& b, int k) {   // 1 <= k <= 16 <= n
    return (b.acc >> (b.n - k)) & ((1u << k) - 1u);
}

SP_JPEG_HD void sp_jpeg_bits_skip(sp_jpeg_bits& b, int k) {
    b.n -= k; b.real -= k;
    if (b.real < 0) { b.real = 0; b.status |= SP_JPEG_ST_TRUNCATED; }
}

SP_JPEG_HD int sp_jpeg_bits_get(sp_jpeg_bits& b, int k) {   // 0 <= k <= 16
    if (k == 0) return 0;
    sp_jpeg_bits_fill(b);
    const int v = (int)sp_jpeg_bits_peek(b, k);
    sp_jpeg_bits_skip(b, k);
    return v;
}

// ---- Huffman tables -------------------------------------------------------------------------------------------------------------------------
struct sp_jpeg_huff {
    int32_t maxcode[17];    // [l] largest code of length l (1..16), -1 when there is none
    int32_t valoff[17];     // [l] index of a length-l code c in `values` is valoff[l] + c
    int32_t nvalues;
    const uint8_t* values;  // nvalues symbols, in code order
    uint16_t lut[1 << SP_JPEG_LOOKAHEAD];   // by the next SP_JPEG_LOOKAHEAD bits: (length << 8) | symbol, 0 = longer than the lookahead
};

// counts[16] (codes of length 1..16) -> maxcode / valoff / nvalues; 0, or SP_JPEG_ST_BAD_TABLE when the counts are no prefix code or
// name more than `capacity` values (the table is then left empty: every decode reports a bad code).  The lut is filled separately.
SP_JPEG_HD int sp_jpeg_huff_build(sp_jpeg_huff& t, const uint8_t* counts, const uint8_t* values, int capacity) {
    int32_t code = 0, k = 0;
    bool ok = true;
    t.values = values;
    t.maxcode[0] = -1; t.valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int c = counts[l - 1];
        t.valoff[l] = k - code;
        k += c; code += c;
        t.maxcode[l] = c ? code - 1 : -1;
        if (code > (1 << l)) ok = false;
        code <<= 1;                                   // <= 2^17: code <= 2^l held so far, or ok is already false and code < 2^25
        if (!ok) code = 0;
    }
    if (k > capacity) ok = false;
    t.nvalues = ok ? k : 0;
    if (!ok) for (int l = 0; l <= 16; ++l) t.maxcode[l] = -1;
    return ok ? 0 : SP_JPEG_ST_BAD_TABLE;
}

// the lut entry of the SP_JPEG_LOOKAHEAD-bit pattern `bits`: the canonical search over the short lengths
SP_JPEG_HD uint16_t sp_jpeg_huff_lut_entry(const sp_jpeg_huff& t, uint32_t bits) {
    for (int l = 1; l <= SP_JPEG_LOOKAHEAD; ++l) {
        const int32_t code = (int32_t)(bits >> (SP_JPEG_LOOKAHEAD - l));
        if (code <= t.maxcode[l]) {
            const int32_t i = t.valoff[l] + code;
            if (i < 0 || i >= t.nvalues) return 0;
            return (uint16_t)((l << 8) | t.values[i]);
        }
    }
    return 0;
}

SP_JPEG_HD int sp_jpeg_huff_decode(const sp_jpeg_huff& t, sp_jpeg_bits& b) {
    sp_jpeg_bits_fill(b);
    const uint32_t e = t.lut[sp_jpeg_bits_peek(b, SP_JPEG_LOOKAHEAD)];
    if (e) { sp_jpeg_bits_skip(b, (int)(e >> 8)); return (int)(e & 0xFF); }
    const uint32_t v = sp_jpeg_bits_peek(b, 16);
    for (int l = SP_JPEG_LOOKAHEAD + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)(v >> (16 - l));
        if (code <= t.maxcode[l]) {
            const int32_t i = t.valoff[l] + code;
            if (i < 0 || i >= t.nvalues) break;
            sp_jpeg_bits_skip(b, l);
            return t.values[i];
        }
    }
    b.status |= SP_JPEG_ST_BAD_CODE;
    return 0;
}

SP_JPEG_HD int sp_jpeg_extend(int v, int s) { return (s && v < (1 << (s - 1))) ? v - (1 << s) + 1 : v; }

// One 8x8 block: DC difference added to `pred`, AC run/size pairs with ZRL and EOB.  Non-zero coefficients are written as int16 at
// out[natural index]; `out` points at 64 writable, zero-filled int16.  Stops at the first error (b.status != 0 on return).
SP_JPEG_HD void sp_jpeg_decode_block(sp_jpeg_bits& b, const sp_jpeg_huff& dc, const sp_jpeg_huff& ac, int32_t& pred, int16_t* out) {
    int s = sp_jpeg_huff_decode(dc, b);
    if (s > 15) { b.status |= SP_JPEG_ST_BAD_CODE; s = 0; }
    const int diff = sp_jpeg_extend(sp_jpeg_bits_get(b, s), s);
    pred = (int32_t)((uint32_t)pred + (uint32_t)diff);
    out[0] = (int16_t)(uint16_t)((uint32_t)pred & 0xFFFFu);
    for (int k = 1; k < 64 && !b.status;) {
        const int rs = sp_jpeg_huff_decode(ac, b);
        const int r = rs >> 4, sz = rs & 15;
        if (sz == 0) {
            if (r != 15) break;          // EOB
            k += 16;                     // ZRL
            continue;
        }
        k += r;
        if (k > 63) { b.status |= SP_JPEG_ST_BAD_RUN; break; }
        out[sp_jpeg_natural(k)] = (int16_t)sp_jpeg_extend(sp_jpeg_bits_get(b, sz), sz);
        k += 1;
    }
}

// ---- IDCT: jidctint "islow", CONST_BITS 13, PASS1_BITS 2 --------------------------------------------------------------------------------------
// One 8-point pass over in[0], in[stride], ...: out[i * ostride] = (value + half) >> shift.  uint32_t arithmetic (wraps like the
// two's-complement code it restates, without undefined behaviour on damaged coefficients); the final shift is arithmetic.
SP_JPEG_HD void sp_jpeg_idct_1d(const int32_t* in, int stride, int32_t* out, int ostride, int shift) {
    typedef uint32_t u;
    const u i0 = (u)in[0], i1 = (u)in[stride], i2 = (u)in[2 * stride], i3 = (u)in[3 * stride], i4 = (u)in[4 * stride], i5 = (u)in[5 * stride],
            i6 = (u)in[6 * stride], i7 = (u)in[7 * stride];
    u z1 = (i2 + i6) * 4433u;
    const u tmp2 = z1 + i6 * (u)-15137, tmp3 = z1 + i2 * 6270u;
    const u tmp0 = (i0 + i4) << 13, tmp1 = (i0 - i4) << 13;
    const u tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    u t0 = i7, t1 = i5, t2 = i3, t3 = i1;
    z1 = t0 + t3;
    u z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const u z5 = (z3 + z4) * 9633u;
    t0 *= 2446u; t1 *= 16819u; t2 *= 25172u; t3 *= 12299u;
    z1 *= (u)-7373; z2 *= (u)-20995; z3 = z3 * (u)-16069 + z5; z4 = z4 * (u)-3196 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    const u half = 1u << (shift - 1);
    out[0] = (int32_t)(tmp10 + t3 + half) >> shift;
    out[7 * ostride] = (int32_t)(tmp10 - t3 + half) >> shift;
    out[ostride] = (int32_t)(tmp11 + t2 + half) >> shift;
    out[6 * ostride] = (int32_t)(tmp11 - t2 + half) >> shift;
    out[2 * ostride] = (int32_t)(tmp12 + t1 + half) >> shift;
    out[5 * ostride] = (int32_t)(tmp12 - t1 + half) >> shift;
    out[3 * ostride] = (int32_t)(tmp13 + t0 + half) >> shift;
    out[4 * ostride] = (int32_t)(tmp13 - t0 + half) >> shift;
}

SP_JPEG_HD int32_t sp_jpeg_dequant(int16_t c, uint16_t q) { return (int32_t)((uint32_t)(int32_t)c * (uint32_t)q); }

SP_JPEG_HD uint8_t sp_jpeg_clamp(int32_t v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// column j of a block: coefficients coef[r * 8 + j] dequantised, pass 1 (descale 11) -> ws[r * ws_stride + j]
SP_JPEG_HD void sp_jpeg_idct_column(const int16_t* coef, const uint16_t* quant, int j, int32_t* ws, int ws_stride) {
    int32_t in[8];
    for (int r = 0; r < 8; ++r) in[r] = sp_jpeg_dequant(coef[r * 8 + j], quant[r * 8 + j]);
    sp_jpeg_idct_1d(in, 1, ws + j, ws_stride, 11);
}

// row r of the workspace: pass 2 (descale 18), + 128, clamp -> px[0..7]
SP_JPEG_HD void sp_jpeg_idct_row(const int32_t* ws_row, uint8_t* px) {
    int32_t o[8];
    sp_jpeg_idct_1d(ws_row, 1, o, 1, 18);
    for (int c = 0; c < 8; ++c) px[c] = sp_jpeg_clamp(o[c] + 128);
}

// ---- "fancy" chroma upsampling ----------------------------------------------------------------------------------------------------------------
// The downsampled plane is cw x ch samples (ceil(W / 2) wide, ceil(H / 2) high for h2v2) inside a plane with `pitch` bytes per row;
// indices are clamped to it, so neither MCU padding nor anything outside the plane is read.  libjpeg runs the filter only on planes
// wider than two samples and replicates otherwise.
SP_JPEG_HD int sp_jpeg_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// h2v1: output column x of downsampled row `row`
SP_JPEG_HD int sp_jpeg_up_h2v1(const uint8_t* row, int cw, int x) {
    const int c = sp_jpeg_clampi(x >> 1, 0, cw - 1);
    const int v = row[c];
    if (cw <= 2) return v;
    if (x & 1) return c == cw - 1 ? v : (3 * v + row[c + 1] + 2) >> 2;
    return c == 0 ? v : (3 * v + row[c - 1] + 1) >> 2;
}

// h2v2: output pixel (x, y)
SP_JPEG_HD int sp_jpeg_up_h2v2(const uint8_t* plane, int pitch, int cw, int ch, int x, int y) {
    const int c = sp_jpeg_clampi(x >> 1, 0, cw - 1), r = sp_jpeg_clampi(y >> 1, 0, ch - 1);
    const uint8_t* r0 = plane + (long long)r * pitch;
    if (cw <= 2) return r0[c];
    const uint8_t* r1 = plane + (long long)sp_jpeg_clampi((y & 1) ? r + 1 : r - 1, 0, ch - 1) * pitch;
    const int s = 3 * r0[c] + r1[c];
    if (x & 1) return c == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * r0[c + 1] + r1[c + 1] + 7) >> 4;
    return c == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * r0[c - 1] + r1[c - 1] + 8) >> 4;
}

// ---- YCbCr -> BGR, 16.16 fixed point (FIX(x) = int(x * 65536 + 0.5)) --------------------------------------------------------------------------
SP_JPEG_HD void sp_jpeg_ycc_to_bgr(int y, int cb, int cr, uint8_t* bgr) {
    cb -= 128; cr -= 128;
    bgr[0] = sp_jpeg_clamp(y + ((116130 * cb + 32768) >> 16));                 // FIX(1.772)
    bgr[1] = sp_jpeg_clamp(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));    // FIX(0.34414), FIX(0.71414)
    bgr[2] = sp_jpeg_clamp(y + ((91881 * cr + 32768) >> 16));                  // FIX(1.402)
}
