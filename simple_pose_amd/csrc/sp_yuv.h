// sp_yuv.h - YUV 4:2:0 (NV12 / I420) <-> packed BGR: the constant table, the two pixel functions and the 2-row x 16-column patch functions
// that the kernels of yuv.hip call, as inline functions shared with a stand-alone CPU program that runs them under the sanitizers
// (tests/yuv_core_main.cpp).  Plain C++: no HIP header, SP_YUV_HD is empty outside hipcc.
// The arithmetic is libjpeg's 16.16 fixed point (include/simple_pose_hip.h states it and the table); BT.601 full range is sp_jpeg.h's
// sp_jpeg_ycc_to_bgr and sp_jpeg_enc.h's sp_jpeg_enc_ycc bit for bit.  Rules of this file:
//   - a patch is rows 2i, 2i + 1 and columns [16k, 16k + 16) of one frame, clipped to the frame: whole 2x2 blocks, so the chroma of a
//     patch is read (or averaged) by the one thread that owns it;
//   - a byte is read or written only inside [row * pitch, row * pitch + row bytes) of its plane; offsets are size_t;
//   - 16- and 8-byte accesses happen only in a frame for which sp_yuv_wide holds (every base and pitch a multiple of 16), on a patch that
//     is full (16 columns, two rows); everything else goes byte by byte through the same pixel functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "simple_pose_hip.h"

#ifdef __HIPCC__
#define SP_YUV_HD __host__ __device__ inline
#else
#define SP_YUV_HD inline
#endif

#define SP_YUV_PATCH_W 16

struct sp_yuv_coef {
    int32_t yoff, ay, rv, bu, gu, gv;                 // YUV -> BGR
    int32_t yr, yg, yb, ur, ug, ub, vr, vg, vb;       // BGR -> YUV
};

// round(c * 65536) of the ITU definitions (Kr / Kb = 0.299 / 0.114 and 0.2126 / 0.0722; limited range: 219 / 255 luma, 224 / 255 chroma);
// BT.601 full range keeps libjpeg's table
SP_YUV_HD sp_yuv_coef sp_yuv_coefs(int matrix, int range) {
    const bool full = range == SP_YUV_FULL;
    if (matrix == SP_YUV_BT709)
        return full ? sp_yuv_coef{0, 65536, 103206, 121609, 12276, 30679, 13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005}
                    : sp_yuv_coef{16, 76309, 117489, 138438, 13975, 34925, 11966, 40254, 4064, -6596, -22189, 28784, 28784, -26145, -2639};
    return full ? sp_yuv_coef{0, 65536, 91881, 116130, 22554, 46802, 19595, 38470, 7471, -11059, -21709, 32768, 32768, -27439, -5329}
                : sp_yuv_coef{16, 76309, 104597, 132201, 25675, 53279, 16829, 33039, 6416, -9714, -19071, 28784, 28784, -24103, -4681};
}

SP_YUV_HD int sp_yuv_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
SP_YUV_HD int sp_yuv_min(int a, int b) { return a < b ? a : b; }

// ---- the two pixel functions -----------------------------------------------------------------------------------------------------------------
// the chroma terms of one (U, V) sample, shared by the (up to) four pixels under it; the rounding constant rides in them
struct sp_yuv_chroma { int32_t r, g, b; };
SP_YUV_HD sp_yuv_chroma sp_yuv_chroma_terms(const sp_yuv_coef& k, int u, int v) {
    const int uu = u - 128, vv = v - 128;
    return sp_yuv_chroma{k.rv * vv + 32768, -k.gu * uu - k.gv * vv + 32768, k.bu * uu + 32768};
}
// B | G << 8 | R << 16 of one pixel.  clamp8(x >> 16) is taken as clamp(x, 0, 0xFFFFFF) >> 16 - the same number, the floor shift being
// monotone - so that each channel is one clamp and one mask at its place in the word.  (Written as clamp8 of the shifted sums and OR-ed
// into a word, hipcc for gfx950 pairs the channels in v_ashr_pk_u8_i32 and reads its result as a zero-extended 32-bit value; on the
// MI355X the bytes above the pair then carried other bits and the 16-byte path wrote wrong R bytes.)
SP_YUV_HD uint32_t sp_yuv_clamp24(int v) { return (uint32_t)(v < 0 ? 0 : (v > 0xFFFFFF ? 0xFFFFFF : v)); }
SP_YUV_HD uint32_t sp_yuv_bgr24(const sp_yuv_coef& k, int y, const sp_yuv_chroma& c) {
    const int yk = k.ay * (y - k.yoff);
    return (sp_yuv_clamp24(yk + c.b) >> 16) | ((sp_yuv_clamp24(yk + c.g) >> 8) & 0xFF00u) | (sp_yuv_clamp24(yk + c.r) & 0xFF0000u);
}
SP_YUV_HD void sp_yuv_to_bgr_px(const sp_yuv_coef& k, int y, int u, int v, uint8_t* bgr) {
    const uint32_t p = sp_yuv_bgr24(k, y, sp_yuv_chroma_terms(k, u, v));
    bgr[0] = (uint8_t)p; bgr[1] = (uint8_t)(p >> 8); bgr[2] = (uint8_t)(p >> 16);
}
// comp 0 / 1 / 2: Y / U / V of one pixel, before the chroma average
SP_YUV_HD int sp_yuv_from_bgr_px(const sp_yuv_coef& k, int b, int g, int r, int comp) {
    if (comp == 0) return (k.yr * r + k.yg * g + k.yb * b + (k.yoff << 16) + 32768) >> 16;
    if (comp == 1) return (k.ur * r + k.ug * g + k.ub * b + (128 << 16) + 32767) >> 16;
    return (k.vr * r + k.vg * g + k.vb * b + (128 << 16) + 32767) >> 16;
}

// ---- what a frame must satisfy (the single-frame entry points refuse it on the host, the kernels skip it) ----------------------------------------
SP_YUV_HD int sp_yuv_chroma_row_bytes(int w, int format) { return format == SP_YUV_NV12 ? 2 * ((w + 1) / 2) : (w + 1) / 2; }

SP_YUV_HD bool sp_yuv_ref_ok(const sp_yuv_ref& f) {
    if (f.h < 1 || f.w < 1 || f.h > 32767 || f.w > 32767) return false;
    if (f.format != SP_YUV_NV12 && f.format != SP_YUV_I420) return false;
    if (f.matrix != SP_YUV_BT601 && f.matrix != SP_YUV_BT709) return false;
    if (f.range != SP_YUV_LIMITED && f.range != SP_YUV_FULL) return false;
    if (!f.y || !f.u || !f.bgr || (f.format == SP_YUV_I420 && !f.v)) return false;
    return f.pitch_y >= f.w && f.pitch_c >= sp_yuv_chroma_row_bytes(f.w, f.format) && f.pitch_bgr >= 3 * f.w;
}

// the 16-byte path: every base and every pitch a multiple of 16 (v is not looked at for NV12)
SP_YUV_HD bool sp_yuv_wide(const sp_yuv_ref& f) {
    uintptr_t m = (uintptr_t)f.y | (uintptr_t)f.u | (uintptr_t)f.bgr | (uintptr_t)(uint32_t)f.pitch_y | (uintptr_t)(uint32_t)f.pitch_c |
                  (uintptr_t)(uint32_t)f.pitch_bgr;
    if (f.format == SP_YUV_I420) m |= (uintptr_t)f.v;
    return (m & 15) == 0;
}

// patches of a frame: chroma rows x ceil(w / 16), column index fastest
SP_YUV_HD int sp_yuv_patch_cols(int w) { return (w + SP_YUV_PATCH_W - 1) / SP_YUV_PATCH_W; }
SP_YUV_HD long long sp_yuv_patches(int h, int w) { return (long long)((h + 1) / 2) * sp_yuv_patch_cols(w); }

// ---- aligned 16- and 8-byte accesses (the caller has established the alignment: sp_yuv_wide) -------------------------------------------------------
struct sp_yuv_w4 { uint32_t w[4]; };
struct sp_yuv_w2 { uint32_t w[2]; };
SP_YUV_HD sp_yuv_w4 sp_yuv_ld16(const uint8_t* p) { sp_yuv_w4 v; __builtin_memcpy(&v, __builtin_assume_aligned(p, 16), 16); return v; }
SP_YUV_HD sp_yuv_w2 sp_yuv_ld8(const uint8_t* p) { sp_yuv_w2 v; __builtin_memcpy(&v, __builtin_assume_aligned(p, 8), 8); return v; }
SP_YUV_HD void sp_yuv_st16(uint8_t* p, const sp_yuv_w4& v) { __builtin_memcpy(__builtin_assume_aligned(p, 16), &v, 16); }
SP_YUV_HD void sp_yuv_st8(uint8_t* p, const sp_yuv_w2& v) { __builtin_memcpy(__builtin_assume_aligned(p, 8), &v, 8); }
SP_YUV_HD int sp_yuv_byte(const uint32_t* w, int j) { return (int)((w[j >> 2] >> ((j & 3) * 8)) & 255u); }

// ---- YUV -> BGR ------------------------------------------------------------------------------------------------------------------------------------
// a full patch of a wide frame: 2 x 16 B of Y and 16 B of chroma in, 2 x 48 B of BGR out
SP_YUV_HD void sp_yuv_patch_to_bgr_wide(const sp_yuv_ref& f, const sp_yuv_coef& k, int br, int pc) {
    const size_t c0 = (size_t)pc * SP_YUV_PATCH_W, r0 = (size_t)br * 2;
    sp_yuv_chroma ct[8];
    if (f.format == SP_YUV_NV12) {
        const sp_yuv_w4 uv = sp_yuv_ld16(f.u + (size_t)br * (size_t)f.pitch_c + c0);
#pragma unroll
        for (int j = 0; j < 8; ++j) ct[j] = sp_yuv_chroma_terms(k, sp_yuv_byte(uv.w, 2 * j), sp_yuv_byte(uv.w, 2 * j + 1));
    } else {
        const sp_yuv_w2 u = sp_yuv_ld8(f.u + (size_t)br * (size_t)f.pitch_c + c0 / 2), v = sp_yuv_ld8(f.v + (size_t)br * (size_t)f.pitch_c + c0 / 2);
#pragma unroll
        for (int j = 0; j < 8; ++j) ct[j] = sp_yuv_chroma_terms(k, sp_yuv_byte(u.w, j), sp_yuv_byte(v.w, j));
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const sp_yuv_w4 y = sp_yuv_ld16(f.y + (r0 + a) * (size_t)f.pitch_y + c0);
        sp_yuv_w4 o[3] = {};
#pragma unroll
        for (int i = 0; i < 16; ++i) {                        // pixel i: bytes 3i .. 3i + 2 of the 48
            const uint32_t p = sp_yuv_bgr24(k, sp_yuv_byte(y.w, i), ct[i >> 1]);
            const int word = (3 * i) >> 2, shift = ((3 * i) & 3) * 8;
            o[word >> 2].w[word & 3] |= p << shift;
            if (shift > 8) o[(word + 1) >> 2].w[(word + 1) & 3] |= p >> (32 - shift);
        }
        uint8_t* d = f.bgr + (r0 + a) * (size_t)f.pitch_bgr + c0 * 3;
        sp_yuv_st16(d, o[0]); sp_yuv_st16(d + 16, o[1]); sp_yuv_st16(d + 32, o[2]);
    }
}

// any patch, byte by byte: the columns [16 pc, min(16 pc + 16, w)) of the rows 2 br and (inside the frame) 2 br + 1
SP_YUV_HD void sp_yuv_patch_to_bgr_narrow(const sp_yuv_ref& f, const sp_yuv_coef& k, int br, int pc) {
    const int c0 = pc * SP_YUV_PATCH_W, c1 = sp_yuv_min(c0 + SP_YUV_PATCH_W, f.w), rows = sp_yuv_min(2, f.h - 2 * br);
    for (int c = c0; c < c1; c += 2) {
        const int j = c >> 1;
        const uint8_t* up = f.format == SP_YUV_NV12 ? f.u + (size_t)br * (size_t)f.pitch_c + 2 * (size_t)j : f.u + (size_t)br * (size_t)f.pitch_c + (size_t)j;
        const int u = up[0], v = f.format == SP_YUV_NV12 ? up[1] : f.v[(size_t)br * (size_t)f.pitch_c + (size_t)j];
        const sp_yuv_chroma ct = sp_yuv_chroma_terms(k, u, v);
        for (int a = 0; a < rows; ++a) {
            const size_t r = (size_t)br * 2 + a;
            for (int b = 0; b < 2 && c + b < c1; ++b) {
                const uint32_t p = sp_yuv_bgr24(k, f.y[r * (size_t)f.pitch_y + (size_t)(c + b)], ct);
                uint8_t* d = f.bgr + r * (size_t)f.pitch_bgr + (size_t)(c + b) * 3;
                d[0] = (uint8_t)p; d[1] = (uint8_t)(p >> 8); d[2] = (uint8_t)(p >> 16);
            }
        }
    }
}

// patch `idx` of the frame (what one kernel thread does per step); `wide`: sp_yuv_wide(f), evaluated once per frame
SP_YUV_HD void sp_yuv_patch_to_bgr(const sp_yuv_ref& f, const sp_yuv_coef& k, bool wide, long long idx) {
    const int pw = sp_yuv_patch_cols(f.w), br = (int)(idx / pw), pc = (int)(idx - (long long)br * pw);
    if (wide && pc * SP_YUV_PATCH_W + SP_YUV_PATCH_W <= f.w && 2 * br + 1 < f.h) sp_yuv_patch_to_bgr_wide(f, k, br, pc);
    else sp_yuv_patch_to_bgr_narrow(f, k, br, pc);
}

// ---- BGR -> YUV ------------------------------------------------------------------------------------------------------------------------------------
// a full patch of a wide frame: 2 x 48 B of BGR in, 2 x 16 B of Y and 16 B of chroma out
SP_YUV_HD void sp_yuv_patch_from_bgr_wide(const sp_yuv_ref& f, const sp_yuv_coef& k, int br, int pc) {
    const size_t c0 = (size_t)pc * SP_YUV_PATCH_W, r0 = (size_t)br * 2;
    int us[8] = {}, vs[8] = {};
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const uint8_t* s = f.bgr + (r0 + a) * (size_t)f.pitch_bgr + c0 * 3;
        uint32_t in[12];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const sp_yuv_w4 t = sp_yuv_ld16(s + 16 * q);
            in[4 * q] = t.w[0]; in[4 * q + 1] = t.w[1]; in[4 * q + 2] = t.w[2]; in[4 * q + 3] = t.w[3];
        }
        sp_yuv_w4 yo = {};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int b = sp_yuv_byte(in, 3 * i), g = sp_yuv_byte(in, 3 * i + 1), r = sp_yuv_byte(in, 3 * i + 2);
            yo.w[i >> 2] |= (uint32_t)sp_yuv_from_bgr_px(k, b, g, r, 0) << ((i & 3) * 8);
            us[i >> 1] += sp_yuv_from_bgr_px(k, b, g, r, 1);
            vs[i >> 1] += sp_yuv_from_bgr_px(k, b, g, r, 2);
        }
        sp_yuv_st16(f.y + (r0 + a) * (size_t)f.pitch_y + c0, yo);
    }
    if (f.format == SP_YUV_NV12) {
        sp_yuv_w4 o = {};
#pragma unroll
        for (int j = 0; j < 8; ++j) o.w[j >> 1] |= ((uint32_t)((us[j] + 2) >> 2) | ((uint32_t)((vs[j] + 2) >> 2) << 8)) << ((j & 1) * 16);
        sp_yuv_st16(f.u + (size_t)br * (size_t)f.pitch_c + c0, o);
    } else {
        sp_yuv_w2 uo = {}, vo = {};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            uo.w[j >> 2] |= (uint32_t)((us[j] + 2) >> 2) << ((j & 3) * 8);
            vo.w[j >> 2] |= (uint32_t)((vs[j] + 2) >> 2) << ((j & 3) * 8);
        }
        sp_yuv_st8(f.u + (size_t)br * (size_t)f.pitch_c + c0 / 2, uo);
        sp_yuv_st8(f.v + (size_t)br * (size_t)f.pitch_c + c0 / 2, vo);
    }
}

// any patch, byte by byte; a 2x2 block that hangs over the frame's last row or column reads the clamped pixel again
SP_YUV_HD void sp_yuv_patch_from_bgr_narrow(const sp_yuv_ref& f, const sp_yuv_coef& k, int br, int pc) {
    const int c0 = pc * SP_YUV_PATCH_W, c1 = sp_yuv_min(c0 + SP_YUV_PATCH_W, f.w);
    for (int c = c0; c < c1; c += 2) {
        int us = 0, vs = 0;
        for (int a = 0; a < 2; ++a) {
            for (int b = 0; b < 2; ++b) {
                const int rr = sp_yuv_min(2 * br + a, f.h - 1), cc = sp_yuv_min(c + b, f.w - 1);
                const uint8_t* s = f.bgr + (size_t)rr * (size_t)f.pitch_bgr + (size_t)cc * 3;
                const int B = s[0], G = s[1], R = s[2];
                if (rr == 2 * br + a && cc == c + b) f.y[(size_t)rr * (size_t)f.pitch_y + (size_t)cc] = (uint8_t)sp_yuv_from_bgr_px(k, B, G, R, 0);
                us += sp_yuv_from_bgr_px(k, B, G, R, 1);
                vs += sp_yuv_from_bgr_px(k, B, G, R, 2);
            }
        }
        const size_t j = (size_t)(c >> 1), row = (size_t)br * (size_t)f.pitch_c;
        if (f.format == SP_YUV_NV12) {
            f.u[row + 2 * j] = (uint8_t)((us + 2) >> 2);
            f.u[row + 2 * j + 1] = (uint8_t)((vs + 2) >> 2);
        } else {
            f.u[row + j] = (uint8_t)((us + 2) >> 2);
            f.v[row + j] = (uint8_t)((vs + 2) >> 2);
        }
    }
}

SP_YUV_HD void sp_yuv_patch_from_bgr(const sp_yuv_ref& f, const sp_yuv_coef& k, bool wide, long long idx) {
    const int pw = sp_yuv_patch_cols(f.w), br = (int)(idx / pw), pc = (int)(idx - (long long)br * pw);
    if (wide && pc * SP_YUV_PATCH_W + SP_YUV_PATCH_W <= f.w && 2 * br + 1 < f.h) sp_yuv_patch_from_bgr_wide(f, k, br, pc);
    else sp_yuv_patch_from_bgr_narrow(f, k, br, pc);
}
