// sp_heat.h - the rules of the heat overlay (sp_heat_overlay_u8c3), ONE definition for the kernels in heat.hip, the CPU program
// tests/heat_core_main.cpp and, restated in numpy, tests/heat_ref.py.  Everything is integer arithmetic except three floating-point steps:
// the fp32 multiply of sp_heat_q, the fp64 inversion sp_invert_affine (sp_affine.h) and the fp64 multiply under the rint of the
// coefficients, so the device computes the host's bits.  Contraction is OFF for the whole file.  The rules are written out in
// include/simple_pose_hip.h above sp_heat_overlay_u8c3.
#pragma once
#include <math.h>
#include <stdint.h>

#include "simple_pose_hip.h"
#include "sp_affine.h"
#include "sp_render.h"

#pragma clang fp contract(off)

#define SP_HEAT_MAX_COORD 16383                  // the last pixel index of the largest image

// One person slot: the forward map in 1/65536 px and the pixels it can reach.  Empty: x0 = INT32_MAX > x1 = -1, so no tile ever lists it.
struct sp_heat_rec {
    int64_t c[6];
    int32_t x0, y0, x1, y1;          // inclusive, clipped to 0 .. SP_HEAT_MAX_COORD
};

SP_RENDER_HD sp_heat_rec sp_heat_empty() {
    sp_heat_rec r;
    for (int i = 0; i < 6; ++i) r.c[i] = 0;
    r.x0 = r.y0 = INT32_MAX;                    // (1, 0) would meet the tile at the origin
    r.x1 = r.y1 = -1;
    return r;
}

// the joints that take part: the mask's bits below `joints`
SP_RENDER_HD uint64_t sp_heat_joints(uint64_t joint_mask, int joints) { return joints >= 64 ? joint_mask : joint_mask & ((1ull << joints) - 1ull); }

// running maximum in which a NaN loses against every number (m starts as a NaN)
SP_RENDER_HD float sp_heat_max(float m, float v) { return (m != m || v > m) ? v : m; }

// m * scale (one fp32 multiply) -> 0 .. 255: NaN 0, >= 255 255, > 0 truncated, anything else 0
SP_RENDER_HD uint32_t sp_heat_q(float m, float scale) {
    const float v = m * scale;
    if (v != v) return 0u;
    if (v >= 255.0f) return 255u;
    if (v > 0.0f) return (uint32_t)(int32_t)v;
    return 0u;
}

// c[i] = rint(65536 F[i]), F the inverse of trans_inv; false: the person is skipped
SP_RENDER_HD bool sp_heat_forward(const float* trans_inv, int64_t* c) {
    double t[6], F[6];
    for (int i = 0; i < 6; ++i) t[i] = (double)trans_inv[i];
    sp_invert_affine(t, F);
    for (int i = 0; i < 6; ++i) {
        const double lim = (i == 2 || i == 5) ? 1048576.0 : 1024.0;
        if (!(fabs(F[i]) <= lim)) return false;                              // (a NaN or an infinity fails the comparison)
    }
    if (F[0] == 0.0 && F[1] == 0.0 && F[3] == 0.0 && F[4] == 0.0) return false;
    for (int i = 0; i < 6; ++i) c[i] = (int64_t)rint(F[i] * 65536.0);
    return true;
}

SP_RENDER_HD int64_t sp_heat_min64(int64_t a, int64_t b) { return a < b ? a : b; }
SP_RENDER_HD int64_t sp_heat_max64(int64_t a, int64_t b) { return a > b ? a : b; }

// Can a pixel of the rectangle X0 .. X1, Y0 .. Y1 (inclusive, non-empty) read a tap of the plane ?  Exact: U and V are affine, so their
// ranges over the rectangle are the ranges over its corners; a tap is read iff -1 <= xi <= hm_w - 1, that is -65536 <= U < 65536 hm_w.
SP_RENDER_HD bool sp_heat_reaches(const int64_t* c, int hm_h, int hm_w, int X0, int Y0, int X1, int Y1) {
    const int64_t ux0 = c[0] * X0, ux1 = c[0] * X1, uy0 = c[1] * Y0, uy1 = c[1] * Y1;
    const int64_t ulo = sp_heat_min64(ux0, ux1) + sp_heat_min64(uy0, uy1) + c[2], uhi = sp_heat_max64(ux0, ux1) + sp_heat_max64(uy0, uy1) + c[2];
    if (uhi < -65536 || ulo >= 65536 * (int64_t)hm_w) return false;
    const int64_t vx0 = c[3] * X0, vx1 = c[3] * X1, vy0 = c[4] * Y0, vy1 = c[4] * Y1;
    const int64_t vlo = sp_heat_min64(vx0, vx1) + sp_heat_min64(vy0, vy1) + c[5], vhi = sp_heat_max64(vx0, vx1) + sp_heat_max64(vy0, vy1) + c[5];
    return !(vhi < -65536 || vlo >= 65536 * (int64_t)hm_h);
}

SP_RENDER_HD int32_t sp_heat_clip(double v) { return v < 0.0 ? 0 : (v > (double)SP_HEAT_MAX_COORD ? SP_HEAT_MAX_COORD : (int32_t)v); }

// The box: a guess in floating point (the image of the plane's rectangle, one cell wider each way, under trans_inv, padded), then a
// proof in integers that nothing outside it reaches a tap; where the proof fails the box becomes everything.  An optimisation only.
SP_RENDER_HD void sp_heat_box(const float* trans_inv, const int64_t* c, int hm_h, int hm_w, sp_heat_rec& r) {
    const int M = SP_HEAT_MAX_COORD;
    double lox = 0, hix = 0, loy = 0, hiy = 0;
    bool finite = true;
    for (int k = 0; k < 4; ++k) {
        const double hx = (k & 1) ? (double)(hm_w + 1) : -2.0, hy = (k & 2) ? (double)(hm_h + 1) : -2.0;
        const double x = (double)trans_inv[0] * hx + (double)trans_inv[1] * hy + (double)trans_inv[2];
        const double y = (double)trans_inv[3] * hx + (double)trans_inv[4] * hy + (double)trans_inv[5];
        finite = finite && fabs(x) <= 1e300 && fabs(y) <= 1e300;
        lox = k == 0 || x < lox ? x : lox; hix = k == 0 || x > hix ? x : hix;
        loy = k == 0 || y < loy ? y : loy; hiy = k == 0 || y > hiy ? y : hiy;
    }
    r.x0 = r.y0 = 0;
    r.x1 = r.y1 = M;
    if (!finite) return;
    // wholly outside 0 .. M on an axis: the guess is empty, and the proof below runs on everything
    const bool none = hix + 3.0 < 0.0 || lox - 3.0 > (double)M || hiy + 3.0 < 0.0 || loy - 3.0 > (double)M;
    const int32_t x0 = sp_heat_clip(floor(lox) - 2.0), x1 = sp_heat_clip(ceil(hix) + 2.0);
    const int32_t y0 = sp_heat_clip(floor(loy) - 2.0), y1 = sp_heat_clip(ceil(hiy) + 2.0);
    if (none) {
        if (!sp_heat_reaches(c, hm_h, hm_w, 0, 0, M, M)) { r.x0 = r.y0 = INT32_MAX; r.x1 = r.y1 = -1; }
        return;
    }
    if (x0 > 0 && sp_heat_reaches(c, hm_h, hm_w, 0, 0, x0 - 1, M)) return;
    if (x1 < M && sp_heat_reaches(c, hm_h, hm_w, x1 + 1, 0, M, M)) return;
    if (y0 > 0 && sp_heat_reaches(c, hm_h, hm_w, x0, 0, x1, y0 - 1)) return;
    if (y1 < M && sp_heat_reaches(c, hm_h, hm_w, x0, y1 + 1, x1, M)) return;
    r.x0 = x0; r.y0 = y0; r.x1 = x1; r.y1 = y1;
}

// The row of person slot p of the image (pick position p: the order does not matter here), or -1: sp_render_kept_row, which clamps the
// count as sp_render_live(..) does and refuses rows outside the frame.
SP_RENDER_HD int sp_heat_row_at(const int32_t* keep, const int32_t* keep_count, const int32_t* seg, int image, int rows, int p) {
    int pick;
    return sp_render_kept_row(keep, keep_count, seg, image, rows, p, false, &pick);
}

// The record of a live slot (the caller found its row and a joint to draw); empty when the forward map is refused.
SP_RENDER_HD sp_heat_rec sp_heat_record(const float* trans_inv, int hm_h, int hm_w) {
    sp_heat_rec r = sp_heat_empty();
    int64_t c[6];
    if (!sp_heat_forward(trans_inv, c)) return r;
    for (int i = 0; i < 6; ++i) r.c[i] = c[i];
    sp_heat_box(trans_inv, c, hm_h, hm_w, r);
    if (r.x0 > r.x1)
        for (int i = 0; i < 6; ++i) r.c[i] = 0;
    return r;
}

// one cell of the plane: the quantised maximum over the joints of `mask` (not 0) at offset `at` of the person's maps, `plane` floats apart
SP_RENDER_HD uint32_t sp_heat_cell(const float* maps, size_t plane, size_t at, uint64_t mask, float scale) {
    float m = NAN;
    for (int j = 0; j < 64 && (mask >> j) != 0ull; ++j)
        if ((mask >> j) & 1ull) m = sp_heat_max(m, maps[(size_t)j * plane + at]);
    return sp_heat_q(m, scale);
}

SP_RENDER_HD uint32_t sp_heat_tap(const unsigned char* plane, int hm_h, int hm_w, int x, int y) {
    return (x >= 0 && x < hm_w && y >= 0 && y < hm_h) ? (uint32_t)plane[y * hm_w + x] : 0u;
}

// val of pixel (X, Y) from U, V in 1/65536 px
SP_RENDER_HD uint32_t sp_heat_sample(const unsigned char* plane, int hm_h, int hm_w, int64_t U, int64_t V) {
    const int64_t u = U >> 8, v = V >> 8;
    const int64_t xl = u >> 8, yl = v >> 8;
    if (xl < -1 || xl >= hm_w || yl < -1 || yl >= hm_h) return 0u;
    const int xi = (int)xl, yi = (int)yl;
    const uint32_t fx = (uint32_t)(u & 255), fy = (uint32_t)(v & 255);
    const uint32_t p00 = sp_heat_tap(plane, hm_h, hm_w, xi, yi), p10 = sp_heat_tap(plane, hm_h, hm_w, xi + 1, yi);
    const uint32_t p01 = sp_heat_tap(plane, hm_h, hm_w, xi, yi + 1), p11 = sp_heat_tap(plane, hm_h, hm_w, xi + 1, yi + 1);
    return ((256u - fx) * (256u - fy) * p00 + fx * (256u - fy) * p10 + (256u - fx) * fy * p01 + fx * fy * p11 + 32768u) >> 16;
}

// the blend weight of Vmax, 0 .. 4096; and one channel
SP_RENDER_HD uint32_t sp_heat_weight(const sp_heat_style& st, uint32_t vmax) {
    return (uint32_t)st.opacity16 * (st.alpha == SP_HEAT_ALPHA_CONSTANT ? 256u : vmax + (vmax >> 7));
}
SP_RENDER_HD uint32_t sp_heat_blend(uint32_t in, uint32_t colour, uint32_t w) { return (in * (4096u - w) + colour * w + 2048u) >> 12; }

// one pixel (bgr: 3 bytes) given Vmax; lut: 256 BGR triples.  true: the pixel changed hands (it may still hold the same bytes)
SP_RENDER_HD bool sp_heat_apply(const sp_heat_style& st, uint32_t vmax, const unsigned char* lut, unsigned char* bgr) {
    if (vmax < (uint32_t)st.threshold) return false;
    const uint32_t w = sp_heat_weight(st, vmax);
    for (int c = 0; c < 3; ++c) bgr[c] = (unsigned char)sp_heat_blend(bgr[c], lut[3 * vmax + c], w);
    return true;
}
