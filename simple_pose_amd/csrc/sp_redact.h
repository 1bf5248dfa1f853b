// sp_redact.h - the rules of the redaction (sp_redact_u8c3), ONE definition for the kernels in redact.hip, the CPU program
// tests/redact_core_main.cpp and, restated in numpy, tests/redact_ref.py.  Everything is integer arithmetic except the overlay's
// quantisation sp_render_q, so the device computes the host's bits.  The rules are written out in include/simple_pose_hip.h above
// sp_redact_u8c3.
#pragma once
#include <stdint.h>

#include "simple_pose_hip.h"
#include "sp_render.h"

#define SP_REDACT_EMPTY 0
#define SP_REDACT_DISC 1
#define SP_REDACT_RECT 2

// One region in 1/16 px.  Disc: (a, b) the centre, c the radius.  Rectangle: (a, b) .. (c, d), a <= c and b <= d.  Empty: x0 > x1, so no
// tile ever looks at it.
struct sp_redact_rec {
    int32_t kind;
    int32_t a, b, c, d;
    int32_t x0, y0, x1, y1;          // the pixels whose closed square meets the region's bounding box (inclusive, not clipped to the image)
};

SP_RENDER_HD int32_t sp_redact_min(int32_t a, int32_t b) { return a < b ? a : b; }
SP_RENDER_HD int32_t sp_redact_max(int32_t a, int32_t b) { return a > b ? a : b; }

SP_RENDER_HD bool sp_redact_cell_ok(int cell) { return cell == 4 || cell == 8 || cell == 16 || cell == 32 || cell == 64; }

SP_RENDER_HD sp_redact_rec sp_redact_empty() {
    sp_redact_rec r;
    r.kind = SP_REDACT_EMPTY;
    r.a = r.b = r.c = r.d = 0;
    r.x0 = r.y0 = 1;
    r.x1 = r.y1 = 0;
    return r;
}

SP_RENDER_HD sp_redact_rec sp_redact_rect(int32_t ax, int32_t ay, int32_t bx, int32_t by) {
    sp_redact_rec r;
    r.kind = SP_REDACT_RECT;
    r.a = ax; r.b = ay; r.c = bx; r.d = by;
    r.x0 = sp_render_floor16(ax); r.y0 = sp_render_floor16(ay);
    r.x1 = sp_render_floor16(bx); r.y1 = sp_render_floor16(by);
    return r;
}

SP_RENDER_HD sp_redact_rec sp_redact_disc(int32_t cx, int32_t cy, int32_t rad) {
    sp_redact_rec r;
    r.kind = SP_REDACT_DISC;
    r.a = cx; r.b = cy; r.c = rad; r.d = 0;
    r.x0 = sp_render_floor16(cx - rad); r.y0 = sp_render_floor16(cy - rad);
    r.x1 = sp_render_floor16(cx + rad); r.y1 = sp_render_floor16(cy + rad);
    return r;
}

// the quantised box with both axes ordered by min / max; false when q rejects one of the four
SP_RENDER_HD bool sp_redact_box(const float* box, int32_t& x1, int32_t& y1, int32_t& x2, int32_t& y2) {
    int32_t a, b, c, d;
    if (!(sp_render_q((double)box[0], a) && sp_render_q((double)box[1], b) && sp_render_q((double)box[2], c) && sp_render_q((double)box[3], d)))
        return false;
    x1 = sp_redact_min(a, c); x2 = sp_redact_max(a, c);
    y1 = sp_redact_min(b, d); y2 = sp_redact_max(b, d);
    return true;
}

// The region of one kept person.  kps: the person's [joints, 3] (x, y, c); box: its (x1, y1, x2, y2, ..).
SP_RENDER_HD sp_redact_rec sp_redact_person_region(const sp_redact_style& st, const double* kps, const float* box) {
    int32_t x1 = 0, y1 = 0, x2 = 0, y2 = 0;
    const bool has_box = sp_redact_box(box, x1, y1, x2, y2);
    if (st.region == SP_REDACT_PERSON) return has_box ? sp_redact_rect(x1, y1, x2, y2) : sp_redact_empty();
    bool any = false;
    int32_t minx = 0, maxx = 0, miny = 0, maxy = 0;
    for (int i = 0; i < st.head_joints; ++i) {
        const double* k = kps + 3 * st.head_joint[i];
        int32_t qx, qy;
        if (!(k[2] > st.in_vis_thre) || !sp_render_q(k[0], qx) || !sp_render_q(k[1], qy)) continue;      // (a NaN c is not visible)
        minx = any ? sp_redact_min(minx, qx) : qx; maxx = any ? sp_redact_max(maxx, qx) : qx;
        miny = any ? sp_redact_min(miny, qy) : qy; maxy = any ? sp_redact_max(maxy, qy) : qy;
        any = true;
    }
    if (any) {
        const int32_t e = sp_redact_max(maxx - minx, maxy - miny);                                        // <= 2^20
        const int32_t s = has_box ? sp_redact_max(x2 - x1, y2 - y1) : 0;                                  // <= 2^20
        const int32_t r0 = sp_redact_max(e >> 1, (int32_t)(((int64_t)s * st.head_min) >> 8));
        const int64_t r = ((int64_t)r0 * st.expand) >> 4;
        return sp_redact_disc((minx + maxx) >> 1, (miny + maxy) >> 1, (int32_t)(r < SP_REDACT_MAX_RADIUS ? r : SP_REDACT_MAX_RADIUS));
    }
    if (st.fallback == SP_REDACT_FALLBACK_NONE || !has_box) return sp_redact_empty();
    if (st.fallback == SP_REDACT_FALLBACK_BOX) return sp_redact_rect(x1, y1, x2, y2);
    return sp_redact_rect(x1, y1, x2, y1 + (int32_t)(((int64_t)(y2 - y1) * st.top_frac) >> 8));
}

// Record p of the image: person slot p < n holds the pose at pick position p (the order does not matter here); slots >= n, and rows
// outside the frame, are empty.
SP_RENDER_HD sp_redact_rec sp_redact_region_at(const sp_redact_style& st, int joints, int rows, int image, const double* kps, const float* box,
                                               const int32_t* keep, const int32_t* keep_count, const int32_t* seg, int p) {
    int pick;                                    // (sp_render_kept_row: the count as sp_render_live(..) clamps it, and the row check)
    const int row = sp_render_kept_row(keep, keep_count, seg, image, rows, p, false, &pick);
    if (row < 0) return sp_redact_empty();
    return sp_redact_person_region(st, kps + (size_t)row * joints * 3, box + (size_t)row * 5);
}

// does the region meet the closed rectangle [16 X0, 16 X1 + 15] x [16 Y0, 16 Y1 + 15] of the pixels X0 .. X1, Y0 .. Y1 ?
SP_RENDER_HD bool sp_redact_hits(const sp_redact_rec& r, int X0, int Y0, int X1, int Y1) {
    const int32_t lx = 16 * X0, hx = 16 * X1 + 15, ly = 16 * Y0, hy = 16 * Y1 + 15;
    if (r.kind == SP_REDACT_RECT) return r.a <= hx && r.c >= lx && r.b <= hy && r.d >= ly;
    if (r.kind != SP_REDACT_DISC) return false;
    const int64_t dx = sp_redact_max(sp_redact_max(lx - r.a, 0), r.a - hx), dy = sp_redact_max(sp_redact_max(ly - r.b, 0), r.b - hy);
    return dx * dx + dy * dy <= (int64_t)r.c * r.c;
}

// one channel of a mosaic cell: the rounded mean of its n source pixels
SP_RENDER_HD uint32_t sp_redact_mean(uint32_t sum, uint32_t n) { return (sum + n / 2) / n; }
