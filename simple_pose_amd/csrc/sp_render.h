// sp_render.h - the pixel rules of the pose overlay (sp_render_poses_u8c3), ONE definition for the kernels in render.hip, the CPU program
// tests/render_core_main.cpp and, restated in numpy, tests/render_ref.py.  Everything is integer arithmetic except one comparison of two
// fp64 products whose factors convert exactly, so the device computes the host's bits.  The rules are written out in
// include/simple_pose_hip.h above sp_render_poses_u8c3.
#pragma once
#include <math.h>
#include <stdint.h>

#include "simple_pose_hip.h"

#ifdef __HIPCC__
#define SP_RENDER_HD __host__ __device__ inline
#else
#define SP_RENDER_HD inline
#endif

#define SP_RENDER_BOX_SLOTS 4

// One capsule: every point within r of the segment A-B, in 1/16 px.  r = -1: an empty slot (x0 > x1, so no tile ever lists it).
struct sp_render_prim {
    int32_t ax, ay, bx, by, r;
    uint32_t colour;                 // B | G << 8 | R << 16
    int32_t x0, y0, x1, y1;          // the pixels that own a sample inside the capsule's bounding square (inclusive, not clipped to the image)
};

SP_RENDER_HD int sp_render_slots(const sp_render_style& st, int joints) { return SP_RENDER_BOX_SLOTS + st.edges + joints; }

SP_RENDER_HD int32_t sp_render_floor16(int32_t v) { return (v >= 0 ? v : v - 15) / 16; }

// q(v) = (int32) rint(v * 16.0), ties to even; false for a NaN, an infinity or |v| > 32768
SP_RENDER_HD bool sp_render_q(double v, int32_t& q) {
    if (!(fabs(v) <= 32768.0)) return false;
    q = (int32_t)rint(v * 16.0);
    return true;
}

SP_RENDER_HD sp_render_prim sp_render_empty() {
    sp_render_prim p;
    p.ax = p.ay = p.bx = p.by = 0;
    p.r = -1;
    p.colour = 0;
    p.x0 = p.y0 = 1;
    p.x1 = p.y1 = 0;
    return p;
}

SP_RENDER_HD sp_render_prim sp_render_capsule(double ax, double ay, double bx, double by, int32_t r, uint32_t colour) {
    sp_render_prim p = sp_render_empty();
    int32_t qax, qay, qbx, qby;
    if (!(sp_render_q(ax, qax) && sp_render_q(ay, qay) && sp_render_q(bx, qbx) && sp_render_q(by, qby))) return p;
    p.ax = qax; p.ay = qay; p.bx = qbx; p.by = qby;
    p.r = r;
    p.colour = colour;
    // pixel x owns the samples 16x + 2 .. 16x + 14: it can be touched iff 16x + 14 >= lo and 16x + 2 <= hi
    p.x0 = sp_render_floor16((qax < qbx ? qax : qbx) - r + 1);
    p.x1 = sp_render_floor16((qax > qbx ? qax : qbx) + r - 2);
    p.y0 = sp_render_floor16((qay < qby ? qay : qby) - r + 1);
    p.y1 = sp_render_floor16((qay > qby ? qay : qby) + r - 2);
    return p;
}

// entry i (cyclic) of a style's palette of n BGR triples, as B | G << 8 | R << 16
SP_RENDER_HD uint32_t sp_render_palette(const unsigned char (*palette)[3], int n, int i) {
    const unsigned char* c = palette[i % n];
    return (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16;
}

// Slot `slot` of one kept person: 4 box edges (top, right, bottom, left), the limbs in skeleton order, the joints in index order.
// kps: the person's [joints, 3] (x, y, c); box: its (x1, y1, x2, y2, ..); pick: its position in the pick order; track_id: 0 when there is none.
SP_RENDER_HD sp_render_prim sp_render_person_prim(const sp_render_style& st, int joints, int slot, const double* kps, const float* box, int pick,
                                                  int track_id) {
    const uint32_t person = sp_render_palette(st.palette, st.palette_n, track_id > 0 ? (track_id - 1) % st.palette_n : pick % st.palette_n);
    const bool by_part = st.colour_by == SP_RENDER_COLOUR_PART;
    if (slot < SP_RENDER_BOX_SLOTS) {
        if (st.box_r == 0) return sp_render_empty();
        const double x1 = (double)box[0], y1 = (double)box[1], x2 = (double)box[2], y2 = (double)box[3];
        switch (slot) {
            case 0: return sp_render_capsule(x1, y1, x2, y1, st.box_r, person);
            case 1: return sp_render_capsule(x2, y1, x2, y2, st.box_r, person);
            case 2: return sp_render_capsule(x2, y2, x1, y2, st.box_r, person);
            default: return sp_render_capsule(x1, y2, x1, y1, st.box_r, person);
        }
    }
    slot -= SP_RENDER_BOX_SLOTS;
    if (slot < st.edges) {
        const double* a = kps + 3 * st.edge[slot][0];
        const double* b = kps + 3 * st.edge[slot][1];
        if (!(a[2] > st.in_vis_thre && b[2] > st.in_vis_thre)) return sp_render_empty();      // (a NaN c is not visible)
        return sp_render_capsule(a[0], a[1], b[0], b[1], st.limb_r, by_part ? sp_render_palette(st.palette, st.palette_n, slot) : person);
    }
    slot -= st.edges;
    const double* a = kps + 3 * slot;
    if (!(a[2] > st.in_vis_thre)) return sp_render_empty();
    return sp_render_capsule(a[0], a[1], a[0], a[1], st.joint_r, by_part ? sp_render_palette(st.palette, st.palette_n, slot) : person);
}

// the image's kept persons: n (clamped to the rows and to the keep list's end, as track.hip's frame_poses) and the offset of its keep list
SP_RENDER_HD int sp_render_live(const int32_t* keep_count, const int32_t* seg, int image, int rows, int& lo) {
    lo = seg[image];
    if (lo < 0 || lo > rows) { lo = 0; return 0; }
    int n = keep_count[image];
    n = n < 0 ? 0 : n;
    n = n > rows ? rows : n;
    return n > rows - lo ? rows - lo : n;
}

// The row of person slot `slot` of the image, or -1: slots >= n (the clamped count) and rows outside the frame are dead.  `pick`: the
// slot's position in the pick order, counted from the list's start or (from_end) from its end, n - 1 - slot.
SP_RENDER_HD int sp_render_kept_row(const int32_t* keep, const int32_t* keep_count, const int32_t* seg, int image, int rows, int slot,
                                    bool from_end, int* pick) {
    int lo;
    const int n = sp_render_live(keep_count, seg, image, rows, lo);
    if (slot >= n) return -1;
    *pick = from_end ? n - 1 - slot : slot;
    const int row = keep[lo + *pick];
    return (row < 0 || row >= rows) ? -1 : row;
}

// Primitive `index` = p * slots + slot of the image.  Person slot p < n holds the pose at pick position n - 1 - p: applying the primitives
// by ascending index paints the persons in reverse pick order, the best pose last.  Person slots >= n (and rows outside the frame) are empty.
SP_RENDER_HD sp_render_prim sp_render_prim_at(const sp_render_style& st, int joints, int rows, int image, const double* kps, const float* box,
                                              const int32_t* track_id, const int32_t* keep, const int32_t* keep_count, const int32_t* seg,
                                              int index) {
    const int per = sp_render_slots(st, joints);
    const int p = index / per, slot = index - p * per;
    int pick;
    const int row = sp_render_kept_row(keep, keep_count, seg, image, rows, p, true, &pick);
    if (row < 0) return sp_render_empty();
    return sp_render_person_prim(st, joints, slot, kps + (size_t)row * joints * 3, box + (size_t)row * 5, pick, track_id ? track_id[row] : 0);
}

// k = how many of the pixel's 16 samples S = (16x + 4i + 2, 16y + 4j + 2) lie inside the capsule.  int64 throughout; the one fp64
// comparison has two products, each rounded once, of factors that convert exactly (|c| < 2^42, r^2 <= 2^20, L < 2^42).
SP_RENDER_HD int sp_render_coverage(const sp_render_prim& p, int x, int y) {
    const int32_t abx = p.bx - p.ax, aby = p.by - p.ay;
    const int64_t L = (int64_t)abx * abx + (int64_t)aby * aby;
    const int64_t r2 = (int64_t)p.r * p.r;
    const double rhs = (double)r2 * (double)L;
    int k = 0;
    for (int j = 0; j < 4; ++j) {
        const int32_t sy = 16 * y + 4 * j + 2, asy = sy - p.ay;
        for (int i = 0; i < 4; ++i) {
            const int32_t sx = 16 * x + 4 * i + 2, asx = sx - p.ax;
            const int64_t t = (int64_t)asx * abx + (int64_t)asy * aby;
            bool in;
            if (L == 0 || t <= 0) {
                in = (int64_t)asx * asx + (int64_t)asy * asy <= r2;
            } else if (t >= L) {
                const int32_t bsx = sx - p.bx, bsy = sy - p.by;
                in = (int64_t)bsx * bsx + (int64_t)bsy * bsy <= r2;
            } else {
                const int64_t c = (int64_t)asx * aby - (int64_t)asy * abx;
                const double cd = (double)c;
                in = cd * cd <= rhs;
            }
            k += in ? 1 : 0;
        }
    }
    return k;
}

// one channel: a = k * opacity in 0 .. 256; a = 0 returns `in`, a = 256 returns `colour`
SP_RENDER_HD uint32_t sp_render_blend(uint32_t in, uint32_t colour, int a) { return (in * (uint32_t)(256 - a) + colour * (uint32_t)a + 128u) >> 8; }

SP_RENDER_HD bool sp_render_touches(const sp_render_prim& p, int x, int y) { return x >= p.x0 && x <= p.x1 && y >= p.y0 && y <= p.y1; }

// one primitive onto one pixel (bgr: 3 bytes).  A pixel outside the bounding box has k = 0 and keeps its bytes.
SP_RENDER_HD void sp_render_apply(const sp_render_prim& p, int opacity, int x, int y, unsigned char* bgr) {
    if (!sp_render_touches(p, x, y)) return;
    const int a = sp_render_coverage(p, x, y) * opacity;
    if (a == 0) return;
    for (int c = 0; c < 3; ++c) bgr[c] = (unsigned char)sp_render_blend(bgr[c], (p.colour >> (8 * c)) & 255u, a);
}
