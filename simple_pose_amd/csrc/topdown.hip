// topdown.hip - detections -> crop geometry on the device (sp_topdown_plan): the step between the detector's NMS and the person warp of
// the top-down path.  Replaces the host loop of datasets/naive_data.py crop_boxes (box_to_center_scale + two get_affine_transform per
// person, commons/joint_utils.py) and the device -> host copy of the boxes that loop needs, so that detector, crops, pose network,
// decode and OKS-NMS can run back to back on one stream (and be captured as one graph).
// Arithmetic: the host functions' own, operation by operation - float32 box arithmetic, float32-rounded triangles, the float64 Cramer
// solve in _solve_affine's order, cv::warpAffine's inversion (sp_invert_affine, shared with warp.hip), float32 rounding of trans_inv.  Contraction is
// OFF for the whole file: every value has the bits the host computes.  rot is always 0 on this path (sin = 0, cos = 1 are exact).
#include "sp_common.h"

#include <stdint.h>

#pragma clang fp contract(off)

namespace {

constexpr int PLAN_NT = 256;
constexpr int PLAN_MAX_CAPACITY = SP_MAX_ROWS;   // the OKS-NMS group limit (nms.hip NMS_MAX_GROUP)

struct PlanGeom {
    float ar;                                    // in_w / in_h as the float32 a weak Python float becomes next to a float32 operand
    double dst_in[6], dst_hm[6];                 // the destination triangles of the input crop and of the heat map (float32 values)
};

struct PlanOut {
    int* seg;
    int* src_index;
    double* m_inv;
    float* trans_inv;
    float* center;
    float* scale;
    double* area;
    double* box_score;
    float* box;
    int* dropped;
};

// _solve_affine (commons/joint_utils.py): the 2x3 map taking the points p[i] to q[i]; Cramer's rule in this operation order
__device__ __forceinline__ void solve_affine(const double (&p)[6], const double (&q)[6], double (&out)[6]) {
    const double x0 = p[0], y0 = p[1], x1 = p[2], y1 = p[3], x2 = p[4], y2 = p[5];
    const double det = x0 * (y1 - y2) - y0 * (x1 - x2) + (x1 * y2 - x2 * y1);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double u0 = q[k], u1 = q[2 + k], u2 = q[4 + k];
        out[k * 3 + 0] = (u0 * (y1 - y2) - y0 * (u1 - u2) + (u1 * y2 - u2 * y1)) / det;
        out[k * 3 + 1] = (x0 * (u1 - u2) - u0 * (x1 - x2) + (x1 * u2 - x2 * u1)) / det;
        out[k * 3 + 2] = (x0 * (y1 * u2 - y2 * u1) - y0 * (x1 * u2 - x2 * u1) + u0 * (x1 * y2 - x2 * y1)) / det;
    }
}

// BasicTransform.__call__ for one float32 box: box_to_center_scale, then get_affine_transform(center, scale, 0, size) for both sizes
__device__ void plan_slot(const float* __restrict__ d, int slot, int image, const PlanGeom& g, const PlanOut& o) {
    const float bx1 = d[0], by1 = d[1], bx2 = d[2], by2 = d[3];
    float w = bx2 - bx1, h = by2 - by1;
    const float cx = bx1 + w * 0.5f, cy = by1 + h * 0.5f;
    if (w > g.ar * h) h = w / g.ar;
    else if (w < g.ar * h) w = h * g.ar;
    float sw = w, sh = h;
    if (cx != -1.f) { sw = w * 1.25f; sh = h * 1.25f; }          // scale * scale_mult unless the centre's x is the sentinel -1
    // get_affine_transform, rot = 0: sn = 0.0, cs = 1.0 (float64); half float32; up float64; offset = scale * (0, 0) float32
    const float half = sw * -0.5f;
    const float offx = sw * 0.f, offy = sh * 0.f;
    const double up0 = 0.0 - (double)half * 0.0, up1 = 0.0 + (double)half * 1.0;
    const float p0x = cx + offx, p0y = cy + offy;
    const float p1x = (float)(((double)cx + up0) + (double)offx), p1y = (float)(((double)cy + up1) + (double)offy);
    const float dx = p0x - p1x, dy = p0y - p1y;
    const float p2x = p1x + (-dy), p2y = p1y + dx;
    const double src[6] = {(double)p0x, (double)p0y, (double)p1x, (double)p1y, (double)p2x, (double)p2y};
    double fwd[6], tinv[6];
    solve_affine(src, g.dst_in, fwd);
    sp_invert_affine(fwd, o.m_inv + (size_t)slot * 6);          // the one the host warps use (sp_common.h)
    solve_affine(g.dst_hm, src, tinv);
#pragma unroll
    for (int i = 0; i < 6; ++i) o.trans_inv[(size_t)slot * 6 + i] = (float)tinv[i];
    o.center[slot * 2] = cx; o.center[slot * 2 + 1] = cy;
    o.scale[slot * 2] = sw; o.scale[slot * 2 + 1] = sh;
    o.area[slot] = (double)(sw * sh);
    o.box_score[slot] = (double)d[4];
    float* bo = o.box + (size_t)slot * 5;
    bo[0] = bx1; bo[1] = by1; bo[2] = bx2; bo[3] = by2; bo[4] = d[4];
    o.src_index[slot] = image;
}

// One workgroup walks the batch image by image; a block scan over the selection flags gives every selected row its slot in (image, row)
// order.  B * max_det rows at most (a few thousand): the kernel is launch latency, not work.
__global__ __launch_bounds__(PLAN_NT) void topdown_plan_kernel(const float* __restrict__ det, const int* __restrict__ counts, int B, int max_det,
                                                               int keep_cls, float min_score, int cap, const PlanGeom g, const PlanOut o) {
    __shared__ int lds[4];
    const int tid = threadIdx.x;
    int base = 0;                                  // selected rows so far (uniform over the block); slots are min(base, cap)
    for (int b = 0; b < B; ++b) {
        const int before = base;
        int n = counts[b];
        n = n < 0 ? 0 : (n > max_det ? max_det : n);
        for (int r0 = 0; r0 < n; r0 += PLAN_NT) {
            const int r = r0 + tid;
            const float* d = det + ((size_t)b * max_det + (r < n ? r : 0)) * 6;
            const int sel = r < n && (keep_cls < 0 || d[5] == (float)keep_cls) && d[4] >= min_score;
            int total;
            const int k = base + sp_block_scan256(sel, lds, total);
            if (sel && k < cap) plan_slot(d, k, b, g, o);
            base += total;
        }
        if (tid == 0) {
            const int lo = before < cap ? before : cap, hi = base < cap ? base : cap;
            o.seg[b] = lo;
            o.dropped[b] = (base - before) - (hi - lo);
        }
    }
    const int live = base < cap ? base : cap;
    if (tid == 0) o.seg[B] = live;
    for (int s = live + tid; s < cap; s += PLAN_NT) {              // dead slots: defined values
        for (int i = 0; i < 6; ++i) { o.m_inv[(size_t)s * 6 + i] = 0.0; o.trans_inv[(size_t)s * 6 + i] = 0.f; }
        o.center[s * 2] = 0.f; o.center[s * 2 + 1] = 0.f;
        o.scale[s * 2] = 0.f; o.scale[s * 2 + 1] = 0.f;
        o.area[s] = 0.0;
        o.box_score[s] = 0.0;
        for (int i = 0; i < 5; ++i) o.box[(size_t)s * 5 + i] = 0.f;
        o.src_index[s] = -1;
    }
}

// _triangle(mid, mid + (0, out_w * -0.5)) of get_affine_transform for an output size: float64 sums stored as float32
void dst_triangle(int out_w, int out_h, double* t) {
    const double mx = out_w * 0.5, my = out_h * 0.5;
    const float p0x = (float)mx, p0y = (float)my;
    const float p1x = (float)(mx + (double)0.f), p1y = (float)(my + (double)(float)(out_w * -0.5));
    const float dx = p0x - p1x, dy = p0y - p1y;
    t[0] = p0x; t[1] = p0y; t[2] = p1x; t[3] = p1y; t[4] = p1x + (-dy); t[5] = p1y + dx;
}

}  // namespace

extern "C" int sp_topdown_plan(const float* det, const int32_t* counts, int batch, int max_det, int keep_cls, float min_score, int capacity,
                               int in_w, int in_h, int hm_w, int hm_h, int32_t* seg, int32_t* src_index, double* m_inv, float* trans_inv,
                               float* center, float* scale, double* area, double* box_score, float* box, int32_t* dropped, void* stream) {
    SP_REQUIRE(det && counts && seg && src_index && m_inv && trans_inv && center && scale && area && box_score && box && dropped,
               "sp_topdown_plan: null pointer");
    SP_REQUIRE(batch > 0 && max_det > 0 && (long long)batch * max_det < (1ll << 24), "sp_topdown_plan: batch %d, max_det %d", batch, max_det);
    SP_REQUIRE(capacity >= 1 && capacity <= PLAN_MAX_CAPACITY, "sp_topdown_plan: capacity %d (1..%d, the OKS-NMS group limit)", capacity,
               PLAN_MAX_CAPACITY);
    SP_REQUIRE(in_w > 0 && in_h > 0 && hm_w > 0 && hm_h > 0, "sp_topdown_plan: input %dx%d, heat map %dx%d", in_w, in_h, hm_w, hm_h);
    PlanGeom g;
    g.ar = (float)((double)in_w / (double)in_h);
    dst_triangle(in_w, in_h, g.dst_in);
    dst_triangle(hm_w, hm_h, g.dst_hm);
    PlanOut o;
    o.seg = seg; o.src_index = src_index; o.m_inv = m_inv; o.trans_inv = trans_inv; o.center = center; o.scale = scale; o.area = area;
    o.box_score = box_score; o.box = box; o.dropped = dropped;
    hipLaunchKernelGGL(topdown_plan_kernel, dim3(1), dim3(PLAN_NT), 0, (hipStream_t)stream, det, counts, batch, max_det, keep_cls, min_score,
                       capacity, g, o);
    return sp_check_launch("topdown_plan_kernel");
}
