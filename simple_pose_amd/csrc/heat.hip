// heat.hip - the heat overlay on the device: the joint heat maps of one image's kept persons (what sp_oks_nms leaves behind), merged,
// warped back into the frame and blended into it through a colour table, so that the one intermediate of the top-down path nobody sees
// becomes part of the frame's own stream of launches (capturable with the rest) and never visits the host.  The reference shows
// max_j(hm) * 255 in a window (commons/transforms.py, draw_heat_map); the rules here live in sp_heat.h (shared with
// tests/heat_core_main.cpp) and are restated for numpy in tests/heat_ref.py; a thread's pixels, the tile's coordinates and the entry
// point's frame checks are sp_frame_tile.h's, shared with the other overlays (the list here is unordered: a maximum needs no order).
// Integer arithmetic and three floating-point steps: contraction OFF for the whole file.
#include "sp_frame_tile.h"
#include "sp_heat.h"

#include <float.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace {

// One workgroup per person slot.  Every thread works out the slot's row and record (a few dozen scalar operations on uniform values);
// thread 0 writes the record.  A dead or refused slot ends there and reads nothing of hm.  Otherwise the workgroup reduces the row's maps
// to the u8 plane: WIDE (hm_w % 4 == 0, hm 16-byte aligned) four cells per thread and step from one 16-byte load per joint, else cell by cell.
__global__ __launch_bounds__(SP_TILE_NT) void heat_planes_kernel(const sp_heat_style st, const float* __restrict__ hm, int joints, int hm_h, int hm_w,
                                                            int wide, const float* __restrict__ trans_inv, const int32_t* __restrict__ keep,
                                                            const int32_t* __restrict__ keep_count, const int32_t* __restrict__ seg, int image,
                                                            int rows, sp_heat_rec* __restrict__ recs, unsigned char* __restrict__ planes) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const int row = sp_heat_row_at(keep, keep_count, seg, image, rows, p);
    const uint64_t mask = sp_heat_joints(st.joint_mask, joints);
    sp_heat_rec r = sp_heat_empty();
    if (row >= 0 && mask != 0ull) r = sp_heat_record(trans_inv + (size_t)row * 6, hm_h, hm_w);
    if (tid == 0) recs[p] = r;
    if (r.x0 > r.x1) return;
    const size_t cells = (size_t)hm_h * hm_w;
    const float* maps = hm + (size_t)row * joints * cells;
    unsigned char* plane = planes + (size_t)p * cells;
    if (wide) {
        uint32_t* plane4 = reinterpret_cast<uint32_t*>(plane);               // cells % 4 == 0 and the planes start 8-byte aligned
        for (size_t g = tid; g < cells / 4; g += SP_TILE_NT) {
            float m0 = NAN, m1 = NAN, m2 = NAN, m3 = NAN;
            for (int j = 0; j < joints; ++j) {
                if (!((mask >> j) & 1ull)) continue;
                const f32x4 v = *reinterpret_cast<const f32x4*>(maps + (size_t)j * cells + 4 * g);
                m0 = sp_heat_max(m0, v[0]); m1 = sp_heat_max(m1, v[1]); m2 = sp_heat_max(m2, v[2]); m3 = sp_heat_max(m3, v[3]);
            }
            plane4[g] = sp_heat_q(m0, st.scale) | sp_heat_q(m1, st.scale) << 8 | sp_heat_q(m2, st.scale) << 16 | sp_heat_q(m3, st.scale) << 24;
        }
    } else {
        for (size_t i = tid; i < cells; i += SP_TILE_NT) plane[i] = (unsigned char)sp_heat_cell(maps, cells, i, mask, st.scale);
    }
}

// One workgroup per tile; thread t owns the four consecutive pixels from x = tx0 + 4 (t & 15) of the row ty0 + (t >> 4).
// 1. scan: per chunk of 256 records a thread takes one; if its box meets the tile and (exact, in int64) its U and V ranges over the tile
//    reach a tap, the slot joins the LDS list.  An empty list: the tile is left alone (in place) or copied.
// 2. every pixel takes the maximum of its sample over the listed persons (the planes are a few KB each and stay in the caches; the four
//    taps are byte loads from global memory), and is blended through the colour table, which sits in LDS.
// 3. store: out of place everything; in place only the threads that changed a pixel.
template <bool WIDE>
__global__ __launch_bounds__(SP_TILE_NT) void heat_tile_kernel(const unsigned char* src, unsigned char* dst, int h, int w,
                                                          const sp_heat_rec* __restrict__ recs, int total,
                                                          const unsigned char* __restrict__ planes, int hm_h, int hm_w, const sp_heat_style st,
                                                          const unsigned char* __restrict__ lut) {
    __shared__ unsigned short list[SP_MAX_ROWS];
    __shared__ unsigned char colours[768];
    __shared__ int count;
    const int tid = threadIdx.x;
    const sp_tile t;
    const int tx0 = t.tx0, ty0 = t.ty0;
    const int tx1 = min(tx0 + SP_TILE_W, w) - 1, ty1 = min(ty0 + SP_TILE_H, h) - 1;    // the tile's last pixels inside the image
    const bool in_place = dst == src;
    if (tid == 0) count = 0;
    __syncthreads();
    // ---- 1. who reaches the tile ------------------------------------------------------------------------------------------------------
    for (int base = 0; base < total; base += SP_TILE_NT) {
        const int i = base + tid;
        if (i >= total) break;
        const sp_heat_rec& r = recs[i];
        if (!sp_box_meets(r, tx0, ty0, tx1, ty1)) continue;
        int64_t c[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) c[k] = r.c[k];
        if (sp_heat_reaches(c, hm_h, hm_w, tx0, ty0, tx1, ty1)) list[atomicAdd(&count, 1)] = (unsigned short)i;    // (at most `total` <= 2048)
    }
    __syncthreads();
    const int n = count;                                                                                         // uniform
    if (n == 0 && in_place) return;
    if (n > 0) {
        for (int i = tid; i < 768; i += SP_TILE_NT) colours[i] = lut[i];
        __syncthreads();
    }
    // ---- the thread's pixels ---------------------------------------------------------------------------------------------------------------
    const int x0 = t.x0, y = t.y;
    if (y >= h || x0 >= w) return;
    const size_t at = ((size_t)y * w + x0) * 3;
    sp_px4 px;
    px.load<WIDE>(src, at, x0, w);
    // ---- 2. the maximum over the listed persons, and the blend ----------------------------------------------------------------------------
    bool changed = false;
    if (n > 0) {
        uint32_t vmax[4] = {0u, 0u, 0u, 0u};
        const size_t cells = (size_t)hm_h * hm_w;
        for (int k = 0; k < n; ++k) {
            const int i = list[k];
            const sp_heat_rec& r = recs[i];
            const unsigned char* plane = planes + (size_t)i * cells;
            const int64_t c0 = r.c[0], c3 = r.c[3];
            int64_t U = c0 * x0 + r.c[1] * y + r.c[2], V = c3 * x0 + r.c[4] * y + r.c[5];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t val = sp_heat_sample(plane, hm_h, hm_w, U, V);
                vmax[q] = val > vmax[q] ? val : vmax[q];
                U += c0; V += c3;
            }
        }
        unsigned char bgr[4][3];
        px.unpack(bgr);
#pragma unroll
        for (int q = 0; q < 4; ++q) changed = sp_heat_apply(st, vmax[q], colours, bgr[q]) || changed;
        px.pack(bgr);
    }
    // ---- 3. store -------------------------------------------------------------------------------------------------------------------------
    if (changed || !in_place) px.store<WIDE>(dst, at, x0, w);
}

}  // namespace

extern "C" int sp_heat_overlay_workspace_bytes(int rows, int hm_h, int hm_w, int64_t* bytes) {
    SP_REQUIRE(bytes, "sp_heat_overlay_workspace_bytes: null pointer");
    const int rc = sp_frame_rows_check("sp_heat_overlay_workspace_bytes", rows);
    if (rc != SP_OK) return rc;
    SP_REQUIRE(hm_h >= 1 && hm_h <= SP_HEAT_MAX_MAP && hm_w >= 1 && hm_w <= SP_HEAT_MAX_MAP,
               "sp_heat_overlay_workspace_bytes: heat map %dx%d (1..%d each way)", hm_w, hm_h, SP_HEAT_MAX_MAP);
    *bytes = (int64_t)rows * ((int64_t)sizeof(sp_heat_rec) + (int64_t)hm_h * hm_w);
    return SP_OK;
}

extern "C" int sp_heat_overlay_u8c3(const unsigned char* src, unsigned char* dst, int h, int w, const float* hm, int joints, int hm_h, int hm_w,
                                    const float* trans_inv, const int32_t* keep, const int32_t* keep_count, const int32_t* seg, int image,
                                    int rows, const sp_heat_style* style_host, const unsigned char* lut, void* workspace, void* stream) {
    SP_REQUIRE(style_host, "sp_heat_overlay_u8c3: null pointer");
    int rc = sp_frame_check("sp_heat_overlay_u8c3", src, dst, h, w, image, rows);
    if (rc != SP_OK) return rc;
    SP_REQUIRE(joints >= 1 && joints <= SP_MAX_JOINTS, "sp_heat_overlay_u8c3: joints %d (1..%d)", joints, SP_MAX_JOINTS);
    SP_REQUIRE(hm_h >= 1 && hm_h <= SP_HEAT_MAX_MAP && hm_w >= 1 && hm_w <= SP_HEAT_MAX_MAP, "sp_heat_overlay_u8c3: heat map %dx%d (1..%d each way)",
               hm_w, hm_h, SP_HEAT_MAX_MAP);
    const sp_heat_style st = *style_host;
    SP_REQUIRE(st.threshold >= 1 && st.threshold <= 255, "sp_heat_overlay_u8c3: threshold %d (1..255)", st.threshold);
    SP_REQUIRE(st.opacity16 >= 0 && st.opacity16 <= 16, "sp_heat_overlay_u8c3: opacity16 %d (sixteenths, 0..16)", st.opacity16);
    SP_REQUIRE(st.alpha == SP_HEAT_ALPHA_CONSTANT || st.alpha == SP_HEAT_ALPHA_VALUE, "sp_heat_overlay_u8c3: alpha %d", st.alpha);
    SP_REQUIRE(st.scale >= 0.0f && st.scale <= FLT_MAX,"sp_heat_overlay_u8c3: scale %g (finite, >= 0)", (double)st.scale);
    if (rows == 0 && dst == src) return SP_OK;
    if (rows > 0) {
        SP_REQUIRE(hm && trans_inv && keep && keep_count && seg && lut && workspace, "sp_heat_overlay_u8c3: null pointer");
        SP_REQUIRE(sp_aligned_to(workspace, 8) && sp_aligned_to(hm, 4) && sp_aligned_to(trans_inv, 4),
                   "sp_heat_overlay_u8c3: workspace must be 8-byte, hm and trans_inv 4-byte aligned");
    }
    const hipStream_t s = (hipStream_t)stream;
    sp_heat_rec* recs = reinterpret_cast<sp_heat_rec*>(workspace);
    unsigned char* planes = reinterpret_cast<unsigned char*>(workspace) + (size_t)rows * sizeof(sp_heat_rec);
    if (rows > 0) {
        const int wide = hm_w % 4 == 0 && sp_aligned_to(hm, 16);
        hipLaunchKernelGGL(heat_planes_kernel, dim3(rows), dim3(SP_TILE_NT), 0, s, st, hm, joints, hm_h, hm_w, wide, trans_inv, keep, keep_count, seg,
                           image, rows, recs, planes);
        rc = sp_check_launch("heat_planes_kernel");
        if (rc != SP_OK) return rc;
    }
    const dim3 grid(sp_ceil_div(w, SP_TILE_W), sp_ceil_div(h, SP_TILE_H));
    if (sp_frame_wide(w, src, dst))
        hipLaunchKernelGGL((heat_tile_kernel<true>), grid, dim3(SP_TILE_NT), 0, s, src, dst, h, w, recs, rows, planes, hm_h, hm_w, st, lut);
    else
        hipLaunchKernelGGL((heat_tile_kernel<false>), grid, dim3(SP_TILE_NT), 0, s, src, dst, h, w, recs, rows, planes, hm_h, hm_w, st, lut);
    return sp_check_launch("heat_tile_kernel");
}
