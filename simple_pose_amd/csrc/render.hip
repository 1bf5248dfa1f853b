// render.hip - the pose overlay on the device: the kept poses of one image (what sp_oks_nms and sp_track_associate leave behind) drawn into
// the frame as capsules - box edges, limbs, joints - so that an annotated frame stays one stream of launches (capturable with the rest of
// the frame) and the person count never reaches the host.  The reference has no drawing code; the pixel rules live in sp_render.h (shared
// with tests/render_core_main.cpp) and are restated for numpy in tests/render_ref.py; the tile, a thread's pixels, the ordered scan and the
// entry point's frame checks are sp_frame_tile.h's, shared with the other overlays.  Integer arithmetic and one fp64 comparison:
// contraction OFF for the whole file.
#include "sp_frame_tile.h"
#include "sp_render.h"

#include <stdint.h>

#pragma clang fp contract(off)

namespace {

constexpr int RND_LIST = 512;                    // primitive indices a tile collects before it applies them

// One thread per (person slot, primitive slot): dead persons' slots are written as empty primitives, so the tile kernel needs no count.
__global__ __launch_bounds__(SP_TILE_NT) void render_prims_kernel(const sp_render_style st, int joints, int rows, int image,
                                                                  const double* __restrict__ kps, const float* __restrict__ box,
                                                                  const int32_t* __restrict__ track_id, const int32_t* __restrict__ keep,
                                                                  const int32_t* __restrict__ keep_count, const int32_t* __restrict__ seg,
                                                                  int total, sp_render_prim* __restrict__ prims) {
    const int i = blockIdx.x * SP_TILE_NT + threadIdx.x;
    if (i >= total) return;
    prims[i] = sp_render_prim_at(st, joints, rows, image, kps, box, track_id, keep, keep_count, seg, i);
}

// The listed primitives, in list order, onto the thread's four pixels.  A function of its own with `prims` __restrict__, not the body of
// the scan's callable: written there the loop is allocated 75 VGPRs instead of 99 and the 640 x 480 frame measures 5 % slower.
__device__ __forceinline__ void apply_list(const sp_render_prim* __restrict__ prims, const int* list, int count, int opacity, int x0, int y, int w,
                                           int h, unsigned char (&px)[4][3]) {
    for (int e = 0; e < count; ++e) {
        const sp_render_prim p = prims[list[e]];           // one address for the whole workgroup
        if (y >= h || y < p.y0 || y > p.y1) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (x0 + q < w) sp_render_apply(p, opacity, x0 + q, y, px[q]);
    }
}

// One workgroup per 64 x 16 tile: the primitives that meet it (sp_tile_scan_ordered), in index order, onto every thread's four pixels.
template <bool WIDE>
__global__ __launch_bounds__(SP_TILE_NT) void render_tile_kernel(const unsigned char* src, unsigned char* dst, int h, int w,
                                                                 const sp_render_prim* __restrict__ prims, int total, int opacity) {
    const sp_tile t;
    const int x0 = t.x0, y = t.y;
    const size_t at = ((size_t)y * w + x0) * 3;
    const bool mine = y < h && x0 < w;
    sp_px4 px;
    if (mine) px.load<WIDE>(src, at, x0, w);
    else px.clear();
    unsigned char bgr[4][3];
    px.unpack(bgr);
    const bool touched = sp_tile_scan_ordered<RND_LIST>(prims, total, t, [&](const int* list, int count) {
        apply_list(prims, list, count, opacity, x0, y, w, h, bgr);
    });
    // store once (in place: a tile nothing touched keeps its bytes without a write)
    if (!mine || (dst == src && !touched)) return;
    px.pack(bgr);
    px.store<WIDE>(dst, at, x0, w);
}

int check_shape(const char* what, int joints, int edges) {
    SP_REQUIRE(joints >= 1 && joints <= SP_MAX_JOINTS, "%s: joints %d (1..%d)", what, joints, SP_MAX_JOINTS);
    SP_REQUIRE(edges >= 0 && edges <= SP_RENDER_MAX_EDGES, "%s: edges %d (0..%d)", what, edges, SP_RENDER_MAX_EDGES);
    return SP_OK;
}

}  // namespace

extern "C" int sp_render_workspace_bytes(int rows, int joints, int edges, int64_t* bytes) {
    SP_REQUIRE(bytes, "sp_render_workspace_bytes: null pointer");
    int rc = sp_frame_rows_check("sp_render_workspace_bytes", rows);
    if (rc == SP_OK) rc = check_shape("sp_render_workspace_bytes", joints, edges);
    if (rc != SP_OK) return rc;
    *bytes = (int64_t)rows * (SP_RENDER_BOX_SLOTS + edges + joints) * (int64_t)sizeof(sp_render_prim);
    return SP_OK;
}

extern "C" int sp_render_poses_u8c3(const unsigned char* src, unsigned char* dst, int h, int w, const double* kps, const float* box,
                                    const int32_t* track_id, const int32_t* keep, const int32_t* keep_count, const int32_t* seg, int image,
                                    int rows, int joints, const sp_render_style* style_host, void* workspace, void* stream) {
    SP_REQUIRE(style_host, "sp_render_poses_u8c3: null pointer");
    int rc = sp_frame_check("sp_render_poses_u8c3", src, dst, h, w, image, rows);
    if (rc != SP_OK) return rc;
    const sp_render_style st = *style_host;
    rc = check_shape("sp_render_poses_u8c3", joints, st.edges);
    if (rc != SP_OK) return rc;
    for (int e = 0; e < st.edges; ++e)
        for (int k = 0; k < 2; ++k)
            SP_REQUIRE(st.edge[e][k] >= 0 && st.edge[e][k] < joints, "sp_render_poses_u8c3: edge[%d][%d] = %d is no joint index (0..%d)", e, k,
                       st.edge[e][k], joints - 1);
    SP_REQUIRE(st.joint_r >= 0 && st.joint_r <= SP_RENDER_MAX_RADIUS && st.limb_r >= 0 && st.limb_r <= SP_RENDER_MAX_RADIUS && st.box_r >= 0 &&
               st.box_r <= SP_RENDER_MAX_RADIUS, "sp_render_poses_u8c3: radius joint_r=%d limb_r=%d box_r=%d (1/16 px, 0..%d)", st.joint_r, st.limb_r,
               st.box_r, SP_RENDER_MAX_RADIUS);
    SP_REQUIRE(st.opacity >= 0 && st.opacity <= 16, "sp_render_poses_u8c3: opacity %d (sixteenths, 0..16)", st.opacity);
    SP_REQUIRE(st.colour_by == SP_RENDER_COLOUR_PERSON || st.colour_by == SP_RENDER_COLOUR_PART, "sp_render_poses_u8c3: colour_by %d", st.colour_by);
    SP_REQUIRE(st.palette_n >= 1 && st.palette_n <= SP_RENDER_MAX_PALETTE, "sp_render_poses_u8c3: palette_n %d (1..%d)", st.palette_n,
               SP_RENDER_MAX_PALETTE);
    if (rows == 0 && dst == src) return SP_OK;
    if (rows > 0) {
        SP_REQUIRE(kps && box && keep && keep_count && seg && workspace, "sp_render_poses_u8c3: null pointer");
        SP_REQUIRE(sp_aligned_to(workspace, 8) && sp_aligned_to(kps, 8), "sp_render_poses_u8c3: workspace and kps must be 8-byte aligned");
    }
    const hipStream_t s = (hipStream_t)stream;
    sp_render_prim* prims = reinterpret_cast<sp_render_prim*>(workspace);
    const int total = rows * sp_render_slots(st, joints);
    if (total > 0) {
        hipLaunchKernelGGL(render_prims_kernel, dim3(sp_ceil_div(total, SP_TILE_NT)), dim3(SP_TILE_NT), 0, s, st, joints, rows, image, kps, box,
                           track_id, keep, keep_count, seg, total, prims);
        rc = sp_check_launch("render_prims_kernel");
        if (rc != SP_OK) return rc;
    }
    const dim3 grid(sp_ceil_div(w, SP_TILE_W), sp_ceil_div(h, SP_TILE_H));
    if (sp_frame_wide(w, src, dst))
        hipLaunchKernelGGL(render_tile_kernel<true>, grid, dim3(SP_TILE_NT), 0, s, src, dst, h, w, prims, total, st.opacity);
    else
        hipLaunchKernelGGL(render_tile_kernel<false>, grid, dim3(SP_TILE_NT), 0, s, src, dst, h, w, prims, total, st.opacity);
    return sp_check_launch("render_tile_kernel");
}
