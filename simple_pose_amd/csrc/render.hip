// render.hip - the pose overlay on the device: the kept poses of one image (what sp_oks_nms and sp_track_associate leave behind) drawn into
// the frame as capsules - box edges, limbs, joints - so that an annotated frame stays one stream of launches (capturable with the rest of
// the frame) and the person count never reaches the host.  The reference has no drawing code; the pixel rules live in sp_render.h (shared
// with tests/render_core_main.cpp) and are restated for numpy in tests/render_ref.py.  Integer arithmetic and one fp64 comparison:
// contraction OFF for the whole file.
#include "sp_common.h"
#include "sp_render.h"

#include <stdint.h>

#pragma clang fp contract(off)

namespace {

constexpr int RND_NT = 256;
constexpr int RND_TILE_W = 64, RND_TILE_H = 16;  // 256 threads x 4 consecutive pixels of one row
constexpr int RND_LIST = 512;                    // primitive indices a tile collects before it applies them
constexpr int RND_MAX_ROWS = 2048;               // the OKS-NMS group limit
constexpr int RND_MAX_JOINTS = 64;
constexpr int RND_MAX_DIM = 16384;

// One thread per (person slot, primitive slot): dead persons' slots are written as empty primitives, so the tile kernel needs no count.
__global__ __launch_bounds__(RND_NT) void render_prims_kernel(const sp_render_style st, int joints, int rows, int image,
                                                              const double* __restrict__ kps, const float* __restrict__ box,
                                                              const int32_t* __restrict__ track_id, const int32_t* __restrict__ keep,
                                                              const int32_t* __restrict__ keep_count, const int32_t* __restrict__ seg, int total,
                                                              sp_render_prim* __restrict__ prims) {
    const int i = blockIdx.x * RND_NT + threadIdx.x;
    if (i >= total) return;
    prims[i] = sp_render_prim_at(st, joints, rows, image, kps, box, track_id, keep, keep_count, seg, i);
}

// the listed primitives, in list order, onto the thread's four pixels
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

// One workgroup per 64 x 16 tile.  The scan keeps the index order without atomics: per chunk of 256 primitives a ballot per wave, the
// four wave counts through LDS, and every hit lands at (hits before its wave) + (hits below its lane).
template <bool WIDE>
__global__ __launch_bounds__(RND_NT) void render_tile_kernel(const unsigned char* src, unsigned char* dst, int h, int w,
                                                             const sp_render_prim* __restrict__ prims, int total, int opacity) {
    __shared__ int list[RND_LIST];
    __shared__ int wave_hits[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx0 = blockIdx.x * RND_TILE_W, ty0 = blockIdx.y * RND_TILE_H;
    const int x0 = tx0 + (tid & 15) * 4, y = ty0 + (tid >> 4);
    const bool in_place = dst == src;
    const size_t at = ((size_t)y * w + x0) * 3;
    unsigned char px[4][3];
    // ---- the thread's pixels (WIDE: w % 4 == 0, so a group of four is inside the row or outside it as a whole) ---------------------------------
    const bool mine = y < h && x0 < w;
    if (mine) {
        if (WIDE) {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(src + at);
            const uint32_t v[3] = {s[0], s[1], s[2]};
#pragma unroll
            for (int b = 0; b < 12; ++b) px[b / 3][b % 3] = (unsigned char)(v[b / 4] >> (8 * (b % 4)));
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) px[q][c] = x0 + q < w ? src[at + q * 3 + c] : 0;
        }
    } else {
#pragma unroll
        for (int b = 0; b < 12; ++b) px[b / 3][b % 3] = 0;
    }
    // ---- scan, list, apply ----------------------------------------------------------------------------------------------------------------
    int count = 0;                               // uniform: every thread adds the same totals
    bool touched = false;
    for (int base = 0; base < total; base += RND_NT) {
        const int i = base + tid;
        bool hit = false;
        if (i < total) {
            const sp_render_prim& p = prims[i];
            hit = p.x0 <= tx0 + RND_TILE_W - 1 && p.x1 >= tx0 && p.y0 <= ty0 + RND_TILE_H - 1 && p.y1 >= ty0;     // (empty: x0 > x1)
        }
        const unsigned long long ballot = __ballot(hit);
        if (lane == 0) wave_hits[wave] = __popcll(ballot);
        __syncthreads();                         // the wave counts; and the list entries of the chunk before
        int before = 0, chunk = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int n = wave_hits[v];
            before += v < wave ? n : 0;
            chunk += n;
        }
        if (count + chunk > RND_LIST) {          // uniform
            apply_list(prims, list, count, opacity, x0, y, w, h, px);
            count = 0;
            __syncthreads();                     // nobody still reads the list
        }
        if (hit) list[count + before + __popcll(ballot & ((1ull << lane) - 1ull))] = i;
        count += chunk;
        touched = touched || chunk > 0;
        __syncthreads();                         // the entries are visible; wave_hits is free for the next chunk
    }
    apply_list(prims, list, count, opacity, x0, y, w, h, px);
    // ---- store once (in place: a tile nothing touched keeps its bytes without a write) ---------------------------------------------------------
    if (!mine || (in_place && !touched)) return;
    if (WIDE) {
        uint32_t v[3] = {0u, 0u, 0u};
#pragma unroll
        for (int b = 0; b < 12; ++b) v[b / 4] |= (uint32_t)px[b / 3][b % 3] << (8 * (b % 4));
        uint32_t* d = reinterpret_cast<uint32_t*>(dst + at);
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2];
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (x0 + q < w) dst[at + q * 3 + c] = px[q][c];
    }
}

bool ranges_overlap(const void* a, const void* b, unsigned long long bytes) {
    const unsigned long long x = (unsigned long long)(uintptr_t)a, y = (unsigned long long)(uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

bool aligned_to(const void* p, unsigned n) { return ((uintptr_t)p & (n - 1)) == 0; }

int check_shape(const char* what, int rows, int joints, int edges) {
    SP_REQUIRE(rows >= 0 && rows <= RND_MAX_ROWS, "%s: rows %d (0..%d, the OKS-NMS group limit)", what, rows, RND_MAX_ROWS);
    SP_REQUIRE(joints >= 1 && joints <= RND_MAX_JOINTS, "%s: joints %d (1..%d)", what, joints, RND_MAX_JOINTS);
    SP_REQUIRE(edges >= 0 && edges <= SP_RENDER_MAX_EDGES, "%s: edges %d (0..%d)", what, edges, SP_RENDER_MAX_EDGES);
    return SP_OK;
}

}  // namespace

extern "C" int sp_render_workspace_bytes(int rows, int joints, int edges, int64_t* bytes) {
    SP_REQUIRE(bytes, "sp_render_workspace_bytes: null pointer");
    const int rc = check_shape("sp_render_workspace_bytes", rows, joints, edges);
    if (rc != SP_OK) return rc;
    *bytes = (int64_t)rows * (SP_RENDER_BOX_SLOTS + edges + joints) * (int64_t)sizeof(sp_render_prim);
    return SP_OK;
}

extern "C" int sp_render_poses_u8c3(const unsigned char* src, unsigned char* dst, int h, int w, const double* kps, const float* box,
                                    const int32_t* track_id, const int32_t* keep, const int32_t* keep_count, const int32_t* seg, int image,
                                    int rows, int joints, const sp_render_style* style_host, void* workspace, void* stream) {
    SP_REQUIRE(src && dst && style_host, "sp_render_poses_u8c3: null pointer");
    SP_REQUIRE(h >= 1 && h <= RND_MAX_DIM && w >= 1 && w <= RND_MAX_DIM, "sp_render_poses_u8c3: image %dx%d (1..%d each way)", w, h, RND_MAX_DIM);
    SP_REQUIRE(image >= 0, "sp_render_poses_u8c3: image index %d", image);
    const sp_render_style st = *style_host;
    const int rc = check_shape("sp_render_poses_u8c3", rows, joints, st.edges);
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
    const unsigned long long bytes = (unsigned long long)h * w * 3;
    SP_REQUIRE(dst == src || !ranges_overlap(src, dst, bytes), "sp_render_poses_u8c3: src and dst overlap without being equal (in place, or apart)");
    if (rows == 0 && dst == src) return SP_OK;
    if (rows > 0) {
        SP_REQUIRE(kps && box && keep && keep_count && seg && workspace, "sp_render_poses_u8c3: null pointer");
        SP_REQUIRE(aligned_to(workspace, 8) && aligned_to(kps, 8), "sp_render_poses_u8c3: workspace and kps must be 8-byte aligned");
    }
    const hipStream_t s = (hipStream_t)stream;
    sp_render_prim* prims = reinterpret_cast<sp_render_prim*>(workspace);
    const int total = rows * sp_render_slots(st, joints);
    if (total > 0) {
        hipLaunchKernelGGL(render_prims_kernel, dim3(sp_ceil_div(total, RND_NT)), dim3(RND_NT), 0, s, st, joints, rows, image, kps, box, track_id, keep,
                           keep_count, seg, total, prims);
        const int rc2 = sp_check_launch("render_prims_kernel");
        if (rc2 != SP_OK) return rc2;
    }
    const dim3 grid(sp_ceil_div(w, RND_TILE_W), sp_ceil_div(h, RND_TILE_H));
    if (w % 4 == 0 && aligned_to(src, 4) && aligned_to(dst, 4))
        hipLaunchKernelGGL(render_tile_kernel<true>, grid, dim3(RND_NT), 0, s, src, dst, h, w, prims, total, st.opacity);
    else
        hipLaunchKernelGGL(render_tile_kernel<false>, grid, dim3(RND_NT), 0, s, src, dst, h, w, prims, total, st.opacity);
    return sp_check_launch("render_tile_kernel");
}
