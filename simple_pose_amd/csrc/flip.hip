// flip.hip - the flip test of top-down evaluation: sp_mirror_w (the mirrored network input) and sp_heat_map_flip_merge (un-mirror the
// second set of heat maps, swap the left/right joints, average with the first set).  Between them sits one forward of the pose program
// on both halves; with these two launches the flip test stays on the frame's stream (and in its graph) instead of going through
// torch's .flip / fancy indexing / add.  The reference has no flip test: the arithmetic is the one stated in include/simple_pose_hip.h
// (one fp32 add, one fp32 multiply by 0.5 per element), so a numpy statement of it agrees bit for bit.
// Both kernels move each byte once: HBM / launch latency bound.  Each has a wide path (16-byte lanes for fp32, 12-byte lanes = four
// pixels for uint8x3; needs w % 4 == 0 and aligned pointers, which the real shapes w = 48 and w = 192 have) and an element-per-lane path.
#include "sp_common.h"

#include <stdint.h>

#pragma clang fp contract(off)

namespace {

constexpr int FLIP_MAX_JOINTS = SP_MAX_JOINTS;

struct FlipPerm { unsigned char p[FLIP_MAX_JOINTS]; };
struct u32x3 { unsigned a, b, c; };                      // four uint8x3 pixels (4-byte aligned)

// ---- sp_mirror_w ------------------------------------------------------------------------------------------------------------------------
// Index type I: unsigned when the element count is below 2^31 (every real shape; i + stride cannot wrap, and the row / column split is a
// 32-bit division), long long above.
// fp32 (or any 4-byte element), four per lane: the lane's destination vector k of a row is source vector wv-1-k with its lanes reversed
template <typename I>
__global__ __launch_bounds__(256) void mirror_w_x4_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, int wv, I total) {
    for (I i = (I)blockIdx.x * 256 + threadIdx.x; i < total; i += (I)gridDim.x * 256) {
        const I r = i / (I)wv;
        const int k = (int)(i - r * (I)wv);
        const u32x4 v = src[(size_t)r * wv + (wv - 1 - k)];
        u32x4 o;
        o[0] = v[3]; o[1] = v[2]; o[2] = v[1]; o[3] = v[0];
        dst[i] = o;
    }
}

// uint8x3, four pixels (three dwords) per lane: pixels p0 p1 p2 p3 of source unit wv-1-k become p3 p2 p1 p0 of destination unit k
template <typename I>
__global__ __launch_bounds__(256) void mirror_w_u8c3x4_kernel(const u32x3* __restrict__ src, u32x3* __restrict__ dst, int wv, I total) {
    for (I i = (I)blockIdx.x * 256 + threadIdx.x; i < total; i += (I)gridDim.x * 256) {
        const I r = i / (I)wv;
        const int k = (int)(i - r * (I)wv);
        const u32x3 v = src[(size_t)r * wv + (wv - 1 - k)];
        // bytes (little endian)  a: p0.0 p0.1 p0.2 p1.0   b: p1.1 p1.2 p2.0 p2.1   c: p2.2 p3.0 p3.1 p3.2
        u32x3 o;
        o.a = (v.c >> 8) | ((v.b >> 16 & 0xffu) << 24);                                            // p3.0 p3.1 p3.2 p2.0
        o.b = (v.b >> 24) | ((v.c & 0xffu) << 8) | ((v.a >> 24) << 16) | ((v.b & 0xffu) << 24);   // p2.1 p2.2 p1.0 p1.1
        o.c = (v.b >> 8 & 0xffu) | (v.a << 8);                                                     // p1.2 p0.0 p0.1 p0.2
        dst[i] = o;
    }
}

// one element of EB bytes per lane: any w, any alignment the element type itself allows (bytes for EB = 3)
template <int EB, typename I>
__global__ __launch_bounds__(256) void mirror_w_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int w, I total) {
    for (I i = (I)blockIdx.x * 256 + threadIdx.x; i < total; i += (I)gridDim.x * 256) {
        const I r = i / (I)w;
        const int x = (int)(i - r * (I)w);
        const size_t s = (size_t)r * w + (w - 1 - x);
        if (EB == 4) {
            reinterpret_cast<unsigned*>(dst)[i] = reinterpret_cast<const unsigned*>(src)[s];
        } else {
            const unsigned char c0 = src[s * 3], c1 = src[s * 3 + 1], c2 = src[s * 3 + 2];
            dst[(size_t)i * 3] = c0; dst[(size_t)i * 3 + 1] = c1; dst[(size_t)i * 3 + 2] = c2;
        }
    }
}

// ---- sp_heat_map_flip_merge ---------------------------------------------------------------------------------------------------------------
// hm and out carry no __restrict__: out == hm is allowed (a lane reads exactly the elements it then writes).
// One element per lane.  rows = batch * joints * h.
__global__ __launch_bounds__(256) void flip_merge_kernel(const float* hm, const float* __restrict__ fl, const FlipPerm perm, int J, int H, int W,
                                                         int shift, float* out, int total) {
    for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {   // (total < 2^31: i + stride may not fit an int)
        const int i = (int)it;
        const int row = i / W, x = i - row * W;
        const int bj = row / H, y = row - bj * H;
        const int b = bj / J, j = bj - b * J;
        const int fx = shift ? (x >= 1 ? x - 1 : 0) : x;                     // the column of f that g[x] takes
        const float g = fl[((size_t)(b * J + perm.p[j]) * H + y) * W + (W - 1 - fx)];
        out[i] = (hm[i] + g) * 0.5f;
    }
}

// Four elements per lane (W = 4 * WV).  Destination vector k holds x = 4k .. 4k+3; with m = WV-1-k the mirrored source vector m holds
// columns W-4-4k .. W-1-4k of the flipped map.  shift = 0: g[4k+i] = fl[W-1-4k-i] = v[3-i].  shift = 1: g[4k+i] = fl[W-4k-i] for
// 4k+i >= 1, i.e. (fl[W-4k], v[3], v[2], v[1]) - the first is element 0 of vector m+1 - and g[0] = f[0] = fl[W-1] = v[3] at k = 0.
__global__ __launch_bounds__(256) void flip_merge_x4_kernel(const f32x4* hm, const f32x4* __restrict__ fl, const FlipPerm perm, int J, int H, int WV,
                                                            int shift, f32x4* out, int total) {
    for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
        const int i = (int)it;
        const int row = i / WV, k = i - row * WV;
        const int bj = row / H, y = row - bj * H;
        const int b = bj / J, j = bj - b * J;
        const size_t m = ((size_t)(b * J + perm.p[j]) * H + y) * WV + (WV - 1 - k);
        const f32x4 v = fl[m];
        f32x4 g;
        if (shift) {
            g[0] = k >= 1 ? reinterpret_cast<const float*>(fl)[(m + 1) * 4] : v[3];
            g[1] = v[3]; g[2] = v[2]; g[3] = v[1];
        } else {
            g[0] = v[3]; g[1] = v[2]; g[2] = v[1]; g[3] = v[0];
        }
        const f32x4 a = hm[i];
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (a[e] + g[e]) * 0.5f;
        out[i] = o;
    }
}

}  // namespace

extern "C" int sp_mirror_w(const void* src, void* dst, int64_t rows, int w, int elem_bytes, void* stream) {
    SP_REQUIRE(src && dst, "sp_mirror_w: null pointer");
    SP_REQUIRE(elem_bytes == 3 || elem_bytes == 4, "sp_mirror_w: elem_bytes %d (3: uint8 BGR pixels, 4: fp32)", elem_bytes);
    SP_REQUIRE(w > 0 && rows >= 0 && rows < (1ll << 31), "sp_mirror_w: rows %lld, w %d", (long long)rows, w);
    if (rows == 0) return SP_OK;
    const long long total = (long long)rows * w;
    SP_REQUIRE(total < (1ll << 40), "sp_mirror_w: %lld elements (tensor too large)", total);
    SP_REQUIRE(!sp_ranges_overlap(src, dst, (unsigned long long)total * elem_bytes),
               "sp_mirror_w: src and dst overlap (out of place only; dst may be the second half of src's allocation)");
    const hipStream_t s = (hipStream_t)stream;
    const bool wide = w % 4 == 0 && sp_aligned_to(src, elem_bytes == 4 ? 16 : 4) && sp_aligned_to(dst, elem_bytes == 4 ? 16 : 4);
    const bool small = total < (1ll << 31);                   // 32-bit index arithmetic in the kernel
#define SP_MIRROR_LAUNCH(kernel, n, ...)                                                                                        \
    do {                                                                                                                        \
        if (small) hipLaunchKernelGGL(kernel<unsigned>, dim3(sp_grid_for(n, 256)), dim3(256), 0, s, __VA_ARGS__, (unsigned)(n)); \
        else hipLaunchKernelGGL(kernel<long long>, dim3(sp_grid_for(n, 256)), dim3(256), 0, s, __VA_ARGS__, (long long)(n));    \
    } while (0)
    if (wide && elem_bytes == 4) {
        SP_MIRROR_LAUNCH(mirror_w_x4_kernel, total / 4, reinterpret_cast<const u32x4*>(src), reinterpret_cast<u32x4*>(dst), w / 4);
        return sp_check_launch("mirror_w_x4_kernel");
    }
    if (wide) {
        SP_MIRROR_LAUNCH(mirror_w_u8c3x4_kernel, total / 4, reinterpret_cast<const u32x3*>(src), reinterpret_cast<u32x3*>(dst), w / 4);
        return sp_check_launch("mirror_w_u8c3x4_kernel");
    }
    const unsigned char* sb = static_cast<const unsigned char*>(src);
    unsigned char* db = static_cast<unsigned char*>(dst);
    if (elem_bytes == 4) {
        SP_REQUIRE(sp_aligned_to(src, 4) && sp_aligned_to(dst, 4), "sp_mirror_w: fp32 pointers must be 4-byte aligned");
        if (small) hipLaunchKernelGGL((mirror_w_kernel<4, unsigned>), dim3(sp_grid_for(total, 256)), dim3(256), 0, s, sb, db, w, (unsigned)total);
        else hipLaunchKernelGGL((mirror_w_kernel<4, long long>), dim3(sp_grid_for(total, 256)), dim3(256), 0, s, sb, db, w, total);
    } else {
        if (small) hipLaunchKernelGGL((mirror_w_kernel<3, unsigned>), dim3(sp_grid_for(total, 256)), dim3(256), 0, s, sb, db, w, (unsigned)total);
        else hipLaunchKernelGGL((mirror_w_kernel<3, long long>), dim3(sp_grid_for(total, 256)), dim3(256), 0, s, sb, db, w, total);
    }
#undef SP_MIRROR_LAUNCH
    return sp_check_launch("mirror_w_kernel");
}

extern "C" int sp_heat_map_flip_merge(const float* hm, const float* hm_flipped, const int32_t* perm_host, int batch, int joints, int h, int w,
                                      int shift, float* out, void* stream) {
    SP_REQUIRE(hm && hm_flipped && perm_host && out, "sp_heat_map_flip_merge: null pointer");
    SP_REQUIRE(joints >= 1 && joints <= FLIP_MAX_JOINTS, "sp_heat_map_flip_merge: joints %d (1..%d)", joints, FLIP_MAX_JOINTS);
    SP_REQUIRE(batch >= 0 && h > 0 && w > 0, "sp_heat_map_flip_merge: bad shape batch=%d h=%d w=%d", batch, h, w);
    const long long total = (long long)batch * joints * h * w;
    SP_REQUIRE(total < (1ll << 31), "sp_heat_map_flip_merge: tensor too large");
    FlipPerm perm;
    bool seen[FLIP_MAX_JOINTS] = {};
    for (int j = 0; j < joints; ++j) {
        const int p = perm_host[j];
        SP_REQUIRE(p >= 0 && p < joints, "sp_heat_map_flip_merge: perm[%d] = %d is out of range 0..%d", j, p, joints - 1);
        SP_REQUIRE(!seen[p], "sp_heat_map_flip_merge: perm is not a permutation (%d appears twice)", p);
        seen[p] = true;
        perm.p[j] = (unsigned char)p;
    }
    for (int j = joints; j < FLIP_MAX_JOINTS; ++j) perm.p[j] = 0;
    if (total == 0) return SP_OK;
    const unsigned long long bytes = (unsigned long long)total * 4;
    SP_REQUIRE(!sp_ranges_overlap(out, hm_flipped, bytes), "sp_heat_map_flip_merge: out overlaps hm_flipped (in place only on hm)");
    SP_REQUIRE(out == hm || !sp_ranges_overlap(out, hm, bytes), "sp_heat_map_flip_merge: out overlaps hm without being hm");
    SP_REQUIRE(sp_aligned_to(hm, 4) && sp_aligned_to(hm_flipped, 4) && sp_aligned_to(out, 4), "sp_heat_map_flip_merge: pointers must be 4-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    if (w % 4 == 0 && sp_aligned_to(hm, 16) && sp_aligned_to(hm_flipped, 16) && sp_aligned_to(out, 16)) {
        hipLaunchKernelGGL(flip_merge_x4_kernel, dim3(sp_grid_for(total / 4, 256)), dim3(256), 0, s, reinterpret_cast<const f32x4*>(hm),
                           reinterpret_cast<const f32x4*>(hm_flipped), perm, joints, h, w / 4, shift ? 1 : 0, reinterpret_cast<f32x4*>(out),
                           (int)(total / 4));
        return sp_check_launch("flip_merge_x4_kernel");
    }
    hipLaunchKernelGGL(flip_merge_kernel, dim3(sp_grid_for(total, 256)), dim3(256), 0, s, hm, hm_flipped, perm, joints, h, w, shift ? 1 : 0, out,
                       (int)total);
    return sp_check_launch("flip_merge_kernel");
}
