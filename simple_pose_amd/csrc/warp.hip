// warp.hip - person crops straight from the full image on the GPU: cv.warpAffine(img, M, (w,h), flags=INTER_LINEAR) for N boxes of
// one 8-bit BGR image in one launch.  Replaces the per-person CPU warp of the detector-driven path (datasets/naive_data.py:50,
// commons/transforms.py:214).  Integer arithmetic of OpenCV's fixed-point bilinear remap, restated from the published algorithm
// (imgproc/imgwarp.cpp; opencv-python is not available to pin against: see oracle/pose_oracle.c sp_oracle_warp_affine_u8c3):
// coordinates in 1/1024 px rounded to 1/32 px, four 15-bit weights, (sum + 2^14) >> 15, BORDER_CONSTANT 0.
// HBM-bound gather: 3 B written per output pixel, <= 12 B read (neighbouring lanes share lines).
// The training-side batch (sp_warp_affine_batch_u8c3_to_nchw_f32: RefineSimpleTransform's warp + horizontal flip + the collate
// normalisation, one source image per sample) runs the same per-pixel function and writes 12 B of fp32 (+ 3 B of optional crop).
// The top-down estimator's crops (sp_warp_affine_plan_u8c3) take their maps and source indices from DEVICE memory (sp_topdown_plan wrote
// them), so that the launch can sit in a captured graph; same per-pixel function, dead slots zero-filled.
// sp_warp_affine_plan_images_u8c3 is that launch for a batch of differently sized images: each slot's source pointer and size come from a
// table of sp_image_ref in device memory.
#include "sp_common.h"

#include <stdint.h>

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int cv_round(double v) { return __double2int_rn(v); }       // saturate_cast<int>(double): half to even
__device__ __forceinline__ int sat_short(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

constexpr int WARP_BATCH = 32;                                // crops per launch: their inverse maps travel as kernel arguments
struct WarpMaps { double m[WARP_BATCH][6]; };

// One output pixel (x, y) of cv.warpAffine for the dst -> src map M: the fixed-point sample position, the four 15-bit weights and
// BORDER_CONSTANT 0.  Shared by every warp kernel so that their pixels cannot drift apart.  `flip`: the source is read as
// np.fliplr(src) - the position is computed in flipped coordinates as usual and only the column index is mirrored at read time
// (c -> W - 1 - c), which gives the bits of warping the flipped image (a flip folded into M would change OpenCV's rounding).
__device__ __forceinline__ void warp_sample_u8c3(const unsigned char* __restrict__ src, int H, int W, bool flip, const double (&M)[6],
                                                 int x, int y, unsigned char (&v)[3]) {
    constexpr int AB_SCALE = 1 << 10, round_delta = AB_SCALE / 32 / 2;
    const int X0 = cv_round((M[1] * y + M[2]) * AB_SCALE) + round_delta;
    const int Y0 = cv_round((M[4] * y + M[5]) * AB_SCALE) + round_delta;
    const int X = (X0 + cv_round(M[0] * x * AB_SCALE)) >> 5, Y = (Y0 + cv_round(M[3] * x * AB_SCALE)) >> 5;
    const int sx = sat_short(X >> 5), sy = sat_short(Y >> 5), fx = X & 31, fy = Y & 31;
    int w0 = (32 - fy) * (32 - fx) * 32, w1 = (32 - fy) * fx * 32, w2 = fy * (32 - fx) * 32, w3 = fy * fx * 32;
    if (w0 == 32768) { w0 = 32767; w3 = 1; }                  // the table's one saturated entry and its correction
    if (sx >= W || sx + 1 < 0 || sy >= H || sy + 1 < 0) { v[0] = 0; v[1] = 0; v[2] = 0; return; }
    const bool x0 = sx >= 0, x1 = sx + 1 < W, y0 = sy >= 0, y1 = sy + 1 < H;
    // columns sx and sx + 1 of the (possibly flipped) image; only read when inside it
    const long long c0 = flip ? W - 1 - sx : sx, step = flip ? -3 : 3;
    const unsigned char* p = src + ((long long)sy * W + c0) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int v0 = (x0 && y0) ? p[k] : 0, v1 = (x1 && y0) ? p[step + k] : 0;
        const int v2 = (x0 && y1) ? p[(long long)W * 3 + k] : 0, v3 = (x1 && y1) ? p[(long long)W * 3 + step + k] : 0;
        const int r = (v0 * w0 + v1 * w1 + v2 * w2 + v3 * w3 + (1 << 14)) >> 15;
        v[k] = (unsigned char)(r < 0 ? 0 : (r > 255 ? 255 : r));
    }
}

__global__ __launch_bounds__(256) void warp_affine_u8c3_kernel(const unsigned char* __restrict__ src, int H, int W, const WarpMaps maps,
                                                               unsigned char* __restrict__ dst, int oh, int ow) {
    const int n = blockIdx.y;
    double M[6];                                              // dst -> src map, inverted on the host exactly as cv::warpAffine does
#pragma unroll
    for (int i = 0; i < 6; ++i) M[i] = maps.m[n][i];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < oh * ow; i += gridDim.x * 256) {
        const int y = i / ow, x = i - y * ow;
        unsigned char v[3];
        warp_sample_u8c3(src, H, W, false, M, x, y, v);
        unsigned char* d = dst + ((size_t)n * oh * ow + i) * 3;
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2];
    }
}

// The body both plan kernels share: slot n's crop of the H x W image S, or zeros when the slot is not live.
__device__ __forceinline__ void plan_slot_u8c3(const unsigned char* __restrict__ S, int H, int W, bool live, const double* __restrict__ m_inv, int n,
                                               unsigned char* __restrict__ dst, int oh, int ow) {
    unsigned char* D = dst + (size_t)n * oh * ow * 3;
    if (!live) {                                              // 16-byte stores where the slot allows it (256 x 192 x 3 B slots do)
        const size_t bytes = (size_t)oh * ow * 3;
        if ((reinterpret_cast<uintptr_t>(D) & 15) == 0 && bytes % 16 == 0) {
            uint4* D4 = reinterpret_cast<uint4*>(D);
            for (size_t i = blockIdx.x * 256 + threadIdx.x; i < bytes / 16; i += (size_t)gridDim.x * 256) D4[i] = make_uint4(0u, 0u, 0u, 0u);
        } else {
            for (size_t i = blockIdx.x * 256 + threadIdx.x; i < bytes; i += (size_t)gridDim.x * 256) D[i] = 0;
        }
        return;
    }
    double M[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) M[i] = m_inv[(size_t)n * 6 + i];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < oh * ow; i += gridDim.x * 256) {
        const int y = i / ow, x = i - y * ow;
        unsigned char v[3];
        warp_sample_u8c3(S, H, W, false, M, x, y, v);
        unsigned char* d = D + (size_t)i * 3;
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2];
    }
}

// The crops of a device-side plan (sp_topdown_plan): slot blockIdx.y reads its map and its source image index from device memory, so
// the launch needs nothing from the host.  Slots from seg[B] on (and any slot whose index is not an image of the batch) are zero-filled.
// Per live crop: out_h * out_w * 3 B written, the 48 B map read, and the box's footprint of the source read once from HBM / L2.
__global__ __launch_bounds__(256) void warp_affine_plan_u8c3_kernel(const unsigned char* __restrict__ src, int B, int H, int W,
                                                                    const double* __restrict__ m_inv, const int* __restrict__ src_index,
                                                                    const int* __restrict__ seg, unsigned char* __restrict__ dst, int oh, int ow) {
    const int n = blockIdx.y;
    const int b = src_index[n];
    const bool live = n < seg[B] && b >= 0 && b < B;
    plan_slot_u8c3(live ? src + (size_t)b * H * W * 3 : src, H, W, live, m_inv, n, dst, oh, ow);
}

// The same for a batch of differently sized images: slot n's source pointer and size come from images[src_index[n]] (sp_image_ref, device
// memory).  A slot whose image has no source or a size outside 1 .. 32767 is zero-filled like a dead slot.
__global__ __launch_bounds__(256) void warp_affine_plan_images_u8c3_kernel(const sp_image_ref* __restrict__ images, int B,
                                                                           const double* __restrict__ m_inv, const int* __restrict__ src_index,
                                                                           const int* __restrict__ seg, unsigned char* __restrict__ dst, int oh,
                                                                           int ow) {
    const int n = blockIdx.y;
    const int b = src_index[n];
    bool live = n < seg[B] && b >= 0 && b < B;
    const unsigned char* S = nullptr;
    int H = 0, W = 0;
    if (live) {
        S = images[b].data; H = images[b].h; W = images[b].w;
        live = S && H > 0 && W > 0 && H <= 32767 && W <= 32767;
    }
    plan_slot_u8c3(S, H, W, live, m_inv, n, dst, oh, ow);
}

// Training batches (RefineSimpleTransform + MSCOCO.collate_fn): every sample has its own source image, size, flip flag and map.
struct WarpSample {
    const unsigned char* src;
    int H, W, flip;
    double m[6];                                              // dst -> src, inverted on the host
};
struct WarpSamples { WarpSample s[WARP_BATCH]; };             // 32 x 72 B: travels as kernel arguments (no upload, graph-capturable)

// One lane per output pixel, x fastest: the three fp32 planes are stored coalesced.  The normalisation is sp_u8hwc_bgr_to_nchw_f32's
// (datasets/coco.py:136: BGR -> RGB, x / 255 - mean).  `crops` (optional): the uint8 HWC crop as sp_warp_affine_u8c3 writes it.
__global__ __launch_bounds__(256) void warp_affine_batch_nchw_kernel(const WarpSamples samples, float* __restrict__ out,
                                                                     unsigned char* __restrict__ crops, int oh, int ow, float m0, float m1,
                                                                     float m2) {
    const int n = blockIdx.y;
    const int hw = oh * ow;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const WarpSample& s = samples.s[n];
    double M[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) M[k] = s.m[k];
    const int y = i / ow, x = i - y * ow;
    unsigned char v[3];
    warp_sample_u8c3(s.src, s.H, s.W, s.flip != 0, M, x, y, v);
    float* o = out + (size_t)n * 3 * hw + i;
    o[0] = (float)v[2] / 255.0f - m0;
    o[hw] = (float)v[1] / 255.0f - m1;
    o[2 * (size_t)hw] = (float)v[0] / 255.0f - m2;
    if (crops) {
        unsigned char* d = crops + ((size_t)n * hw + i) * 3;
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2];
    }
}

}  // namespace

extern "C" int sp_warp_affine_u8c3(const unsigned char* src, int src_h, int src_w, const double* m_fwd_host, int crops, unsigned char* dst,
                                   int out_h, int out_w, void* stream) {
    SP_REQUIRE(src && m_fwd_host && dst, "sp_warp_affine_u8c3: null pointer");
    SP_REQUIRE(src_h > 0 && src_w > 0 && src_h <= 32767 && src_w <= 32767 && crops > 0 && out_h > 0 && out_w > 0,
               "sp_warp_affine_u8c3: bad shape src %dx%d crops=%d out %dx%d", src_h, src_w, crops, out_h, out_w);
    const int blocks = sp_ceil_div((long long)out_h * out_w, 256 * 4);
    for (int c0 = 0; c0 < crops; c0 += WARP_BATCH) {
        const int nb = crops - c0 < WARP_BATCH ? crops - c0 : WARP_BATCH;
        WarpMaps maps;
        for (int n = 0; n < nb; ++n) sp_invert_affine(m_fwd_host + (size_t)(c0 + n) * 6, maps.m[n]);
        hipLaunchKernelGGL(warp_affine_u8c3_kernel, dim3(blocks, nb), dim3(256), 0, (hipStream_t)stream, src, src_h, src_w, maps,
                           dst + (size_t)c0 * out_h * out_w * 3, out_h, out_w);
    }
    return sp_check_launch("warp_affine_u8c3_kernel");
}

extern "C" int sp_warp_affine_plan_u8c3(const unsigned char* src, int batch, int src_h, int src_w, const double* m_inv, const int32_t* src_index,
                                        const int32_t* seg, int capacity, unsigned char* dst, int out_h, int out_w, void* stream) {
    SP_REQUIRE(src && m_inv && src_index && seg && dst, "sp_warp_affine_plan_u8c3: null pointer");
    SP_REQUIRE(batch > 0 && src_h > 0 && src_w > 0 && src_h <= 32767 && src_w <= 32767 && out_h > 0 && out_w > 0 &&
                   (long long)out_h * out_w < (1ll << 28),
               "sp_warp_affine_plan_u8c3: bad shape batch=%d src %dx%d out %dx%d", batch, src_h, src_w, out_h, out_w);
    SP_REQUIRE(capacity >= 1 && capacity <= 2048, "sp_warp_affine_plan_u8c3: capacity %d (1..2048)", capacity);
    const int blocks = sp_ceil_div((long long)out_h * out_w, 256 * 4);
    hipLaunchKernelGGL(warp_affine_plan_u8c3_kernel, dim3(blocks, capacity), dim3(256), 0, (hipStream_t)stream, src, batch, src_h, src_w, m_inv,
                       src_index, seg, dst, out_h, out_w);
    return sp_check_launch("warp_affine_plan_u8c3_kernel");
}

extern "C" int sp_warp_affine_plan_images_u8c3(const sp_image_ref* images_dev, int batch, const double* m_inv, const int32_t* src_index,
                                               const int32_t* seg, int capacity, unsigned char* dst, int out_h, int out_w, void* stream) {
    SP_REQUIRE(images_dev && m_inv && src_index && seg && dst, "sp_warp_affine_plan_images_u8c3: null pointer");
    SP_REQUIRE(batch >= 1 && out_h > 0 && out_w > 0 && (long long)out_h * out_w < (1ll << 28),
               "sp_warp_affine_plan_images_u8c3: bad shape batch=%d (>= 1) out %dx%d", batch, out_h, out_w);
    SP_REQUIRE(capacity >= 1 && capacity <= 2048, "sp_warp_affine_plan_images_u8c3: capacity %d (1..2048)", capacity);
    const int blocks = sp_ceil_div((long long)out_h * out_w, 256 * 4);
    hipLaunchKernelGGL(warp_affine_plan_images_u8c3_kernel, dim3(blocks, capacity), dim3(256), 0, (hipStream_t)stream, images_dev, batch, m_inv,
                       src_index, seg, dst, out_h, out_w);
    return sp_check_launch("warp_affine_plan_images_u8c3_kernel");
}

extern "C" int sp_warp_affine_batch_u8c3_to_nchw_f32(const unsigned char* const* srcs_host, const int* src_hw_host, const int* flip_host,
                                                     const double* m_fwd_host, int batch, int out_h, int out_w, const float* mean_rgb_host,
                                                     float* out, unsigned char* crops, void* stream) {
    SP_REQUIRE(srcs_host && src_hw_host && m_fwd_host && mean_rgb_host && out, "sp_warp_affine_batch_u8c3_to_nchw_f32: null pointer");
    SP_REQUIRE(batch > 0 && out_h > 0 && out_w > 0 && (long long)out_h * out_w < (1ll << 31),
               "sp_warp_affine_batch_u8c3_to_nchw_f32: bad shape batch=%d out %dx%d", batch, out_h, out_w);
    for (int n = 0; n < batch; ++n) {
        const int h = src_hw_host[2 * n], w = src_hw_host[2 * n + 1];
        SP_REQUIRE(srcs_host[n], "sp_warp_affine_batch_u8c3_to_nchw_f32: sample %d: null source", n);
        SP_REQUIRE(h > 0 && w > 0 && h <= 32767 && w <= 32767, "sp_warp_affine_batch_u8c3_to_nchw_f32: sample %d: bad source %dx%d", n, h, w);
    }
    const long long hw = (long long)out_h * out_w;
    const int blocks = sp_ceil_div(hw, 256);
    for (int c0 = 0; c0 < batch; c0 += WARP_BATCH) {
        const int nb = batch - c0 < WARP_BATCH ? batch - c0 : WARP_BATCH;
        WarpSamples s;
        for (int n = 0; n < nb; ++n) {
            WarpSample& d = s.s[n];
            d.src = srcs_host[c0 + n];
            d.H = src_hw_host[2 * (c0 + n)];
            d.W = src_hw_host[2 * (c0 + n) + 1];
            d.flip = flip_host ? (flip_host[c0 + n] != 0) : 0;
            sp_invert_affine(m_fwd_host + (size_t)(c0 + n) * 6, d.m);
        }
        for (int n = nb; n < WARP_BATCH; ++n) s.s[n] = WarpSample{};   // unused slots: defined kernel arguments
        hipLaunchKernelGGL(warp_affine_batch_nchw_kernel, dim3(blocks, nb), dim3(256), 0, (hipStream_t)stream, s, out + (size_t)c0 * 3 * hw,
                           crops ? crops + (size_t)c0 * hw * 3 : nullptr, out_h, out_w, mean_rgb_host[0], mean_rgb_host[1], mean_rgb_host[2]);
    }
    return sp_check_launch("warp_affine_batch_nchw_kernel");
}
