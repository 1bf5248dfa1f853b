// pointwise.hip - HBM-bound layout / pooling / fuse / loss kernels on NHWC tensors, 16 B per lane.
//
// The kernels that exist for both dtypes are `template <bool BF16>` over one 16-byte vector of V = 4 fp32 or 8 bf16 channels: unpack to
// float[V], compute in fp32, pack (= round, in bf16) once.  The `_bf16` entry points are wrappers over the same launchers.
#include "sp_common.h"
#include <type_traits>

namespace {

template <bool BF16>
__device__ __forceinline__ void unpack(const u32x4 q, float* o) {
    if constexpr (BF16) {
        const bf16x8 a = __builtin_bit_cast(bf16x8, q);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (float)a[e];
    } else {
        const f32x4 a = __builtin_bit_cast(f32x4, q);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = a[e];
    }
}

template <bool BF16>
__device__ __forceinline__ u32x4 pack(const float* v) {
    if constexpr (BF16) {
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (__bf16)v[e];
        return __builtin_bit_cast(u32x4, o);
    } else {
        return __builtin_bit_cast(u32x4, f32x4{v[0], v[1], v[2], v[3]});
    }
}

// fp32 NCHW [B,C,H,W] (C <= V) -> NHWC [B,H,W,V] of fp32 or bf16, zero-filled tail channels.  Reads are coalesced along W per plane.
// <false, 4>: the fp32 input layout; <true, 8>: bf16 NHWC8; <true, 4>: bf16 NHWC4 (the bf16 stem reads two neighbouring pixels as one
// 8-channel "pair pixel")
template <bool BF16, int V>
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ x, void* __restrict__ y, int C, int hw, long long total) {
    typedef typename std::conditional<BF16, __bf16, float>::type T;
    typedef T vec_t __attribute__((ext_vector_type(V)));
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / hw;
        const int pix = (int)(i - b * hw);
        const float* src = x + b * C * hw + pix;
        vec_t v;
#pragma unroll
        for (int c = 0; c < V; ++c) v[c] = (T)(c < C ? src[(long long)c * hw] : 0.f);
        reinterpret_cast<vec_t*>(y)[i] = v;
    }
}

// nn.MaxPool2d(3,2,1), NHWC, one lane = V channels of one output pixel; NaN propagates like torch
template <bool BF16>
__global__ void maxpool3x3s2_kernel(const u32x4* __restrict__ x, u32x4* __restrict__ y, int H, int W, int CV, int Ho, int Wo, long long total) {
    constexpr int V = BF16 ? 8 : 4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % CV);
        long long r = i / CV;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const long long b = r / Ho;
        float m[V];
#pragma unroll
        for (int e = 0; e < V; ++e) m[e] = -__builtin_inff();
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * 2 - 1 + ky;
            if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * 2 - 1 + kx;
                if ((unsigned)ix >= (unsigned)W) continue;
                float v[V];
                unpack<BF16>(x[((b * H + iy) * W + ix) * CV + c], v);
#pragma unroll
                for (int e = 0; e < V; ++e) m[e] = sp_pmax(m[e], v[e]);
            }
        }
        y[i] = pack<BF16>(m);
    }
}

// y[b, Y, X, :] = base[b, Y, X, :] + x[b, Y/f, X/f, :]  (nearest upsample + add [+ relu]); base may alias y
template <bool BF16>
__global__ void upsample_add_kernel(const u32x4* __restrict__ x, const u32x4* base, u32x4* y, int h, int w, int CV, int f, int relu, long long total) {
    constexpr int V = BF16 ? 8 : 4;
    const int W = w * f, H = h * f;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % CV);
        long long r = i / CV;
        const int X = (int)(r % W); r /= W;
        const int Y = (int)(r % H);
        const long long b = r / H;
        float a[V], v[V];
        unpack<BF16>(x[((b * h + Y / f) * w + X / f) * CV + c], a);
        unpack<BF16>(base[i], v);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            v[e] += a[e];
            if (relu) v[e] = v[e] > 0.f ? v[e] : 0.f;
        }
        y[i] = pack<BF16>(v);
    }
}

// nn.PixelShuffle(2): y[b,2Y+i,2X+j,k] = x[b,Y,X,4k+2i+j]; one lane gathers V output channels (stride 4 in the source pixel) and stores
// 16 B.  A permutation: the elements are copied, never converted.
template <bool BF16>
__global__ void pixel_shuffle2_kernel(const void* __restrict__ x, u32x4* __restrict__ y, int h, int w, int C, long long total) {
    constexpr int V = BF16 ? 8 : 4;
    typedef typename std::conditional<BF16, __bf16, float>::type T;
    typedef T vec_t __attribute__((ext_vector_type(V)));
    const int CoV = C / (4 * V), W2 = 2 * w, H2 = 2 * h;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int kv = (int)(i % CoV);
        long long r = i / CoV;
        const int X = (int)(r % W2); r /= W2;
        const int Y = (int)(r % H2);
        const long long b = r / H2;
        const int sub = ((Y & 1) << 1) | (X & 1);
        const T* src = reinterpret_cast<const T*>(x) + ((b * h + (Y >> 1)) * w + (X >> 1)) * C + kv * (4 * V) + sub;
        vec_t v;
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = src[4 * e];
        y[i] = __builtin_bit_cast(u32x4, v);
    }
}

// backward of nn.PixelShuffle(2) (a permutation): one lane reads 16 B of dy (4 channels of one output pixel) and scatters them to
// stride-4 channels of the source pixel
__global__ void pixel_unshuffle2_kernel(const f32x4* __restrict__ dy, float* __restrict__ dx, int h, int w, int C, long long total) {
    const int Co = C >> 2, Co4 = Co >> 2, W2 = 2 * w, H2 = 2 * h;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int k4 = (int)(i % Co4);
        long long r = i / Co4;
        const int X = (int)(r % W2); r /= W2;
        const int Y = (int)(r % H2);
        const long long b = r / H2;
        const int sub = ((Y & 1) << 1) | (X & 1);
        float* dst = dx + ((b * h + (Y >> 1)) * w + (X >> 1)) * C + (k4 << 4) + sub;
        const f32x4 v = dy[i];
        dst[0] = v.x; dst[4] = v.y; dst[8] = v.z; dst[12] = v.w;
    }
}

// backward of nn.PixelShuffle(2) on a bf16 gradient (PoseTrainer grad_dtype "bf16", DUC head): gather form - one lane owns 8 consecutive
// channels of a source pixel = output channels k0, k0 + 1 of its four sub-pixels (source channel 4 k + sub), reads four 4-byte pairs and
// stores 16 bytes
__global__ void pixel_unshuffle2_bf16_kernel(const unsigned int* __restrict__ dy, u32x4* __restrict__ dx, int h, int w, int C, long long total) {
    const int C8 = C >> 3, Co = C >> 2, W2 = 2 * w;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c8 = (int)(i % C8);
        long long r = i / C8;
        const int x = (int)(r % w); r /= w;
        const int y = (int)(r % h);
        const long long b = r / h;
        const int k0 = c8 << 1;                       // output channels k0, k0 + 1
        unsigned int pr[4];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const long long o = ((b * 2 * h + (2 * y + (sub >> 1))) * W2 + (2 * x + (sub & 1))) * Co + k0;
            pr[sub] = dy[o >> 1];                     // (k0 is even: the pair is 4-byte aligned)
        }
        u32x4 v;                                      // source order: (k0,0) (k0,1) (k0,2) (k0,3) (k0+1,0) ... (k0+1,3)
        v[0] = (pr[0] & 0xffffu) | (pr[1] << 16);
        v[1] = (pr[2] & 0xffffu) | (pr[3] << 16);
        v[2] = (pr[0] >> 16) | (pr[1] & 0xffff0000u);
        v[3] = (pr[2] >> 16) | (pr[3] & 0xffff0000u);
        dx[i] = v;
    }
}

// HRNet fuse stage, all upsampled terms of one output in ONE pass (round 4):  y = [relu]( ((base + up(x0, f0)) + up(x1, f1)) + up(x2, f2) )
// - `y = y + fuse_layers[i][j](x[j])` for j >= i of HighResolutionModule.forward (pose_hrnet.py:250-257), f = 1 being the identity term.
// The chained form ran one launch per term, each reading and re-writing the high-resolution sum (and, in bf16, rounding it every time);
// here base and every term are read once, the sum is formed in fp32 in the reference's order and rounded once.  fp32: same bits as the chain.
struct UpTerms {
    const void* x[3];
    int h[3], w[3], f[3];
    int n;
};
template <bool BF16>
__global__ void upsample_add_n_kernel(const void* __restrict__ base, const UpTerms t, void* __restrict__ y, int H, int W, int CV, int relu,
                                      long long total) {
    constexpr int V = BF16 ? 8 : 4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % CV);
        long long r = i / CV;
        const int X = (int)(r % W); r /= W;
        const int Y = (int)(r % H);
        const long long b = r / H;
        float v[V];
        u32x4 raw[4];
        raw[0] = reinterpret_cast<const u32x4*>(base)[i];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < t.n) raw[k + 1] = reinterpret_cast<const u32x4*>(t.x[k])[((b * t.h[k] + Y / t.f[k]) * t.w[k] + X / t.f[k]) * CV + c];
        unpack<BF16>(raw[0], v);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < t.n) {
                float a[V];
                unpack<BF16>(raw[k + 1], a);
#pragma unroll
                for (int e = 0; e < V; ++e) v[e] += a[e];
            }
        if (relu) {
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
        }
        reinterpret_cast<u32x4*>(y)[i] = pack<BF16>(v);
    }
}

// SELayer squeeze (nets/commons.py:8,15): y[b, c] = mean over the HW pixels of x[b, :, c].  One workgroup per (b, slab of up to 64
// vector lanes) x 4 pixel stripes, fp64 accumulation in a fixed order; the result in the tensor's dtype (bf16: the two FCs run as bf16
// 1x1 convolutions on the [B,1,1,C] tensor)
template <bool BF16>
__global__ __launch_bounds__(256) void global_avg_pool_kernel(const u32x4* __restrict__ x, void* __restrict__ y, int HW, int CV) {
    constexpr int V = BF16 ? 8 : 4;
    const int b = blockIdx.y;
    const int lanes_c = CV < 64 ? CV : 64;
    const int stripes = 256 / lanes_c;
    const int tc = threadIdx.x % lanes_c, ts = threadIdx.x / lanes_c;
    const int cv = blockIdx.x * lanes_c + tc;
    __shared__ double sm[256 * V];
    double acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0;
    if (cv < CV && ts < stripes)
        for (int p = ts; p < HW; p += stripes) {
            float v[V];
            unpack<BF16>(x[((size_t)b * HW + p) * CV + cv], v);
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] += (double)v[e];
        }
#pragma unroll
    for (int e = 0; e < V; ++e) sm[threadIdx.x * V + e] = acc[e];
    __syncthreads();
    if (ts == 0 && cv < CV) {
        for (int k = 1; k < stripes; ++k)
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] += sm[(k * lanes_c + tc) * V + e];
        float o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = (float)(acc[e] / (double)HW);
        if constexpr (BF16) {
            reinterpret_cast<u32x4*>(y)[(size_t)b * CV + cv] = pack<true>(o);
        } else {                                       // (scalar stores: the fp32 result need not be 16-byte aligned)
#pragma unroll
            for (int e = 0; e < 4; ++e) reinterpret_cast<float*>(y)[((size_t)b * CV + cv) * 4 + e] = o[e];
        }
    }
}

// SELayer excite + block tail: y = relu(x * sigmoid(g[b, c]) + identity)   (nets/commons.py:17-18, pose_resnet_dconv.py:126-131),
// fp32 arithmetic in either dtype
template <bool BF16>
__global__ void se_gate_add_relu_kernel(const u32x4* __restrict__ x, const u32x4* __restrict__ g, const u32x4* __restrict__ idn,
                                        u32x4* __restrict__ y, int HW, int CV, long long total) {
    constexpr int V = BF16 ? 8 : 4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cv = (int)(i % CV);
        const long long b = i / ((long long)HW * CV);
        float gv[V], v[V], r[V], o[V];
        unpack<BF16>(g[b * CV + cv], gv);
        unpack<BF16>(x[i], v);
        unpack<BF16>(idn[i], r);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float sg = 1.f / (1.f + expf(-gv[e]));
            const float t = v[e] * sg + r[e];
            o[e] = t > 0.f ? t : 0.f;
        }
        y[i] = pack<BF16>(o);
    }
}

// datasets/coco.py:136 collate normalisation on the GPU: BGR u8 HWC -> RGB fp32 NCHW, x/255 - mean[c] (no std division)
__global__ void u8hwc_bgr_to_nchw_kernel(const unsigned char* __restrict__ img, float* __restrict__ out, int hw, float m0, float m1, float m2,
                                         long long total) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / hw;
        const int pix = (int)(i - b * hw);
        const unsigned char* p = img + i * 3;
        float* o = out + b * 3 * hw + pix;
        o[0] = (float)p[2] / 255.0f - m0;
        o[hw] = (float)p[1] / 255.0f - m1;
        o[2 * (long long)hw] = (float)p[0] / 255.0f - m2;
    }
}

// The same normalisation straight into the network's input layout: BGR u8 HWC -> RGB NHWC4 fp32 / NHWC8 bf16 (pad channels 0).
// One pass instead of normalise (NCHW fp32) + layout change: 3 B read, 16 B written per pixel.
template <int BF16OUT>   // 0: NHWC4 fp32, 1: NHWC8 bf16, 2: NHWC4 bf16
__global__ void u8hwc_bgr_to_nhwc_kernel(const unsigned char* __restrict__ img, u32x4* __restrict__ out, float m0, float m1, float m2,
                                         long long total) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const unsigned char* p = img + i * 3;
        const float r = (float)p[2] / 255.0f - m0, g = (float)p[1] / 255.0f - m1, b = (float)p[0] / 255.0f - m2;
        if constexpr (BF16OUT == 2) {
            typedef __bf16 bf16x4_ __attribute__((ext_vector_type(4)));
            const bf16x4_ v = {(__bf16)r, (__bf16)g, (__bf16)b, (__bf16)0.f};
            reinterpret_cast<unsigned long long*>(out)[i] = __builtin_bit_cast(unsigned long long, v);
        } else if constexpr (BF16OUT == 1) {
            typedef __bf16 bf16x8_ __attribute__((ext_vector_type(8)));
            bf16x8_ v = {(__bf16)r, (__bf16)g, (__bf16)b, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
            out[i] = __builtin_bit_cast(u32x4, v);
        } else {
            const f32x4 v = {r, g, b, 0.f};
            out[i] = __builtin_bit_cast(u32x4, v);
        }
    }
}

// metrics/pose_metrics.py:212-245 HeatMapAcc on arg-max coordinates: per joint, share of valid samples (label x,y > 1) whose
// normalised distance |pred - label| / (W/f, H/f) is below the threshold; mean over joints that have a valid sample.
__global__ __launch_bounds__(256) void heat_map_acc_kernel(const float* __restrict__ pred, const float* __restrict__ label,
                                                           const float* __restrict__ mask, int B, int J, float nx, float ny, float thresh,
                                                           float* __restrict__ acc) {
    __shared__ float jacc[256];
    __shared__ int jok[256];
    for (int j = threadIdx.x; j < J; j += 256) {
        int valid = 0, hit = 0;
        for (int b = 0; b < B; ++b) {
            // ddp...:130-131 feeds maps multiplied by the joint mask: a zero mask zeroes both maps -> both arg-max cells are (0,0)
            if (mask && mask[b * J + j] == 0.f) continue;
            const float lx = label[(b * J + j) * 2], ly = label[(b * J + j) * 2 + 1];
            if (lx > 1.f && ly > 1.f) {
                const float dx = pred[(b * J + j) * 2] / nx - lx / nx, dy = pred[(b * J + j) * 2 + 1] / ny - ly / ny;
                ++valid;
                if (sqrtf(dx * dx + dy * dy) < thresh) ++hit;
            }
        }
        jok[j] = valid > 0;
        jacc[j] = valid > 0 ? (float)hit / (float)valid : 0.f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        int cnt = 0;
        for (int j = 0; j < J; ++j) if (jok[j]) { s += jacc[j]; ++cnt; }
        *acc = cnt > 0 ? s / (float)cnt : 0.f;
    }
}

// masked MSE: per-block double partial sums (deterministic), then one block folds them.
__global__ void mse_partial_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, const float* __restrict__ mask,
                                   float* __restrict__ grad, int hw, long long total, double inv_n, double* __restrict__ part) {
    double acc = 0.0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const float w = mask[i / hw];
        const float d = pred[i] * w - tgt[i] * w;
        acc += (double)d * (double)d;
        if (grad) grad[i] = (float)((double)d * (double)w * inv_n);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, SP_WAVE);
    __shared__ double wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__global__ void mse_final_kernel(const double* __restrict__ part, int n, double inv_n, float* __restrict__ loss) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) acc += part[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, SP_WAVE);
    if (threadIdx.x == 0) *loss = (float)(0.5 * acc * inv_n);
}

// ---- launchers shared by the fp32 entry point and its `_bf16` twin (same checks; the limits that differ are spelled out) -----------
#define SP_PW_LAUNCH(kernel, total, ...) \
    hipLaunchKernelGGL(kernel, dim3(sp_grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__)

template <bool BF16>
int launch_maxpool(const void* x, void* y, int batch, int h, int w, int c, void* stream) {
    constexpr int V = BF16 ? 8 : 4;
    constexpr const char* fn = BF16 ? "sp_maxpool3x3s2_nhwc_bf16" : "sp_maxpool3x3s2_nhwc";
    SP_REQUIRE(x && y, "%s: null pointer", fn);
    SP_REQUIRE(batch > 0 && h > 0 && w > 0 && c > 0 && c % V == 0, "%s: bad shape (c %% %d != 0?)", fn, V);
    const int ho = (h + 2 - 3) / 2 + 1, wo = (w + 2 - 3) / 2 + 1;
    const long long total = (long long)batch * ho * wo * (c / V);
    SP_REQUIRE((long long)batch * h * w * c < (1ll << (BF16 ? 30 : 31)), "%s: tensor too large", fn);
    SP_PW_LAUNCH(maxpool3x3s2_kernel<BF16>, total, reinterpret_cast<const u32x4*>(x), reinterpret_cast<u32x4*>(y), h, w, c / V, ho, wo, total);
    return sp_check_launch("maxpool3x3s2_kernel");
}

template <bool BF16>
int launch_pixel_shuffle2(const void* x, void* y, int batch, int h, int w, int c, void* stream) {
    constexpr int V = BF16 ? 8 : 4;
    constexpr const char* fn = BF16 ? "sp_pixel_shuffle2_nhwc_bf16" : "sp_pixel_shuffle2_nhwc";
    SP_REQUIRE(x && y, "%s: null pointer", fn);
    SP_REQUIRE(batch > 0 && h > 0 && w > 0 && c > 0 && c % (4 * V) == 0, "%s: c=%d must be a multiple of %d", fn, c, 4 * V);
    const long long total = (long long)batch * h * w * c / V;
    SP_REQUIRE(BF16 || total * 4 < (1ll << 31), "%s: tensor too large", fn);
    SP_PW_LAUNCH(pixel_shuffle2_kernel<BF16>, total, x, reinterpret_cast<u32x4*>(y), h, w, c, total);
    return sp_check_launch("pixel_shuffle2_kernel");
}

template <bool BF16>
int launch_upsample_add(const void* x, const void* base, void* y, int batch, int h, int w, int c, int factor, int relu, void* stream) {
    constexpr int V = BF16 ? 8 : 4;
    constexpr const char* fn = BF16 ? "sp_upsample_add_nhwc_bf16" : "sp_upsample_add_nhwc";
    SP_REQUIRE(x && base && y, "%s: null pointer", fn);
    SP_REQUIRE(batch > 0 && h > 0 && w > 0 && c > 0 && c % V == 0 && factor >= 1, "%s: bad shape", fn);
    const long long total = (long long)batch * h * factor * w * factor * (c / V);
    SP_REQUIRE(BF16 || total * 4 < (1ll << 31), "%s: tensor too large", fn);
    SP_PW_LAUNCH(upsample_add_kernel<BF16>, total, reinterpret_cast<const u32x4*>(x), reinterpret_cast<const u32x4*>(base), reinterpret_cast<u32x4*>(y),
                 h, w, c / V, factor, relu, total);
    return sp_check_launch("upsample_add_kernel");
}

template <bool BF16>
int launch_global_avg_pool(const void* x, void* y, int batch, int hw, int c, void* stream) {
    constexpr int V = BF16 ? 8 : 4;
    constexpr const char* fn = BF16 ? "sp_global_avg_pool_nhwc_bf16" : "sp_global_avg_pool_nhwc";
    SP_REQUIRE(x && y, "%s: null pointer", fn);
    SP_REQUIRE(batch > 0 && hw > 0 && c > 0 && c % V == 0, "%s: bad shape", fn);
    const int cv = c / V, lanes = cv < 64 ? cv : 64;
    hipLaunchKernelGGL(global_avg_pool_kernel<BF16>, dim3((cv + lanes - 1) / lanes, batch), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const u32x4*>(x), y, hw, cv);
    return sp_check_launch("global_avg_pool_kernel");
}

template <bool BF16>
int launch_se_gate_add_relu(const void* x, const void* gate_logits, const void* identity, void* y, int batch, int hw, int c, void* stream) {
    constexpr int V = BF16 ? 8 : 4;
    constexpr const char* fn = BF16 ? "sp_se_gate_add_relu_nhwc_bf16" : "sp_se_gate_add_relu_nhwc";
    SP_REQUIRE(x && gate_logits && identity && y, "%s: null pointer", fn);
    SP_REQUIRE(batch > 0 && hw > 0 && c > 0 && c % V == 0, "%s: bad shape", fn);
    const long long total = (long long)batch * hw * (c / V);
    SP_REQUIRE(total * 16 < (1ll << (BF16 ? 32 : 33)), "%s: tensor too large", fn);      // (fp32: 2^31 elements, bf16: 2^32 bytes)
    SP_PW_LAUNCH(se_gate_add_relu_kernel<BF16>, total, reinterpret_cast<const u32x4*>(x), reinterpret_cast<const u32x4*>(gate_logits),
                 reinterpret_cast<const u32x4*>(identity), reinterpret_cast<u32x4*>(y), hw, c / V, total);
    return sp_check_launch("se_gate_add_relu_kernel");
}

}  // namespace

extern "C" int sp_maxpool3x3s2_nhwc(const float* x, float* y, int batch, int h, int w, int c, void* stream) {
    return launch_maxpool<false>(x, y, batch, h, w, c, stream);
}
extern "C" int sp_maxpool3x3s2_nhwc_bf16(const void* x, void* y, int batch, int h, int w, int c, void* stream) {
    return launch_maxpool<true>(x, y, batch, h, w, c, stream);
}

extern "C" int sp_pixel_shuffle2_nhwc(const float* x, float* y, int batch, int h, int w, int c, void* stream) {
    return launch_pixel_shuffle2<false>(x, y, batch, h, w, c, stream);
}
extern "C" int sp_pixel_shuffle2_nhwc_bf16(const void* x, void* y, int batch, int h, int w, int c, void* stream) {
    return launch_pixel_shuffle2<true>(x, y, batch, h, w, c, stream);
}

extern "C" int sp_upsample_add_nhwc(const float* x, const float* base, float* y, int batch, int h, int w, int c, int factor, int relu, void* stream) {
    return launch_upsample_add<false>(x, base, y, batch, h, w, c, factor, relu, stream);
}
extern "C" int sp_upsample_add_nhwc_bf16(const void* x, const void* base, void* y, int batch, int h, int w, int c, int factor, int relu, void* stream) {
    return launch_upsample_add<true>(x, base, y, batch, h, w, c, factor, relu, stream);
}

extern "C" int sp_global_avg_pool_nhwc(const float* x, float* y, int batch, int hw, int c, void* stream) {
    return launch_global_avg_pool<false>(x, y, batch, hw, c, stream);
}
extern "C" int sp_global_avg_pool_nhwc_bf16(const void* x, void* y, int batch, int hw, int c, void* stream) {
    return launch_global_avg_pool<true>(x, y, batch, hw, c, stream);
}

extern "C" int sp_se_gate_add_relu_nhwc(const float* x, const float* gate_logits, const float* identity, float* y, int batch, int hw, int c, void* stream) {
    return launch_se_gate_add_relu<false>(x, gate_logits, identity, y, batch, hw, c, stream);
}
extern "C" int sp_se_gate_add_relu_nhwc_bf16(const void* x, const void* gate_logits, const void* identity, void* y, int batch, int hw, int c, void* stream) {
    return launch_se_gate_add_relu<true>(x, gate_logits, identity, y, batch, hw, c, stream);
}

extern "C" int sp_nchw_to_nhwc4(const float* x, float* y, int batch, int channels, int h, int w, void* stream) {
    SP_REQUIRE(x && y, "sp_nchw_to_nhwc4: null pointer");
    SP_REQUIRE(batch > 0 && h > 0 && w > 0 && channels >= 1 && channels <= 4, "sp_nchw_to_nhwc4: bad shape B=%d C=%d H=%d W=%d", batch, channels, h, w);
    const long long total = (long long)batch * h * w;
    SP_REQUIRE(total * 4 < (1ll << 31), "sp_nchw_to_nhwc4: tensor too large");
    SP_PW_LAUNCH((nchw_to_nhwc_kernel<false, 4>), total, x, y, channels, h * w, total);
    return sp_check_launch("nchw_to_nhwc_kernel");
}

extern "C" int sp_nchw_to_nhwc8_bf16(const float* x, void* y, int batch, int channels, int h, int w, void* stream) {
    SP_REQUIRE(x && y, "sp_nchw_to_nhwc8_bf16: null pointer");
    SP_REQUIRE(batch > 0 && h > 0 && w > 0 && channels >= 1 && channels <= 8, "sp_nchw_to_nhwc8_bf16: bad shape");
    const long long total = (long long)batch * h * w;
    SP_REQUIRE(total * 8 < (1ll << 30), "sp_nchw_to_nhwc8_bf16: tensor too large");
    SP_PW_LAUNCH((nchw_to_nhwc_kernel<true, 8>), total, x, y, channels, h * w, total);
    return sp_check_launch("nchw_to_nhwc_kernel");
}

extern "C" int sp_nchw_to_nhwc4_bf16(const float* x, void* y, int batch, int channels, int h, int w, void* stream) {
    SP_REQUIRE(x && y, "sp_nchw_to_nhwc4_bf16: null pointer");
    SP_REQUIRE(batch > 0 && h > 0 && w > 0 && w % 2 == 0 && channels >= 1 && channels <= 4, "sp_nchw_to_nhwc4_bf16: bad shape B=%d C=%d H=%d W=%d (W even)",
               batch, channels, h, w);
    const long long total = (long long)batch * h * w;
    SP_REQUIRE(total * 8 < (1ll << 31), "sp_nchw_to_nhwc4_bf16: tensor too large");
    SP_PW_LAUNCH((nchw_to_nhwc_kernel<true, 4>), total, x, y, channels, h * w, total);
    return sp_check_launch("nchw_to_nhwc_kernel");
}

extern "C" int sp_pixel_unshuffle2_nhwc(const float* dy, float* dx, int batch, int h, int w, int c, void* stream) {
    SP_REQUIRE(dy && dx, "sp_pixel_unshuffle2_nhwc: null pointer");
    SP_REQUIRE(batch > 0 && h > 0 && w > 0 && c > 0 && c % 16 == 0, "sp_pixel_unshuffle2_nhwc: c=%d must be a multiple of 16", c);
    const long long total = (long long)batch * h * w * c / 4;
    SP_REQUIRE(total * 4 < (1ll << 31), "sp_pixel_unshuffle2_nhwc: tensor too large");
    hipLaunchKernelGGL(pixel_unshuffle2_kernel, dim3(sp_grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const f32x4*>(dy), dx, h, w, c, total);
    return sp_check_launch("pixel_unshuffle2_kernel");
}

extern "C" int sp_pixel_unshuffle2_nhwc_bf16(const void* dy, void* dx, int batch, int h, int w, int c, void* stream) {
    SP_REQUIRE(dy && dx, "sp_pixel_unshuffle2_nhwc_bf16: null pointer");
    SP_REQUIRE(batch > 0 && h > 0 && w > 0 && c > 0 && c % 32 == 0, "sp_pixel_unshuffle2_nhwc_bf16: c=%d must be a multiple of 32", c);
    const long long total = (long long)batch * h * w * c / 8;
    SP_REQUIRE(total * 8 < (1ll << 31), "sp_pixel_unshuffle2_nhwc_bf16: tensor too large");
    hipLaunchKernelGGL(pixel_unshuffle2_bf16_kernel, dim3(sp_grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned int*>(dy), reinterpret_cast<u32x4*>(dx), h, w, c, total);
    return sp_check_launch("pixel_unshuffle2_bf16_kernel");
}

extern "C" int sp_u8hwc_bgr_to_nchw_f32(const unsigned char* img, float* out, int batch, int h, int w, const float* mean_rgb_host, void* stream) {
    SP_REQUIRE(img && out && mean_rgb_host, "sp_u8hwc_bgr_to_nchw_f32: null pointer");
    SP_REQUIRE(batch > 0 && h > 0 && w > 0, "sp_u8hwc_bgr_to_nchw_f32: bad shape");
    const long long total = (long long)batch * h * w;
    hipLaunchKernelGGL(u8hwc_bgr_to_nchw_kernel, dim3(sp_grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, img, out, h * w,
                       mean_rgb_host[0], mean_rgb_host[1], mean_rgb_host[2], total);
    return sp_check_launch("u8hwc_bgr_to_nchw_kernel");
}

extern "C" int sp_u8hwc_bgr_to_nhwc(const unsigned char* img, void* out, int out_bf16, int batch, int h, int w, const float* mean_rgb_host,
                                    void* stream) {
    SP_REQUIRE(img && out && mean_rgb_host, "sp_u8hwc_bgr_to_nhwc: null pointer");
    SP_REQUIRE(batch > 0 && h > 0 && w > 0, "sp_u8hwc_bgr_to_nhwc: bad shape");
    const long long total = (long long)batch * h * w;
    SP_REQUIRE(total * 16 < (1ll << 31), "sp_u8hwc_bgr_to_nhwc: tensor too large");
    SP_REQUIRE(out_bf16 >= 0 && out_bf16 <= 2 && (out_bf16 != 2 || w % 2 == 0), "sp_u8hwc_bgr_to_nhwc: out_bf16 must be 0, 1 or 2 (2: w even)");
#define SP_U8_LAUNCH(MODE) hipLaunchKernelGGL(u8hwc_bgr_to_nhwc_kernel<MODE>, dim3(sp_grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, img, \
                                              reinterpret_cast<u32x4*>(out), mean_rgb_host[0], mean_rgb_host[1], mean_rgb_host[2], total)
    if (out_bf16 == 2) SP_U8_LAUNCH(2);
    else if (out_bf16 == 1) SP_U8_LAUNCH(1);
    else SP_U8_LAUNCH(0);
#undef SP_U8_LAUNCH
    return sp_check_launch("u8hwc_bgr_to_nhwc_kernel");
}

extern "C" int sp_heat_map_acc(const float* pred_coords, const float* label_coords, const float* mask, int batch, int joints, int h, int w,
                               float distance_thresh, float norm_frac, float* acc_out, void* stream) {
    SP_REQUIRE(pred_coords && label_coords && acc_out, "sp_heat_map_acc: null pointer");
    SP_REQUIRE(batch > 0 && joints > 0 && joints <= 256 && h > 0 && w > 0 && norm_frac > 0.f, "sp_heat_map_acc: bad argument (joints <= 256)");
    hipLaunchKernelGGL(heat_map_acc_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pred_coords, label_coords, mask, batch, joints,
                       (float)w / norm_frac, (float)h / norm_frac, distance_thresh, acc_out);
    return sp_check_launch("heat_map_acc_kernel");
}

extern "C" int sp_upsample_add_n_nhwc(const void* base, int bf16, int n_terms, const void* const* xs, const int32_t* factors, void* y, int batch,
                                      int out_h, int out_w, int c, int relu, void* stream) {
    SP_REQUIRE(base && xs && factors && y, "sp_upsample_add_n_nhwc: null pointer");
    const int vec = bf16 ? 8 : 4;
    SP_REQUIRE(n_terms >= 1 && n_terms <= 3 && batch > 0 && out_h > 0 && out_w > 0 && c > 0 && c % vec == 0,
               "sp_upsample_add_n_nhwc: bad shape (1..3 terms, c %% %d == 0)", vec);
    UpTerms t;
    t.n = n_terms;
    for (int k = 0; k < 3; ++k) { t.x[k] = nullptr; t.h[k] = t.w[k] = t.f[k] = 1; }
    for (int k = 0; k < n_terms; ++k) {
        const int f = factors[k];
        SP_REQUIRE(xs[k] && f >= 1 && out_h % f == 0 && out_w % f == 0, "sp_upsample_add_n_nhwc: term %d: factor %d must divide %dx%d", k, f, out_h, out_w);
        t.x[k] = xs[k]; t.f[k] = f; t.h[k] = out_h / f; t.w[k] = out_w / f;
    }
    const long long total = (long long)batch * out_h * out_w * (c / vec);
    SP_REQUIRE(total * 16 < (1ll << 33), "sp_upsample_add_n_nhwc: tensor too large");
    if (bf16) hipLaunchKernelGGL(upsample_add_n_kernel<true>, dim3(sp_grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, base, t, y, out_h, out_w, c / vec,
                                 relu, total);
    else hipLaunchKernelGGL(upsample_add_n_kernel<false>, dim3(sp_grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, base, t, y, out_h, out_w, c / vec,
                            relu, total);
    return sp_check_launch("upsample_add_n_kernel");
}

extern "C" int sp_masked_mse(const float* pred, const float* target, const float* mask, int batch, int joints, int hw,
                             float* loss_out, float* grad, void* workspace, void* stream) {
    SP_REQUIRE(pred && target && mask && loss_out && workspace, "sp_masked_mse: null pointer");
    SP_REQUIRE(batch > 0 && joints > 0 && hw > 0, "sp_masked_mse: bad shape");
    const long long total = (long long)batch * joints * hw;
    int g = sp_grid_for(total, 256);
    if (g > 512) g = 512;  // workspace holds 512 doubles
    const double inv_n = 1.0 / (double)total;
    hipLaunchKernelGGL(mse_partial_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, pred, target, mask, grad, hw, total, inv_n,
                       reinterpret_cast<double*>(workspace));
    hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<const double*>(workspace), g, inv_n, loss_out);
    return sp_check_launch("mse kernels");
}
