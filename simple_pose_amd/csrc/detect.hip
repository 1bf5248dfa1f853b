// detect.hip - the YOLOv5 person detector's non-convolution launches (fp32): letterbox + Focus input, SPP, slice-to-slice nearest
// upsampling, the head decode and the batched YOLO NMS with merge (detector/yolov5_detector.py, detector/nets/{commons,yolov5}.py), and
// tiled detection's three launches (tiling.py: the letterbox of rectangles of a frame, the scatter into frame coordinates, the fusion).
// The convolutions run on the implicit GEMM (conv_igemm.hip: SP_CONV_HARDSWISH, SP_CONV_OUT_SLICE).
#include "sp_common.h"

#include <stdint.h>

namespace {

// ---- letterbox: OpenCV's 8-bit INTER_LINEAR restated -------------------------------------------------------------------------------------
// fx = (float)((dx + 0.5) * scale - 0.5), sx = floor(fx), fx -= sx, clamped at both borders (fx = 0); coefficients saturate_cast<short>(c * 2048)
// (round half to even) for c = 1 - fx and c = fx separately; rows: S[x0] * a0 + S[x1] * a1 (int), columns: (h0 * b0 + h1 * b1 + 2^21) >> 22.
__device__ __forceinline__ void lin_coef(int d, double scale, int ssize, int& s0, int& s1, int& a0, int& a1) {
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
    s0 = s;
    s1 = s + 1 < ssize ? s + 1 : ssize - 1;
    a0 = __float2int_rn((1.f - f) * 2048.f);
    a1 = __float2int_rn(f * 2048.f);
}

// one image's letterbox: source, resize target and placement on the canvas
struct LbImage {
    const unsigned char* src;
    int sh, sw, nh, nw, top, left;
    int pitch;          // pixels per source row: sw for a contiguous image, the frame's width for a tile of it
    double sy, sx;      // source / destination size ratios (OpenCV's scale_y / scale_x)
    int kind;           // 0 copy, 1 bilinear, 2 INTER_AREA 2x
};

// OpenCV: inv_scale = dsize / ssize, scale = 1 / inv_scale.  Host and device: two IEEE double divisions, the same bits on both
__host__ __device__ __forceinline__ void lb_scales(LbImage& im) {
    im.sx = 1.0 / ((double)im.nw / im.sw);
    im.sy = 1.0 / ((double)im.nh / im.sh);
    im.kind = (im.nh == im.sh && im.nw == im.sw) ? 0 : ((im.sw == 2 * im.nw && im.sh == 2 * im.nh) ? 2 : 1);
}

struct LbArgs {
    LbImage im;         // image 0; image b's source follows at b * sh * sw * 3
    int B, oh, ow, mode;
};

// BGR values of canvas pixel (oy, ox) of one image: the source coefficients are computed once per pixel for its three channels
__device__ __forceinline__ void canvas_px(const LbImage& a, int oy, int ox, int v[3]) {
    const int y = oy - a.top, x = ox - a.left;
    if (y < 0 || y >= a.nh || x < 0 || x >= a.nw) { v[0] = v[1] = v[2] = 114; return; }
    const unsigned char* S = a.src;
    if (a.kind == 0) {
        const unsigned char* p = S + ((size_t)y * a.pitch + x) * 3;
        for (int c = 0; c < 3; ++c) v[c] = p[c];
        return;
    }
    if (a.kind == 2) {
        const unsigned char* p0 = S + ((size_t)(2 * y) * a.pitch + 2 * x) * 3;
        const unsigned char* p1 = p0 + (size_t)a.pitch * 3;
        for (int c = 0; c < 3; ++c) v[c] = (p0[c] + p0[3 + c] + p1[c] + p1[3 + c] + 2) >> 2;
        return;
    }
    int x0, x1, ax0, ax1, y0, y1, by0, by1;
    lin_coef(x, a.sx, a.sw, x0, x1, ax0, ax1);
    lin_coef(y, a.sy, a.sh, y0, y1, by0, by1);
    const unsigned char* R0 = S + (size_t)y0 * a.pitch * 3;
    const unsigned char* R1 = S + (size_t)y1 * a.pitch * 3;
    for (int c = 0; c < 3; ++c) {
        const int h0 = R0[x0 * 3 + c] * ax0 + R0[x1 * 3 + c] * ax1;
        const int h1 = R1[x0 * 3 + c] * ax0 + R1[x1 * 3 + c] * ax1;
        const long long t = ((long long)h0 * by0 + (long long)h1 * by1 + (1ll << 21)) >> 22;
        v[c] = t < 0 ? 0 : (t > 255 ? 255 : (int)t);
    }
}

// output element i of the launch (SP_LETTERBOX_U8: canvas pixel r = oy * ow + ox of its image; SP_LETTERBOX_FOCUS: Focus cell
// r = fy * (ow / 2) + fx), shared by the dense and the table launch
__device__ __forceinline__ void letterbox_store(const LbImage& im, int mode, int ow, int r, long long i, void* out) {
    int px[3];
    if (mode == SP_LETTERBOX_U8) {
        const int oy = r / ow, ox = r - oy * ow;
        unsigned char* o = reinterpret_cast<unsigned char*>(out) + i * 3;
        canvas_px(im, oy, ox, px);
        for (int c = 0; c < 3; ++c) o[c] = (unsigned char)px[c];
        return;
    }
    const int fw = ow / 2, fy = r / fw, fx = r - fy * fw;
    float v[12];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int oy = 2 * fy + (g & 1), ox = 2 * fx + (g >> 1);         // Focus: (::2, ::2), (1::2, ::2), (::2, 1::2), (1::2, 1::2)
        canvas_px(im, oy, ox, px);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[3 * g + c] = (float)px[2 - c] / 255.f;     // BGR -> RGB, .div(255.0)
    }
    f32x4* o = reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + i * 12);
    o[0] = f32x4{v[0], v[1], v[2], v[3]};
    o[1] = f32x4{v[4], v[5], v[6], v[7]};
    o[2] = f32x4{v[8], v[9], v[10], v[11]};
}

__global__ void letterbox_kernel(const LbArgs a, void* out) {
    const long long per = a.mode == SP_LETTERBOX_U8 ? (long long)a.oh * a.ow : (long long)(a.oh / 2) * (a.ow / 2);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.B * per) return;
    const int b = (int)(i / per);
    LbImage im = a.im;
    im.src += (size_t)b * im.sh * im.sw * 3;
    letterbox_store(im, a.mode, a.ow, (int)(i - b * per), i, out);
}

// every image's geometry from the table (sp_image_ref, device memory): differently sized sources on one canvas size.  An entry without a
// source or with an empty size gives an all-padding canvas instead of a read
__global__ void letterbox_images_kernel(const sp_image_ref* __restrict__ images, int B, int oh, int ow, int mode, void* out) {
    const long long per = mode == SP_LETTERBOX_U8 ? (long long)oh * ow : (long long)(oh / 2) * (ow / 2);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * per) return;
    const int b = (int)(i / per);
    const sp_image_ref ref = images[b];
    LbImage im;
    im.src = ref.data; im.sh = ref.h; im.sw = ref.w; im.nh = ref.new_h; im.nw = ref.new_w; im.top = ref.top; im.left = ref.left;
    if (!im.src || im.sh <= 0 || im.sw <= 0 || im.nh <= 0 || im.nw <= 0) { im.nh = im.nw = 0; im.sh = im.sw = 1; }
    im.pitch = im.sw;
    lb_scales(im);
    letterbox_store(im, mode, ow, (int)(i - b * per), i, out);
}

// letterbox_images_kernel for rectangles of larger frames (sp_tile_ref): the row pitch comes from the table, everything else is the same
__global__ void letterbox_tiles_kernel(const sp_tile_ref* __restrict__ tiles, int B, int oh, int ow, int mode, void* out) {
    const long long per = mode == SP_LETTERBOX_U8 ? (long long)oh * ow : (long long)(oh / 2) * (ow / 2);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * per) return;
    const int b = (int)(i / per);
    const sp_tile_ref ref = tiles[b];
    LbImage im;
    im.src = ref.data; im.sh = ref.h; im.sw = ref.w; im.nh = ref.new_h; im.nw = ref.new_w; im.top = ref.top; im.left = ref.left;
    im.pitch = ref.pitch;
    if (!im.src || im.sh <= 0 || im.sw <= 0 || im.nh <= 0 || im.nw <= 0 || im.pitch < im.sw) { im.nh = im.nw = 0; im.sh = im.sw = im.pitch = 1; }
    lb_scales(im);
    letterbox_store(im, mode, ow, (int)(i - b * per), i, out);
}

__global__ void focus_nchw_kernel(const float* __restrict__ x, int B, int h, int w, float* __restrict__ out) {
    const int fh = h / 2, fw = w / 2;
    const long long n = (long long)B * fh * fw;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = (int)(i / ((long long)fh * fw));
    const int r = (int)(i - (long long)b * fh * fw), fy = r / fw, fx = r - fy * fw;
    float v[12];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int y = 2 * fy + (g & 1), xx = 2 * fx + (g >> 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[3 * g + c] = x[(((size_t)b * 3 + c) * h + y) * w + xx];
    }
    f32x4* o = reinterpret_cast<f32x4*>(out + i * 12);
    o[0] = f32x4{v[0], v[1], v[2], v[3]};
    o[1] = f32x4{v[4], v[5], v[6], v[7]};
    o[2] = f32x4{v[8], v[9], v[10], v[11]};
}

// ---- SPP: max pools 5 / 9 / 13 (stride 1, padding k // 2) of slice 0 into slices 1..3; one thread per (pixel, 4 channels) --------------
__global__ void spp_kernel(float* buf, int B, int h, int w, int c, int ct) {
    const int c4 = c / 4;
    const long long n = (long long)B * h * w * c4;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int q = (int)(i % c4);
    const long long pix = i / c4;
    const int b = (int)(pix / ((long long)h * w));
    const int r = (int)(pix - (long long)b * h * w), y = r / w, x = r - y * w;
    const float NEG = -__builtin_huge_valf();
    f32x4 m5 = {NEG, NEG, NEG, NEG}, m9 = m5, m13 = m5;
    for (int dy = -6; dy <= 6; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= h) continue;
        const int ay = dy < 0 ? -dy : dy;
        for (int dx = -6; dx <= 6; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= w) continue;
            const int ax = dx < 0 ? -dx : dx;
            const f32x4 v = *reinterpret_cast<const f32x4*>(buf + (((size_t)b * h + yy) * w + xx) * ct + 4 * q);
            const int rr = ay > ax ? ay : ax;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                m13[e] = fmaxf(m13[e], v[e]);
                if (rr <= 4) m9[e] = fmaxf(m9[e], v[e]);
                if (rr <= 2) m5[e] = fmaxf(m5[e], v[e]);
            }
        }
    }
    float* o = buf + pix * ct + 4 * q;
    *reinterpret_cast<f32x4*>(o + c) = m5;
    *reinterpret_cast<f32x4*>(o + 2 * c) = m9;
    *reinterpret_cast<f32x4*>(o + 3 * c) = m13;
}

__global__ void upsample2_slice_kernel(const float* __restrict__ src, int sct, float* __restrict__ dst, int dct, int B, int h, int w, int c) {
    const int c4 = c / 4, H = 2 * h, W = 2 * w;
    const long long n = (long long)B * H * W * c4;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int q = (int)(i % c4);
    const long long pix = i / c4;
    const int b = (int)(pix / ((long long)H * W));
    const int r = (int)(pix - (long long)b * H * W), y = r / W, x = r - y * W;
    *reinterpret_cast<f32x4*>(dst + pix * dct + 4 * q) =
        *reinterpret_cast<const f32x4*>(src + (((size_t)b * h + y / 2) * w + x / 2) * sct + 4 * q);
}

// ---- head decode -------------------------------------------------------------------------------------------------------------------------
struct HeadArgs {
    const float* in[3];
    int ny[3], nx[3], row0[4];
    float stride[3];
    float anchor[3][4][2];
    int B, A, no, as, N;
};

__global__ void head_decode_kernel(const HeadArgs a, float* __restrict__ out) {
    const long long n = (long long)a.B * a.N;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = (int)(i / a.N), row = (int)(i - (long long)b * a.N);
    const int l = row < a.row0[1] ? 0 : (row < a.row0[2] ? 1 : 2);
    const int ny = a.ny[l], nx = a.nx[l];
    int r = row - a.row0[l];
    const int an = r / (ny * nx);
    r -= an * ny * nx;
    const int y = r / nx, x = r - y * nx;
    const float* v = a.in[l] + (((size_t)b * ny + y) * nx + x) * (a.A * a.as) + an * a.as;
    float* o = out + i * a.no;
    for (int k = 0; k < a.no; ++k) {
#pragma clang fp contract(off)
        const float s = 1.f / (1.f + expf(-v[k]));
        float t;
        if (k < 2) t = (s * 2.f - 0.5f + (float)(k == 0 ? x : y)) * a.stride[l];
        else if (k < 4) { const float u = s * 2.f; t = u * u * a.anchor[l][an][k - 2]; }
        else t = s;
        o[k] = t;
    }
}

// ---- YOLO NMS ----------------------------------------------------------------------------------------------------------------------------
constexpr int CAP = SP_YOLO_NMS_MAX_CANDIDATES;
constexpr int NT = 256;

struct NmsWs {          // per image: [CAP] boxes (x1, y1, x2, y2, not offset), [CAP] (score, cls), [CAP] order; then counts
    float4* box;
    float2* sc;
    int* order;
    int* n_cand;        // [B]
    int* n_out;         // [B]
};

__device__ __forceinline__ float box_iou1(float4 a, float4 b) {
#pragma clang fp contract(off)
    const float area_a = (a.z - a.x) * (a.w - a.y), area_b = (b.z - b.x) * (b.w - b.y);
    const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f), h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
    const float inter = w * h;
    return inter / (area_a + area_b - inter);
}

// candidates of image blockIdx.x in (row, class) order; counts all, stores the first CAP.  `status` (sp_yolo_nms_device; else null): the
// overflow is decided here instead of on the host - bit 0 set and the image's candidate count forced to 0
__global__ __launch_bounds__(NT) void nms_candidates_kernel(const float* __restrict__ pred, int N, int no, float conf, int multi, NmsWs ws,
                                                            int* __restrict__ status) {
    __shared__ int lds[4];
    const int b = blockIdx.x;
    const float* P = pred + (size_t)b * N * no;
    float4* box = ws.box + (size_t)b * CAP;
    float2* sc = ws.sc + (size_t)b * CAP;
    const int nc = no - 5;
    int base = 0;
    for (int r0 = 0; r0 < N; r0 += NT) {
        const int r = r0 + threadIdx.x;
        int cnt = 0, best = 0;
        float obj = 0.f, bestv = 0.f;
        if (r < N) {
            obj = P[(size_t)r * no + 4];
            if (obj > conf) {
                if (multi) {
                    for (int j = 0; j < nc; ++j) cnt += (P[(size_t)r * no + 5 + j] * obj > conf);
                } else {
                    bestv = P[(size_t)r * no + 5] * obj;
                    for (int j = 1; j < nc; ++j) {
                        const float v = P[(size_t)r * no + 5 + j] * obj;
                        if (v > bestv) { bestv = v; best = j; }
                    }
                    cnt = bestv > conf;
                }
            }
        }
        int total;
        int k = base + sp_block_scan256(cnt, lds, total);
        if (cnt) {
            const float* p = P + (size_t)r * no;
            float4 bx;
            {
#pragma clang fp contract(off)
                bx = make_float4(p[0] - p[2] / 2.f, p[1] - p[3] / 2.f, p[0] + p[2] / 2.f, p[1] + p[3] / 2.f);
            }
            if (multi) {
                for (int j = 0; j < nc; ++j) {
                    const float v = p[5 + j] * obj;
                    if (v > conf) {
                        if (k < CAP) { box[k] = bx; sc[k] = make_float2(v, (float)j); }
                        ++k;
                    }
                }
            } else if (k < CAP) {
                box[k] = bx;
                sc[k] = make_float2(bestv, (float)best);
            }
        }
        base += total;
    }
    if (threadIdx.x == 0) {
        if (status) {
            status[b] = base > CAP ? 1 : 0;
            if (base > CAP) base = 0;
        }
        ws.n_cand[b] = base;
    }
}

// descending score, ties to the lower candidate index: order[rank(i)] = i
__global__ __launch_bounds__(NT) void nms_rank_kernel(NmsWs ws) {
    __shared__ float tile[NT];
    const int b = blockIdx.y;
    const int n = ws.n_cand[b];
    if ((int)blockIdx.x * NT >= n) return;
    const float2* sc = ws.sc + (size_t)b * CAP;
    const int i = blockIdx.x * NT + threadIdx.x;
    const float si = i < n ? sc[i].x : 0.f;
    int rank = 0;
    for (int t0 = 0; t0 < n; t0 += NT) {
        const int j = t0 + threadIdx.x;
        tile[threadIdx.x] = j < n ? sc[j].x : 0.f;
        __syncthreads();
        const int lim = n - t0 < NT ? n - t0 : NT;
        for (int jj = 0; jj < lim; ++jj) {
            const float sj = tile[jj];
            rank += (sj > si) || (sj == si && t0 + jj < i);
        }
        __syncthreads();
    }
    if (i < n) ws.order[(size_t)b * CAP + rank] = i;
}

// greedy scan (torchvision.ops.nms order, truncated at max_det), merge, redundancy filter, output
__global__ __launch_bounds__(NT) void nms_select_kernel(NmsWs ws, float iou_thr, int merge, int agnostic, int max_det, float* __restrict__ out,
                                                        int* __restrict__ counts_dev) {
    __shared__ float4 kb[SP_YOLO_NMS_MAX_DET];       // kept boxes (class-offset)
    __shared__ int kidx[SP_YOLO_NMS_MAX_DET];
    __shared__ float4 cb[NT];
    __shared__ int alive[NT];
    __shared__ unsigned long long masks[NT][NT / 64];
    __shared__ int s_nk;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = ws.n_cand[b];
    const float4* box = ws.box + (size_t)b * CAP;
    const float2* sc = ws.sc + (size_t)b * CAP;
    const int* order = ws.order + (size_t)b * CAP;
    auto offset_box = [&](int ci) {
#pragma clang fp contract(off)
        const float4 v = box[ci];
        const float c = agnostic ? 0.f : sc[ci].y * 4096.f;
        return make_float4(v.x + c, v.y + c, v.z + c, v.w + c);
    };
    if (tid == 0) s_nk = 0;
    __syncthreads();
    for (int base = 0; base < n; base += NT) {
        const int nk = s_nk;
        if (nk >= max_det) break;
        const int pos = base + tid;
        const bool valid = pos < n;
        const float4 bx = valid ? offset_box(order[pos]) : make_float4(0.f, 0.f, 0.f, 0.f);
        bool a = valid;
        for (int k = 0; k < nk && a; ++k)
            if (box_iou1(kb[k], bx) > iou_thr) a = false;
        cb[tid] = bx;
        alive[tid] = a;
        __syncthreads();
        unsigned long long m[NT / 64] = {0ull, 0ull, 0ull, 0ull};
        if (a)
            for (int s = 0; s < tid; ++s)
                if (alive[s] && box_iou1(cb[s], bx) > iou_thr) m[s >> 6] |= 1ull << (s & 63);
#pragma unroll
        for (int q = 0; q < NT / 64; ++q) masks[tid][q] = m[q];
        __syncthreads();
        if (tid == 0) {
            unsigned long long keep[NT / 64] = {0ull, 0ull, 0ull, 0ull};
            int k = nk;
            for (int t = 0; t < NT && k < max_det; ++t) {
                if (!alive[t]) continue;
                if ((masks[t][0] & keep[0]) | (masks[t][1] & keep[1]) | (masks[t][2] & keep[2]) | (masks[t][3] & keep[3])) continue;
                keep[t >> 6] |= 1ull << (t & 63);
                kb[k] = cb[t];
                kidx[k] = order[base + t];
                ++k;
            }
            s_nk = k;
        }
        __syncthreads();
    }
    const int nk = s_nk;
    float* O = out + (size_t)b * max_det * 6;
    const bool do_merge = merge && n > 1 && n < 3000;
    // merge: one wave per kept box, lanes over the candidates in index order, fixed butterfly -> deterministic.  The merged box and the
    // redundancy count go back into kb / alive-sized scratch (cb is reused for nothing else from here)
    __shared__ float4 mbox[SP_YOLO_NMS_MAX_DET];
    __shared__ int mcnt[SP_YOLO_NMS_MAX_DET];
    if (do_merge) {
        const int lane = tid & 63, wave = tid >> 6;
        for (int k = wave; k < nk; k += NT / 64) {
            const float4 kbx = kb[k];
            float sw = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
            int cnt = 0;
            for (int j = lane; j < n; j += 64) {
                if (box_iou1(kbx, offset_box(j)) > iou_thr) {
                    const float w = sc[j].x;
                    const float4 v = box[j];
                    sw += w; s0 += w * v.x; s1 += w * v.y; s2 += w * v.z; s3 += w * v.w;
                    ++cnt;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                sw += __shfl_xor(sw, o, 64); s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64);
                s2 += __shfl_xor(s2, o, 64); s3 += __shfl_xor(s3, o, 64); cnt += __shfl_xor(cnt, o, 64);
            }
            if (lane == 0) { mbox[k] = make_float4(s0 / sw, s1 / sw, s2 / sw, s3 / sw); mcnt[k] = cnt; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        int r = 0;
        for (int k = 0; k < nk; ++k) {
            if (do_merge && mcnt[k] <= 1) continue;
            const int ci = kidx[k];
            const float4 v = do_merge ? mbox[k] : box[ci];
            float* o = O + (size_t)r * 6;
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; o[4] = sc[ci].x; o[5] = sc[ci].y;
            ++r;
        }
        ws.n_out[b] = r;
        if (counts_dev) counts_dev[b] = r;                  // sp_yolo_nms_device: the result count stays on the device
    }
}

// clip_coords to the letterboxed image, then the un-letterbox: one detection row (its box columns), shared by both launches below
__device__ __forceinline__ void box_to_source(const float* s, float* d, float img_h, float img_w, float left, float top, float ratio) {
    d[0] = (fminf(fmaxf(s[0], 0.f), img_w) - left) / ratio;
    d[1] = (fminf(fmaxf(s[1], 0.f), img_h) - top) / ratio;
    d[2] = (fminf(fmaxf(s[2], 0.f), img_w) - left) / ratio;
    d[3] = (fminf(fmaxf(s[3], 0.f), img_h) - top) / ratio;
}

__global__ void boxes_to_source_kernel(float* det, int rows, float img_h, float img_w, float left, float top, float ratio) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    float* d = det + (size_t)i * 6;
    box_to_source(d, d, img_h, img_w, left, top, ratio);
}

// one detector group of a mixed batch: block b of the group's NMS output goes, un-letterboxed with image b's own offsets and ratio, to
// block images[b].dst_index of the call-wide arrays; rows from the count on are written as zeros
__global__ void boxes_to_source_images_kernel(const float* __restrict__ det, const int* __restrict__ counts, const int* __restrict__ status,
                                              const sp_image_ref* __restrict__ images, int B, int max_det, float img_h, float img_w,
                                              float* __restrict__ det_all, int* __restrict__ counts_all, int* __restrict__ status_all) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * max_det) return;
    const int b = i / max_det, r = i - b * max_det;
    const sp_image_ref ref = images[b];
    if (ref.dst_index < 0) return;
    const int n = counts[b];
    const float* s = det + (size_t)i * 6;
    float* d = det_all + ((size_t)ref.dst_index * max_det + r) * 6;
    if (r < n) {
        box_to_source(s, d, img_h, img_w, (float)ref.left, (float)ref.top, ref.ratio);
        d[4] = s[4]; d[5] = s[5];
    } else {
        for (int k = 0; k < 6; ++k) d[k] = 0.f;
    }
    if (r == 0) { counts_all[ref.dst_index] = n; status_all[ref.dst_index] = status[b]; }
}

// ---- tiled detection: the passes of a frame (the whole frame, its overlapping tiles) fused on the device --------------------------------
// one net-shape group of passes: pass p's NMS rows go, un-letterboxed and moved by the pass's origin, to block (image, slot) of the
// candidate buffer [frames, passes, max_det, 6]; rows from the count on are written as zeros; the status word is OR-ed into the frame's
__global__ void boxes_to_frame_tiles_kernel(const float* __restrict__ det, const int* __restrict__ counts, const int* __restrict__ status,
                                            const sp_tile_ref* __restrict__ tiles, int n, int passes, int max_det, float img_h, float img_w,
                                            float* __restrict__ cand, int* __restrict__ cand_counts, int* __restrict__ status_frames) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * max_det) return;
    const int p = i / max_det, r = i - p * max_det;
    const sp_tile_ref ref = tiles[p];
    if (ref.image < 0 || ref.slot < 0 || ref.slot >= passes) return;
    const int cnt = counts[p];
    const size_t blk = (size_t)ref.image * passes + ref.slot;
    const float* s = det + (size_t)i * 6;
    float* d = cand + (blk * max_det + r) * 6;
    if (r < cnt) {
#pragma clang fp contract(off)
        float v[4];
        box_to_source(s, v, img_h, img_w, (float)ref.left, (float)ref.top, ref.ratio);
        const float x0 = (float)ref.x0, y0 = (float)ref.y0;
        d[0] = v[0] + x0; d[1] = v[1] + y0; d[2] = v[2] + x0; d[3] = v[3] + y0;
        d[4] = s[4]; d[5] = s[5];
    } else {
        for (int k = 0; k < 6; ++k) d[k] = 0.f;
    }
    if (r == 0) {
        cand_counts[blk] = cnt;
        if (status[p]) atomicOr(status_frames + ref.image, status[p]);
    }
}

// the "candidates from rows" front end of the merge: frame blockIdx.x's blocks in slot order, each block's rows [0, count) in their
// order, packed into the NMS workspace (boxes as they are: the merge compares classes instead of offsetting boxes)
__global__ __launch_bounds__(NT) void merge_candidates_kernel(const float* __restrict__ cand, const int* __restrict__ cand_counts, int passes,
                                                              int max_det, NmsWs ws) {
    __shared__ int start[SP_TILE_MAX_PASSES + 1];
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int p = 0; p < passes; ++p) {
            start[p] = acc;
            const int c = cand_counts[(size_t)b * passes + p];
            acc += c < 0 ? 0 : (c > max_det ? max_det : c);
        }
        start[passes] = acc;
        ws.n_cand[b] = acc;
    }
    __syncthreads();
    float4* box = ws.box + (size_t)b * CAP;
    float2* sc = ws.sc + (size_t)b * CAP;
    for (int i = threadIdx.x; i < passes * max_det; i += NT) {
        const int p = i / max_det, r = i - p * max_det;
        if (r >= start[p + 1] - start[p]) continue;
        const float* s = cand + (((size_t)b * passes + p) * max_det + r) * 6;
        const int k = start[p] + r;                 // < passes * max_det <= CAP (checked on the host)
        box[k] = make_float4(s[0], s[1], s[2], s[3]);
        sc[k] = make_float2(s[4], s[5]);
    }
}

// box_iou1's intersection over the smaller area (IoS); SP_TILE_IOU is box_iou1 itself
__device__ __forceinline__ float box_ios1(float4 a, float4 b) {
#pragma clang fp contract(off)
    const float area_a = (a.z - a.x) * (a.w - a.y), area_b = (b.z - b.x) * (b.w - b.y);
    const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f), h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
    const float inter = w * h;
    return inter / fminf(area_a, area_b);
}

// greedy scan over the ranked candidates, nms_select_kernel's block scheme: a candidate is kept unless an already kept one of its class
// (any class: agnostic) has metric > thresh (a NaN metric compares false and does not suppress); truncated at max_det, rows past the
// count written as zeros
__global__ __launch_bounds__(NT) void merge_select_kernel(NmsWs ws, int metric, float thresh, int agnostic, int max_det, float* __restrict__ out,
                                                          int* __restrict__ counts) {
    __shared__ float4 kb[SP_YOLO_NMS_MAX_DET];
    __shared__ int kcls[SP_YOLO_NMS_MAX_DET];
    __shared__ int kidx[SP_YOLO_NMS_MAX_DET];
    __shared__ float4 cb[NT];
    __shared__ int ccls[NT];
    __shared__ int alive[NT];
    __shared__ unsigned long long masks[NT][NT / 64];
    __shared__ int s_nk;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = ws.n_cand[b];
    const float4* box = ws.box + (size_t)b * CAP;
    const float2* sc = ws.sc + (size_t)b * CAP;
    const int* order = ws.order + (size_t)b * CAP;
    auto hits = [&](float4 k, int kc, float4 c, int cc) {
        if (!agnostic && kc != cc) return false;
        return (metric == SP_TILE_IOS ? box_ios1(k, c) : box_iou1(k, c)) > thresh;
    };
    if (tid == 0) s_nk = 0;
    __syncthreads();
    for (int base = 0; base < n; base += NT) {
        const int nk = s_nk;
        if (nk >= max_det) break;
        const int pos = base + tid;
        int ci = pos < n ? order[pos] : -1;
        const bool valid = ci >= 0 && ci < n;       // (NaN scores leave holes in the ranking: such a position is skipped, never read through)
        if (!valid) ci = 0;
        const float4 bx = valid ? box[ci] : make_float4(0.f, 0.f, 0.f, 0.f);
        const int cls = valid ? (int)sc[ci].y : -1;
        bool a = valid;
        for (int k = 0; k < nk && a; ++k)
            if (hits(kb[k], kcls[k], bx, cls)) a = false;
        cb[tid] = bx;
        ccls[tid] = cls;
        alive[tid] = a;
        __syncthreads();
        unsigned long long m[NT / 64] = {0ull, 0ull, 0ull, 0ull};
        if (a)
            for (int s = 0; s < tid; ++s)
                if (alive[s] && hits(cb[s], ccls[s], bx, cls)) m[s >> 6] |= 1ull << (s & 63);
#pragma unroll
        for (int q = 0; q < NT / 64; ++q) masks[tid][q] = m[q];
        __syncthreads();
        if (tid == 0) {
            unsigned long long keep[NT / 64] = {0ull, 0ull, 0ull, 0ull};
            int k = nk;
            for (int t = 0; t < NT && k < max_det; ++t) {
                if (!alive[t]) continue;
                if ((masks[t][0] & keep[0]) | (masks[t][1] & keep[1]) | (masks[t][2] & keep[2]) | (masks[t][3] & keep[3])) continue;
                keep[t >> 6] |= 1ull << (t & 63);
                kb[k] = cb[t];
                kcls[k] = ccls[t];
                kidx[k] = order[base + t];
                ++k;
            }
            s_nk = k;
        }
        __syncthreads();
    }
    const int nk = s_nk;
    float* O = out + (size_t)b * max_det * 6;
    for (int r = tid; r < max_det; r += NT) {
        float* o = O + (size_t)r * 6;
        if (r < nk) {
            const int ci = kidx[r];
            const float4 v = box[ci];
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; o[4] = sc[ci].x; o[5] = sc[ci].y;
        } else {
            for (int k = 0; k < 6; ++k) o[k] = 0.f;
        }
    }
    if (tid == 0) counts[b] = nk;
}

int64_t nms_ws_layout(int B, NmsWs* ws, void* base) {
    char* p = reinterpret_cast<char*>(base);
    int64_t off = 0;
    auto take = [&](int64_t bytes) { char* q = p ? p + off : nullptr; off += (bytes + 255) / 256 * 256; return q; };
    NmsWs w;
    w.box = reinterpret_cast<float4*>(take((int64_t)B * CAP * 16));
    w.sc = reinterpret_cast<float2*>(take((int64_t)B * CAP * 8));
    w.order = reinterpret_cast<int*>(take((int64_t)B * CAP * 4));
    w.n_cand = reinterpret_cast<int*>(take((int64_t)B * 4));
    w.n_out = reinterpret_cast<int*>(take((int64_t)B * 4));
    if (ws) *ws = w;
    return off;
}

}  // namespace

extern "C" int sp_yolo_letterbox(const unsigned char* src, int batch, int src_h, int src_w, int new_h, int new_w, int top, int left, int out_h,
                                 int out_w, int mode, void* out, void* stream) {
    SP_REQUIRE(src && out, "sp_yolo_letterbox: null pointer");
    SP_REQUIRE(batch > 0 && src_h > 0 && src_w > 0 && new_h > 0 && new_w > 0 && top >= 0 && left >= 0 && top + new_h <= out_h &&
                   left + new_w <= out_w && (long long)batch * out_h * out_w * 12 < (1ll << 31),
               "sp_yolo_letterbox: bad geometry (src %dx%d -> %dx%d at (%d, %d) in %dx%d)", src_h, src_w, new_h, new_w, top, left, out_h, out_w);
    SP_REQUIRE(mode == SP_LETTERBOX_U8 || (mode == SP_LETTERBOX_FOCUS && out_h % 2 == 0 && out_w % 2 == 0),
               "sp_yolo_letterbox: mode %d (Focus output needs an even canvas)", mode);
    LbArgs a;
    a.im.src = src; a.im.sh = src_h; a.im.sw = src_w; a.im.nh = new_h; a.im.nw = new_w; a.im.top = top; a.im.left = left;
    a.im.pitch = src_w;
    lb_scales(a.im);
    a.B = batch; a.oh = out_h; a.ow = out_w; a.mode = mode;
    const long long n = mode == SP_LETTERBOX_U8 ? (long long)batch * out_h * out_w : (long long)batch * (out_h / 2) * (out_w / 2);
    hipLaunchKernelGGL(letterbox_kernel, dim3(sp_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, a, out);
    return sp_check_launch("letterbox_kernel");
}

extern "C" int sp_yolo_letterbox_images(const sp_image_ref* images_dev, int batch, int out_h, int out_w, int mode, void* out, void* stream) {
    SP_REQUIRE(images_dev && out, "sp_yolo_letterbox_images: null pointer");
    SP_REQUIRE(batch >= 1 && out_h > 0 && out_w > 0 && out_h % 2 == 0 && out_w % 2 == 0 && (long long)batch * out_h * out_w * 12 < (1ll << 31),
               "sp_yolo_letterbox_images: batch %d (>= 1), canvas %dx%d (even sizes)", batch, out_h, out_w);
    SP_REQUIRE(mode == SP_LETTERBOX_U8 || mode == SP_LETTERBOX_FOCUS, "sp_yolo_letterbox_images: mode %d", mode);
    const long long n = mode == SP_LETTERBOX_U8 ? (long long)batch * out_h * out_w : (long long)batch * (out_h / 2) * (out_w / 2);
    hipLaunchKernelGGL(letterbox_images_kernel, dim3(sp_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, images_dev, batch, out_h, out_w, mode,
                       out);
    return sp_check_launch("letterbox_images_kernel");
}

extern "C" int sp_yolo_focus_nchw(const float* x, int batch, int h, int w, float* out, void* stream) {
    SP_REQUIRE(x && out, "sp_yolo_focus_nchw: null pointer");
    SP_REQUIRE(batch > 0 && h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0 && (long long)batch * h * w * 3 < (1ll << 31),
               "sp_yolo_focus_nchw: bad shape %dx%dx%d", batch, h, w);
    const long long n = (long long)batch * (h / 2) * (w / 2);
    hipLaunchKernelGGL(focus_nchw_kernel, dim3(sp_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, x, batch, h, w, out);
    return sp_check_launch("focus_nchw_kernel");
}

extern "C" int sp_yolo_spp_nhwc(float* buf, int batch, int h, int w, int c, int c_total, void* stream) {
    SP_REQUIRE(buf, "sp_yolo_spp_nhwc: null pointer");
    SP_REQUIRE(batch > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0 && c_total % 4 == 0 && c_total >= 4 * c &&
                   (long long)batch * h * w * c_total < (1ll << 31),
               "sp_yolo_spp_nhwc: c %d / c_total %d (multiples of 4, c_total >= 4c)", c, c_total);
    const long long n = (long long)batch * h * w * (c / 4);
    hipLaunchKernelGGL(spp_kernel, dim3(sp_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, buf, batch, h, w, c, c_total);
    return sp_check_launch("spp_kernel");
}

extern "C" int sp_upsample2_slice_nhwc(const float* src, int src_c_total, float* dst, int dst_c_total, int batch, int h, int w, int c, void* stream) {
    SP_REQUIRE(src && dst, "sp_upsample2_slice_nhwc: null pointer");
    SP_REQUIRE(batch > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0 && src_c_total % 4 == 0 && dst_c_total % 4 == 0 && c <= src_c_total &&
                   c <= dst_c_total && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0 &&
                   (long long)batch * 4 * h * w * dst_c_total < (1ll << 31),
               "sp_upsample2_slice_nhwc: channels %d of %d -> %d (multiples of 4, 16-byte aligned slices)", c, src_c_total, dst_c_total);
    const long long n = (long long)batch * 4 * h * w * (c / 4);
    hipLaunchKernelGGL(upsample2_slice_kernel, dim3(sp_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, src, src_c_total, dst, dst_c_total,
                       batch, h, w, c);
    return sp_check_launch("upsample2_slice_kernel");
}

extern "C" int sp_yolo_head_decode(const float* head0, const float* head1, const float* head2, int batch, const int* grid_hw, int anchors, int no,
                                   int a_stride, const float* strides, const float* anchor_wh, float* out, void* stream) {
    SP_REQUIRE(head0 && head1 && head2 && grid_hw && strides && anchor_wh && out, "sp_yolo_head_decode: null pointer");
    SP_REQUIRE(batch > 0 && anchors > 0 && anchors <= 4 && no >= 5 && a_stride >= no && a_stride % 4 == 0,
               "sp_yolo_head_decode: anchors %d (1..4), no %d, a_stride %d (>= no, %% 4 == 0)", anchors, no, a_stride);
    HeadArgs a;
    a.in[0] = head0; a.in[1] = head1; a.in[2] = head2;
    a.B = batch; a.A = anchors; a.no = no; a.as = a_stride;
    a.row0[0] = 0;
    for (int l = 0; l < 3; ++l) {
        a.ny[l] = grid_hw[2 * l]; a.nx[l] = grid_hw[2 * l + 1];
        SP_REQUIRE(a.ny[l] > 0 && a.nx[l] > 0, "sp_yolo_head_decode: level %d grid %dx%d", l, a.ny[l], a.nx[l]);
        a.stride[l] = strides[l];
        for (int an = 0; an < 4; ++an)
            for (int k = 0; k < 2; ++k) a.anchor[l][an][k] = an < anchors ? anchor_wh[(l * anchors + an) * 2 + k] : 0.f;
        a.row0[l + 1] = a.row0[l] + anchors * a.ny[l] * a.nx[l];
    }
    a.N = a.row0[3];
    SP_REQUIRE((long long)batch * a.N * no < (1ll << 31), "sp_yolo_head_decode: output too large");
    const long long n = (long long)batch * a.N;
    hipLaunchKernelGGL(head_decode_kernel, dim3(sp_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, a, out);
    return sp_check_launch("head_decode_kernel");
}

extern "C" int sp_yolo_nms_workspace(int batch, int64_t* bytes) {
    SP_REQUIRE(bytes && batch > 0, "sp_yolo_nms_workspace: bad argument");
    *bytes = nms_ws_layout(batch, nullptr, nullptr);
    return SP_OK;
}

extern "C" int sp_yolo_nms(const float* pred, int batch, int n_rows, int no, float conf_thresh, float iou_thresh, int merge, int multi_label,
                           int agnostic, int max_det, void* workspace, int64_t workspace_bytes, float* out, int* counts, int* n_candidates,
                           void* stream) {
    SP_REQUIRE(pred && workspace && out && counts, "sp_yolo_nms: null pointer");
    SP_REQUIRE(batch > 0 && n_rows > 0 && no >= 6 && max_det > 0 && max_det <= SP_YOLO_NMS_MAX_DET && (long long)batch * n_rows * no < (1ll << 31),
               "sp_yolo_nms: batch %d, rows %d, no %d (>= 6), max_det %d (1..%d)", batch, n_rows, no, max_det, SP_YOLO_NMS_MAX_DET);
    NmsWs ws;
    const int64_t need = nms_ws_layout(batch, &ws, workspace);
    SP_REQUIRE(workspace_bytes >= need, "sp_yolo_nms: workspace %lld bytes, need %lld (sp_yolo_nms_workspace)", (long long)workspace_bytes,
               (long long)need);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(nms_candidates_kernel, dim3(batch), dim3(NT), 0, s, pred, n_rows, no, conf_thresh, multi_label ? 1 : 0, ws,
                       (int*)nullptr);
    int rc = sp_check_launch("nms_candidates_kernel");
    if (rc != SP_OK) return rc;
    if (hipMemcpyAsync(counts, ws.n_cand, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        sp_set_error("sp_yolo_nms: reading the candidate counts failed");
        return SP_ELAUNCH;
    }
    int n_max = 0;
    for (int b = 0; b < batch; ++b) {
        SP_REQUIRE(counts[b] <= CAP, "sp_yolo_nms: image %d has %d candidates after the multi-label expansion, above the cap of %d "
                   "(raise conf_thresh)", b, counts[b], CAP);
        n_max = counts[b] > n_max ? counts[b] : n_max;
        if (n_candidates) n_candidates[b] = counts[b];
    }
    if (n_max > 0) {
        hipLaunchKernelGGL(nms_rank_kernel, dim3(sp_ceil_div(n_max, NT), batch), dim3(NT), 0, s, ws);
        rc = sp_check_launch("nms_rank_kernel");
        if (rc != SP_OK) return rc;
    }
    hipLaunchKernelGGL(nms_select_kernel, dim3(batch), dim3(NT), 0, s, ws, iou_thresh, merge ? 1 : 0, agnostic ? 1 : 0, max_det, out,
                       (int*)nullptr);
    rc = sp_check_launch("nms_select_kernel");
    if (rc != SP_OK) return rc;
    if (hipMemcpyAsync(counts, ws.n_out, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        sp_set_error("sp_yolo_nms: reading the result counts failed");
        return SP_ELAUNCH;
    }
    return SP_OK;
}

// sp_yolo_nms with every decision left on the device: nothing here reads a count, so the three launches can be captured
extern "C" int sp_yolo_nms_device(const float* pred, int batch, int n_rows, int no, float conf_thresh, float iou_thresh, int merge, int multi_label,
                                  int agnostic, int max_det, void* workspace, int64_t workspace_bytes, float* out, int32_t* counts, int32_t* status,
                                  void* stream) {
    SP_REQUIRE(pred && workspace && out && counts && status, "sp_yolo_nms_device: null pointer");
    SP_REQUIRE(batch > 0 && n_rows > 0 && no >= 6 && max_det > 0 && max_det <= SP_YOLO_NMS_MAX_DET && (long long)batch * n_rows * no < (1ll << 31),
               "sp_yolo_nms_device: batch %d, rows %d, no %d (>= 6), max_det %d (1..%d)", batch, n_rows, no, max_det, SP_YOLO_NMS_MAX_DET);
    NmsWs ws;
    const int64_t need = nms_ws_layout(batch, &ws, workspace);
    SP_REQUIRE(workspace_bytes >= need, "sp_yolo_nms_device: workspace %lld bytes, need %lld (sp_yolo_nms_workspace)", (long long)workspace_bytes,
               (long long)need);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(nms_candidates_kernel, dim3(batch), dim3(NT), 0, s, pred, n_rows, no, conf_thresh, multi_label ? 1 : 0, ws, status);
    int rc = sp_check_launch("nms_candidates_kernel");
    if (rc != SP_OK) return rc;
    hipLaunchKernelGGL(nms_rank_kernel, dim3(CAP / NT, batch), dim3(NT), 0, s, ws);      // blocks beyond n_cand[b] return at once
    rc = sp_check_launch("nms_rank_kernel");
    if (rc != SP_OK) return rc;
    hipLaunchKernelGGL(nms_select_kernel, dim3(batch), dim3(NT), 0, s, ws, iou_thresh, merge ? 1 : 0, agnostic ? 1 : 0, max_det, out, counts);
    return sp_check_launch("nms_select_kernel");
}

extern "C" int sp_yolo_boxes_to_source(float* det, int rows, float img_h, float img_w, float left, float top, float ratio, void* stream) {
    SP_REQUIRE(det && rows >= 0 && ratio > 0.f, "sp_yolo_boxes_to_source: bad argument");
    if (rows == 0) return SP_OK;
    hipLaunchKernelGGL(boxes_to_source_kernel, dim3(sp_ceil_div(rows, 256)), dim3(256), 0, (hipStream_t)stream, det, rows, img_h, img_w, left, top, ratio);
    return sp_check_launch("boxes_to_source_kernel");
}

extern "C" int sp_yolo_boxes_to_source_images(const float* det_group, const int32_t* counts_group, const int32_t* status_group,
                                              const sp_image_ref* images_dev, int batch, int max_det, float img_h, float img_w, float* det_all,
                                              int32_t* counts_all, int32_t* status_all, void* stream) {
    SP_REQUIRE(det_group && counts_group && status_group && images_dev && det_all && counts_all && status_all,
               "sp_yolo_boxes_to_source_images: null pointer");
    SP_REQUIRE(batch >= 1 && max_det > 0 && max_det <= SP_YOLO_NMS_MAX_DET && img_h > 0.f && img_w > 0.f,
               "sp_yolo_boxes_to_source_images: batch %d (>= 1), max_det %d (1..%d)", batch, max_det, SP_YOLO_NMS_MAX_DET);
    hipLaunchKernelGGL(boxes_to_source_images_kernel, dim3(sp_ceil_div(batch * max_det, 256)), dim3(256), 0, (hipStream_t)stream, det_group,
                       counts_group, status_group, images_dev, batch, max_det, img_h, img_w, det_all, counts_all, status_all);
    return sp_check_launch("boxes_to_source_images_kernel");
}

extern "C" int sp_yolo_letterbox_tiles(const sp_tile_ref* tiles_dev, int batch, int out_h, int out_w, int mode, void* out, void* stream) {
    SP_REQUIRE(tiles_dev && out, "sp_yolo_letterbox_tiles: null pointer");
    SP_REQUIRE(batch >= 1 && out_h > 0 && out_w > 0 && out_h % 2 == 0 && out_w % 2 == 0 && (long long)batch * out_h * out_w * 12 < (1ll << 31),
               "sp_yolo_letterbox_tiles: batch %d (>= 1), canvas %dx%d (even sizes)", batch, out_h, out_w);
    SP_REQUIRE(mode == SP_LETTERBOX_U8 || mode == SP_LETTERBOX_FOCUS, "sp_yolo_letterbox_tiles: mode %d", mode);
    const long long n = mode == SP_LETTERBOX_U8 ? (long long)batch * out_h * out_w : (long long)batch * (out_h / 2) * (out_w / 2);
    hipLaunchKernelGGL(letterbox_tiles_kernel, dim3(sp_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, tiles_dev, batch, out_h, out_w, mode,
                       out);
    return sp_check_launch("letterbox_tiles_kernel");
}

extern "C" int sp_yolo_boxes_to_frame_tiles(const float* det_group, const int32_t* counts_group, const int32_t* status_group,
                                            const sp_tile_ref* tiles_dev, int batch, int passes, int max_det, float img_h, float img_w,
                                            float* cand, int32_t* cand_counts, int32_t* status_frames, void* stream) {
    SP_REQUIRE(det_group && counts_group && status_group && tiles_dev && cand && cand_counts && status_frames,
               "sp_yolo_boxes_to_frame_tiles: null pointer");
    SP_REQUIRE(batch >= 1 && passes >= 1 && passes <= SP_TILE_MAX_PASSES && max_det > 0 && max_det <= SP_YOLO_NMS_MAX_DET && img_h > 0.f &&
                   img_w > 0.f && (long long)batch * max_det < (1ll << 31) / 6,
               "sp_yolo_boxes_to_frame_tiles: batch %d (>= 1), passes %d (1..%d), max_det %d (1..%d)", batch, passes, SP_TILE_MAX_PASSES, max_det,
               SP_YOLO_NMS_MAX_DET);
    hipLaunchKernelGGL(boxes_to_frame_tiles_kernel, dim3(sp_ceil_div(batch * max_det, 256)), dim3(256), 0, (hipStream_t)stream, det_group,
                       counts_group, status_group, tiles_dev, batch, passes, max_det, img_h, img_w, cand, cand_counts, status_frames);
    return sp_check_launch("boxes_to_frame_tiles_kernel");
}

extern "C" int sp_yolo_merge_passes(const float* cand, const int32_t* cand_counts, int frames, int passes, int max_det, int metric, float thresh,
                                    int agnostic, void* workspace, int64_t workspace_bytes, float* det, int32_t* counts, void* stream) {
    SP_REQUIRE(cand && cand_counts && workspace && det && counts, "sp_yolo_merge_passes: null pointer");
    SP_REQUIRE(frames >= 1 && passes >= 1 && passes <= SP_TILE_MAX_PASSES && max_det > 0 && max_det <= SP_YOLO_NMS_MAX_DET &&
                   passes * max_det <= CAP,
               "sp_yolo_merge_passes: frames %d (>= 1), passes %d (1..%d), max_det %d (1..%d), passes * max_det <= %d", frames, passes,
               SP_TILE_MAX_PASSES, max_det, SP_YOLO_NMS_MAX_DET, CAP);
    SP_REQUIRE((metric == SP_TILE_IOU || metric == SP_TILE_IOS) && thresh > 0.f && thresh <= 1.f,
               "sp_yolo_merge_passes: metric %d (SP_TILE_IOU, SP_TILE_IOS), thresh %g (0 < thresh <= 1)", metric, (double)thresh);
    NmsWs ws;
    const int64_t need = nms_ws_layout(frames, &ws, workspace);
    SP_REQUIRE(workspace_bytes >= need, "sp_yolo_merge_passes: workspace %lld bytes, need %lld (sp_yolo_nms_workspace)", (long long)workspace_bytes,
               (long long)need);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(merge_candidates_kernel, dim3(frames), dim3(NT), 0, s, cand, cand_counts, passes, max_det, ws);
    int rc = sp_check_launch("merge_candidates_kernel");
    if (rc != SP_OK) return rc;
    hipLaunchKernelGGL(nms_rank_kernel, dim3(sp_ceil_div(passes * max_det, NT), frames), dim3(NT), 0, s, ws);    // blocks beyond n_cand[b] return at once
    rc = sp_check_launch("nms_rank_kernel");
    if (rc != SP_OK) return rc;
    hipLaunchKernelGGL(merge_select_kernel, dim3(frames), dim3(NT), 0, s, ws, metric, thresh, agnostic ? 1 : 0, max_det, det, counts);
    return sp_check_launch("merge_select_kernel");
}
