// jpeg_enc.hip - baseline JPEG encoding on the device: sp_jpeg_enc_plan (host, no GPU call: sp_jpeg_enc_plan.h) and sp_jpeg_encode_batch
// over a batch of images with mixed sizes, sampling and quality.  Every byte-defining step is a function of sp_jpeg_enc.h, the same code a
// CPU program runs under the sanitizers; the kernels add only the work split and the addressing, whose bounds the host entry point checks
// against the arena sizes before anything is launched.  Grids are (x, image); an image with less work than the largest leaves early.
//   jpeg_enc_coef_kernel     one lane per block: 64 (chroma: up to 256) pixels in, 64 int16 + a bit count out.  ALU bound (colour + DCT).
//   jpeg_enc_dcbits_kernel   one lane per block: adds the bits of the DC difference (needs the neighbour's DC, hence its own launch).
//   jpeg_enc_scan_*<KIND>    exclusive prefix sum in three launches: chunk sums, one workgroup per image over the chunk sums, every
//                            chunk again plus its offset.  KIND 0 bits per block, 1 bytes per restart segment, 2 FF bytes of the stream.
//   jpeg_enc_zero_kernel     zeroes the words of the unstuffed stream the emit kernel ORs into.
//   jpeg_enc_emit_kernel     one lane per block: Huffman codes at the block's bit offset, atomic OR on the words blocks share.
//   the apply launch of KIND 2 writes the file: header, stuffed data, restart markers, EOI.
#include "sp_common.h"

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "sp_jpeg_enc.h"
#include "sp_jpeg_enc_plan.h"

namespace {

constexpr int T = SP_JPEG_ENC_CHUNK;                 // threads per workgroup = elements per scan chunk
enum { TOT_BITS = 0, TOT_UBYTES = 1, TOT_FF = 2, TOT_REFUSED = 3 };

// the image's arrays
struct EncCtx {
    uint64_t* totals;
    int16_t* coef;
    uint16_t* bits;
    uint64_t* pos;
    uint64_t* seg;
    uint64_t* chunk;      // chunk sums of scans 0 and 1
    uint64_t* chunk2;     // ... of scan 2
    uint32_t* stream;     // the unstuffed stream, as words
};

__device__ __forceinline__ EncCtx enc_ctx(const sp_jpeg_enc_desc& d, uint8_t* workspace) {
    uint8_t* w = workspace + d.ws_offset;
    EncCtx c;
    c.totals = reinterpret_cast<uint64_t*>(w);
    c.coef = reinterpret_cast<int16_t*>(w + d.ws_coef);
    c.bits = reinterpret_cast<uint16_t*>(w + d.ws_bits);
    c.pos = reinterpret_cast<uint64_t*>(w + d.ws_pos);
    c.seg = reinterpret_cast<uint64_t*>(w + d.ws_seg);
    c.chunk = reinterpret_cast<uint64_t*>(w + d.ws_chunk);
    c.chunk2 = reinterpret_cast<uint64_t*>(w + d.ws_bytes);
    c.stream = reinterpret_cast<uint32_t*>(w + d.ws_bytes + sp_jpeg_enc_stream_chunk_bytes(d.out_capacity));
    return c;
}

// ---- stage coef -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(T) void jpeg_enc_coef_kernel(const sp_jpeg_enc_desc* __restrict__ descs, uint8_t* __restrict__ workspace) {
    const sp_jpeg_enc_desc& d = descs[blockIdx.y];
    const int b = blockIdx.x * T + threadIdx.x;
    if (b >= d.blocks) return;
    const EncCtx c = enc_ctx(d, workspace);
    const sp_jpeg_enc_blk k = sp_jpeg_enc_locate(d, b);
    int16_t zz[64];
    sp_jpeg_enc_block(reinterpret_cast<const uint8_t*>(d.src), d, k, zz);
    u32x4* out = reinterpret_cast<u32x4*>(c.coef + (size_t)b * 64);            // 128-byte aligned: ws_offset and ws_coef are multiples of 64
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        u32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (uint32_t)(uint16_t)zz[i * 8 + 2 * j] | ((uint32_t)(uint16_t)zz[i * 8 + 2 * j + 1] << 16);
        out[i] = v;
    }
    c.bits[b] = (uint16_t)sp_jpeg_enc_ac_bits(zz, d.hlen[k.comp ? 3 : 1]);
}

__global__ __launch_bounds__(T) void jpeg_enc_dcbits_kernel(const sp_jpeg_enc_desc* __restrict__ descs, uint8_t* __restrict__ workspace) {
    const sp_jpeg_enc_desc& d = descs[blockIdx.y];
    const int b = blockIdx.x * T + threadIdx.x;
    if (b >= d.blocks) return;
    const EncCtx c = enc_ctx(d, workspace);
    const sp_jpeg_enc_blk k = sp_jpeg_enc_locate(d, b);
    c.bits[b] = (uint16_t)(c.bits[b] + sp_jpeg_enc_dc_bits(sp_jpeg_enc_dc_diff(c.coef, d, b, k), d.hlen[k.comp ? 2 : 0]));
}

// ---- prefix sums ------------------------------------------------------------------------------------------------------------------------------
// exclusive prefix sum over the T threads of a workgroup (Hillis-Steele through LDS); `total` = the sum.  lds: T uint64.
__device__ __forceinline__ uint64_t enc_block_scan(uint64_t v, uint64_t* lds, uint64_t& total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int o = 1; o < T; o <<= 1) {
        const uint64_t x = t >= o ? lds[t - o] : 0;
        __syncthreads();
        lds[t] += x;
        __syncthreads();
    }
    const uint64_t incl = lds[t];
    total = lds[T - 1];
    __syncthreads();
    return incl - v;
}

// elements of scan KIND in this image (KIND 2: known on the device only; none once the image is refused)
template <int KIND>
__device__ __forceinline__ uint64_t enc_scan_count(const sp_jpeg_enc_desc& d, const EncCtx& c) {
    if (KIND == 0) return (uint64_t)d.blocks;
    if (KIND == 1) return (uint64_t)d.segments;
    return c.totals[TOT_REFUSED] ? 0 : (c.totals[TOT_UBYTES] + SP_JPEG_ENC_LANE_BYTES - 1) / SP_JPEG_ENC_LANE_BYTES;
}

// the 16 stream bytes of element i of scan 2 (bytes at and past `ubytes` read as 0: the words up to the next multiple of 4 are zeroed
// by the emit stage, and nothing past them is read)
__device__ __forceinline__ void enc_stream_bytes(const EncCtx& c, uint64_t i, uint64_t ubytes, uint32_t* w) {
    const uint64_t words = (ubytes + 3) / 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = i * 4 + j < words ? c.stream[i * 4 + j] : 0u;
}

__device__ __forceinline__ int enc_count_ff(uint32_t w) {
    int n = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) n += ((w >> (8 * j)) & 0xFFu) == 0xFFu;
    return n;
}

template <int KIND>
__device__ __forceinline__ uint64_t enc_scan_elem(const sp_jpeg_enc_desc& d, const EncCtx& c, uint64_t i) {
    if (KIND == 0) return c.bits[i];
    if (KIND == 1) {                                   // bytes of restart segment i: its bits rounded up
        int s, first, end;
        sp_jpeg_enc_segment(d, (int)i * (d.restart_interval > 0 ? d.restart_interval * d.blocks_per_mcu : d.blocks), s, first, end);
        return (c.pos[end] - c.pos[first] + 7) / 8;
    }
    uint32_t w[4];
    enc_stream_bytes(c, i, c.totals[TOT_UBYTES], w);   // bytes past ubytes are zero, never FF
    return (uint64_t)(enc_count_ff(w[0]) + enc_count_ff(w[1]) + enc_count_ff(w[2]) + enc_count_ff(w[3]));
}

template <int KIND>
__device__ __forceinline__ uint64_t* enc_scan_chunks(const EncCtx& c) { return KIND == 2 ? c.chunk2 : c.chunk; }

template <int KIND>
__global__ __launch_bounds__(T) void jpeg_enc_scan_reduce_kernel(const sp_jpeg_enc_desc* __restrict__ descs, uint8_t* __restrict__ workspace) {
    __shared__ uint64_t lds[T];
    const sp_jpeg_enc_desc& d = descs[blockIdx.y];
    const EncCtx c = enc_ctx(d, workspace);
    const uint64_t n = enc_scan_count<KIND>(d, c);
    if ((uint64_t)blockIdx.x * T >= n) return;         // uniform over the workgroup
    const uint64_t i = (uint64_t)blockIdx.x * T + threadIdx.x;
    uint64_t total;
    enc_block_scan(i < n ? enc_scan_elem<KIND>(d, c, i) : 0, lds, total);
    if (threadIdx.x == 0) enc_scan_chunks<KIND>(c)[blockIdx.x] = total;
}

// one workgroup per image: the chunk sums become exclusive offsets, T at a time with a carry; then what the total decides
template <int KIND>
__global__ __launch_bounds__(T) void jpeg_enc_scan_chunks_kernel(const sp_jpeg_enc_desc* __restrict__ descs, uint8_t* __restrict__ workspace,
                                                                  int32_t* __restrict__ length, int32_t* __restrict__ status) {
    __shared__ uint64_t lds[T];
    const sp_jpeg_enc_desc& d = descs[blockIdx.x];
    const EncCtx c = enc_ctx(d, workspace);
    const uint64_t chunks = (enc_scan_count<KIND>(d, c) + T - 1) / T;
    uint64_t* sums = enc_scan_chunks<KIND>(c);
    uint64_t carry = 0;
    for (uint64_t base = 0; base < chunks; base += T) {             // uniform trip count: barriers inside
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < chunks ? sums[i] : 0;
        uint64_t total;
        const uint64_t ex = enc_block_scan(v, lds, total);
        if (i < chunks) sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x != 0) return;
    if (KIND == 0) c.totals[TOT_BITS] = carry;
    if (KIND == 1) {
        c.totals[TOT_UBYTES] = carry;
        c.totals[TOT_REFUSED] = carry > (uint64_t)sp_jpeg_enc_stream_cap(d, d.out_capacity);
    }
    if (KIND == 2) {
        c.totals[TOT_FF] = carry;
        const uint64_t bytes = sp_jpeg_enc_file_bytes(d, c.totals[TOT_UBYTES], carry);
        const bool refused = c.totals[TOT_REFUSED] || bytes > (uint64_t)d.out_capacity;
        if (refused) c.totals[TOT_REFUSED] = 1;
        length[blockIdx.x] = refused ? 0 : (int32_t)bytes;           // out_capacity < 2^31 (host check)
        status[blockIdx.x] = refused ? SP_JPEG_ENC_STATUS_OVERFLOW : 0;
    }
}

// every chunk again plus its offset.  KIND 0 -> pos, KIND 1 -> seg (each with the total as one more entry); KIND 2 writes the file.
template <int KIND>
__global__ __launch_bounds__(T) void jpeg_enc_scan_apply_kernel(const sp_jpeg_enc_desc* __restrict__ descs, uint8_t* __restrict__ workspace,
                                                                 uint8_t* __restrict__ out) {
    __shared__ uint64_t lds[T];
    const sp_jpeg_enc_desc& d = descs[blockIdx.y];
    const EncCtx c = enc_ctx(d, workspace);
    if (KIND == 2 && c.totals[TOT_REFUSED]) return;     // set by the launch before this one when the stuffed file does not fit either
    const uint64_t n = enc_scan_count<KIND>(d, c);
    if ((uint64_t)blockIdx.x * T >= n) return;
    const uint64_t i = (uint64_t)blockIdx.x * T + threadIdx.x;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    uint64_t v = 0;
    if (KIND == 2) {
        if (i < n) enc_stream_bytes(c, i, c.totals[TOT_UBYTES], w);
        v = (uint64_t)(enc_count_ff(w[0]) + enc_count_ff(w[1]) + enc_count_ff(w[2]) + enc_count_ff(w[3]));
    } else if (i < n) {
        v = enc_scan_elem<KIND>(d, c, i);
    }
    uint64_t total;
    const uint64_t ex = enc_scan_chunks<KIND>(c)[blockIdx.x] + enc_block_scan(v, lds, total);
    if (KIND != 2) {
        uint64_t* dst = KIND == 0 ? c.pos : c.seg;
        if (i < n) dst[i] = ex;
        if (i + 1 == n) dst[n] = ex + v;
        return;
    }
    uint8_t* file = out + d.out_offset;
    if (blockIdx.x == 0)
        for (int t = threadIdx.x; t < d.header_bytes; t += T) file[t] = d.header[t];
    if (i >= n) return;
    const uint64_t ubytes = c.totals[TOT_UBYTES];
    uint64_t u = i * SP_JPEG_ENC_LANE_BYTES, ff = ex;
    // the segment of the lane's first byte: the last s with seg[s] <= u
    const int nseg = d.segments;
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (c.seg[mid] <= u) lo = mid; else hi = mid - 1;
    }
    int s = lo;
    uint64_t seg_end = c.seg[s + 1];
    for (int j = 0; j < SP_JPEG_ENC_LANE_BYTES && u < ubytes; ++j, ++u) {
        if (u >= seg_end) { ++s; seg_end = c.seg[s + 1]; }          // s + 1 <= nseg: u < ubytes = seg[nseg]
        ff += sp_jpeg_enc_place_byte(file, d.header_bytes, u, ff, s, nseg, seg_end, (uint8_t)(w[j >> 2] >> (8 * (j & 3))));
    }
}

// ---- stage emit -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(T) void jpeg_enc_zero_kernel(const sp_jpeg_enc_desc* __restrict__ descs, uint8_t* __restrict__ workspace) {
    const sp_jpeg_enc_desc& d = descs[blockIdx.y];
    const EncCtx c = enc_ctx(d, workspace);
    if (c.totals[TOT_REFUSED]) return;
    const uint64_t words = (c.totals[TOT_UBYTES] + 3) / 4;            // <= (out_capacity + 3) / 4: inside the stream region
    for (uint64_t i = (uint64_t)blockIdx.x * T + threadIdx.x; i < words; i += (uint64_t)gridDim.x * T) c.stream[i] = 0u;
}

struct EncAtomicOr {
    __device__ void operator()(uint32_t* p, uint32_t v) const { atomicOr(p, v); }
};

__global__ __launch_bounds__(T) void jpeg_enc_emit_kernel(const sp_jpeg_enc_desc* __restrict__ descs, uint8_t* __restrict__ workspace) {
    const sp_jpeg_enc_desc& d = descs[blockIdx.y];
    const int b = blockIdx.x * T + threadIdx.x;
    if (b >= d.blocks) return;
    const EncCtx c = enc_ctx(d, workspace);
    if (c.totals[TOT_REFUSED]) return;
    const sp_jpeg_enc_blk k = sp_jpeg_enc_locate(d, b);
    int s, first, end;
    sp_jpeg_enc_segment(d, b, s, first, end);
    int16_t zz[64];
    const u32x4* in = reinterpret_cast<const u32x4*>(c.coef + (size_t)b * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const u32x4 v = in[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            zz[i * 8 + 2 * j] = (int16_t)(v[j] & 0xFFFFu);
            zz[i * 8 + 2 * j + 1] = (int16_t)(v[j] >> 16);
        }
    }
    sp_jpeg_enc_writer w;
    sp_jpeg_enc_writer_init(w, c.stream, (c.totals[TOT_UBYTES] + 3) / 4, 8 * c.seg[s] + (c.pos[b] - c.pos[first]));
    const int t = k.comp ? 2 : 0;
    sp_jpeg_enc_emit_block(w, zz, sp_jpeg_enc_dc_diff(c.coef, d, b, k), d.hcode[t], d.hlen[t], d.hcode[t + 1], d.hlen[t + 1], b + 1 == end, EncAtomicOr());
}

template <int KIND>
int enc_scan(const sp_jpeg_enc_desc* descs_dev, int count, int64_t max_elems, uint8_t* ws, uint8_t* out, int32_t* length, int32_t* status, hipStream_t s) {
    const dim3 grid(sp_ceil_div(max_elems > 0 ? max_elems : 1, T), count);
    hipLaunchKernelGGL(jpeg_enc_scan_reduce_kernel<KIND>, grid, dim3(T), 0, s, descs_dev, ws);
    int rc = sp_check_launch("jpeg_enc_scan_reduce_kernel");
    if (rc != SP_OK) return rc;
    hipLaunchKernelGGL(jpeg_enc_scan_chunks_kernel<KIND>, dim3(count), dim3(T), 0, s, descs_dev, ws, length, status);
    rc = sp_check_launch("jpeg_enc_scan_chunks_kernel");
    if (rc != SP_OK) return rc;
    hipLaunchKernelGGL(jpeg_enc_scan_apply_kernel<KIND>, grid, dim3(T), 0, s, descs_dev, ws, out);
    return sp_check_launch("jpeg_enc_scan_apply_kernel");
}

}  // namespace

extern "C" int sp_jpeg_enc_plan(int width, int height, int subsampling, int quality, int restart_interval, sp_jpeg_enc_desc* desc) {
    char err[256];
    const int rc = sp_jpeg_enc_plan_impl(width, height, subsampling, quality, restart_interval, desc, err, (int)sizeof(err));
    if (rc != SP_OK) sp_set_error("%s", err);
    return rc;
}

extern "C" int sp_jpeg_encode_batch(const sp_jpeg_enc_desc* descs_host, const sp_jpeg_enc_desc* descs_dev, int count, void* workspace,
                                    int64_t workspace_size, uint8_t* out, int64_t out_size, int32_t* length, int32_t* status, int stages, void* stream) {
    SP_REQUIRE(count >= 0 && count <= 65535, "sp_jpeg_encode_batch: count %d (0..65535)", count);
    if (count == 0) return SP_OK;
    // the host descriptors first, the device pointers last: a call with bad sizes is refused whatever the pointers are
    SP_REQUIRE(descs_host, "sp_jpeg_encode_batch: null pointer (descs_host)");
    SP_REQUIRE(stages > 0 && (stages & ~SP_JPEG_ENC_STAGE_ALL) == 0, "sp_jpeg_encode_batch: stages %d", stages);
    int64_t max_blocks = 0, max_segments = 0, max_cap = 0;
    for (int i = 0; i < count; ++i) {
        const sp_jpeg_enc_desc& d = descs_host[i];
        sp_jpeg_enc_desc plan;
        char err[256];
        SP_REQUIRE(sp_jpeg_enc_plan_impl(d.width, d.height, d.subsampling, d.quality, d.restart_interval, &plan, err, (int)sizeof(err)) == SP_OK &&
                       memcmp(&plan, &d, offsetof(sp_jpeg_enc_desc, src)) == 0,
                   "sp_jpeg_encode_batch: image %d: the descriptor is not what sp_jpeg_enc_plan gives for %dx%d, %d, quality %d, interval %d", i, d.width,
                   d.height, d.subsampling, d.quality, d.restart_interval);
        SP_REQUIRE(d.src != 0, "sp_jpeg_encode_batch: image %d: null pointer (src)", i);
        SP_REQUIRE(d.out_capacity >= 0 && d.out_capacity <= INT32_MAX && d.out_offset >= 0 && d.out_offset <= out_size - d.out_capacity,
                   "sp_jpeg_encode_batch: image %d: output [%lld, +%lld) outside the %lld-byte arena", i, (long long)d.out_offset, (long long)d.out_capacity,
                   (long long)out_size);
        SP_REQUIRE(d.ws_offset >= 0 && d.ws_offset % 64 == 0 && d.ws_offset <= workspace_size - d.ws_bytes - SP_JPEG_ENC_STREAM_WS(d.out_capacity),
                   "sp_jpeg_encode_batch: image %d: workspace [%lld, +%lld) outside the %lld-byte arena (or offset not a multiple of 64)", i,
                   (long long)d.ws_offset, (long long)(d.ws_bytes + SP_JPEG_ENC_STREAM_WS(d.out_capacity)), (long long)workspace_size);
        max_blocks = d.blocks > max_blocks ? d.blocks : max_blocks;
        max_segments = d.segments > max_segments ? d.segments : max_segments;
        max_cap = d.out_capacity > max_cap ? d.out_capacity : max_cap;
    }
    SP_REQUIRE(descs_dev && workspace && out && length && status, "sp_jpeg_encode_batch: null pointer");
    SP_REQUIRE(((uintptr_t)workspace & 63) == 0 && ((uintptr_t)descs_dev & 7) == 0 && ((uintptr_t)length & 3) == 0 && ((uintptr_t)status & 3) == 0,
               "sp_jpeg_encode_batch: misaligned pointer (workspace 64, descs_dev 8, length 4, status 4)");
    const hipStream_t s = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const dim3 per_block(sp_ceil_div(max_blocks, T), count);
    int rc;
    if (stages & SP_JPEG_ENC_STAGE_COEF) {
        hipLaunchKernelGGL(jpeg_enc_coef_kernel, per_block, dim3(T), 0, s, descs_dev, ws);
        if ((rc = sp_check_launch("jpeg_enc_coef_kernel")) != SP_OK) return rc;
        hipLaunchKernelGGL(jpeg_enc_dcbits_kernel, per_block, dim3(T), 0, s, descs_dev, ws);
        if ((rc = sp_check_launch("jpeg_enc_dcbits_kernel")) != SP_OK) return rc;
    }
    if (stages & SP_JPEG_ENC_STAGE_SCAN) {
        if ((rc = enc_scan<0>(descs_dev, count, max_blocks, ws, out, length, status, s)) != SP_OK) return rc;
        if ((rc = enc_scan<1>(descs_dev, count, max_segments, ws, out, length, status, s)) != SP_OK) return rc;
    }
    if (stages & SP_JPEG_ENC_STAGE_EMIT) {
        const int gz = sp_ceil_div((max_cap + 3) / 4 > 0 ? (max_cap + 3) / 4 : 1, T);
        hipLaunchKernelGGL(jpeg_enc_zero_kernel, dim3(gz > 4096 ? 4096 : gz, count), dim3(T), 0, s, descs_dev, ws);
        if ((rc = sp_check_launch("jpeg_enc_zero_kernel")) != SP_OK) return rc;
        hipLaunchKernelGGL(jpeg_enc_emit_kernel, per_block, dim3(T), 0, s, descs_dev, ws);
        if ((rc = sp_check_launch("jpeg_enc_emit_kernel")) != SP_OK) return rc;
    }
    if (stages & SP_JPEG_ENC_STAGE_STUFF)
        return enc_scan<2>(descs_dev, count, (max_cap + SP_JPEG_ENC_LANE_BYTES - 1) / SP_JPEG_ENC_LANE_BYTES, ws, out, length, status, s);
    return SP_OK;
}
