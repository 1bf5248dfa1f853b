// jpeg.hip - baseline JPEG decoding on the device: sp_jpeg_parse (host, no GPU call: sp_jpeg_parse.h) and sp_jpeg_decode_batch, three
// launches (and one that zeroes the coefficients) over a batch of files with mixed sizes and sampling.  Every pixel-defining or byte-touching step is a function of sp_jpeg.h,
// the same code a CPU program runs under the sanitizers; the kernels add only the work split and the addressing, whose bounds the host
// entry point checks against the arena sizes before anything is launched.
//   jpeg_entropy_kernel  one wave per image; serial Huffman decode per restart segment, 64 segments side by side.  Latency bound: a
//                        dependent chain of byte loads and table look-ups per symbol; parallelism = images x restart segments.
//   jpeg_idct_kernel     8 lanes per block, columns then rows through LDS.  2 B in + 1 B out per sample: HBM bound.
//   jpeg_color_kernel    one lane per chroma cell (1x1, 2x1 or 2x2 pixels).  1.5 - 3 B in + 3 B out per pixel: HBM bound.
#include "sp_common.h"

#include <stdint.h>

#include "sp_jpeg.h"
#include "sp_jpeg_parse.h"
#include "sp_jpeg_zero.h"

namespace {

// one set of status bits: the core's names are the header's
static_assert(SP_JPEG_ST_TRUNCATED == SP_JPEG_STATUS_TRUNCATED && SP_JPEG_ST_BAD_CODE == SP_JPEG_STATUS_BAD_CODE && SP_JPEG_ST_BAD_RUN == SP_JPEG_STATUS_BAD_RUN &&
                  SP_JPEG_ST_SEGMENTS == SP_JPEG_STATUS_SEGMENTS && SP_JPEG_ST_BAD_TABLE == SP_JPEG_STATUS_BAD_TABLE,
              "sp_jpeg.h and simple_pose_hip.h disagree on the status bits");

constexpr int IDCT_BLOCKS = 32;                      // 8x8 blocks per 256-thread workgroup
constexpr int WS_PITCH = 9;                          // workspace row pitch in dwords (8 + 1: the row pass reads a column of rows)

struct JpegGeom {
    int bw[3], bh[3];                                // blocks per row / column of each component
    int first[4];                                    // first block of each component in the image's coefficient / plane region; [nc] = total
};

__device__ __forceinline__ JpegGeom jpeg_geom(const sp_jpeg_desc& d) {
    JpegGeom g;
    int acc = 0;
    for (int c = 0; c < 3; ++c) {
        g.bw[c] = c < d.components ? d.mcus_x * d.h_samp[c] : 0;
        g.bh[c] = c < d.components ? d.mcus_y * d.v_samp[c] : 0;
        g.first[c] = acc;
        acc += g.bw[c] * g.bh[c];
    }
    g.first[3] = acc;
    return g;
}

// ---- zero the coefficient regions --------------------------------------------------------------------------------------------------------------
// grid (x, image): the image's own region only (sp_jpeg_zero.h, shared with jpeg_prog.hip)
__global__ __launch_bounds__(256) void jpeg_zero_coef_kernel(const sp_jpeg_desc* __restrict__ descs, int16_t* __restrict__ coef) {
    const sp_jpeg_desc& d = descs[blockIdx.y];
    sp_jpeg_zero_region(coef + d.coef_offset, d.coef_count, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// ---- entropy decode ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const sp_jpeg_desc* __restrict__ descs, const uint8_t* __restrict__ bytes,
                                                          const int32_t* __restrict__ seg_offsets, int16_t* __restrict__ coef,
                                                          int32_t* __restrict__ status) {
    __shared__ sp_jpeg_huff tabs[6];                 // [2 * component + class]
    const sp_jpeg_desc& d = descs[blockIdx.x];
    const int lane = threadIdx.x;
    const int nc = d.components;
    int st = 0;
    if (lane < 2 * nc) {
        const int c = lane >> 1, cls = lane & 1;
        const int t = 4 * cls + ((cls ? d.ac_sel[c] : d.dc_sel[c]) & 3);
        st |= sp_jpeg_huff_build(tabs[lane], d.huff_counts[t], d.huff_values[t], 256);
    }
    __syncthreads();
    for (int t = 0; t < 2 * nc; ++t)
        for (int i = lane; i < (1 << SP_JPEG_LOOKAHEAD); i += 64) tabs[t].lut[i] = sp_jpeg_huff_lut_entry(tabs[t], (uint32_t)i);
    __syncthreads();

    // per-component scalars by name, not arrays indexed by the component: they stay in registers
    const int mcus_x = d.mcus_x, mcus = mcus_x * d.mcus_y;
    const int h0 = d.h_samp[0], v0 = d.v_samp[0];
    const int h1 = nc == 3 ? d.h_samp[1] : 0, v1 = nc == 3 ? d.v_samp[1] : 0, h2 = nc == 3 ? d.h_samp[2] : 0, v2 = nc == 3 ? d.v_samp[2] : 0;
    const int bw0 = mcus_x * h0, bw1 = mcus_x * h1, bw2 = mcus_x * h2;
    const int first1 = bw0 * d.mcus_y * v0, first2 = first1 + bw1 * d.mcus_y * v1;
    const int ri = d.restart_interval > 0 ? d.restart_interval : mcus;               // <= 65535 (host check), mcus <= 2^22
    const int expected = (mcus + ri - 1) / ri;
    const int nseg = d.segments;
    if (lane == 0 && nseg != expected) st |= SP_JPEG_ST_SEGMENTS;
    const uint8_t* file = bytes + d.file_offset;
    const int32_t* segs = seg_offsets + d.seg_index;
    int16_t* out = coef + d.coef_offset;
    const int fbytes = d.file_bytes, ecs_end = d.ecs_end;
    for (int s = lane; s < nseg && s < expected; s += 64) {
        // the segment's bytes, clamped into the file whatever the table says
        const int begin = sp_jpeg_clampi(segs[s], 0, fbytes);
        const int end = sp_jpeg_clampi(s + 1 < nseg ? segs[s + 1] - 2 : ecs_end, begin, fbytes);
        sp_jpeg_bits b;
        sp_jpeg_bits_init(b, file + begin, file + end);
        int32_t pred0 = 0, pred1 = 0, pred2 = 0;
        // the h x v blocks of one component in MCU (mx, my); block index < first + bw * (mcus_y * v): mx < mcus_x, my < mcus_y
        auto component = [&](int first, int bw, int h, int v, const sp_jpeg_huff& dc, const sp_jpeg_huff& ac, int32_t& pred, int mx, int my) {
            for (int vy = 0; vy < v && !b.status; ++vy)
                for (int hx = 0; hx < h && !b.status; ++hx)
                    sp_jpeg_decode_block(b, dc, ac, pred, out + (size_t)(first + (my * v + vy) * bw + mx * h + hx) * 64);
        };
        const int last = min(mcus, (s + 1) * ri);
        for (int mcu = s * ri; mcu < last && !b.status; ++mcu) {
            const int my = mcu / mcus_x, mx = mcu - my * mcus_x;
            component(0, bw0, h0, v0, tabs[0], tabs[1], pred0, mx, my);
            if (nc == 3) {
                component(first1, bw1, h1, v1, tabs[2], tabs[3], pred1, mx, my);
                component(first2, bw2, h2, v2, tabs[4], tabs[5], pred2, mx, my);
            }
        }
        st |= b.status;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) st |= __shfl_xor(st, off, SP_WAVE);
    if (lane == 0) status[blockIdx.x] = st;
}

// ---- dequantise + IDCT ------------------------------------------------------------------------------------------------------------------------
// grid (x, image): workgroup x takes blocks [32 k, 32 k + 32) of the image for k = x, x + gridDim.x, ...; lane j of a block's 8 lanes
// does column j, then row j.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const sp_jpeg_desc* __restrict__ descs, const int16_t* __restrict__ coef,
                                                        uint8_t* __restrict__ planes) {
    __shared__ int32_t ws[IDCT_BLOCKS][8 * WS_PITCH];
    const sp_jpeg_desc& d = descs[blockIdx.y];
    const JpegGeom g = jpeg_geom(d);
    const int total = g.first[3];
    const int sub = threadIdx.x >> 3, j = threadIdx.x & 7;
    const int16_t* in = coef + d.coef_offset;
    uint8_t* pl = planes + d.plane_offset;
    for (int base = blockIdx.x * IDCT_BLOCKS; base < total; base += gridDim.x * IDCT_BLOCKS) {    // uniform trip count: barriers inside
        const int blk = base + sub;
        const bool live = blk < total;
        int c = 0;
        if (live) {
            c = blk >= g.first[2] && d.components == 3 ? 2 : (blk >= g.first[1] && d.components == 3 ? 1 : 0);
            sp_jpeg_idct_column(in + (size_t)blk * 64, d.quant[d.quant_sel[c] & 3], j, ws[sub], WS_PITCH);
        }
        __syncthreads();
        if (live) {
            uint8_t px[8];
            sp_jpeg_idct_row(ws[sub] + j * WS_PITCH, px);
            const int local = blk - g.first[c];
            const int by = local / g.bw[c], bx = local - by * g.bw[c];
            const int pitch = g.bw[c] * 8;
            u32x2 o;
            o[0] = px[0] | (px[1] << 8) | (px[2] << 16) | ((unsigned)px[3] << 24);
            o[1] = px[4] | (px[5] << 8) | (px[6] << 16) | ((unsigned)px[7] << 24);
            // plane_offset % 8 == 0 (checked by the host), every plane is a whole number of 64-byte blocks, pitch and bx * 8 are multiples of 8
            *reinterpret_cast<u32x2*>(pl + (size_t)g.first[c] * 64 + (size_t)(by * 8 + j) * pitch + bx * 8) = o;
        }
        __syncthreads();
    }
}

// ---- upsample + colour ------------------------------------------------------------------------------------------------------------------------
// grid (x, image): one lane per chroma cell of hs x vs pixels (hs, vs = the luma sampling factors), grid-stride over the image's cells.
__global__ __launch_bounds__(256) void jpeg_color_kernel(const sp_jpeg_desc* __restrict__ descs, const uint8_t* __restrict__ planes,
                                                         uint8_t* __restrict__ out) {
    const sp_jpeg_desc& d = descs[blockIdx.y];
    const JpegGeom g = jpeg_geom(d);
    const int W = d.width, H = d.height;
    const int hs = d.h_samp[0], vs = d.v_samp[0];
    const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;          // the downsampled plane (cells)
    const uint8_t* py = planes + d.plane_offset;
    const uint8_t* pcb = py + (size_t)g.first[1] * 64;
    const uint8_t* pcr = py + (size_t)g.first[2] * 64;
    const int ypitch = g.bw[0] * 8, cpitch = g.bw[1] * 8;
    uint8_t* dst = out + d.out_offset;
    const int cells = cw * ch;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < cells; i += gridDim.x * 256) {
        const int cy = i / cw, cx = i - cy * cw;
        for (int dy = 0; dy < vs; ++dy) {
            const int y = cy * vs + dy;
            if (y >= H) break;
            for (int dx = 0; dx < hs; ++dx) {
                const int x = cx * hs + dx;
                if (x >= W) break;
                const int Y = py[(size_t)y * ypitch + x];
                uint8_t* p = dst + ((size_t)y * W + x) * 3;
                if (d.components == 1) {
                    p[0] = p[1] = p[2] = (uint8_t)Y;
                    continue;
                }
                int cb, cr;
                if (hs == 2 && vs == 2) {
                    cb = sp_jpeg_up_h2v2(pcb, cpitch, cw, ch, x, y);
                    cr = sp_jpeg_up_h2v2(pcr, cpitch, cw, ch, x, y);
                } else if (hs == 2) {
                    cb = sp_jpeg_up_h2v1(pcb + (size_t)y * cpitch, cw, x);
                    cr = sp_jpeg_up_h2v1(pcr + (size_t)y * cpitch, cw, x);
                } else {
                    cb = pcb[(size_t)y * cpitch + x];
                    cr = pcr[(size_t)y * cpitch + x];
                }
                sp_jpeg_ycc_to_bgr(Y, cb, cr, p);
            }
        }
    }
}

}  // namespace

extern "C" int sp_jpeg_parse(const uint8_t* data, int64_t size, sp_jpeg_desc* desc, int32_t* seg_offsets, int32_t seg_capacity) {
    char err[256];
    err[0] = 0;
    const int rc = sp_jpeg_parse_impl(data, size, desc, seg_offsets, seg_capacity, err, (int)sizeof(err));
    if (rc != SP_OK) sp_set_error("%s", err);
    return rc;
}

extern "C" int sp_jpeg_decode_batch(const sp_jpeg_desc* descs_host, const sp_jpeg_desc* descs_dev, int count, const uint8_t* bytes, int64_t bytes_size,
                                    const int32_t* seg_offsets, int64_t seg_count, int16_t* coef, int64_t coef_size, uint8_t* planes,
                                    int64_t planes_size, uint8_t* out, int64_t out_size, int32_t* status, int stages, void* stream) {
    SP_REQUIRE(count >= 0 && count <= 65535, "sp_jpeg_decode_batch: count %d (0..65535)", count);
    if (count == 0) return SP_OK;
    // the host descriptors first, the device pointers last: a call with bad sizes is refused whatever the pointers are
    SP_REQUIRE(descs_host, "sp_jpeg_decode_batch: null pointer (descs_host)");
    SP_REQUIRE(stages > 0 && (stages & ~SP_JPEG_STAGE_ALL) == 0, "sp_jpeg_decode_batch: stages %d", stages);
    int64_t max_blocks = 0, max_cells = 0;
    for (int i = 0; i < count; ++i) {
        const sp_jpeg_desc& d = descs_host[i];
        int32_t bw[3], bh[3];
        int64_t blocks = 0;
        SP_REQUIRE(sp_jpeg_geometry(d, bw, bh, blocks), "sp_jpeg_decode_batch: image %d: size %dx%d, %d components or sampling not supported", i, d.width,
                   d.height, d.components);
        SP_REQUIRE(d.coef_count == blocks * 64 && d.plane_bytes == blocks * 64 && d.out_bytes == (int64_t)d.width * d.height * 3,
                   "sp_jpeg_decode_batch: image %d: coef_count / plane_bytes / out_bytes do not follow from the size", i);
        SP_REQUIRE(d.file_bytes >= 0 && d.file_offset >= 0 && d.file_offset + d.file_bytes <= bytes_size,
                   "sp_jpeg_decode_batch: image %d: file bytes [%lld, +%d) outside the %lld-byte buffer", i, (long long)d.file_offset, d.file_bytes,
                   (long long)bytes_size);
        SP_REQUIRE(d.ecs_offset >= 0 && d.ecs_offset <= d.ecs_end && d.ecs_end <= d.file_bytes, "sp_jpeg_decode_batch: image %d: entropy data [%d, %d) outside the file",
                   i, d.ecs_offset, d.ecs_end);
        SP_REQUIRE(d.segments >= 1 && d.seg_index >= 0 && (int64_t)d.seg_index + d.segments <= seg_count,
                   "sp_jpeg_decode_batch: image %d: segments [%d, +%d) outside the %lld-entry table", i, d.seg_index, d.segments, (long long)seg_count);
        SP_REQUIRE(d.restart_interval >= 0 && d.restart_interval <= 65535, "sp_jpeg_decode_batch: image %d: restart interval %d (0..65535)", i,
                   d.restart_interval);
        SP_REQUIRE(d.coef_offset >= 0 && d.coef_offset + d.coef_count <= coef_size, "sp_jpeg_decode_batch: image %d: coefficients outside the arena", i);
        SP_REQUIRE(d.plane_offset >= 0 && d.plane_offset % 8 == 0 && d.plane_offset + d.plane_bytes <= planes_size,
                   "sp_jpeg_decode_batch: image %d: planes outside the arena (or offset not a multiple of 8)", i);
        SP_REQUIRE(d.out_offset >= 0 && d.out_offset + d.out_bytes <= out_size, "sp_jpeg_decode_batch: image %d: output outside the arena", i);
        for (int c = 0; c < d.components; ++c)
            SP_REQUIRE(d.quant_sel[c] >= 0 && d.quant_sel[c] <= 3 && d.dc_sel[c] >= 0 && d.dc_sel[c] <= 3 && d.ac_sel[c] >= 0 && d.ac_sel[c] <= 3,
                       "sp_jpeg_decode_batch: image %d: table selector out of range", i);
        const int hs = d.h_samp[0], vs = d.v_samp[0];
        const int64_t cells = (int64_t)((d.width + hs - 1) / hs) * ((d.height + vs - 1) / vs);
        max_blocks = blocks > max_blocks ? blocks : max_blocks;
        max_cells = cells > max_cells ? cells : max_cells;
    }
    SP_REQUIRE(descs_dev && bytes && seg_offsets && coef && planes && out && status, "sp_jpeg_decode_batch: null pointer");
    SP_REQUIRE(((uintptr_t)planes & 7) == 0 && ((uintptr_t)coef & 1) == 0 && ((uintptr_t)seg_offsets & 3) == 0 && ((uintptr_t)descs_dev & 7) == 0,
               "sp_jpeg_decode_batch: misaligned pointer (planes 8, descs_dev 8, seg_offsets 4, coef 2)");
    const hipStream_t s = (hipStream_t)stream;
    if (stages & SP_JPEG_STAGE_ENTROPY) {
        hipLaunchKernelGGL(jpeg_zero_coef_kernel, dim3(sp_grid_for(max_blocks * 8, 256), count), dim3(256), 0, s, descs_dev, coef);
        const int rz = sp_check_launch("jpeg_zero_coef_kernel");
        if (rz != SP_OK) return rz;
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(count), dim3(64), 0, s, descs_dev, bytes, seg_offsets, coef, status);
        const int rc = sp_check_launch("jpeg_entropy_kernel");
        if (rc != SP_OK) return rc;
    }
    if (stages & SP_JPEG_STAGE_IDCT) {
        const int gx = (int)((max_blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS);
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3(gx > 1024 ? 1024 : gx, count), dim3(256), 0, s, descs_dev, coef, planes);
        const int rc = sp_check_launch("jpeg_idct_kernel");
        if (rc != SP_OK) return rc;
    }
    if (stages & SP_JPEG_STAGE_COLOR) {
        hipLaunchKernelGGL(jpeg_color_kernel, dim3(sp_grid_for(max_cells, 256), count), dim3(256), 0, s, descs_dev, planes, out);
        return sp_check_launch("jpeg_color_kernel");
    }
    return SP_OK;
}
