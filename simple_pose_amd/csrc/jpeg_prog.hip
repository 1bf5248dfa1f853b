// jpeg_prog.hip - the entropy stage of progressive (SOF2, multi-scan) JPEG files on the device: sp_jpeg_parse_scans (host, no GPU call:
// sp_jpeg_parse_scans.h) and sp_jpeg_progressive_entropy, which fills the coefficient arena that jpeg.hip's IDCT and colour kernels read.
// Every byte-touching step is a function of sp_jpeg.h / sp_jpeg_prog.h, the same code a CPU program runs under the sanitizers; the kernel
// adds the work split, and the host entry point checks every range against the arena sizes before anything is launched.
//   jpeg_prog_entropy_kernel  one 64-lane workgroup per file walks the file's scans in file order; per scan: the scan's Huffman tables
//                             into LDS, then lane s decodes restart segments s, s + 64, ... of that scan.  Latency bound like the baseline
//                             kernel, and serial over the scans of a file; parallelism = files x restart segments of one scan.
#include "sp_common.h"

#include <stdint.h>

#include "sp_jpeg.h"
#include "sp_jpeg_parse_scans.h"
#include "sp_jpeg_prog.h"
#include "sp_jpeg_zero.h"

namespace {

constexpr int MAX_SCANS = 256;                       // scans per file (libjpeg-turbo's own scripts have 6 or 10)

// grid (x, file): the file's own coefficient region only
__global__ __launch_bounds__(256) void jpeg_prog_zero_coef_kernel(const sp_jpeg_desc* __restrict__ descs, int16_t* __restrict__ coef) {
    const sp_jpeg_desc& d = descs[blockIdx.y];
    sp_jpeg_zero_region(coef + d.coef_offset, d.coef_count, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// `coef` is read and written (refinement scans), by different lanes in different scans: no __restrict__ on it.
__global__ __launch_bounds__(64) void jpeg_prog_entropy_kernel(const sp_jpeg_desc* __restrict__ descs, const sp_jpeg_scan* __restrict__ scans,
                                                               const int32_t* __restrict__ scan_range, const uint8_t* __restrict__ bytes,
                                                               const int32_t* __restrict__ seg_offsets, int16_t* coef, int32_t* __restrict__ status) {
    __shared__ sp_jpeg_huff tabs[3];                 // the tables of the scan in hand (sp_jpeg_prog_tables of them)
    const sp_jpeg_desc& d = descs[blockIdx.x];
    const int lane = threadIdx.x;
    const uint8_t* file = bytes + d.file_offset;
    const int32_t* segs = seg_offsets + d.seg_index;
    int16_t* out = coef + d.coef_offset;
    const int fbytes = d.file_bytes;
    const int scan_begin = scan_range[blockIdx.x], scan_end = min(scan_range[blockIdx.x + 1], scan_begin + MAX_SCANS);
    int st = 0;
    for (int sc = scan_begin; sc < scan_end; ++sc) {             // uniform over the workgroup: barriers inside
        const sp_jpeg_scan& s = scans[sc];
        sp_jpeg_prog_geom g;
        sp_jpeg_prog_geometry(d, s, g);
        const int ntab = sp_jpeg_prog_tables(g);
        if (lane < ntab) st |= sp_jpeg_huff_build(tabs[lane], s.huff_counts[lane], s.huff_values[lane], 256);
        __syncthreads();
        for (int t = 0; t < ntab; ++t)
            for (int i = lane; i < (1 << SP_JPEG_LOOKAHEAD); i += 64) tabs[t].lut[i] = sp_jpeg_huff_lut_entry(tabs[t], (uint32_t)i);
        __syncthreads();
        const int ri = sp_jpeg_prog_interval(g, s.restart_interval);                 // <= 65535 (host check), g.mcus <= 2^22
        const int expected = (g.mcus + ri - 1) / ri;
        const int nseg = s.segments;
        if (lane == 0 && nseg != expected) st |= SP_JPEG_ST_SEGMENTS;
        const int32_t* ssegs = segs + s.seg_index;
        for (int k = lane; k < nseg && k < expected; k += 64) {
            // the segment's bytes, clamped into the file whatever the table says
            const int begin = sp_jpeg_clampi(ssegs[k], 0, fbytes);
            const int end = sp_jpeg_clampi(k + 1 < nseg ? ssegs[k + 1] - 2 : s.ecs_end, begin, fbytes);
            st |= sp_jpeg_prog_segment(file + begin, file + end, tabs, g, k * ri, min(g.mcus, (k + 1) * ri), out);
        }
        // The end of the scan.  A refinement scan reads the coefficients that earlier scans wrote to global memory, in general from other
        // lanes (the segments of two scans split the blocks differently); all of it happens inside this one workgroup, so the workgroup
        // barrier (with its fence) orders those writes before the next scan's reads.  It also keeps `tabs` until every lane is done.
        __syncthreads();
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) st |= __shfl_xor(st, off, SP_WAVE);
    if (lane == 0) status[blockIdx.x] = st;
}

}  // namespace

extern "C" int sp_jpeg_parse_scans(const uint8_t* data, int64_t size, sp_jpeg_desc* desc, sp_jpeg_scan* scans, int32_t scan_capacity,
                                   int32_t* scan_count, int32_t* seg_offsets, int32_t seg_capacity) {
    char err[256];
    err[0] = 0;
    const int rc = sp_jpeg_parse_scans_impl(data, size, desc, scans, scan_capacity, scan_count, seg_offsets, seg_capacity, err, (int)sizeof(err));
    if (rc != SP_OK) sp_set_error("%s", err);
    return rc;
}

extern "C" int sp_jpeg_progressive_entropy(const sp_jpeg_desc* descs_host, const sp_jpeg_desc* descs_dev, int count, const sp_jpeg_scan* scans_host,
                                           const sp_jpeg_scan* scans_dev, const int32_t* scan_range_host, const int32_t* scan_range_dev,
                                           int64_t scan_total, const uint8_t* bytes, int64_t bytes_size, const int32_t* seg_offsets, int64_t seg_count,
                                           int16_t* coef, int64_t coef_size, int32_t* status, void* stream) {
    SP_REQUIRE(count >= 0 && count <= 65535, "sp_jpeg_progressive_entropy: count %d (0..65535)", count);
    if (count == 0) return SP_OK;
    // the host arrays first, the device pointers last: a call with bad sizes is refused whatever the pointers are
    SP_REQUIRE(descs_host && scans_host && scan_range_host, "sp_jpeg_progressive_entropy: null pointer (descs_host, scans_host or scan_range_host)");
    SP_REQUIRE(scan_total >= 0, "sp_jpeg_progressive_entropy: scan_total %lld", (long long)scan_total);
    int64_t max_blocks = 0;
    for (int i = 0; i < count; ++i) {
        const sp_jpeg_desc& d = descs_host[i];
        int32_t bw[3], bh[3];
        int64_t blocks = 0;
        SP_REQUIRE(sp_jpeg_geometry(d, bw, bh, blocks), "sp_jpeg_progressive_entropy: image %d: size %dx%d, %d components or sampling not supported", i, d.width,
                   d.height, d.components);
        SP_REQUIRE(d.coef_count == blocks * 64, "sp_jpeg_progressive_entropy: image %d: coef_count does not follow from the size", i);
        SP_REQUIRE(d.file_bytes >= 0 && d.file_offset >= 0 && d.file_offset + d.file_bytes <= bytes_size,
                   "sp_jpeg_progressive_entropy: image %d: file bytes [%lld, +%d) outside the %lld-byte buffer", i, (long long)d.file_offset, d.file_bytes,
                   (long long)bytes_size);
        SP_REQUIRE(d.segments >= 1 && d.seg_index >= 0 && (int64_t)d.seg_index + d.segments <= seg_count,
                   "sp_jpeg_progressive_entropy: image %d: segments [%d, +%d) outside the %lld-entry table", i, d.seg_index, d.segments, (long long)seg_count);
        SP_REQUIRE(d.coef_offset >= 0 && d.coef_offset + d.coef_count <= coef_size, "sp_jpeg_progressive_entropy: image %d: coefficients outside the arena", i);
        const int64_t r0 = scan_range_host[i], r1 = scan_range_host[i + 1];
        SP_REQUIRE(r0 >= 0 && r0 <= r1 && r1 <= scan_total, "sp_jpeg_progressive_entropy: image %d: scan range [%lld, %lld) outside the %lld records", i, (long long)r0,
                   (long long)r1, (long long)scan_total);
        SP_REQUIRE(r1 - r0 >= 1 && r1 - r0 <= MAX_SCANS, "sp_jpeg_progressive_entropy: image %d: %lld scans (1..%d)", i, (long long)(r1 - r0), MAX_SCANS);
        for (int64_t k = r0; k < r1; ++k) {
            const sp_jpeg_scan& s = scans_host[k];
            const int sn = (int)(k - r0);
            bool comps = s.components >= 1 && s.components <= d.components;
            for (int j = 0; comps && j < s.components; ++j) comps = s.comp[j] >= 0 && s.comp[j] < d.components && (j == 0 || s.comp[j] > s.comp[j - 1]);
            SP_REQUIRE(comps, "sp_jpeg_progressive_entropy: image %d scan %d: component list", i, sn);
            SP_REQUIRE(s.ss >= 0 && s.ss <= s.se && s.se <= 63 && (s.ss == 0 ? s.se == 0 : s.components == 1) && s.ah >= 0 && s.ah <= 13 && s.al >= 0 && s.al <= 13,
                       "sp_jpeg_progressive_entropy: image %d scan %d: Ss %d Se %d Ah %d Al %d with %d components", i, sn, s.ss, s.se, s.ah, s.al, s.components);
            SP_REQUIRE(s.restart_interval >= 0 && s.restart_interval <= 65535, "sp_jpeg_progressive_entropy: image %d scan %d: restart interval %d (0..65535)", i, sn,
                       s.restart_interval);
            SP_REQUIRE(s.ecs_offset >= 0 && s.ecs_offset <= s.ecs_end && s.ecs_end <= d.file_bytes,
                       "sp_jpeg_progressive_entropy: image %d scan %d: entropy data [%d, %d) outside the file", i, sn, s.ecs_offset, s.ecs_end);
            SP_REQUIRE(s.segments >= 1 && s.seg_index >= 0 && (int64_t)s.seg_index + s.segments <= d.segments,
                       "sp_jpeg_progressive_entropy: image %d scan %d: segments [%d, +%d) outside the file's %d", i, sn, s.seg_index, s.segments, d.segments);
        }
        max_blocks = blocks > max_blocks ? blocks : max_blocks;
    }
    SP_REQUIRE(descs_dev && scans_dev && scan_range_dev && bytes && seg_offsets && coef && status, "sp_jpeg_progressive_entropy: null pointer");
    SP_REQUIRE(((uintptr_t)coef & 1) == 0 && ((uintptr_t)seg_offsets & 3) == 0 && ((uintptr_t)scan_range_dev & 3) == 0 && ((uintptr_t)descs_dev & 7) == 0 &&
                   ((uintptr_t)scans_dev & 3) == 0,
               "sp_jpeg_progressive_entropy: misaligned pointer (descs_dev 8, scans_dev 4, scan_range_dev 4, seg_offsets 4, coef 2)");
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_prog_zero_coef_kernel, dim3(sp_grid_for(max_blocks * 8, 256), count), dim3(256), 0, s, descs_dev, coef);
    const int rz = sp_check_launch("jpeg_prog_zero_coef_kernel");
    if (rz != SP_OK) return rz;
    hipLaunchKernelGGL(jpeg_prog_entropy_kernel, dim3(count), dim3(64), 0, s, descs_dev, scans_dev, scan_range_dev, bytes, seg_offsets, coef, status);
    return sp_check_launch("jpeg_prog_entropy_kernel");
}
