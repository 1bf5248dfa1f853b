// redact.hip - redaction on the device: the heads or the whole persons of one image (what sp_oks_nms leaves behind) hidden behind a mosaic
// or a constant colour, so that a frame that is stored or forwarded stays one stream of launches (capturable with the rest of the frame)
// and never visits the host on the way.  The reference has no such code; the rules live in sp_redact.h (shared with
// tests/redact_core_main.cpp) and are restated for numpy in tests/redact_ref.py; the box test, the limits and the entry point's
// frame checks are sp_frame_tile.h's, shared with the other overlays.  The tile kernel keeps its own coordinates and packed pixel words
// (its tile is 16 * RB rows high, RB row blocks per thread, and its scan fills a cell mask, no list): written on sp_tile and sp_px4 the
// cell-4 mosaic measured 2 to 4 % slower in two sessions (docs/LAB_NOTES.md, section 14); as it stands the kernels compile to the
// instructions they had before the header existed.  Integer arithmetic and sp_render_q: contraction OFF for the whole file.
#include "sp_frame_tile.h"
#include "sp_redact.h"

#include <stdint.h>

#pragma clang fp contract(off)

namespace {

constexpr int RDC_TILE_W = SP_TILE_W;            // a tile is 64 x (16 * RB) pixels, RB = max(16, cell) / 16: a whole number of cells both ways
constexpr int RDC_MAX_CELLS = 64;                // cell 4: 16 x 4 cells per tile

// One thread per person slot: dead slots are written as empty records, so the tile kernel needs no count.
__global__ __launch_bounds__(SP_TILE_NT) void redact_regions_kernel(const sp_redact_style st, int joints, int rows, int image,
                                                                const double* __restrict__ kps, const float* __restrict__ box,
                                                                const int32_t* __restrict__ keep, const int32_t* __restrict__ keep_count,
                                                                const int32_t* __restrict__ seg, sp_redact_rec* __restrict__ recs) {
    const int i = blockIdx.x * SP_TILE_NT + threadIdx.x;
    if (i >= rows) return;
    recs[i] = sp_redact_region_at(st, joints, rows, image, kps, box, keep, keep_count, seg, i);
}

// One workgroup per tile; thread t owns the four consecutive pixels from x = tx0 + 4 (t & 15) of the rows ty0 + 16 rb + (t >> 4), rb < RB.
// Four such pixels lie in one cell (a cell's width is a multiple of 4), and the four rows of a wave lie in one cell row.
// 1. scan: per chunk of 256 records a thread takes one; if its bounding box meets the tile, it tests the cells the box covers and sets
//    their bits in an LDS mask.  No bit set: the tile is left alone (in place) or copied.
// 2. sums: the thread's four pixels per channel, B and G packed into one word (a wave's total is at most 64 * 4 * 255 < 2^16), reduced
//    by xor-shuffles over the lanes of the same cell, then one LDS atomic per wave and cell; 3 * cells threads turn the sums into means.
// 3. write: the pixels of hit cells are replaced; in place only those are stored.
template <bool WIDE, int RB>
__global__ __launch_bounds__(SP_TILE_NT) void redact_tile_kernel(const unsigned char* src, unsigned char* dst, int h, int w,
                                                             const sp_redact_rec* __restrict__ recs, int total, int lc, int mode,
                                                             uint32_t fill) {
    __shared__ unsigned int mask[2];
    __shared__ unsigned int sums[RDC_MAX_CELLS * 3];
    const int tid = threadIdx.x, lane = tid & 63;
    const int cell = 1 << lc, cells_x = RDC_TILE_W >> lc, cells = cells_x * ((16 * RB) >> lc);
    const int tx0 = blockIdx.x * RDC_TILE_W, ty0 = blockIdx.y * (16 * RB);
    const int tx1 = min(tx0 + RDC_TILE_W, w) - 1, ty1 = min(ty0 + 16 * RB, h) - 1;      // the tile's last pixels inside the image
    const bool in_place = dst == src;
    if (tid < 2) mask[tid] = 0u;
    for (int i = tid; i < RDC_MAX_CELLS * 3; i += SP_TILE_NT) sums[i] = 0u;
    __syncthreads();
    // ---- 1. which cells are hit -------------------------------------------------------------------------------------------------------
    for (int base = 0; base < total; base += SP_TILE_NT) {
        const int i = base + tid;
        if (i >= total) break;
        const sp_redact_rec r = recs[i];
        if (!sp_box_meets(r, tx0, ty0, tx1, ty1)) continue;
        const int cx0 = (max(r.x0, tx0) - tx0) >> lc, cx1 = (min(r.x1, tx1) - tx0) >> lc;
        const int cy0 = (max(r.y0, ty0) - ty0) >> lc, cy1 = (min(r.y1, ty1) - ty0) >> lc;
        for (int cy = cy0; cy <= cy1; ++cy)
            for (int cx = cx0; cx <= cx1; ++cx) {
                const int X0 = tx0 + cx * cell, Y0 = ty0 + cy * cell;
                if (sp_redact_hits(r, X0, Y0, min(X0 + cell - 1, w - 1), min(Y0 + cell - 1, h - 1))) {
                    const int c = cy * cells_x + cx;
                    atomicOr(&mask[c >> 5], 1u << (c & 31));
                }
            }
    }
    __syncthreads();
    const unsigned long long hit = (unsigned long long)mask[0] | (unsigned long long)mask[1] << 32;               // uniform
    if (hit == 0ull && in_place) return;
    // ---- the thread's pixels: 12 bytes per row block, byte b = channel b % 3 of pixel b / 3 -------------------------------------------------
    const int x0 = tx0 + (tid & 15) * 4, yr = ty0 + (tid >> 4);
    uint32_t v[RB][3];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int y = yr + 16 * rb;
        v[rb][0] = v[rb][1] = v[rb][2] = 0u;
        if (y >= h || x0 >= w) continue;
        const size_t at = ((size_t)y * w + x0) * 3;
        if (WIDE) {                              // w % 4 == 0: a group of four is inside the row as a whole
            const uint32_t* s = reinterpret_cast<const uint32_t*>(src + at);
            v[rb][0] = s[0]; v[rb][1] = s[1]; v[rb][2] = s[2];
        } else {
#pragma unroll
            for (int b = 0; b < 12; ++b)
                if (x0 + b / 3 < w) v[rb][b / 4] |= (uint32_t)src[at + b] << (8 * (b % 4));
        }
    }
    // ---- 2. the cell sums (pixels outside the image add zeros) ----------------------------------------------------------------------------
    const int cxm = (tid & 15) >> (lc - 2);      // the thread's cell column
    if (hit != 0ull && mode == SP_REDACT_MOSAIC) {
        const int xbits = min(lc - 2, 4);        // lanes that differ in these low bits share the cell, and so do a wave's four rows
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            uint32_t bg = 0u, rr = 0u;
#pragma unroll
            for (int b = 0; b < 12; ++b) {
                const uint32_t val = (v[rb][b / 4] >> (8 * (b % 4))) & 255u;
                if (b % 3 == 0) bg += val;
                else if (b % 3 == 1) bg += val << 16;
                else rr += val;
            }
            for (int k = 0; k < xbits; ++k) {
                bg += __shfl_xor(bg, 1 << k, SP_WAVE);
                rr += __shfl_xor(rr, 1 << k, SP_WAVE);
            }
            bg += __shfl_xor(bg, 16, SP_WAVE); rr += __shfl_xor(rr, 16, SP_WAVE);
            bg += __shfl_xor(bg, 32, SP_WAVE); rr += __shfl_xor(rr, 32, SP_WAVE);
            if ((lane & 48) == 0 && (lane & ((1 << xbits) - 1)) == 0) {
                const int c = (((tid >> 4) + 16 * rb) >> lc) * cells_x + cxm;
                atomicAdd(&sums[c * 3 + 0], bg & 0xffffu);
                atomicAdd(&sums[c * 3 + 1], bg >> 16);
                atomicAdd(&sums[c * 3 + 2], rr);
            }
        }
        __syncthreads();
        if (tid < cells * 3) {
            const int c = tid / 3, cx = c % cells_x, cy = c / cells_x;
            const int X0 = tx0 + cx * cell, Y0 = ty0 + cy * cell;
            const int nx = min(X0 + cell, w) - X0, ny = min(Y0 + cell, h) - Y0;
            if (nx > 0 && ny > 0) sums[tid] = sp_redact_mean(sums[tid], (uint32_t)(nx * ny));
        }
        __syncthreads();
    }
    // ---- 3. replace and store ---------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int y = yr + 16 * rb;
        if (y >= h || x0 >= w) continue;
        const int c = (((tid >> 4) + 16 * rb) >> lc) * cells_x + cxm;
        const bool mine = (hit >> c) & 1ull;
        if (in_place && !mine) continue;
        if (mine) {
            uint32_t B = fill & 255u, G = (fill >> 8) & 255u, R = (fill >> 16) & 255u;
            if (mode == SP_REDACT_MOSAIC) { B = sums[c * 3 + 0]; G = sums[c * 3 + 1]; R = sums[c * 3 + 2]; }
            v[rb][0] = B | G << 8 | R << 16 | B << 24;
            v[rb][1] = G | R << 8 | B << 16 | G << 24;
            v[rb][2] = R | B << 8 | G << 16 | R << 24;
        }
        const size_t at = ((size_t)y * w + x0) * 3;
        if (WIDE) {
            uint32_t* d = reinterpret_cast<uint32_t*>(dst + at);
            d[0] = v[rb][0]; d[1] = v[rb][1]; d[2] = v[rb][2];
        } else {
#pragma unroll
            for (int b = 0; b < 12; ++b)
                if (x0 + b / 3 < w) dst[at + b] = (unsigned char)(v[rb][b / 4] >> (8 * (b % 4)));
        }
    }
}

template <bool WIDE>
void launch_tiles(hipStream_t s, const unsigned char* src, unsigned char* dst, int h, int w, const sp_redact_rec* recs, int total,
                  const sp_redact_style& st) {
    int lc = 2;
    while ((1 << lc) < st.cell) ++lc;
    const uint32_t fill = (uint32_t)st.fill[0] | (uint32_t)st.fill[1] << 8 | (uint32_t)st.fill[2] << 16;
    const int rb = st.cell <= 16 ? 1 : st.cell / 16;
    const dim3 grid(sp_ceil_div(w, RDC_TILE_W), sp_ceil_div(h, 16 * rb));
    if (rb == 1)
        hipLaunchKernelGGL((redact_tile_kernel<WIDE, 1>), grid, dim3(SP_TILE_NT), 0, s, src, dst, h, w, recs, total, lc, st.mode, fill);
    else if (rb == 2)
        hipLaunchKernelGGL((redact_tile_kernel<WIDE, 2>), grid, dim3(SP_TILE_NT), 0, s, src, dst, h, w, recs, total, lc, st.mode, fill);
    else
        hipLaunchKernelGGL((redact_tile_kernel<WIDE, 4>), grid, dim3(SP_TILE_NT), 0, s, src, dst, h, w, recs, total, lc, st.mode, fill);
}

}  // namespace

extern "C" int sp_redact_workspace_bytes(int rows, int64_t* bytes) {
    SP_REQUIRE(bytes, "sp_redact_workspace_bytes: null pointer");
    const int rc = sp_frame_rows_check("sp_redact_workspace_bytes", rows);
    if (rc != SP_OK) return rc;
    *bytes = (int64_t)rows * (int64_t)sizeof(sp_redact_rec);
    return SP_OK;
}

extern "C" int sp_redact_u8c3(const unsigned char* src, unsigned char* dst, int h, int w, const double* kps, const float* box,
                              const int32_t* keep, const int32_t* keep_count, const int32_t* seg, int image, int rows, int joints,
                              const sp_redact_style* style_host, void* workspace, void* stream) {
    SP_REQUIRE(style_host, "sp_redact_u8c3: null pointer");
    int rc = sp_frame_check("sp_redact_u8c3", src, dst, h, w, image, rows);
    if (rc != SP_OK) return rc;
    SP_REQUIRE(joints >= 1 && joints <= SP_MAX_JOINTS, "sp_redact_u8c3: joints %d (1..%d)", joints, SP_MAX_JOINTS);
    const sp_redact_style st = *style_host;
    SP_REQUIRE(st.region == SP_REDACT_HEAD || st.region == SP_REDACT_PERSON, "sp_redact_u8c3: region %d", st.region);
    SP_REQUIRE(st.mode == SP_REDACT_MOSAIC || st.mode == SP_REDACT_FILL, "sp_redact_u8c3: mode %d", st.mode);
    SP_REQUIRE(sp_redact_cell_ok(st.cell), "sp_redact_u8c3: cell %d (4, 8, 16, 32 or 64 pixels)", st.cell);
    SP_REQUIRE(st.expand >= 16 && st.expand <= 64, "sp_redact_u8c3: expand %d (sixteenths, 16..64)", st.expand);
    SP_REQUIRE(st.head_min >= 0 && st.head_min <= 256, "sp_redact_u8c3: head_min %d (1/256 of the box side, 0..256)", st.head_min);
    SP_REQUIRE(st.top_frac >= 0 && st.top_frac <= 256, "sp_redact_u8c3: top_frac %d (1/256 of the box height, 0..256)", st.top_frac);
    SP_REQUIRE(st.fallback >= SP_REDACT_FALLBACK_BOX_TOP && st.fallback <= SP_REDACT_FALLBACK_NONE, "sp_redact_u8c3: fallback %d", st.fallback);
    SP_REQUIRE(st.head_joints >= 1 && st.head_joints <= SP_REDACT_MAX_HEAD_JOINTS, "sp_redact_u8c3: head_joints %d (1..%d)", st.head_joints,
               SP_REDACT_MAX_HEAD_JOINTS);
    if (st.region == SP_REDACT_HEAD)
        for (int i = 0; i < st.head_joints; ++i)
            SP_REQUIRE(st.head_joint[i] >= 0 && st.head_joint[i] < joints, "sp_redact_u8c3: head_joint[%d] = %d is no joint index (0..%d)", i,
                       st.head_joint[i], joints - 1);
    if (rows == 0 && dst == src) return SP_OK;
    if (rows > 0) {
        SP_REQUIRE(kps && box && keep && keep_count && seg && workspace, "sp_redact_u8c3: null pointer");
        SP_REQUIRE(sp_aligned_to(workspace, 4) && sp_aligned_to(kps, 8), "sp_redact_u8c3: workspace must be 4-byte, kps 8-byte aligned");
    }
    const hipStream_t s = (hipStream_t)stream;
    sp_redact_rec* recs = reinterpret_cast<sp_redact_rec*>(workspace);
    if (rows > 0) {
        hipLaunchKernelGGL(redact_regions_kernel, dim3(sp_ceil_div(rows, SP_TILE_NT)), dim3(SP_TILE_NT), 0, s, st, joints, rows, image, kps, box, keep,
                           keep_count, seg, recs);
        rc = sp_check_launch("redact_regions_kernel");
        if (rc != SP_OK) return rc;
    }
    if (sp_frame_wide(w, src, dst))
        launch_tiles<true>(s, src, dst, h, w, recs, rows, st);
    else
        launch_tiles<false>(s, src, dst, h, w, recs, rows, st);
    return sp_check_launch("redact_tile_kernel");
}
