// labels.hip - the overlay's text on the device: one label per kept person (track id, pose score, detector confidence) and one caption per
// image (person count, image index, free text), formatted from the frame's own buffers and rasterised in place behind the capsules of
// render.hip, so that the numbers never reach the host and the annotated frame stays one stream of launches (capturable with the rest).
// The reference has no drawing code; the rules live in sp_label.h (shared with tests/label_core_main.cpp) and are restated for numpy in
// tests/label_ref.py.  Integer arithmetic, sp_render_q and one fp64 product: contraction OFF for the whole file.
#include "sp_common.h"
#include "sp_label.h"

#include <stdint.h>

#pragma clang fp contract(off)

namespace {

constexpr int LBL_NT = 256;
constexpr int LBL_TILE_W = 64, LBL_TILE_H = 16;  // 256 threads x 4 consecutive pixels of one row
constexpr int LBL_LIST = 512;                    // record indices a tile collects before it applies them
constexpr int LBL_MAX_ROWS = 2048;               // the OKS-NMS group limit
constexpr int LBL_MAX_DIM = 16384;
constexpr int LBL_FONT_BYTES = SP_FONT_GLYPHS * SP_FONT_ROWS;

__constant__ unsigned char d_font[SP_FONT_GLYPHS][SP_FONT_ROWS] = SP_FONT_5X7_INIT;      // sp_font.h's initialiser: the host's table

// One thread per record: the person slots' labels (`labels` of them: rows, or none), then the caption.  Empty records are written too,
// so the tile kernel needs no count.
__global__ __launch_bounds__(LBL_NT) void label_format_kernel(const sp_label_style st, int h, int w, int rows, int image,
                                                              const float* __restrict__ box, const double* __restrict__ score,
                                                              const int32_t* __restrict__ track_id, const int32_t* __restrict__ keep,
                                                              const int32_t* __restrict__ keep_count, const int32_t* __restrict__ seg,
                                                              const unsigned char* __restrict__ caption, int labels, int total,
                                                              sp_label_rec* __restrict__ recs) {
    const int i = blockIdx.x * LBL_NT + threadIdx.x;
    if (i >= total) return;
    if (i < labels)
        sp_label_person(st, h, w, rows, image, box, score, track_id, keep, keep_count, seg, i, recs + i);
    else
        sp_label_caption(st, h, w, rows, image, keep_count, seg, caption + (size_t)image * SP_LABEL_CAPTION_BYTES, recs + i);
}

template <bool WIDE>
__device__ __forceinline__ void load_pixels(const unsigned char* img, size_t at, int x0, int w, unsigned char (&px)[4][3]) {
    if (WIDE) {                                  // w % 4 == 0: a group of four is inside the row as a whole
        const uint32_t* s = reinterpret_cast<const uint32_t*>(img + at);
        const uint32_t v[3] = {s[0], s[1], s[2]};
#pragma unroll
        for (int b = 0; b < 12; ++b) px[b / 3][b % 3] = (unsigned char)(v[b / 4] >> (8 * (b % 4)));
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) px[q][c] = x0 + q < w ? img[at + q * 3 + c] : 0;
    }
}

// the listed records, in list order, onto the thread's four pixels
__device__ __forceinline__ void apply_list(const sp_label_rec* __restrict__ recs, const int* list, int count, const unsigned char* font, int x0,
                                           int y, int w, unsigned char (&px)[4][3]) {
    for (int e = 0; e < count; ++e) {
        const sp_label_rec& r = recs[list[e]];             // one address for the whole workgroup; the characters are read where they lie
        if (y < r.y0 || y > r.y1 || x0 > r.x1 || x0 + 3 < r.x0) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (x0 + q < w) sp_label_apply(r, font, x0 + q, y, px[q]);
    }
}

// One workgroup per 64 x 16 tile, in place.  The scan keeps the index order without atomics, as render_tile_kernel's: per chunk of 256
// records a ballot per wave, the four wave counts through LDS, and every hit lands at (hits before its wave) + (hits below its lane).
// The pixels are read only once the tile has something to apply, so a tile nothing touches costs the scan alone.
template <bool WIDE>
__global__ __launch_bounds__(LBL_NT) void label_tile_kernel(unsigned char* img, int h, int w, const sp_label_rec* __restrict__ recs, int total) {
    __shared__ int list[LBL_LIST];
    __shared__ int wave_hits[4];
    __shared__ unsigned char font[LBL_FONT_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx0 = blockIdx.x * LBL_TILE_W, ty0 = blockIdx.y * LBL_TILE_H;
    const int x0 = tx0 + (tid & 15) * 4, y = ty0 + (tid >> 4);
    const bool mine = y < h && x0 < w;
    const size_t at = ((size_t)y * w + x0) * 3;
    unsigned char px[4][3];
    bool loaded = false;                         // uniform
    int count = 0;                               // uniform: every thread adds the same totals
    for (int base = 0; base < total; base += LBL_NT) {
        const int i = base + tid;
        bool hit = false;
        if (i < total) {
            const sp_label_rec& r = recs[i];
            hit = r.x0 <= tx0 + LBL_TILE_W - 1 && r.x1 >= tx0 && r.y0 <= ty0 + LBL_TILE_H - 1 && r.y1 >= ty0;     // (empty: x0 > x1)
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
        if (count + chunk > LBL_LIST) {          // uniform; count > 0 here, since a chunk has at most 256 hits
            if (!loaded) {
                for (int b = tid; b < LBL_FONT_BYTES; b += LBL_NT) font[b] = (&d_font[0][0])[b];
                if (mine) load_pixels<WIDE>(img, at, x0, w, px);
                loaded = true;
                __syncthreads();                 // the font
            }
            if (mine) apply_list(recs, list, count, font, x0, y, w, px);
            count = 0;
            __syncthreads();                     // nobody still reads the list
        }
        if (hit) list[count + before + __popcll(ballot & ((1ull << lane) - 1ull))] = i;
        count += chunk;
        __syncthreads();                         // the entries are visible; wave_hits is free for the next chunk
    }
    if (count == 0 && !loaded) return;           // uniform: nothing touches the tile
    if (!loaded) {
        for (int b = tid; b < LBL_FONT_BYTES; b += LBL_NT) font[b] = (&d_font[0][0])[b];
        if (mine) load_pixels<WIDE>(img, at, x0, w, px);
        __syncthreads();
    }
    if (!mine) return;
    apply_list(recs, list, count, font, x0, y, w, px);
    if (WIDE) {
        uint32_t v[3] = {0u, 0u, 0u};
#pragma unroll
        for (int b = 0; b < 12; ++b) v[b / 4] |= (uint32_t)px[b / 3][b % 3] << (8 * (b % 4));
        uint32_t* d = reinterpret_cast<uint32_t*>(img + at);
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2];
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (x0 + q < w) img[at + q * 3 + c] = px[q][c];
    }
}

bool aligned_to(const void* p, unsigned n) { return ((uintptr_t)p & (n - 1)) == 0; }

}  // namespace

extern "C" int sp_render_font_glyph(int ch, unsigned char rows7[7]) {
    if (!rows7) {
        sp_set_error("sp_render_font_glyph: null pointer");
        return -1;
    }
    if (ch < SP_FONT_FIRST || ch > SP_FONT_LAST) {
        sp_set_error("sp_render_font_glyph: character %d has no glyph (printable ASCII, %d..%d)", ch, SP_FONT_FIRST, SP_FONT_LAST);
        return -1;
    }
    for (int r = 0; r < SP_FONT_ROWS; ++r) rows7[r] = SP_FONT_5X7[ch - SP_FONT_FIRST][r];
    return SP_OK;
}

extern "C" int sp_render_labels_workspace_bytes(int rows, int64_t* bytes) {
    SP_REQUIRE(bytes, "sp_render_labels_workspace_bytes: null pointer");
    SP_REQUIRE(rows >= 0 && rows <= LBL_MAX_ROWS, "sp_render_labels_workspace_bytes: rows %d (0..%d, the OKS-NMS group limit)", rows, LBL_MAX_ROWS);
    *bytes = ((int64_t)rows + 1) * (int64_t)sizeof(sp_label_rec);
    return SP_OK;
}

extern "C" int sp_render_labels_u8c3(unsigned char* img, int h, int w, const float* box, const double* score, const int32_t* track_id,
                                     const int32_t* keep, const int32_t* keep_count, const int32_t* seg, int image, int rows,
                                     const sp_label_style* style_host, const unsigned char* caption_dev, void* workspace, void* stream) {
    SP_REQUIRE(img && style_host, "sp_render_labels_u8c3: null pointer");
    SP_REQUIRE(h >= 1 && h <= LBL_MAX_DIM && w >= 1 && w <= LBL_MAX_DIM, "sp_render_labels_u8c3: image %dx%d (1..%d each way)", w, h, LBL_MAX_DIM);
    SP_REQUIRE(image >= 0, "sp_render_labels_u8c3: image index %d", image);
    SP_REQUIRE(rows >= 0 && rows <= LBL_MAX_ROWS, "sp_render_labels_u8c3: rows %d (0..%d, the OKS-NMS group limit)", rows, LBL_MAX_ROWS);
    const sp_label_style st = *style_host;
    SP_REQUIRE(st.template_len >= 0 && st.template_len <= SP_LABEL_MAX_TEMPLATE, "sp_render_labels_u8c3: template length %d (0..%d)",
               st.template_len, SP_LABEL_MAX_TEMPLATE);
    for (int t = 0; t < st.template_len; ++t) {
        const int c = st.label_template[t];
        SP_REQUIRE(c != SP_LABEL_FIELD_N && c != SP_LABEL_FIELD_IMAGE, "sp_render_labels_u8c3: template byte %d is caption field 0x%02x in a label", t, c);
        SP_REQUIRE(sp_label_printable(c) || (c >= SP_LABEL_FIELD_ID && c <= SP_LABEL_FIELD_CONF),
                   "sp_render_labels_u8c3: template byte %d is 0x%02x, neither printable ASCII nor a field (0x01..0x05)", t, c);
    }
    SP_REQUIRE(st.label_scale >= 1 && st.label_scale <= SP_LABEL_MAX_SCALE && st.caption_scale >= 1 && st.caption_scale <= SP_LABEL_MAX_SCALE,
               "sp_render_labels_u8c3: scale label=%d caption=%d (1..%d)", st.label_scale, st.caption_scale, SP_LABEL_MAX_SCALE);
    SP_REQUIRE(st.label_opacity >= 0 && st.label_opacity <= 16 && st.caption_opacity >= 0 && st.caption_opacity <= 16,
               "sp_render_labels_u8c3: opacity label=%d caption=%d (sixteenths, 0..16)", st.label_opacity, st.caption_opacity);
    SP_REQUIRE(st.caption_corner >= SP_LABEL_CORNER_TL && st.caption_corner <= SP_LABEL_CORNER_BR, "sp_render_labels_u8c3: caption_corner %d",
               st.caption_corner);
    SP_REQUIRE(st.palette_n >= 1 && st.palette_n <= SP_RENDER_MAX_PALETTE, "sp_render_labels_u8c3: palette_n %d (1..%d)", st.palette_n,
               SP_RENDER_MAX_PALETTE);
    const int labels = st.template_len > 0 ? rows : 0;
    const int total = labels + (caption_dev ? 1 : 0);
    if (total == 0) return SP_OK;
    SP_REQUIRE(keep_count && seg && workspace, "sp_render_labels_u8c3: null pointer");
    if (labels > 0) SP_REQUIRE(box && score && keep, "sp_render_labels_u8c3: null pointer");
    SP_REQUIRE(aligned_to(workspace, 4) && (!score || aligned_to(score, 8)), "sp_render_labels_u8c3: workspace must be 4-byte, score 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    sp_label_rec* recs = reinterpret_cast<sp_label_rec*>(workspace);
    hipLaunchKernelGGL(label_format_kernel, dim3(sp_ceil_div(total, LBL_NT)), dim3(LBL_NT), 0, s, st, h, w, rows, image, box, score, track_id, keep,
                       keep_count, seg, caption_dev, labels, total, recs);
    const int rc = sp_check_launch("label_format_kernel");
    if (rc != SP_OK) return rc;
    const dim3 grid(sp_ceil_div(w, LBL_TILE_W), sp_ceil_div(h, LBL_TILE_H));
    if (w % 4 == 0 && aligned_to(img, 4))
        hipLaunchKernelGGL(label_tile_kernel<true>, grid, dim3(LBL_NT), 0, s, img, h, w, recs, total);
    else
        hipLaunchKernelGGL(label_tile_kernel<false>, grid, dim3(LBL_NT), 0, s, img, h, w, recs, total);
    return sp_check_launch("label_tile_kernel");
}
