// labels.hip - the overlay's text on the device: one label per kept person (track id, pose score, detector confidence) and one caption per
// image (person count, image index, free text), formatted from the frame's own buffers and rasterised in place behind the capsules of
// render.hip, so that the numbers never reach the host and the annotated frame stays one stream of launches (capturable with the rest).
// The reference has no drawing code; the rules live in sp_label.h (shared with tests/label_core_main.cpp) and are restated for numpy in
// tests/label_ref.py; the tile, a thread's pixels, the ordered scan and the entry point's frame checks are sp_frame_tile.h's, shared with
// the other overlays.  Integer arithmetic, sp_render_q and one fp64 product: contraction OFF for the whole file.
#include "sp_frame_tile.h"
#include "sp_label.h"

#include <stdint.h>

#pragma clang fp contract(off)

namespace {

constexpr int LBL_LIST = 512;                    // record indices a tile collects before it applies them
constexpr int LBL_FONT_BYTES = SP_FONT_GLYPHS * SP_FONT_ROWS;

__constant__ unsigned char d_font[SP_FONT_GLYPHS][SP_FONT_ROWS] = SP_FONT_5X7_INIT;      // sp_font.h's initialiser: the host's table

// One thread per record: the person slots' labels (`labels` of them: rows, or none), then the caption.  Empty records are written too,
// so the tile kernel needs no count.
__global__ __launch_bounds__(SP_TILE_NT) void label_format_kernel(const sp_label_style st, int h, int w, int rows, int image,
                                                                  const float* __restrict__ box, const double* __restrict__ score,
                                                                  const int32_t* __restrict__ track_id, const int32_t* __restrict__ keep,
                                                                  const int32_t* __restrict__ keep_count, const int32_t* __restrict__ seg,
                                                                  const unsigned char* __restrict__ caption, int labels, int total,
                                                                  sp_label_rec* __restrict__ recs) {
    const int i = blockIdx.x * SP_TILE_NT + threadIdx.x;
    if (i >= total) return;
    if (i < labels)
        sp_label_person(st, h, w, rows, image, box, score, track_id, keep, keep_count, seg, i, recs + i);
    else
        sp_label_caption(st, h, w, rows, image, keep_count, seg, caption + (size_t)image * SP_LABEL_CAPTION_BYTES, recs + i);
}

// One workgroup per 64 x 16 tile, in place: the records that meet it (sp_tile_scan_ordered), in index order, onto every thread's four
// pixels.  The font and the pixels are read only once the tile has something to apply, so a tile nothing touches costs the scan alone.
template <bool WIDE>
__global__ __launch_bounds__(SP_TILE_NT) void label_tile_kernel(unsigned char* img, int h, int w, const sp_label_rec* __restrict__ recs, int total) {
    __shared__ unsigned char font[LBL_FONT_BYTES];
    const sp_tile t;
    const int x0 = t.x0, y = t.y;
    const bool mine = y < h && x0 < w;
    const size_t at = ((size_t)y * w + x0) * 3;
    sp_px4 px;
    unsigned char bgr[4][3];
    bool loaded = false;                         // uniform
    const bool touched = sp_tile_scan_ordered<LBL_LIST>(recs, total, t, [&](const int* list, int count) {
        if (!loaded) {
            for (int b = threadIdx.x; b < LBL_FONT_BYTES; b += SP_TILE_NT) font[b] = (&d_font[0][0])[b];
            if (mine) {
                px.load<WIDE>(img, at, x0, w);
                px.unpack(bgr);
            }
            loaded = true;
            __syncthreads();                     // the font
        }
        if (!mine) return;
        for (int e = 0; e < count; ++e) {
            const sp_label_rec& r = recs[list[e]];         // one address for the whole workgroup; the characters are read where they lie
            if (y < r.y0 || y > r.y1 || x0 > r.x1 || x0 + 3 < r.x0) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (x0 + q < w) sp_label_apply(r, font, x0 + q, y, bgr[q]);
        }
    });
    if (!touched || !mine) return;
    px.pack(bgr);
    px.store<WIDE>(img, at, x0, w);
}

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
    const int rc = sp_frame_rows_check("sp_render_labels_workspace_bytes", rows);
    if (rc != SP_OK) return rc;
    *bytes = ((int64_t)rows + 1) * (int64_t)sizeof(sp_label_rec);
    return SP_OK;
}

extern "C" int sp_render_labels_u8c3(unsigned char* img, int h, int w, const float* box, const double* score, const int32_t* track_id,
                                     const int32_t* keep, const int32_t* keep_count, const int32_t* seg, int image, int rows,
                                     const sp_label_style* style_host, const unsigned char* caption_dev, void* workspace, void* stream) {
    SP_REQUIRE(style_host, "sp_render_labels_u8c3: null pointer");
    int rc = sp_frame_check("sp_render_labels_u8c3", img, img, h, w, image, rows);       // in place
    if (rc != SP_OK) return rc;
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
    SP_REQUIRE(sp_aligned_to(workspace, 4) && (!score || sp_aligned_to(score, 8)), "sp_render_labels_u8c3: workspace must be 4-byte, score 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    sp_label_rec* recs = reinterpret_cast<sp_label_rec*>(workspace);
    hipLaunchKernelGGL(label_format_kernel, dim3(sp_ceil_div(total, SP_TILE_NT)), dim3(SP_TILE_NT), 0, s, st, h, w, rows, image, box, score, track_id, keep,
                       keep_count, seg, caption_dev, labels, total, recs);
    rc = sp_check_launch("label_format_kernel");
    if (rc != SP_OK) return rc;
    const dim3 grid(sp_ceil_div(w, SP_TILE_W), sp_ceil_div(h, SP_TILE_H));
    if (sp_frame_wide(w, img, img))
        hipLaunchKernelGGL(label_tile_kernel<true>, grid, dim3(SP_TILE_NT), 0, s, img, h, w, recs, total);
    else
        hipLaunchKernelGGL(label_tile_kernel<false>, grid, dim3(SP_TILE_NT), 0, s, img, h, w, recs, total);
    return sp_check_launch("label_tile_kernel");
}
