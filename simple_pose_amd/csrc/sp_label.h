// sp_label.h - the rules of the overlay's text (sp_render_labels_u8c3), ONE definition for the kernels in labels.hip, the CPU program
// tests/label_core_main.cpp and, restated in numpy, tests/label_ref.py: how a person's label and an image's caption are formatted, where
// their plates sit and what every pixel of a plate becomes.  Integer arithmetic except sp_render_q and the one product of the number
// format, so the device computes the host's bits.  The rules are written out in include/simple_pose_hip.h above sp_render_labels_u8c3.
// Text is written straight into the record (no per-thread character array), digits from the highest power of ten down.
#pragma once
#include <math.h>
#include <stdint.h>

#include "simple_pose_hip.h"
#include "sp_font.h"
#include "sp_render.h"

// One plate with its text.  Empty: x0 > x1, so no tile ever lists it.
struct sp_label_rec {
    int32_t x0, y0, x1, y1;          // the plate clipped to the image (inclusive)
    int32_t ux0, uy0, ux1, uy1;      // the plate as placed: font pixels are counted from (ux0, uy0)
    uint32_t plate, text;            // B | G << 8 | R << 16
    int32_t alpha;                   // 16 * opacity, 0 .. 256
    int32_t scale, len;
    unsigned char ch[SP_LABEL_CAPTION_BYTES];   // printable ASCII, `len` of them
};

SP_RENDER_HD bool sp_label_printable(int c) { return c >= SP_FONT_FIRST && c <= SP_FONT_LAST; }

SP_RENDER_HD void sp_label_clear(sp_label_rec* r) {
    r->x0 = r->y0 = 1;
    r->x1 = r->y1 = 0;
    r->ux0 = r->uy0 = r->ux1 = r->uy1 = 0;
    r->plate = r->text = 0;
    r->alpha = 0;
    r->scale = 1;
    r->len = 0;
    for (int i = 0; i < SP_LABEL_CAPTION_BYTES; ++i) r->ch[i] = 0;
}

SP_RENDER_HD void sp_label_put(sp_label_rec* r, int cap, int c) {
    if (r->len < cap) r->ch[r->len++] = (unsigned char)c;
}

SP_RENDER_HD void sp_label_put_uint(sp_label_rec* r, int cap, uint64_t v) {
    uint64_t p = 1;
    while (v / p >= 10) p *= 10;
    for (; p > 0; p /= 10) sp_label_put(r, cap, '0' + (int)((v / p) % 10));
}

// {score}, {conf}: "?" for a value that is not finite or is < 0, else c = rint(min(v, 99.99) * 100) as c / 100 '.' two digits
SP_RENDER_HD void sp_label_put_number(sp_label_rec* r, int cap, double v) {
    if (!(v >= 0.0) || !(v <= 1.7976931348623157e308)) {
        sp_label_put(r, cap, '?');
        return;
    }
    const int64_t c = (int64_t)rint((v < 99.99 ? v : 99.99) * 100.0);
    sp_label_put_uint(r, cap, (uint64_t)(c / 100));
    sp_label_put(r, cap, '.');
    sp_label_put(r, cap, '0' + (int)((c % 100) / 10));
    sp_label_put(r, cap, '0' + (int)(c % 10));
}

// the plate of r->len characters at r->scale with its corner at (x0, y0), clipped to the image; empty text or nothing left: an empty record
SP_RENDER_HD void sp_label_place(sp_label_rec* r, int x0, int y0, int h, int w) {
    const int width = (SP_FONT_CELL_W * r->len + 1) * r->scale, height = (SP_FONT_CELL_H + 1) * r->scale;
    r->ux0 = x0;
    r->uy0 = y0;
    r->ux1 = x0 + width - 1;
    r->uy1 = y0 + height - 1;
    r->x0 = r->ux0 < 0 ? 0 : r->ux0;
    r->y0 = r->uy0 < 0 ? 0 : r->uy0;
    r->x1 = r->ux1 > w - 1 ? w - 1 : r->ux1;
    r->y1 = r->uy1 > h - 1 ? h - 1 : r->uy1;
    if (r->len == 0 || r->x0 > r->x1 || r->y0 > r->y1) {
        r->x0 = r->y0 = 1;
        r->x1 = r->y1 = 0;
    }
}

// Record p of the image: the label of the pose at pick position n - 1 - p, empty for p >= n (and for a row outside the frame).
SP_RENDER_HD void sp_label_person(const sp_label_style& st, int h, int w, int rows, int image, const float* box, const double* score,
                                  const int32_t* track_id, const int32_t* keep, const int32_t* keep_count, const int32_t* seg, int p,
                                  sp_label_rec* r) {
    sp_label_clear(r);
    int pick;
    const int row = sp_render_kept_row(keep, keep_count, seg, image, rows, p, true, &pick);
    if (row < 0) return;
    const float* b = box + (size_t)row * 5;
    int32_t qx, qy;
    if (!(sp_render_q((double)b[0], qx) && sp_render_q((double)b[1], qy))) return;
    const int id = track_id ? track_id[row] : 0;
    for (int t = 0; t < st.template_len; ++t) {
        const int c = st.label_template[t];
        if (c == SP_LABEL_FIELD_ID) sp_label_put_uint(r, SP_LABEL_MAX_CHARS, id > 0 ? (uint64_t)id : (uint64_t)pick + 1);
        else if (c == SP_LABEL_FIELD_SCORE) sp_label_put_number(r, SP_LABEL_MAX_CHARS, score[row]);
        else if (c == SP_LABEL_FIELD_CONF) sp_label_put_number(r, SP_LABEL_MAX_CHARS, (double)b[4]);
        else sp_label_put(r, SP_LABEL_MAX_CHARS, sp_label_printable(c) ? c : '?');
    }
    r->plate = sp_render_palette(st.palette, st.palette_n, id > 0 ? (id - 1) % st.palette_n : pick % st.palette_n);
    const int lum = 29 * (int)(r->plate & 255u) + 150 * (int)((r->plate >> 8) & 255u) + 77 * (int)((r->plate >> 16) & 255u);
    r->text = lum >= 32768 ? 0u : 0xFFFFFFu;
    r->alpha = 16 * st.label_opacity;
    r->scale = st.label_scale;
    const int s = r->scale, width = (SP_FONT_CELL_W * r->len + 1) * s;
    const int bx = sp_render_floor16(qx), by = sp_render_floor16(qy);
    int y0 = by - (SP_FONT_CELL_H + 1) * s;
    if (y0 < 0) y0 = by;
    int x0 = bx;
    if (x0 + width > w) x0 = w - width;
    if (x0 < 0) x0 = 0;
    sp_label_place(r, x0, y0, h, w);
}

// The image's caption: `text` is its 64 bytes (ending at the first NUL).
SP_RENDER_HD void sp_label_caption(const sp_label_style& st, int h, int w, int rows, int image, const int32_t* keep_count, const int32_t* seg,
                                   const unsigned char* text, sp_label_rec* r) {
    sp_label_clear(r);
    int lo;
    const int n = sp_render_live(keep_count, seg, image, rows, lo);
    for (int t = 0; t < SP_LABEL_CAPTION_BYTES && text[t] != 0; ++t) {
        const int c = text[t];
        if (c == SP_LABEL_FIELD_N) sp_label_put_uint(r, SP_LABEL_CAPTION_BYTES, (uint64_t)n);
        else if (c == SP_LABEL_FIELD_IMAGE) sp_label_put_uint(r, SP_LABEL_CAPTION_BYTES, (uint64_t)image);
        else sp_label_put(r, SP_LABEL_CAPTION_BYTES, sp_label_printable(c) ? c : '?');
    }
    r->plate = 0u;
    r->text = 0xFFFFFFu;
    r->alpha = 16 * st.caption_opacity;
    r->scale = st.caption_scale;
    const int s = r->scale, width = (SP_FONT_CELL_W * r->len + 1) * s, height = (SP_FONT_CELL_H + 1) * s;
    const bool right = st.caption_corner == SP_LABEL_CORNER_TR || st.caption_corner == SP_LABEL_CORNER_BR;
    const bool bottom = st.caption_corner == SP_LABEL_CORNER_BL || st.caption_corner == SP_LABEL_CORNER_BR;
    sp_label_place(r, right ? w - s - width : s, bottom ? h - s - height : s, h, w);
}

// one record onto one pixel (bgr: 3 bytes); `font`: the 95 x 7 glyph rows.  A pixel off the clipped plate keeps its bytes.
SP_RENDER_HD void sp_label_apply(const sp_label_rec& r, const unsigned char* font, int x, int y, unsigned char* bgr) {
    if (x < r.x0 || x > r.x1 || y < r.y0 || y > r.y1) return;
    const int fx = (x - r.ux0) / r.scale - 1, fy = (y - r.uy0) / r.scale - 1;        // (both differences are >= 0 on the plate)
    bool on = false;
    if (fx >= 0 && fy >= 0 && fy < SP_FONT_ROWS) {
        const int i = fx / SP_FONT_CELL_W, col = fx - SP_FONT_CELL_W * i;
        if (i < r.len && col < SP_FONT_COLS) on = (font[(r.ch[i] - SP_FONT_FIRST) * SP_FONT_ROWS + fy] >> (SP_FONT_COLS - 1 - col)) & 1;
    }
    const uint32_t colour = on ? r.text : r.plate;
    for (int c = 0; c < 3; ++c) bgr[c] = (unsigned char)sp_render_blend(bgr[c], (colour >> (8 * c)) & 255u, r.alpha);
}
