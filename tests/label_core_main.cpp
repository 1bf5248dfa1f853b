// TEST PROGRAM (tests/test_label_core_cpu.py builds it with -fsanitize=address,undefined): the overlay text's rules of
// simple_pose_amd/csrc/sp_label.h driven on the CPU with the work split of the kernels in labels.hip (one record per person slot and one for
// the caption, then every pixel through the record array in index order, the glyphs from sp_font.h's table).  Every buffer is a heap
// allocation of exactly the size the library's caller has to provide, so a read or write outside one is an AddressSanitizer report.
//   label_core_main <scene.bin> <out.bgr>
// scene.bin: int32 {h, w, rows, images, image, has_track_id, has_caption, alloc_rows}, sp_label_style, box float [alloc_rows, 5],
// score double [alloc_rows], track_id int32 [alloc_rows], keep int32 [alloc_rows], keep_count int32 [images], seg int32 [images + 1],
// caption uint8 [images, 64], pixels uint8 [h, w, 3].  (rows: what the call is told; alloc_rows: what the arrays hold.)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sp_label.h"

template <typename T>
static T* take(FILE* f, size_t n) {
    T* p = (T*)malloc(n * sizeof(T) ? n * sizeof(T) : 1);        // exactly n elements
    if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "scene file is too short\n"); exit(2); }
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: label_core_main <scene.bin> <out.bgr>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t* hd = take<int32_t>(f, 8);
    const int h = hd[0], w = hd[1], rows = hd[2], images = hd[3], image = hd[4], has_id = hd[5], has_caption = hd[6], alloc = hd[7];
    sp_label_style* st = take<sp_label_style>(f, 1);
    float* box = take<float>(f, (size_t)alloc * 5);
    double* score = take<double>(f, (size_t)alloc);
    int32_t* tid = take<int32_t>(f, (size_t)alloc);
    int32_t* keep = take<int32_t>(f, (size_t)alloc);
    int32_t* keep_count = take<int32_t>(f, (size_t)images);
    int32_t* seg = take<int32_t>(f, (size_t)images + 1);
    unsigned char* caption = take<unsigned char>(f, (size_t)images * SP_LABEL_CAPTION_BYTES);
    unsigned char* px = take<unsigned char>(f, (size_t)h * w * 3);
    fclose(f);

    const int labels = st->template_len > 0 ? rows : 0, total = labels + (has_caption ? 1 : 0);
    sp_label_rec* recs = (sp_label_rec*)malloc(total ? sizeof(sp_label_rec) * (size_t)total : 1);
    int live = 0;
    for (int i = 0; i < total; ++i) {                            // label_format_kernel
        if (i < labels)
            sp_label_person(*st, h, w, rows, image, box, score, has_id ? tid : nullptr, keep, keep_count, seg, i, recs + i);
        else
            sp_label_caption(*st, h, w, rows, image, keep_count, seg, caption + (size_t)image * SP_LABEL_CAPTION_BYTES, recs + i);
        live += recs[i].x0 <= recs[i].x1;
    }
    unsigned char* font = (unsigned char*)malloc(SP_FONT_GLYPHS * SP_FONT_ROWS);       // the tile's LDS copy
    memcpy(font, SP_FONT_5X7, SP_FONT_GLYPHS * SP_FONT_ROWS);
    for (int y = 0; y < h; ++y)                                  // label_tile_kernel, without the tiles: their lists keep this order
        for (int x = 0; x < w; ++x)
            for (int i = 0; i < total; ++i) sp_label_apply(recs[i], font, x, y, px + ((size_t)y * w + x) * 3);
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(px, 1, (size_t)h * w * 3, o) != (size_t)h * w * 3) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fclose(o);
    printf("OK %dx%d records %d live %d\n", w, h, total, live);
    free(hd); free(st); free(box); free(score); free(tid); free(keep); free(keep_count); free(seg); free(caption); free(px); free(recs); free(font);
    return 0;
}
