// TEST PROGRAM (tests/test_redact_core_cpu.py builds it with -fsanitize=address,undefined): the redaction rules of
// simple_pose_amd/csrc/sp_redact.h driven on the CPU with the work split of the kernels in redact.hip (one record per person slot, then
// every cell against the record array, its sums from the source).  Every buffer is a heap allocation of exactly the size the library's
// caller has to provide, so a read or write outside one is an AddressSanitizer report.
//   redact_core_main <scene.bin> <out.bgr>
// scene.bin: int32 {h, w, rows, joints, images, image}, sp_redact_style, kps double [rows, joints, 3], box float [rows, 5],
// keep int32 [rows], keep_count int32 [images], seg int32 [images + 1], pixels uint8 [h, w, 3].
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sp_redact.h"

template <typename T>
static T* take(FILE* f, size_t n) {
    T* p = (T*)malloc(n * sizeof(T) ? n * sizeof(T) : 1);        // exactly n elements
    if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "scene file is too short\n"); exit(2); }
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: redact_core_main <scene.bin> <out.bgr>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t* hd = take<int32_t>(f, 6);
    const int h = hd[0], w = hd[1], rows = hd[2], joints = hd[3], images = hd[4], image = hd[5];
    sp_redact_style* st = take<sp_redact_style>(f, 1);
    double* kps = take<double>(f, (size_t)rows * joints * 3);
    float* box = take<float>(f, (size_t)rows * 5);
    int32_t* keep = take<int32_t>(f, (size_t)rows);
    int32_t* keep_count = take<int32_t>(f, (size_t)images);
    int32_t* seg = take<int32_t>(f, (size_t)images + 1);
    unsigned char* src = take<unsigned char>(f, (size_t)h * w * 3);
    fclose(f);
    if (!sp_redact_cell_ok(st->cell)) { fprintf(stderr, "cell %d\n", st->cell); return 2; }

    sp_redact_rec* recs = (sp_redact_rec*)malloc(rows ? sizeof(sp_redact_rec) * (size_t)rows : 1);
    int live = 0;
    for (int i = 0; i < rows; ++i) {                             // redact_regions_kernel
        recs[i] = sp_redact_region_at(*st, joints, rows, image, kps, box, keep, keep_count, seg, i);
        live += recs[i].kind != SP_REDACT_EMPTY;
    }
    unsigned char* dst = (unsigned char*)malloc((size_t)h * w * 3);
    memcpy(dst, src, (size_t)h * w * 3);
    const int cell = st->cell;
    int hit_cells = 0;
    for (int Y0 = 0; Y0 < h; Y0 += cell)                         // redact_tile_kernel, without the tiles
        for (int X0 = 0; X0 < w; X0 += cell) {
            const int X1 = (X0 + cell < w ? X0 + cell : w) - 1, Y1 = (Y0 + cell < h ? Y0 + cell : h) - 1;
            bool hit = false;
            for (int i = 0; i < rows; ++i) {
                const sp_redact_rec& r = recs[i];
                const bool near = r.x0 <= X1 && r.x1 >= X0 && r.y0 <= Y1 && r.y1 >= Y0;      // the tile kernel's bounding-box test
                const bool in = sp_redact_hits(r, X0, Y0, X1, Y1);
                if (in && !near) { fprintf(stderr, "record %d hits a cell outside its bounding box\n", i); return 3; }
                hit = hit || in;
            }
            if (!hit) continue;
            ++hit_cells;
            uint32_t sum[3] = {0u, 0u, 0u};
            const uint32_t n = (uint32_t)(X1 - X0 + 1) * (uint32_t)(Y1 - Y0 + 1);
            for (int y = Y0; y <= Y1; ++y)
                for (int x = X0; x <= X1; ++x)
                    for (int c = 0; c < 3; ++c) sum[c] += src[((size_t)y * w + x) * 3 + c];
            for (int y = Y0; y <= Y1; ++y)
                for (int x = X0; x <= X1; ++x)
                    for (int c = 0; c < 3; ++c)
                        dst[((size_t)y * w + x) * 3 + c] =
                            st->mode == SP_REDACT_FILL ? st->fill[c] : (unsigned char)sp_redact_mean(sum[c], n);
        }
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(dst, 1, (size_t)h * w * 3, o) != (size_t)h * w * 3) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fclose(o);
    printf("OK %dx%d records %d live %d cells %d\n", w, h, rows, live, hit_cells);
    free(hd); free(st); free(kps); free(box); free(keep); free(keep_count); free(seg); free(src); free(recs); free(dst);
    return 0;
}
