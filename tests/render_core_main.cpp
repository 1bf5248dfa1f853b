// TEST PROGRAM (tests/test_render_core_cpu.py builds it with -fsanitize=address,undefined): the overlay's pixel rules of
// simple_pose_amd/csrc/sp_render.h driven on the CPU with the work split of the kernels in render.hip (one primitive per slot, then every
// pixel through the primitive array in index order).  Every buffer is a heap allocation of exactly the size the library's caller has to
// provide, so a read or write outside one is an AddressSanitizer report.
//   render_core_main <scene.bin> <out.bgr>
// scene.bin: int32 {h, w, rows, joints, images, image, has_track_id}, sp_render_style, kps double [rows, joints, 3], box float [rows, 5],
// track_id int32 [rows], keep int32 [rows], keep_count int32 [images], seg int32 [images + 1], pixels uint8 [h, w, 3].
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sp_render.h"

template <typename T>
static T* take(FILE* f, size_t n) {
    T* p = (T*)malloc(n * sizeof(T) ? n * sizeof(T) : 1);        // exactly n elements
    if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "scene file is too short\n"); exit(2); }
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: render_core_main <scene.bin> <out.bgr>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t* hd = take<int32_t>(f, 7);
    const int h = hd[0], w = hd[1], rows = hd[2], joints = hd[3], images = hd[4], image = hd[5], has_id = hd[6];
    sp_render_style* st = take<sp_render_style>(f, 1);
    double* kps = take<double>(f, (size_t)rows * joints * 3);
    float* box = take<float>(f, (size_t)rows * 5);
    int32_t* tid = take<int32_t>(f, (size_t)rows);
    int32_t* keep = take<int32_t>(f, (size_t)rows);
    int32_t* keep_count = take<int32_t>(f, (size_t)images);
    int32_t* seg = take<int32_t>(f, (size_t)images + 1);
    unsigned char* px = take<unsigned char>(f, (size_t)h * w * 3);
    fclose(f);

    const int total = rows * sp_render_slots(*st, joints);
    sp_render_prim* prims = (sp_render_prim*)malloc(total ? sizeof(sp_render_prim) * (size_t)total : 1);
    int live = 0;
    for (int i = 0; i < total; ++i) {                            // render_prims_kernel
        prims[i] = sp_render_prim_at(*st, joints, rows, image, kps, box, has_id ? tid : nullptr, keep, keep_count, seg, i);
        live += prims[i].r >= 0;
    }
    for (int y = 0; y < h; ++y)                                  // render_tile_kernel, without the tiles: their lists keep this order
        for (int x = 0; x < w; ++x)
            for (int i = 0; i < total; ++i) sp_render_apply(prims[i], st->opacity, x, y, px + ((size_t)y * w + x) * 3);
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(px, 1, (size_t)h * w * 3, o) != (size_t)h * w * 3) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fclose(o);
    printf("OK %dx%d primitives %d live %d\n", w, h, total, live);
    free(hd); free(st); free(kps); free(box); free(tid); free(keep); free(keep_count); free(seg); free(px); free(prims);
    return 0;
}
