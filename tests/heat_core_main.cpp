// TEST PROGRAM (tests/test_heat_core_cpu.py builds it with -fsanitize=address,undefined): the heat overlay's rules of
// simple_pose_amd/csrc/sp_heat.h driven on the CPU with the work split of the kernels in heat.hip (one record and one u8 plane per person
// slot, then 64 x 16 tiles that list the records whose box and whose exact U / V ranges reach them).  Every buffer is a heap allocation
// of exactly the size the library's caller has to provide, so a read or write outside one is an AddressSanitizer report.  Every pixel is
// also sampled against EVERY live record: a box or a tile test that changes a value ends the program with exit code 3.
//   heat_core_main <scene.bin> <out.bgr>
// scene.bin: int32 {h, w, rows, joints, hm_h, hm_w, images, image}, sp_heat_style, hm float [rows, joints, hm_h, hm_w],
// trans_inv float [rows, 6], keep int32 [rows], keep_count int32 [images], seg int32 [images + 1], lut uint8 [256, 3], pixels uint8 [h, w, 3].
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sp_heat.h"

template <typename T>
static T* take(FILE* f, size_t n) {
    T* p = (T*)malloc(n * sizeof(T) ? n * sizeof(T) : 1);        // exactly n elements
    if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "scene file is too short\n"); exit(2); }
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: heat_core_main <scene.bin> <out.bgr>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t* hd = take<int32_t>(f, 8);
    const int h = hd[0], w = hd[1], rows = hd[2], joints = hd[3], hm_h = hd[4], hm_w = hd[5], images = hd[6], image = hd[7];
    sp_heat_style* st = take<sp_heat_style>(f, 1);
    const size_t cells = (size_t)hm_h * hm_w;
    float* hm = take<float>(f, (size_t)rows * joints * cells);
    float* trans_inv = take<float>(f, (size_t)rows * 6);
    int32_t* keep = take<int32_t>(f, (size_t)rows);
    int32_t* keep_count = take<int32_t>(f, (size_t)images);
    int32_t* seg = take<int32_t>(f, (size_t)images + 1);
    unsigned char* lut = take<unsigned char>(f, 768);
    unsigned char* src = take<unsigned char>(f, (size_t)h * w * 3);
    fclose(f);

    sp_heat_rec* recs = (sp_heat_rec*)malloc(rows ? sizeof(sp_heat_rec) * (size_t)rows : 1);
    unsigned char* planes = (unsigned char*)malloc(rows ? (size_t)rows * cells : 1);
    memset(planes, 0xEE, rows ? (size_t)rows * cells : 1);       // a dead slot's plane is never written, and never read
    const uint64_t mask = sp_heat_joints(st->joint_mask, joints);
    int live = 0;
    for (int p = 0; p < rows; ++p) {                             // heat_planes_kernel
        const int row = sp_heat_row_at(keep, keep_count, seg, image, rows, p);
        recs[p] = sp_heat_empty();
        if (row >= 0 && mask != 0ull) recs[p] = sp_heat_record(trans_inv + (size_t)row * 6, hm_h, hm_w);
        if (recs[p].x0 > recs[p].x1) continue;
        ++live;
        for (size_t i = 0; i < cells; ++i) planes[(size_t)p * cells + i] = (unsigned char)sp_heat_cell(hm + (size_t)row * joints * cells, cells, i, mask, st->scale);
    }
    unsigned char* dst = (unsigned char*)malloc((size_t)h * w * 3);
    memcpy(dst, src, (size_t)h * w * 3);
    int* list = (int*)malloc(rows ? sizeof(int) * (size_t)rows : 1);
    long changed = 0, listed = 0;
    for (int ty0 = 0; ty0 < h; ty0 += 16)                        // heat_tile_kernel
        for (int tx0 = 0; tx0 < w; tx0 += 64) {
            const int tx1 = (tx0 + 64 < w ? tx0 + 64 : w) - 1, ty1 = (ty0 + 16 < h ? ty0 + 16 : h) - 1;
            int n = 0;
            for (int i = 0; i < rows; ++i) {
                const sp_heat_rec& r = recs[i];
                if (r.x0 <= tx1 && r.x1 >= tx0 && r.y0 <= ty1 && r.y1 >= ty0 && sp_heat_reaches(r.c, hm_h, hm_w, tx0, ty0, tx1, ty1)) list[n++] = i;
            }
            listed += n;
            for (int y = ty0; y <= ty1; ++y)
                for (int x = tx0; x <= tx1; ++x) {
                    uint32_t vmax = 0u, every = 0u;
                    for (int k = 0; k < n; ++k) {
                        const sp_heat_rec& r = recs[list[k]];
                        const uint32_t v = sp_heat_sample(planes + (size_t)list[k] * cells, hm_h, hm_w, r.c[0] * x + r.c[1] * y + r.c[2],
                                                          r.c[3] * x + r.c[4] * y + r.c[5]);
                        vmax = v > vmax ? v : vmax;
                    }
                    for (int i = 0; i < rows; ++i) {             // without boxes and lists: every slot whose forward map was accepted
                        const sp_heat_rec& r = recs[i];
                        if (r.x0 > r.x1) continue;
                        const uint32_t v = sp_heat_sample(planes + (size_t)i * cells, hm_h, hm_w, r.c[0] * x + r.c[1] * y + r.c[2],
                                                          r.c[3] * x + r.c[4] * y + r.c[5]);
                        every = v > every ? v : every;
                    }
                    if (every != vmax) { fprintf(stderr, "pixel (%d, %d): %u through the lists, %u without them\n", x, y, vmax, every); return 3; }
                    changed += sp_heat_apply(*st, vmax, lut, dst + ((size_t)y * w + x) * 3) ? 1 : 0;
                }
        }
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(dst, 1, (size_t)h * w * 3, o) != (size_t)h * w * 3) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fclose(o);
    printf("OK %dx%d records %d live %d listed %ld blended %ld\n", w, h, rows, live, listed, changed);
    free(hd); free(st); free(hm); free(trans_inv); free(keep); free(keep_count); free(seg); free(lut); free(src); free(recs); free(planes); free(dst);
    free(list);
    return 0;
}
