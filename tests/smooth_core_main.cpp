// TEST PROGRAM (tests/test_smooth_core_cpu.py builds it with -fsanitize=address,undefined -ffp-contract=off): the key-point smoother's rules
// of simple_pose_amd/csrc/sp_smooth.h driven on the CPU with the work split of track_smooth_kernel in track.hip (one row at a time: copy, is
// it kept, find the id's slot, take the slot over, then one joint at a time).  Every buffer is a heap allocation of exactly the size the
// library's caller has to provide, so a read or write outside one is an AddressSanitizer report.
//   smooth_core_main <sequence.bin> <out.bin>
// sequence.bin: int32 {slots, joints, rows, frames}, double {min_cutoff, beta, d_cutoff, max_gap, in_vis_thre}, then per frame: double now,
// kps double [rows, joints, 3], box float [rows, 5], track_id int32 [rows], keep int32 [rows], keep_count int32 [1], seg int32 [2],
// t_id int32 [slots].  out.bin, per frame: kps_smooth double [rows, joints, 3], s_id int32 [slots], s_x double [slots, joints, 2],
// s_dx double [slots, joints, 2], s_t double [slots, joints], s_n int32 [slots, joints].
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sp_smooth.h"

template <typename T>
static T* take(FILE* f, size_t n) {
    T* p = (T*)malloc(n * sizeof(T) ? n * sizeof(T) : 1);        // exactly n elements
    if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "sequence file is too short\n"); exit(2); }
    return p;
}

template <typename T>
static T* zeros(size_t n) {
    T* p = (T*)malloc(n * sizeof(T));
    memset(p, 0, n * sizeof(T));
    return p;
}

template <typename T>
static void put(FILE* o, const T* p, size_t n) {
    if (fwrite(p, sizeof(T), n, o) != n) { fprintf(stderr, "cannot write the output\n"); exit(2); }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: smooth_core_main <sequence.bin> <out.bin>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) { fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]); return 2; }
    int32_t* hd = take<int32_t>(f, 4);
    const int slots = hd[0], J = hd[1], rows = hd[2], frames = hd[3];
    double* pr = take<double>(f, 5);
    const sp_smooth_params prm = {pr[0], pr[1], pr[2], pr[3], pr[4]};
    int32_t* s_id = zeros<int32_t>((size_t)slots);
    double* s_x = zeros<double>((size_t)slots * J * 2);
    double* s_dx = zeros<double>((size_t)slots * J * 2);
    double* s_t = zeros<double>((size_t)slots * J);
    int32_t* s_n = zeros<int32_t>((size_t)slots * J);
    long filtered = 0;
    for (int fr = 0; fr < frames; ++fr) {
        double* now = take<double>(f, 1);
        double* kps = take<double>(f, (size_t)rows * J * 3);
        float* box = take<float>(f, (size_t)rows * 5);
        int32_t* tid = take<int32_t>(f, (size_t)rows);
        int32_t* keep = take<int32_t>(f, (size_t)rows);
        int32_t* keep_count = take<int32_t>(f, 1);
        int32_t* seg = take<int32_t>(f, 2);
        int32_t* t_id = take<int32_t>(f, (size_t)slots);
        double* out = (double*)malloc(sizeof(double) * (size_t)rows * J * 3);
        int lo = seg[0], n = 0;                                  // frame_poses of track.hip
        if (lo < 0 || lo > rows) lo = 0;
        else {
            n = keep_count[0] < 0 ? 0 : keep_count[0];
            n = n > slots ? slots : n;
            n = n > rows - lo ? rows - lo : n;
        }
        for (int row = 0; row < rows; ++row) {                   // one workgroup of track_smooth_kernel
            const double* src = kps + (size_t)row * J * 3;
            double* dst = out + (size_t)row * J * 3;
            bool kept = false;
            for (int p = 0; p < n; ++p) kept |= keep[lo + p] == row;
            const int id = tid[row];
            int slot = slots;
            for (int t = slots - 1; t >= 0; --t)
                if (t_id[t] == id) slot = t;
            if (!kept || id <= 0 || slot >= slots) {
                for (int i = 0; i < J * 3; ++i) dst[i] = src[i];
                continue;
            }
            const bool fresh = s_id[slot] != id;
            if (fresh) s_id[slot] = id;
            const double size = sp_smooth_size(box + (size_t)row * 5);
            for (int j = 0; j < J; ++j) {                        // one lane
                const size_t sj = (size_t)slot * J + j;
                if (fresh) s_n[sj] = 0;
                sp_smooth_joint(prm, src[j * 3], src[j * 3 + 1], src[j * 3 + 2], now[0], size, s_x + sj * 2, s_dx + sj * 2, s_t + sj, s_n + sj,
                                dst + j * 3);
                ++filtered;
            }
        }
        put(o, out, (size_t)rows * J * 3);
        put(o, s_id, (size_t)slots);
        put(o, s_x, (size_t)slots * J * 2);
        put(o, s_dx, (size_t)slots * J * 2);
        put(o, s_t, (size_t)slots * J);
        put(o, s_n, (size_t)slots * J);
        free(now); free(kps); free(box); free(tid); free(keep); free(keep_count); free(seg); free(t_id); free(out);
    }
    fclose(f);
    fclose(o);
    printf("OK frames %d rows %d joints filtered %ld\n", frames, rows, filtered);
    free(hd); free(pr); free(s_id); free(s_x); free(s_dx); free(s_t); free(s_n);
    return 0;
}
