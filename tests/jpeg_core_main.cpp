// TEST PROGRAM (tests/test_jpeg_core_sanitized.py builds it with -fsanitize=address,undefined): the decoder core of
// simple_pose_amd/csrc/sp_jpeg.h and the host parser sp_jpeg_parse.h, driven on the CPU with the work split of the kernels in jpeg.hip
// (per restart segment, per block, per pixel).  Every buffer is a heap allocation of exactly the size the library's caller has to
// provide, so a read or write outside one is an AddressSanitizer report.
//   jpeg_core_main <manifest>      lines: <name> <file.jpg> <expected.bgr | -> <fuzz 0|1>
// Prints one line per case; exit status 0 when every case with expected pixels matched and every fuzzed input ended in a status.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "sp_jpeg_parse.h"

static bool read_file(const char* path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize((size_t)n);
    const bool ok = n == 0 || fread(out.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}

// Decode `n` bytes at `src`.  Returns the parse code (< 0), or the status word (>= 0) with the pixels in `bgr`.
static int decode(const uint8_t* src, size_t n, std::vector<uint8_t>& bgr, int& w, int& h) {
    uint8_t* file = (uint8_t*)malloc(n ? n : 1);             // exactly n bytes: reading file[n] is a report
    memcpy(file, src, n);
    sp_jpeg_desc d;
    char err[256];
    int32_t nseg_cap = 0;
    int rc = sp_jpeg_parse_impl(file, (int64_t)n, &d, nullptr, 0, err, sizeof(err));
    if (rc != SP_OK) { free(file); return rc; }
    nseg_cap = d.segments;
    int32_t* segs = (int32_t*)malloc(sizeof(int32_t) * (size_t)nseg_cap);
    rc = sp_jpeg_parse_impl(file, (int64_t)n, &d, segs, nseg_cap, err, sizeof(err));
    if (rc != SP_OK || d.segments != nseg_cap) { free(file); free(segs); return rc != SP_OK ? rc : SP_EINVAL; }
    int32_t bw[3] = {0, 0, 0}, bh[3] = {0, 0, 0}, first[4] = {0, 0, 0, 0};
    int64_t blocks = 0;
    if (!sp_jpeg_geometry(d, bw, bh, blocks)) { free(file); free(segs); return SP_EINVAL; }
    for (int c = 0; c < d.components; ++c) first[c + 1] = first[c] + bw[c] * bh[c];
    for (int c = d.components; c < 3; ++c) first[c + 1] = first[c];
    int16_t* coef = (int16_t*)calloc((size_t)d.coef_count, sizeof(int16_t));
    uint8_t* planes = (uint8_t*)malloc((size_t)d.plane_bytes);
    memset(planes, 0, (size_t)d.plane_bytes);
    bgr.assign((size_t)d.out_bytes, 0);
    w = d.width; h = d.height;

    // entropy (jpeg_entropy_kernel)
    sp_jpeg_huff* tabs = (sp_jpeg_huff*)malloc(sizeof(sp_jpeg_huff) * 6);
    int st = 0;
    for (int t = 0; t < 2 * d.components; ++t) {
        const int c = t >> 1, cls = t & 1;
        const int sel = 4 * cls + ((cls ? d.ac_sel[c] : d.dc_sel[c]) & 3);
        st |= sp_jpeg_huff_build(tabs[t], d.huff_counts[sel], d.huff_values[sel], 256);
        for (int i = 0; i < (1 << SP_JPEG_LOOKAHEAD); ++i) tabs[t].lut[i] = sp_jpeg_huff_lut_entry(tabs[t], (uint32_t)i);
    }
    const int mcus = d.mcus_x * d.mcus_y;
    const int ri = d.restart_interval > 0 ? d.restart_interval : mcus;
    const int expected = (mcus + ri - 1) / ri;
    if (d.segments != expected) st |= SP_JPEG_ST_SEGMENTS;
    for (int s = 0; s < d.segments && s < expected; ++s) {
        const int begin = sp_jpeg_clampi(segs[s], 0, d.file_bytes);
        const int end = sp_jpeg_clampi(s + 1 < d.segments ? segs[s + 1] - 2 : d.ecs_end, begin, d.file_bytes);
        sp_jpeg_bits b;
        sp_jpeg_bits_init(b, file + begin, file + end);
        int32_t pred[3] = {0, 0, 0};
        const int last = mcus < (s + 1) * ri ? mcus : (s + 1) * ri;
        for (int mcu = s * ri; mcu < last && !b.status; ++mcu) {
            const int my = mcu / d.mcus_x, mx = mcu - my * d.mcus_x;
            for (int c = 0; c < d.components && !b.status; ++c)
                for (int vy = 0; vy < d.v_samp[c] && !b.status; ++vy)
                    for (int hx = 0; hx < d.h_samp[c] && !b.status; ++hx) {
                        const int blk = first[c] + (my * d.v_samp[c] + vy) * bw[c] + mx * d.h_samp[c] + hx;
                        sp_jpeg_decode_block(b, tabs[2 * c], tabs[2 * c + 1], pred[c], coef + (size_t)blk * 64);
                    }
        }
        st |= b.status;
    }
    // IDCT (jpeg_idct_kernel)
    for (int blk = 0; blk < first[3]; ++blk) {
        const int c = (d.components == 3 && blk >= first[2]) ? 2 : ((d.components == 3 && blk >= first[1]) ? 1 : 0);
        int32_t ws[8 * 9];
        for (int j = 0; j < 8; ++j) sp_jpeg_idct_column(coef + (size_t)blk * 64, d.quant[d.quant_sel[c] & 3], j, ws, 9);
        const int local = blk - first[c], by = local / bw[c], bx = local - by * bw[c], pitch = bw[c] * 8;
        for (int j = 0; j < 8; ++j) sp_jpeg_idct_row(ws + j * 9, planes + (size_t)first[c] * 64 + (size_t)(by * 8 + j) * pitch + bx * 8);
    }
    // colour (jpeg_color_kernel)
    const int hs = d.h_samp[0], vs = d.v_samp[0];
    const int cw = (d.width + hs - 1) / hs, ch = (d.height + vs - 1) / vs;
    const uint8_t* py = planes;
    const uint8_t* pcb = planes + (size_t)first[1] * 64;
    const uint8_t* pcr = planes + (size_t)first[2] * 64;
    const int ypitch = bw[0] * 8, cpitch = bw[1] * 8;
    for (int y = 0; y < d.height; ++y)
        for (int x = 0; x < d.width; ++x) {
            const int Y = py[(size_t)y * ypitch + x];
            uint8_t* p = bgr.data() + ((size_t)y * d.width + x) * 3;
            if (d.components == 1) { p[0] = p[1] = p[2] = (uint8_t)Y; continue; }
            int cb, cr;
            if (hs == 2 && vs == 2) {
                cb = sp_jpeg_up_h2v2(pcb, cpitch, cw, ch, x, y);
                cr = sp_jpeg_up_h2v2(pcr, cpitch, cw, ch, x, y);
            } else if (hs == 2) {
                cb = sp_jpeg_up_h2v1(pcb + (size_t)y * cpitch, cw, x);
                cr = sp_jpeg_up_h2v1(pcr + (size_t)y * cpitch, cw, x);
            } else {
                cb = pcb[(size_t)y * cpitch + x];
                cr = pcr[(size_t)y * cpitch + x];
            }
            sp_jpeg_ycc_to_bgr(Y, cb, cr, p);
        }
    free(tabs); free(planes); free(coef); free(segs); free(file);
    return st;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <manifest>\n", argv[0]); return 2; }
    FILE* mf = fopen(argv[1], "r");
    if (!mf) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char name[256], jpg[1024], exp[1024];
    int fuzz = 0, failures = 0;
    while (fscanf(mf, "%255s %1023s %1023s %d", name, jpg, exp, &fuzz) == 4) {
        std::vector<uint8_t> file, want, got;
        if (!read_file(jpg, file)) { printf("FAIL %s: cannot read %s\n", name, jpg); ++failures; continue; }
        int w = 0, h = 0;
        const int rc = decode(file.data(), file.size(), got, w, h);
        if (strcmp(exp, "-") != 0) {
            if (!read_file(exp, want)) { printf("FAIL %s: cannot read %s\n", name, exp); ++failures; continue; }
            size_t diff = 0;
            if (rc == 0 && want.size() == got.size())
                for (size_t i = 0; i < want.size(); ++i) diff += want[i] != got[i];
            const bool ok = rc == 0 && want.size() == got.size() && diff == 0;
            printf("%s %s: rc %d, %dx%d, %zu differing bytes\n", ok ? "OK" : "FAIL", name, rc, w, h, diff);
            failures += !ok;
        } else {
            printf("%s %s: rc %d\n", rc < 0 ? "OK" : "FAIL", name, rc);      // a rejection case: the parser has to refuse it
            failures += !(rc < 0);
        }
        if (fuzz) {
            sp_jpeg_desc d;
            char err[256];
            if (sp_jpeg_parse_impl(file.data(), (int64_t)file.size(), &d, nullptr, 0, err, sizeof(err)) != SP_OK) { ++failures; continue; }
            int clean = 0, flagged = 0, refused = 0;
            for (size_t cut = (size_t)d.ecs_offset; cut < file.size(); ++cut) {          // every truncation of the entropy data
                const int r = decode(file.data(), cut, got, w, h);
                (r < 0 ? refused : (r ? flagged : clean)) += 1;
            }
            printf("FUZZ %s truncations: %d refused, %d flagged, %d clean\n", name, refused, flagged, clean);
            clean = flagged = refused = 0;
            uint64_t rng = 0x9E3779B97F4A7C15ull ^ (uint64_t)file.size();
            for (int k = 0; k < 200; ++k) {                                                // 200 seeded single-byte corruptions
                rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                std::vector<uint8_t> bad(file);
                const size_t at = (size_t)((rng >> 33) % file.size());
                bad[at] = (uint8_t)(bad[at] ^ (uint8_t)(1u + ((rng >> 20) % 255u)));
                const int r = decode(bad.data(), bad.size(), got, w, h);
                (r < 0 ? refused : (r ? flagged : clean)) += 1;
            }
            printf("FUZZ %s corruptions: %d refused, %d flagged, %d clean\n", name, refused, flagged, clean);
        }
    }
    fclose(mf);
    printf("%s: %d failures\n", failures ? "FAILED" : "PASSED", failures);
    return failures ? 1 : 0;
}
