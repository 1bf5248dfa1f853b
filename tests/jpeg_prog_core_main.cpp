// TEST PROGRAM (tests/test_jpeg_prog_core_sanitized.py builds it with -fsanitize=address,undefined): the progressive entropy core of
// simple_pose_amd/csrc/sp_jpeg_prog.h and the host parser sp_jpeg_parse_scans.h, driven on the CPU with the work split of
// jpeg_prog_entropy_kernel (scan after scan, per restart segment), then the IDCT and colour functions of sp_jpeg.h with the work split of
// jpeg.hip.  Every buffer is a heap allocation of exactly the size the library's caller has to provide, so a read or write outside one is
// an AddressSanitizer report.
//   jpeg_prog_core_main <manifest>      lines: <name> <file.jpg> <expected.bgr | -> <fuzz 0|1>
// Prints one line per case; exit status 0 when every case with expected pixels matched, every rejection case was refused and every
// fuzzed input ended in a parser code or a status.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sp_jpeg_parse_scans.h"
#include "sp_jpeg_prog.h"

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
    int32_t nscan = 0;
    int rc = sp_jpeg_parse_scans_impl(file, (int64_t)n, &d, nullptr, 0, &nscan, nullptr, 0, err, sizeof(err));
    if (rc != SP_OK) { free(file); return rc; }
    const int32_t scan_cap = nscan, seg_cap = d.segments;
    sp_jpeg_scan* scans = (sp_jpeg_scan*)malloc(sizeof(sp_jpeg_scan) * (size_t)scan_cap);      // exactly the counts the first call reported
    int32_t* segs = (int32_t*)malloc(sizeof(int32_t) * (size_t)seg_cap);
    rc = sp_jpeg_parse_scans_impl(file, (int64_t)n, &d, scans, scan_cap, &nscan, segs, seg_cap, err, sizeof(err));
    if (rc != SP_OK || nscan != scan_cap || d.segments != seg_cap) { free(file); free(scans); free(segs); return rc != SP_OK ? rc : SP_EINVAL; }
    int32_t bw[3] = {0, 0, 0}, bh[3] = {0, 0, 0}, first[4] = {0, 0, 0, 0};
    int64_t blocks = 0;
    if (!sp_jpeg_geometry(d, bw, bh, blocks)) { free(file); free(scans); free(segs); return SP_EINVAL; }
    for (int c = 0; c < d.components; ++c) first[c + 1] = first[c] + bw[c] * bh[c];
    for (int c = d.components; c < 3; ++c) first[c + 1] = first[c];
    int16_t* coef = (int16_t*)calloc((size_t)d.coef_count, sizeof(int16_t));
    uint8_t* planes = (uint8_t*)malloc((size_t)d.plane_bytes);
    memset(planes, 0, (size_t)d.plane_bytes);
    bgr.assign((size_t)d.out_bytes, 0);
    w = d.width; h = d.height;

    // entropy (jpeg_prog_entropy_kernel)
    sp_jpeg_huff* tabs = (sp_jpeg_huff*)malloc(sizeof(sp_jpeg_huff) * 3);
    int st = 0;
    for (int sc = 0; sc < nscan; ++sc) {
        const sp_jpeg_scan& s = scans[sc];
        sp_jpeg_prog_geom g;
        sp_jpeg_prog_geometry(d, s, g);
        const int ntab = sp_jpeg_prog_tables(g);
        for (int t = 0; t < ntab; ++t) {
            st |= sp_jpeg_huff_build(tabs[t], s.huff_counts[t], s.huff_values[t], 256);
            for (int i = 0; i < (1 << SP_JPEG_LOOKAHEAD); ++i) tabs[t].lut[i] = sp_jpeg_huff_lut_entry(tabs[t], (uint32_t)i);
        }
        const int ri = sp_jpeg_prog_interval(g, s.restart_interval);
        const int expected = (g.mcus + ri - 1) / ri;
        if (s.segments != expected) st |= SP_JPEG_ST_SEGMENTS;
        const int32_t* ssegs = segs + s.seg_index;
        for (int k = 0; k < s.segments && k < expected; ++k) {
            const int begin = sp_jpeg_clampi(ssegs[k], 0, d.file_bytes);
            const int end = sp_jpeg_clampi(k + 1 < s.segments ? ssegs[k + 1] - 2 : s.ecs_end, begin, d.file_bytes);
            const int last = g.mcus < (k + 1) * ri ? g.mcus : (k + 1) * ri;
            st |= sp_jpeg_prog_segment(file + begin, file + end, tabs, g, k * ri, last, coef);
        }
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
    free(tabs); free(planes); free(coef); free(segs); free(scans); free(file);
    return st;
}

// offset of the first FF `marker` among the header segments of a well-formed file, 0 when there is none
static size_t find_marker(const std::vector<uint8_t>& f, int marker) {
    size_t pos = 2;
    while (pos + 4 <= f.size() && f[pos] == 0xFF) {
        if (f[pos + 1] == marker) return pos;
        pos += 2 + (((size_t)f[pos + 2] << 8) | f[pos + 3]);
    }
    return 0;
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
            const size_t sof = find_marker(file, 0xC2), sos = find_marker(file, 0xDA);
            if (!sof || !sos) { printf("FAIL %s: no SOF2 / SOS\n", name); ++failures; continue; }
            int clean = 0, flagged = 0, refused = 0;
            for (size_t cut = sos; cut < file.size(); ++cut) {                             // every truncation after the first SOS
                const int r = decode(file.data(), cut, got, w, h);
                (r < 0 ? refused : (r ? flagged : clean)) += 1;
            }
            printf("FUZZ %s truncations: %d refused, %d flagged, %d clean\n", name, refused, flagged, clean);
            clean = flagged = refused = 0;
            uint64_t rng = 0x9E3779B97F4A7C15ull ^ (uint64_t)file.size();
            for (int k = 0; k < 300; ++k) {                                                // 300 seeded single-byte corruptions after SOF
                rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                std::vector<uint8_t> bad(file);
                const size_t at = sof + (size_t)((rng >> 33) % (file.size() - sof));
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
