// The patch functions of simple_pose_amd/csrc/sp_yuv.h (what one thread of the kernels in yuv.hip does per step) run serially on the CPU,
// under AddressSanitizer + UBSan (tests/test_yuv_core_cpu.py compiles and runs this), over frames in exactly-sized heap buffers: a read or a
// write one byte outside a plane's [first row, last row + row bytes) is a sanitizer report.  Every frame is compared with a straightforward
// per-pixel loop over the contract (include/simple_pose_hip.h) written here, and every output byte outside the image rows (pitch padding)
// must keep its fill.  Then, over all 2^24 triples: BT.601 full range decodes as sp_jpeg.h's sp_jpeg_ycc_to_bgr and encodes as
// sp_jpeg_enc.h's sp_jpeg_enc_ycc.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sp_jpeg_enc.h"
#include "sp_yuv.h"

namespace {

int failures = 0;
long long wide_patches = 0, narrow_patches = 0;
uint32_t rng_state = 12345u;
uint8_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (uint8_t)(rng_state >> 24); }

// a plane of `rows` rows of `row_bytes` at `pitch`, starting `offset` bytes into a 16-byte aligned heap block that ends with its last row
struct Plane {
    uint8_t* block = nullptr;
    uint8_t* p = nullptr;
    int rows = 0, row_bytes = 0, pitch = 0;
    size_t size = 0;
    Plane(int rows_, int row_bytes_, int pitch_, int offset, bool random) : rows(rows_), row_bytes(row_bytes_), pitch(pitch_) {
        size = (size_t)offset + (size_t)(rows - 1) * pitch + row_bytes;
        void* m = nullptr;
        if (posix_memalign(&m, 16, size) != 0) abort();
        block = (uint8_t*)m;
        p = block + offset;
        for (size_t i = 0; i < size; ++i) block[i] = random ? rnd() : 0xA5;
    }
    Plane(const Plane&) = delete;
    ~Plane() { free(block); }
    uint8_t& at(int r, int c) { return p[(size_t)r * pitch + c]; }
    // every byte outside the rows still 0xA5
    bool padding_intact() const {
        for (size_t i = 0; i < size; ++i) {
            const long long o = (long long)i - (p - block);
            const bool inside = o >= 0 && (o % pitch) < row_bytes && o / pitch < rows;
            if (!inside && block[i] != 0xA5) return false;
        }
        return true;
    }
};

int clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
int mini(int a, int b) { return a < b ? a : b; }

void run_case(int h, int w, int format, int matrix, int range, bool to_bgr, int pad, int offset, int py_fixed = 0, int pc_fixed = 0, int pb_fixed = 0) {
    const int ch = (h + 1) / 2, cw = (w + 1) / 2, cb = format == SP_YUV_NV12 ? 2 * cw : cw;
    const int py = py_fixed ? py_fixed : w + pad, pc = pc_fixed ? pc_fixed : cb + pad, pb = pb_fixed ? pb_fixed : 3 * w + pad;
    Plane Y(h, w, py, offset, to_bgr), U(ch, cb, pc, offset, to_bgr), V(ch, cb, pc, offset, to_bgr), B(h, 3 * w, pb, offset, !to_bgr);
    sp_yuv_ref f;
    f.y = Y.p; f.u = U.p; f.v = format == SP_YUV_I420 ? V.p : nullptr; f.bgr = B.p;
    f.h = h; f.w = w; f.pitch_y = py; f.pitch_c = pc; f.pitch_bgr = pb; f.format = format; f.matrix = matrix; f.range = range;
    char name[160];
    snprintf(name, sizeof name, "%s %dx%d %s m%d r%d pitch %d/%d/%d offset %d", to_bgr ? "to_bgr" : "from_bgr", h, w, format == SP_YUV_NV12 ? "nv12" : "i420",
             matrix, range, py, pc, pb, offset);
    if (!sp_yuv_ref_ok(f)) { printf("FAIL %s: sp_yuv_ref_ok refuses it\n", name); ++failures; return; }
    const sp_yuv_coef k = sp_yuv_coefs(matrix, range);
    const bool wide = sp_yuv_wide(f);
    const long long n = sp_yuv_patches(h, w);
    for (long long i = 0; i < n; ++i) {
        const int pw = sp_yuv_patch_cols(w), br = (int)(i / pw), pcx = (int)(i % pw);
        (wide && pcx * 16 + 16 <= w && 2 * br + 1 < h ? wide_patches : narrow_patches) += 1;
        if (to_bgr) sp_yuv_patch_to_bgr(f, k, wide, i);
        else sp_yuv_patch_from_bgr(f, k, wide, i);
    }
    // the contract, pixel by pixel
    long long bad = 0;
    auto chroma_at = [&](int i, int j, int comp) -> uint8_t& { return format == SP_YUV_NV12 ? U.at(i, 2 * j + comp) : (comp ? V.at(i, j) : U.at(i, j)); };
    if (to_bgr) {
        for (int r = 0; r < h; ++r)
            for (int c = 0; c < w; ++c) {
                const int yy = Y.at(r, c) - k.yoff, uu = chroma_at(r >> 1, c >> 1, 0) - 128, vv = chroma_at(r >> 1, c >> 1, 1) - 128;
                const int R = clamp8((k.ay * yy + k.rv * vv + 32768) >> 16), G = clamp8((k.ay * yy - k.gu * uu - k.gv * vv + 32768) >> 16),
                          Bl = clamp8((k.ay * yy + k.bu * uu + 32768) >> 16);
                bad += B.at(r, 3 * c) != Bl || B.at(r, 3 * c + 1) != G || B.at(r, 3 * c + 2) != R;
            }
        if (!B.padding_intact()) { printf("FAIL %s: a byte outside the image rows was written\n", name); ++failures; }
    } else {
        auto px = [&](int r, int c, int comp) {
            r = mini(r, h - 1); c = mini(c, w - 1);
            const int Bl = B.at(r, 3 * c), G = B.at(r, 3 * c + 1), R = B.at(r, 3 * c + 2);
            if (comp == 0) return (k.yr * R + k.yg * G + k.yb * Bl + (k.yoff << 16) + 32768) >> 16;
            if (comp == 1) return (k.ur * R + k.ug * G + k.ub * Bl + (128 << 16) + 32767) >> 16;
            return (k.vr * R + k.vg * G + k.vb * Bl + (128 << 16) + 32767) >> 16;
        };
        for (int r = 0; r < h; ++r)
            for (int c = 0; c < w; ++c) bad += Y.at(r, c) != px(r, c, 0);
        for (int i = 0; i < ch; ++i)
            for (int j = 0; j < cw; ++j)
                for (int comp = 1; comp <= 2; ++comp) {
                    const int s = px(2 * i, 2 * j, comp) + px(2 * i, 2 * j + 1, comp) + px(2 * i + 1, 2 * j, comp) + px(2 * i + 1, 2 * j + 1, comp);
                    bad += chroma_at(i, j, comp - 1) != ((s + 2) >> 2);
                }
        if (!Y.padding_intact() || !U.padding_intact() || (format == SP_YUV_I420 && !V.padding_intact())) {
            printf("FAIL %s: a byte outside the plane rows was written\n", name);
            ++failures;
        }
    }
    if (bad) { printf("FAIL %s: %lld samples differ from the per-pixel loop\n", name, bad); ++failures; }
    else printf("OK %s\n", name);
}

void jpeg_equivalence() {
    const sp_yuv_coef k = sp_yuv_coefs(SP_YUV_BT601, SP_YUV_FULL);
    long long dec = 0, enc = 0;
    for (int a = 0; a < 256; ++a)
        for (int b = 0; b < 256; ++b)
            for (int c = 0; c < 256; ++c) {
                uint8_t p[3], q[3];
                sp_yuv_to_bgr_px(k, a, b, c, p);
                sp_jpeg_ycc_to_bgr(a, b, c, q);
                dec += p[0] != q[0] || p[1] != q[1] || p[2] != q[2];
                for (int comp = 0; comp < 3; ++comp) enc += sp_yuv_from_bgr_px(k, a, b, c, comp) != sp_jpeg_enc_ycc(a, b, c, comp);
            }
    printf("JPEG decode: %lld of 16777216 triples differ from sp_jpeg_ycc_to_bgr\n", dec);
    printf("JPEG encode: %lld of 50331648 samples differ from sp_jpeg_enc_ycc\n", enc);
    failures += (dec != 0) + (enc != 0);
}

}  // namespace

int main() {
    const int shapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {2, 2}, {3, 5}, {5, 3}, {17, 23}, {16, 64}, {33, 130}};
    int mode = 0;
    for (const auto& s : shapes)
        for (int format = 0; format < 2; ++format)
            for (int dir = 0; dir < 2; ++dir)
                for (int pad = 0; pad <= 13; pad += 13)
                    for (int offset = 0; offset < 2; ++offset, ++mode) run_case(s[0], s[1], format, (mode >> 1) & 1, mode & 1, dir == 0, pad, offset);
    // the 16-byte path with a tail: 33x130 in 16-byte pitches (128 columns of full patches, 2 tail columns, one odd last row), all four modes
    for (int format = 0; format < 2; ++format)
        for (int dir = 0; dir < 2; ++dir)
            for (int m = 0; m < 4; ++m)
                for (int offset = 0; offset < 2; ++offset) run_case(33, 130, format, m >> 1, m & 1, dir == 0, 0, offset, 144, format == SP_YUV_NV12 ? 144 : 80, 400);
    printf("PATCHES wide %lld narrow %lld\n", wide_patches, narrow_patches);
    if (wide_patches == 0 || narrow_patches == 0) { printf("FAIL: one of the two paths never ran\n"); ++failures; }
    jpeg_equivalence();
    printf("%s: %d failures\n", failures ? "FAILED" : "PASSED", failures);
    return failures ? 1 : 0;
}
