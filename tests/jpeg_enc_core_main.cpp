// tests/jpeg_enc_core_main.cpp - the JPEG encoder's integer core (simple_pose_amd/csrc/sp_jpeg_enc.h) and host planner
// (sp_jpeg_enc_plan.h) as a stand-alone CPU program, built with -fsanitize=address,undefined by tests/test_jpeg_enc_core_sanitized.py.
// It runs the stages of sp_jpeg_encode_batch serially through the same inline functions the kernels call (block by block, the three
// prefix sums as plain loops), compares every fixture case with the file libjpeg-turbo wrote, and for the cases marked so encodes into
// every capacity from 0 to the true length: each has to end in SP_JPEG_ENC_STATUS_OVERFLOW with nothing written, in exactly allocated
// buffers the sanitizer watches.
//
//   jpeg_enc_core_main manifest.txt       lines: name image.bgr width height subsampling quality interval expected.jpg sweep(0/1)
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "sp_jpeg_enc_plan.h"

static std::vector<uint8_t> read_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct PlainOr {
    void operator()(uint32_t* p, uint32_t v) const { *p |= v; }
};

// -> status; `out` holds exactly `cap` bytes
static int encode(const uint8_t* src, const sp_jpeg_enc_desc& d, uint8_t* out, int64_t cap, int64_t& length) {
    length = 0;
    // stage coef
    std::vector<int16_t> coef((size_t)d.blocks * 64);
    std::vector<uint16_t> bits(d.blocks);
    for (int b = 0; b < d.blocks; ++b) {
        const sp_jpeg_enc_blk k = sp_jpeg_enc_locate(d, b);
        sp_jpeg_enc_block(src, d, k, coef.data() + (size_t)b * 64);
        bits[b] = (uint16_t)sp_jpeg_enc_ac_bits(coef.data() + (size_t)b * 64, d.hlen[k.comp ? 3 : 1]);
    }
    for (int b = 0; b < d.blocks; ++b) {
        const sp_jpeg_enc_blk k = sp_jpeg_enc_locate(d, b);
        bits[b] = (uint16_t)(bits[b] + sp_jpeg_enc_dc_bits(sp_jpeg_enc_dc_diff(coef.data(), d, b, k), d.hlen[k.comp ? 2 : 0]));
    }
    // stage scan
    std::vector<uint64_t> pos(d.blocks + 1), seg(d.segments + 1);
    for (int b = 0; b < d.blocks; ++b) pos[b + 1] = pos[b] + bits[b];
    for (int s = 0, b = 0; s < d.segments; ++s) {
        int ss, first, end;
        sp_jpeg_enc_segment(d, b, ss, first, end);
        if (ss != s || first != b) { printf("segment %d: starts at block %d, not %d\n", s, first, b); exit(2); }
        seg[s + 1] = seg[s] + (pos[end] - pos[first] + 7) / 8;
        b = end;
    }
    const uint64_t ubytes = seg[d.segments];
    if (ubytes > (uint64_t)sp_jpeg_enc_stream_cap(d, cap)) return SP_JPEG_ENC_STATUS_OVERFLOW;
    // stage emit
    std::vector<uint32_t> stream((ubytes + 3) / 4);
    for (int b = 0; b < d.blocks; ++b) {
        const sp_jpeg_enc_blk k = sp_jpeg_enc_locate(d, b);
        int s, first, end;
        sp_jpeg_enc_segment(d, b, s, first, end);
        sp_jpeg_enc_writer w;
        sp_jpeg_enc_writer_init(w, stream.data(), stream.size(), 8 * seg[s] + (pos[b] - pos[first]));
        const int t = k.comp ? 2 : 0;
        sp_jpeg_enc_emit_block(w, coef.data() + (size_t)b * 64, sp_jpeg_enc_dc_diff(coef.data(), d, b, k), d.hcode[t], d.hlen[t], d.hcode[t + 1],
                               d.hlen[t + 1], b + 1 == end, PlainOr());
    }
    // stage stuff
    const uint8_t* ub = reinterpret_cast<const uint8_t*>(stream.data());
    uint64_t ff = 0;
    for (uint64_t u = 0; u < ubytes; ++u) ff += ub[u] == 0xFF;
    const uint64_t bytes = sp_jpeg_enc_file_bytes(d, ubytes, ff);
    if (bytes > (uint64_t)cap) return SP_JPEG_ENC_STATUS_OVERFLOW;
    for (int i = 0; i < d.header_bytes; ++i) out[i] = d.header[i];
    ff = 0;
    for (uint64_t u = 0, s = 0; u < ubytes; ++u) {
        if (u >= seg[s + 1]) ++s;
        ff += sp_jpeg_enc_place_byte(out, d.header_bytes, u, ff, (int)s, d.segments, seg[s + 1], ub[u]);
    }
    length = (int64_t)bytes;
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s manifest.txt\n", argv[0]);
        return 2;
    }
    std::ifstream mf(argv[1]);
    std::string line;
    int failures = 0;
    while (std::getline(mf, line)) {
        std::istringstream ls(line);
        std::string name, image, expected;
        int w, h, sub, q, r, sweep;
        if (!(ls >> name >> image >> w >> h >> sub >> q >> r >> expected >> sweep)) continue;
        const std::vector<uint8_t> src = read_file(image), want = read_file(expected);
        sp_jpeg_enc_desc d;
        char err[256];
        if (sp_jpeg_enc_plan_impl(w, h, sub, q, r, &d, err, (int)sizeof(err)) != SP_OK || src.size() != (size_t)w * h * 3) {
            printf("FAIL %s: plan: %s\n", name.c_str(), err);
            ++failures;
            continue;
        }
        std::vector<uint8_t> out(want.size());
        int64_t length = 0;
        const int st = encode(src.data(), d, out.data(), (int64_t)out.size(), length);
        if (st != 0 || length != (int64_t)want.size() || out != want) {
            printf("FAIL %s: status %d, %lld bytes against %zu\n", name.c_str(), st, (long long)length, want.size());
            ++failures;
            continue;
        }
        printf("OK %s %lld bytes\n", name.c_str(), (long long)length);
        if (sweep) {
            int bad = 0;
            for (size_t cap = 0; cap < want.size(); ++cap) {
                std::vector<uint8_t> small(cap, 0xA5);
                const int s2 = encode(src.data(), d, small.data(), (int64_t)cap, length);
                bool touched = false;
                for (uint8_t v : small) touched |= v != 0xA5;
                if (s2 != SP_JPEG_ENC_STATUS_OVERFLOW || length != 0 || touched) ++bad;
            }
            printf("SWEEP %s capacities 0..%zu: %d not refused cleanly\n", name.c_str(), want.size() - 1, bad);
            failures += bad;
        }
    }
    // every refusal of the planner
    sp_jpeg_enc_desc d;
    char err[256];
    const int refusals[][6] = {{0, 8, 420, 75, 0, SP_JPEG_ESIZE},     {8, 16385, 420, 75, 0, SP_JPEG_ESIZE}, {8, 8, 411, 75, 0, SP_JPEG_ESAMPLING},
                               {8, 8, 420, 0, 0, SP_EINVAL},          {8, 8, 420, 101, 0, SP_EINVAL},        {8, 8, 420, 75, -1, SP_EINVAL},
                               {8, 8, 420, 75, 65536, SP_EINVAL}};
    for (const auto& c : refusals)
        if (sp_jpeg_enc_plan_impl(c[0], c[1], c[2], c[3], c[4], &d, err, (int)sizeof(err)) != c[5]) {
            printf("FAIL plan(%d, %d, %d, %d, %d) is not refused with %d\n", c[0], c[1], c[2], c[3], c[4], c[5]);
            ++failures;
        }
    printf("PASSED: %d failures\n", failures);
    return failures ? 1 : 0;
}
