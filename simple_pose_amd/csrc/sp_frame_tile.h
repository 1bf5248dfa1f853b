// sp_frame_tile.h - what the four frame overlays (render.hip, labels.hip, redact.hip, heat.hip) share around their own rules: each is one
// record kernel and then one tile kernel of 256 threads, a workgroup per 64 x 16 pixel tile and four consecutive pixels per thread.  Here,
// once: the tile's shape and coordinates, a thread's four pixels with their two load / store paths, the ordered list scan, and on the host
// the checks and the path choice every entry point makes.  The limits (SP_MAX_ROWS, SP_MAX_JOINTS, SP_MAX_DIM) and the pointer checks are
// sp_common.h's.  (redact.hip's tile kernel, 16 * RB rows per tile, takes the box test and keeps its own coordinates and pixel words: see there.)
// Device and launch code: the rule headers (sp_render.h ..), which plain C++ programs compile too, do not include it.
#pragma once
#include "sp_common.h"

#include <stdint.h>

constexpr int SP_TILE_NT = 256;
constexpr int SP_TILE_W = 64, SP_TILE_H = 16;    // 256 threads x 4 consecutive pixels of one row

// ---- the tile of this workgroup and the pixels of this thread ----------------------------------------------------------------------------------
struct sp_tile {
    int tx0, ty0;                                // the tile's first pixel
    int x0, y;                                   // the thread's pixels: x0 .. x0 + 3 of row y (a tile of 16 k rows: of the rows y + 16, .. too)
    __device__ __forceinline__ explicit sp_tile(int tile_h = SP_TILE_H)
        : tx0(blockIdx.x * SP_TILE_W), ty0(blockIdx.y * tile_h), x0(tx0 + (threadIdx.x & 15) * 4), y(ty0 + (threadIdx.x >> 4)) {}
};

// does the record's box (inclusive; an empty record has x0 > x1) meet the pixels tx0 .. tx1, ty0 .. ty1 ?
template <class Rec>
__device__ __forceinline__ bool sp_box_meets(const Rec& r, int tx0, int ty0, int tx1, int ty1) {
    return r.x0 <= tx1 && r.x1 >= tx0 && r.y0 <= ty1 && r.y1 >= ty0;
}

// Four consecutive BGR pixels as their 12 bytes in three words: byte b = channel b % 3 of pixel b / 3.  WIDE (sp_frame_wide: w % 4 == 0 and
// 4-byte aligned images) moves the words, and a group of four is inside the row as a whole; otherwise bytes, clipped at w, zeros beyond.
// `at`: the byte offset of pixel (x0, y).
struct sp_px4 {
    uint32_t v[3];

    __device__ __forceinline__ void clear() { v[0] = v[1] = v[2] = 0u; }

    template <bool WIDE>
    __device__ __forceinline__ void load(const unsigned char* img, size_t at, int x0, int w) {
        if (WIDE) {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(img + at);
            v[0] = s[0]; v[1] = s[1]; v[2] = s[2];
        } else {
            clear();
#pragma unroll
            for (int b = 0; b < 12; ++b)
                if (x0 + b / 3 < w) v[b / 4] |= (uint32_t)img[at + b] << (8 * (b % 4));
        }
    }

    template <bool WIDE>
    __device__ __forceinline__ void store(unsigned char* img, size_t at, int x0, int w) const {
        if (WIDE) {
            uint32_t* d = reinterpret_cast<uint32_t*>(img + at);
            d[0] = v[0]; d[1] = v[1]; d[2] = v[2];
        } else {
#pragma unroll
            for (int b = 0; b < 12; ++b)
                if (x0 + b / 3 < w) img[at + b] = (unsigned char)byte(b);
        }
    }

    __device__ __forceinline__ uint32_t byte(int b) const { return (v[b / 4] >> (8 * (b % 4))) & 255u; }

    // the four pixels as the bytes the rules work on (bgr[q]: pixel q), and back: once each per kernel, around all the rules it applies
    __device__ __forceinline__ void unpack(unsigned char (&bgr)[4][3]) const {
#pragma unroll
        for (int b = 0; b < 12; ++b) bgr[b / 3][b % 3] = (unsigned char)byte(b);
    }
    __device__ __forceinline__ void pack(const unsigned char (&bgr)[4][3]) {
        clear();
#pragma unroll
        for (int b = 0; b < 12; ++b) v[b / 4] |= (uint32_t)bgr[b / 3][b % 3] << (8 * (b % 4));
    }
};

// ---- the ordered list scan -------------------------------------------------------------------------------------------------------------------
// Which of recs[0 .. total) meet the tile, handed to `apply(list, count)` in index order, at most LIST indices at a time.  The order is kept
// without atomics: per chunk of 256 records a ballot per wave, the four wave counts through LDS, and every hit lands at (hits before its
// wave) + (hits below its lane).  A list that the next chunk could overflow is applied first.  Every thread of the workgroup calls this and
// `apply` (count is uniform, and > 0); true: something met the tile.
template <int LIST, class Rec, class Apply>
__device__ __forceinline__ bool sp_tile_scan_ordered(const Rec* __restrict__ recs, int total, const sp_tile& t, Apply&& apply) {
    __shared__ int list[LIST];
    __shared__ int wave_hits[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int count = 0;                               // uniform: every thread adds the same totals
    bool touched = false;
    for (int base = 0; base < total; base += SP_TILE_NT) {
        const int i = base + tid;
        const bool hit = i < total && sp_box_meets(recs[i], t.tx0, t.ty0, t.tx0 + SP_TILE_W - 1, t.ty0 + SP_TILE_H - 1);
        const unsigned long long ballot = __ballot(hit);
        if (lane == 0) wave_hits[wave] = __popcll(ballot);
        __syncthreads();                         // the wave counts; and the list entries of the chunk before
        int before = 0, chunk = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int n = wave_hits[v];
            before += v < wave ? n : 0;
            chunk += n;
        }
        if (count + chunk > LIST) {              // uniform; count > 0 here, since a chunk has at most 256 hits
            apply(list, count);
            count = 0;
            __syncthreads();                     // nobody still reads the list
        }
        if (hit) list[count + before + __popcll(ballot & ((1ull << lane) - 1ull))] = i;
        count += chunk;
        touched = touched || chunk > 0;
        __syncthreads();                         // the entries are visible; wave_hits is free for the next chunk
    }
    if (count > 0) apply(list, count);
    return touched;
}

// ---- host side: what every entry point checks before its own style, and the path it picks -----------------------------------------------------------
inline int sp_frame_rows_check(const char* who, int rows) {
    SP_REQUIRE(rows >= 0 && rows <= SP_MAX_ROWS, "%s: rows %d (0..%d, the OKS-NMS group limit)", who, rows, SP_MAX_ROWS);
    return SP_OK;
}

inline int sp_frame_check(const char* who, const void* src, const void* dst, int h, int w, int image, int rows) {
    SP_REQUIRE(src && dst, "%s: null pointer", who);
    SP_REQUIRE(h >= 1 && h <= SP_MAX_DIM && w >= 1 && w <= SP_MAX_DIM, "%s: image %dx%d (1..%d each way)", who, w, h, SP_MAX_DIM);
    SP_REQUIRE(image >= 0, "%s: image index %d", who, image);
    const int rc = sp_frame_rows_check(who, rows);
    if (rc != SP_OK) return rc;
    SP_REQUIRE(dst == src || !sp_ranges_overlap(src, dst, (unsigned long long)h * w * 3),
               "%s: src and dst overlap without being equal (in place, or apart)", who);
    return SP_OK;
}

inline bool sp_frame_wide(int w, const void* src, const void* dst) { return w % 4 == 0 && sp_aligned_to(src, 4) && sp_aligned_to(dst, 4); }
