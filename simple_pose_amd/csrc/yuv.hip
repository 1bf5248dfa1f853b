// yuv.hip - video frames in and out: YUV 4:2:0 (NV12 / I420, pitched planes) <-> packed BGR, one launch per call, for one frame (described
// by the kernel's arguments) or a table of differently sized frames in device memory (sp_yuv_ref, one grid row per frame).  Everything that
// defines a byte lives in sp_yuv.h (the constant table, the pixel functions, the 2-row x 16-column patch functions), shared with the
// stand-alone CPU program tests/yuv_core_main.cpp; this file only hands patches to threads and checks arguments.
// HBM-bound, 4.5 B per pixel: a thread owns whole 2x2 blocks, so chroma is read (averaged) once and no thread needs another's pixels.
// Full patches of a frame whose bases and pitches are multiples of 16 move 16 B per access (Y rows, the NV12 chroma row, three stores /
// loads per 48 B BGR row; 8 B for the I420 chroma rows); tails, the last row of an odd height and unaligned frames go byte by byte.
#include "sp_common.h"
#include "sp_yuv.h"

#include <stdint.h>

namespace {

// one frame, both directions: grid-stride over its patches, patch column fastest (neighbouring lanes, neighbouring 16 / 48 B pieces of a row)
template <bool TO_BGR>
__device__ __forceinline__ void yuv_frame(const sp_yuv_ref& f) {
    if (!sp_yuv_ref_ok(f)) return;                            // (the single-frame calls have refused it on the host; a table entry is skipped)
    const sp_yuv_coef k = sp_yuv_coefs(f.matrix, f.range);
    const bool wide = sp_yuv_wide(f);
    const long long n = sp_yuv_patches(f.h, f.w);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        if (TO_BGR) sp_yuv_patch_to_bgr(f, k, wide, i);
        else sp_yuv_patch_from_bgr(f, k, wide, i);
    }
}

template <bool TO_BGR>
__global__ __launch_bounds__(256) void yuv420_frame_kernel(const sp_yuv_ref f) { yuv_frame<TO_BGR>(f); }

template <bool TO_BGR>
__global__ __launch_bounds__(256) void yuv420_images_kernel(const sp_yuv_ref* __restrict__ frames) {
    const sp_yuv_ref f = frames[blockIdx.y];
    yuv_frame<TO_BGR>(f);
}

// [p, p + (rows - 1) * pitch + row_bytes) of two planes share a byte
bool overlap(const unsigned char* a, int rows_a, int pitch_a, int bytes_a, const unsigned char* b, int rows_b, int pitch_b, int bytes_b) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)(rows_a - 1) * (uintptr_t)pitch_a + (uintptr_t)bytes_a;
    const uintptr_t b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)(rows_b - 1) * (uintptr_t)pitch_b + (uintptr_t)bytes_b;
    return a0 < b1 && b0 < a1;
}

// the host checks of the single-frame calls (sp_yuv_ref_ok's conditions one by one, for the message), then the overlap rules
int check_frame(const char* who, const sp_yuv_ref& f, bool to_bgr) {
    SP_REQUIRE(f.h >= 1 && f.w >= 1 && f.h <= 32767 && f.w <= 32767, "%s: bad size %dx%d (1 .. 32767 a side)", who, f.h, f.w);
    SP_REQUIRE(f.format == SP_YUV_NV12 || f.format == SP_YUV_I420, "%s: format %d (SP_YUV_NV12 = 0, SP_YUV_I420 = 1)", who, f.format);
    SP_REQUIRE(f.matrix == SP_YUV_BT601 || f.matrix == SP_YUV_BT709, "%s: matrix %d (SP_YUV_BT601 = 0, SP_YUV_BT709 = 1)", who, f.matrix);
    SP_REQUIRE(f.range == SP_YUV_LIMITED || f.range == SP_YUV_FULL, "%s: range %d (SP_YUV_LIMITED = 0, SP_YUV_FULL = 1)", who, f.range);
    SP_REQUIRE(f.y && f.u && f.bgr && (f.format == SP_YUV_NV12 || f.v), "%s: null pointer", who);
    const int cb = sp_yuv_chroma_row_bytes(f.w, f.format), ch = (f.h + 1) / 2;
    SP_REQUIRE(f.pitch_y >= f.w, "%s: pitch_y %d below the row (%d bytes)", who, f.pitch_y, f.w);
    SP_REQUIRE(f.pitch_c >= cb, "%s: pitch_c %d below the chroma row (%d bytes)", who, f.pitch_c, cb);
    SP_REQUIRE(f.pitch_bgr >= 3 * f.w, "%s: pitch_bgr %d below the row (%d bytes)", who, f.pitch_bgr, 3 * f.w);
    const bool i420 = f.format == SP_YUV_I420;
    SP_REQUIRE(!overlap(f.bgr, f.h, f.pitch_bgr, 3 * f.w, f.y, f.h, f.pitch_y, f.w) && !overlap(f.bgr, f.h, f.pitch_bgr, 3 * f.w, f.u, ch, f.pitch_c, cb) &&
                   !(i420 && overlap(f.bgr, f.h, f.pitch_bgr, 3 * f.w, f.v, ch, f.pitch_c, cb)),
               "%s: the BGR image overlaps a plane", who);
    if (!to_bgr)
        SP_REQUIRE(!overlap(f.y, f.h, f.pitch_y, f.w, f.u, ch, f.pitch_c, cb) && !(i420 && overlap(f.y, f.h, f.pitch_y, f.w, f.v, ch, f.pitch_c, cb)) &&
                       !(i420 && overlap(f.u, ch, f.pitch_c, cb, f.v, ch, f.pitch_c, cb)),
                   "%s: the output planes overlap each other", who);
    return SP_OK;
}

template <bool TO_BGR>
int launch_frame(const char* who, const sp_yuv_ref& f, void* stream) {
    const int rc = check_frame(who, f, TO_BGR);
    if (rc != SP_OK) return rc;
    hipLaunchKernelGGL(yuv420_frame_kernel<TO_BGR>, dim3(sp_grid_for(sp_yuv_patches(f.h, f.w), 256)), dim3(256), 0, (hipStream_t)stream, f);
    return sp_check_launch(who);
}

template <bool TO_BGR>
int launch_images(const char* who, const sp_yuv_ref* frames_dev, int count, int max_h, int max_w, void* stream) {
    SP_REQUIRE(count >= 0 && count <= 65535, "%s: count %d (0 .. 65535)", who, count);
    if (count == 0) return SP_OK;
    SP_REQUIRE(frames_dev, "%s: null pointer", who);
    SP_REQUIRE(max_h >= 1 && max_w >= 1 && max_h <= 32767 && max_w <= 32767, "%s: bad bounds %dx%d (1 .. 32767 a side)", who, max_h, max_w);
    hipLaunchKernelGGL(yuv420_images_kernel<TO_BGR>, dim3(sp_grid_for(sp_yuv_patches(max_h, max_w), 256), count), dim3(256), 0, (hipStream_t)stream,
                       frames_dev);
    return sp_check_launch(who);
}

sp_yuv_ref make_ref(const unsigned char* y, const unsigned char* u, const unsigned char* v, const unsigned char* bgr, int h, int w, int pitch_y,
                    int pitch_c, int pitch_bgr, int format, int matrix, int range) {
    sp_yuv_ref f;
    f.y = const_cast<unsigned char*>(y); f.u = const_cast<unsigned char*>(u); f.v = const_cast<unsigned char*>(v);
    f.bgr = const_cast<unsigned char*>(bgr);
    f.h = h; f.w = w; f.pitch_y = pitch_y; f.pitch_c = pitch_c; f.pitch_bgr = pitch_bgr;
    f.format = format; f.matrix = matrix; f.range = range;
    return f;
}

}  // namespace

extern "C" int sp_yuv420_to_bgr_u8c3(const unsigned char* y, const unsigned char* u, const unsigned char* v, int h, int w, int pitch_y, int pitch_c,
                                     int format, int matrix, int range, unsigned char* bgr, int pitch_bgr, void* stream) {
    return launch_frame<true>("sp_yuv420_to_bgr_u8c3", make_ref(y, u, v, bgr, h, w, pitch_y, pitch_c, pitch_bgr, format, matrix, range), stream);
}

extern "C" int sp_bgr_to_yuv420_u8c3(const unsigned char* bgr, int pitch_bgr, int h, int w, int format, int matrix, int range, unsigned char* y,
                                     unsigned char* u, unsigned char* v, int pitch_y, int pitch_c, void* stream) {
    return launch_frame<false>("sp_bgr_to_yuv420_u8c3", make_ref(y, u, v, bgr, h, w, pitch_y, pitch_c, pitch_bgr, format, matrix, range), stream);
}

extern "C" int sp_yuv420_to_bgr_images_u8c3(const sp_yuv_ref* frames_dev, int count, int max_h, int max_w, void* stream) {
    return launch_images<true>("sp_yuv420_to_bgr_images_u8c3", frames_dev, count, max_h, max_w, stream);
}

extern "C" int sp_bgr_to_yuv420_images_u8c3(const sp_yuv_ref* frames_dev, int count, int max_h, int max_w, void* stream) {
    return launch_images<false>("sp_bgr_to_yuv420_images_u8c3", frames_dev, count, max_h, max_w, stream);
}

extern "C" int sp_yuv420_wide_path(const void* y, const void* u, const void* v, const void* bgr, int pitch_y, int pitch_c, int pitch_bgr, int format) {
    return sp_yuv_wide(make_ref((const unsigned char*)y, (const unsigned char*)u, (const unsigned char*)v, (const unsigned char*)bgr, 1, 1, pitch_y,
                                pitch_c, pitch_bgr, format, 0, 0))
               ? 1
               : 0;
}
