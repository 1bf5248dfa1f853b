// sp_common.h - shared helpers of libsimple_pose_hip (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "simple_pose_hip.h"
#include "sp_device.h"

// ---- error plumbing (thread-local message, never throws across the C boundary) ----------------
void sp_set_error(const char* fmt, ...);
int sp_check_launch(const char* what);

// ---- kernel-name query (sp_conv2d_kernel_name): while a query is active on the calling thread, a launch function records the name
// of the kernel instantiation it WOULD launch (as rocprofv3 reports it, without the namespace / argument decoration) and returns
// SP_OK without launching - the name comes out of the dispatch code itself, so it cannot drift from it
bool sp_name_query_active();
void sp_name_query_begin();
const char* sp_name_query_end();
void sp_name_query_set(const char* fmt, ...);

#define SP_REQUIRE(cond, ...)        \
    do {                             \
        if (!(cond)) {               \
            sp_set_error(__VA_ARGS__); \
            return SP_EINVAL;        \
        }                            \
    } while (0)

static inline int sp_ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// ---- limits every entry point that takes a frame's buffers shares ---------------------------------
constexpr int SP_MAX_ROWS = 2048;                // rows of one frame: the OKS-NMS group limit
constexpr int SP_MAX_JOINTS = 64;
constexpr int SP_MAX_DIM = 16384;                // image height and width

// ---- pointer checks of the host entry points -------------------------------------------------------
static inline bool sp_ranges_overlap(const void* a, const void* b, unsigned long long bytes) {
    const unsigned long long x = (unsigned long long)(uintptr_t)a, y = (unsigned long long)(uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

static inline bool sp_aligned_to(const void* p, unsigned n) { return ((uintptr_t)p & (n - 1)) == 0; }

// ---- launch helpers (the ONE place these two rules live; every launcher goes through them) -------
// CUs of the current device, cached per device index; 256 (the MI355X) when the query fails or the index is outside the cache.
int sp_device_cus();

// > 64 KiB of dynamic LDS needs an explicit opt-in, once per kernel instantiation AND per device (the attribute belongs to the
// function on the device that is current: a process driving several GPUs must not inherit device 0's opt-in).  `reserved` holds
// what the kernel has been granted per device index; the attribute is set only when `bytes` exceeds it, so a kernel whose LDS
// size depends on the shape grows its reservation and a fixed-size one pays one hipGetDevice per launch.  A benign race: two
// threads may both set the same attribute, and the larger request is simply made again by whoever finds the smaller one recorded.
// On failure: sp_set_error (`what`, the bytes, the device, the runtime's message) and SP_ELAUNCH.
int sp_reserve_lds_for(const void* kernel, int* reserved, int bytes, const char* what);

template <auto Kernel>
int sp_reserve_lds(int bytes, const char* what) {
    static int reserved[64];
    return sp_reserve_lds_for(reinterpret_cast<const void*>(Kernel), reserved, bytes, what);
}

// ---- device helpers ------------------------------------------------------------------------------
// torch.max semantics: larger value wins, NaN beats everything, ties -> lower index.
__device__ __forceinline__ bool sp_better(float a, int ia, float b, int ib) {
    const bool an = (a != a), bn = (b != b);
    if (an || bn) return an && (!bn || ia < ib);
    return (a > b) || (a == b && ia < ib);
}

__device__ __forceinline__ void sp_wave_argmax(float& v, int& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, SP_WAVE);
        const int oi = __shfl_xor(i, off, SP_WAVE);
        if (sp_better(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

// exclusive prefix sum over the 256 threads of a block (four waves); returns the prefix, `total` = the block sum.  lds: 4 ints.
__device__ __forceinline__ int sp_block_scan256(int v, int* lds, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += lds[w];
    total = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return base + x - v;
}

// sp_invert_affine (cv::warpAffine's inversion of a forward 2x3 map): stated once in sp_affine.h, which the CPU test programs read too
#include "sp_affine.h"
