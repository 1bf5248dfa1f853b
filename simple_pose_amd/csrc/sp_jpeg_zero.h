// sp_jpeg_zero.h - zeroing of one image's coefficient region, shared by the zeroing kernels of jpeg.hip and jpeg_prog.hip (both entropy
// stages write only non-zero coefficients).  Device code; include after sp_common.h.
#pragma once
#include <stdint.h>

#include "sp_device.h"

// Thread `tid` of `threads`: the region's own n int16 only (what lies between two regions is the caller's).  16-byte stores over the
// aligned body, single int16 stores over the at most 7 + 7 elements around it (threads >= 8).
__device__ __forceinline__ void sp_jpeg_zero_region(int16_t* p, int n, int tid, int threads) {
    const int head = min(n, (int)((16 - ((uintptr_t)p & 15)) & 15) / 2);          // elements up to the first 16-byte boundary
    const int vecs = (n - head) / 8;
    u32x4* body = reinterpret_cast<u32x4*>(p + head);
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (int i = tid; i < vecs; i += threads) body[i] = zero;
    if (tid < head) p[tid] = 0;
    const int tail0 = head + vecs * 8;
    if (tid < n - tail0) p[tail0 + tid] = 0;
}
