// sp_device.h - vector types and device primitives shared by the kernels of libsimple_pose_hip (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void_t;

#define SP_WAVE 64

// grid of a grid-stride kernel over `total` items: capped, the loop covers the rest
inline int sp_grid_for(long long total, int block) {
    long long g = (total + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

// running maximum in which NaN propagates like torch's max pooling
__device__ __forceinline__ float sp_pmax(float m, float v) { return (v > m || v != v) ? v : m; }

// raw buffer descriptor over [base, base + bytes): stride 0, range-checked, so an offset >= bytes reads zeros
__device__ __forceinline__ u32x4 sp_make_rsrc(const void* base, unsigned bytes) {
    const unsigned long long a = reinterpret_cast<unsigned long long>(base);
    u32x4 r;                                   // (readfirstlane: an "s" asm operand must be provably wave-uniform)
    r[0] = __builtin_amdgcn_readfirstlane((unsigned)a);
    r[1] = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32) & 0xffffu);      // stride 0: raw buffer
    r[2] = __builtin_amdgcn_readfirstlane(bytes);                              // num_records (bytes)
    r[3] = 0x00020000u;
    return r;
}

// One LDS-DMA piece: 64 lanes x 16 bytes, lane l's bytes from `rsrc` base + voff + soff (zeros when voff is out of range), written
// to LDS at lds_addr + 16 * l (wave-uniform base in M0).  Inline asm on purpose: hipcc treats the builtin form as an LDS store it
// must wait for (`s_waitcnt vmcnt(0)` in front of every later LDS access), which would drain the ring at every K tile; issued
// from asm the transfers are invisible to its bookkeeping and ordered by the calling kernel's own counted `s_waitcnt vmcnt(N)` + s_barrier.
// M0 is written in the statement that uses it (hipcc keeps nothing live in M0 across statements on gfx950, and it does not accept
// "m0" in a clobber list - "inline asm clobber list contains reserved registers" - so the dependence cannot be declared); `s_nop 4` covers the
// M0-write -> LDS-DMA and the VALU-written-SGPR -> VMEM wait states, which nothing pads inside an asm statement.
// Three operand forms: descriptor + scalar offset, descriptor alone (soff = 0 as an immediate), and the compiler's own descriptor type.
__device__ __forceinline__ void sp_dma16(unsigned lds_addr, unsigned voff, u32x4 rsrc, unsigned soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(__builtin_amdgcn_readfirstlane(lds_addr)), "v"(voff),
                 "s"(rsrc), "s"(__builtin_amdgcn_readfirstlane(soff))
                 : "memory");
}
__device__ __forceinline__ void sp_dma16(unsigned lds_addr, unsigned voff, u32x4 rsrc) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(__builtin_amdgcn_readfirstlane(lds_addr)), "v"(voff),
                 "s"(rsrc)
                 : "memory");
}
__device__ __forceinline__ void sp_dma16(unsigned lds_addr, unsigned voff, __amdgpu_buffer_rsrc_t rsrc) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(__builtin_amdgcn_readfirstlane(lds_addr)), "v"(voff), "s"(rsrc)
                 : "memory");
}
