// sp_affine.h - the inversion of a 2x3 affine map, ONE statement of it for the device, the host and the CPU test programs (plain C++:
// no HIP header is needed to read this file; sp_common.h includes it for every kernel file).
#pragma once

#ifdef __HIPCC__
#define SP_AFFINE_HD __host__ __device__ inline
#else
#define SP_AFFINE_HD inline
#endif

// cv::warpAffine without WARP_INVERSE_MAP: the forward 2x3 map inverted in double, this way.  ONE statement of it for the host callers
// (sp_warp_affine_*), the device callers (sp_topdown_plan, the heat overlay's forward map) and tests/heat_core_main.cpp, whose maps must
// agree bit for bit: contraction is off inside (a compiler without the pragma is given -ffp-contract=off).
SP_AFFINE_HD void sp_invert_affine(const double* fwd, double* inv) {
#pragma clang fp contract(off)
    double M[6];
    for (int i = 0; i < 6; ++i) M[i] = fwd[i];
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1. / D : 0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
    const double b1 = -M[0] * M[2] - M[1] * M[5], b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1; M[5] = b2;
    for (int i = 0; i < 6; ++i) inv[i] = M[i];
}
