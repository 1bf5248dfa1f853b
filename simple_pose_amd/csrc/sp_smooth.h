// sp_smooth.h - the One-Euro filter of one tracked joint (sp_track_smooth), ONE definition for the kernel in track.hip, the CPU program
// tests/smooth_core_main.cpp and, restated in numpy, tests/smooth_ref.py.  All arithmetic is fp64 with contraction OFF, in exactly the
// order written here; the only operations are + - * /, fabs, comparisons and exact fp32 -> fp64 conversions - deliberately no sqrt and no
// exp - so the device computes the host's bits.  One comparison is added to the published recursion: a sample equal to the filtered value
// leaves it as it is, because a * x + (1 - a) * x rounds to x only within an ulp and a constant pose has to come out exactly unchanged.
// The rules are written out in include/simple_pose_hip.h above sp_track_smooth.
// (Casiez, Roussel, Vogel: "1 Euro Filter: A Simple Speed-based Low-pass Filter for Noisy Input in Interactive Systems", CHI 2012.)
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define SP_SMOOTH_HD __host__ __device__ inline
#else
#define SP_SMOOTH_HD inline
#endif

#define SP_SMOOTH_TWO_PI 6.283185307179586

struct sp_smooth_params {
    double min_cutoff, beta, d_cutoff;   // Hz, 1 / body size, Hz
    double max_gap;                      // seconds: a joint not updated for longer starts again
    double in_vis_thre;                  // a sample is usable iff its c > in_vis_thre
};

// every finite double, and nothing else
SP_SMOOTH_HD bool sp_smooth_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// The row's body size: max(x2 - x1, y2 - y1) of its box (x1, y1, x2, y2, ..), subtraction and max in fp32 (w > h ? w : h), widened;
// 1.0 unless that is > 0 (a NaN included).
SP_SMOOTH_HD double sp_smooth_size(const float* box) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float w = box[2] - box[0], h = box[3] - box[1];
    const double size = (double)(w > h ? w : h);
    return size > 0.0 ? size : 1.0;
}

// One joint, one sample (x, y, c) at time `now`.  State: xh[2] (the filtered position), dxh[2] (the filtered speed, px / s), *t_last,
// *n (samples accepted; 0 = uninitialised).  out[3] = the filtered sample; c is never filtered.  Returns whether the sample was accepted
// (the state was written).
SP_SMOOTH_HD bool sp_smooth_joint(const sp_smooth_params& p, double x, double y, double c, double now, double size, double* xh, double* dxh,
                                  double* t_last, int32_t* n, double* out) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    out[0] = x; out[1] = y; out[2] = c;
    if (!(c > p.in_vis_thre) || !sp_smooth_finite(x) || !sp_smooth_finite(y)) return false;       // not usable: raw out, state untouched
    const double Te = now - *t_last;
    if (*n == 0 || !(Te > 0.0) || Te > p.max_gap) {                                        // first sample, or too old: (re)initialise
        xh[0] = x; xh[1] = y;
        dxh[0] = 0.0; dxh[1] = 0.0;
        *n = 1;
        *t_last = now;
        return true;
    }
    const double s[2] = {x, y};
    for (int a = 0; a < 2; ++a) {
        const double d = (s[a] - xh[a]) / Te;
        const double rd = (SP_SMOOTH_TWO_PI * p.d_cutoff) * Te;
        const double ad = rd / (rd + 1.0);
        dxh[a] = ad * d + (1.0 - ad) * dxh[a];
        const double fc = p.min_cutoff + p.beta * (fabs(dxh[a]) / size);
        const double r = (SP_SMOOTH_TWO_PI * fc) * Te;
        const double al = r / (r + 1.0);
        if (s[a] != xh[a]) xh[a] = al * s[a] + (1.0 - al) * xh[a];           // (equal: x^ stays, exactly)
        out[a] = xh[a];
    }
    *n = *n + 1;
    *t_last = now;
    return true;
}
