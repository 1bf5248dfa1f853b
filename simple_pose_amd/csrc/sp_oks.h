// sp_oks.h - what the two OKS users (nms.hip: oks_nms; cocoeval.hip: the keypoint evaluator) share: numpy's summation order and
// COCO's per-joint sigmas.  Both restate numpy float64 code operation by operation, so both sum the per-joint terms as numpy does.
#pragma once
#include <hip/hip_runtime.h>

// numpy float64 add.reduce over a contiguous run: 8 interleaved accumulators over the multiple-of-8 prefix, combined as
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), tail in order; n < 8: in order.  (n <= 128: numpy's PW_BLOCKSIZE, above it numpy recurses.)
__device__ inline double np_pairwise_sum(const double* a, int n) {
#pragma clang fp contract(off)
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

// naive_data.py:131-133 / COCOeval's kpt_oks_sigmas: the 17 COCO values; sigma_j = sp_coco_sigma10(j) / 10.0
inline double sp_coco_sigma10(int j) {
    static const double coco[17] = {.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89};
    return coco[j];
}
