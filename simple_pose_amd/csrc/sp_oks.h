// sp_oks.h - what the OKS users (nms.hip: oks_nms; track.hip: the tracker's association; cocoeval.hip: the keypoint evaluator) share:
// numpy's summation order, COCO's per-joint sigmas, and oks_iou of one pair (nms.hip and track.hip call the one oks_one below).  All
// restate numpy float64 code operation by operation, so all sum the per-joint terms as numpy does.
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

// ---- oks_iou of one pair (nms.hip's greedy loop, track.hip's similarity matrix) ------------------------------------------------------
constexpr int NMS_MAX_JOINTS = 64;

struct NmsVar { double v[NMS_MAX_JOINTS]; };             // (2 sigma_j)^2, travels as a kernel argument

// naive_data.py:131-133: `sigmas_host` (`joints` doubles in HOST memory) or, when NULL, COCO's 17
inline void sp_oks_fill_var(NmsVar& var, const double* sigmas_host, int joints) {
    for (int j = 0; j < joints; ++j) {
        const double s = sigmas_host ? sigmas_host[j] : sp_coco_sigma10(j) / 10.0;
        var.v[j] = (s * 2) * (s * 2);
    }
}

// oks_iou (naive_data.py:120-150) of the pick against one candidate; vis_thresh < 0: in_vis_thresh None (every joint counts)
__device__ inline double oks_one(const double* pick /* [J][3] */, const double* __restrict__ cand, double pick_area, double cand_area,
                                 const NmsVar& var, int J, double vis_thresh) {
#pragma clang fp contract(off)
    double term[NMS_MAX_JOINTS];
    float vis_sum = 0.f;
    const double denom = (pick_area + cand_area) / 2 + 1e-12;
    for (int j = 0; j < J; ++j) {
        const double dx = cand[j * 3] - pick[j * 3], dy = cand[j * 3 + 1] - pick[j * 3 + 1];
        const double e = (dx * dx + dy * dy) / var.v[j] / denom / 2;
        float vis = 1.f;
        if (vis_thresh >= 0) vis = (cand[j * 3 + 2] > vis_thresh && pick[j * 3 + 2] > vis_thresh) ? 1.f : 0.f;
        term[j] = exp(-e) * (double)vis;
        vis_sum += vis;
    }
    const float den = vis_sum + (float)1e-12;            // float32 + weak python float stays float32
    return np_pairwise_sum(term, J) / (double)den;
}
