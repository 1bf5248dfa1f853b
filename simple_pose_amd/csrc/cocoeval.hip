// cocoeval.hip - COCO keypoint AP / AR: the algorithm of pycocotools' COCOeval(gt, dt, "keypoints") evaluate() + accumulate().
// Replaces what metrics/pose_metrics.py:182-209 (evaluate_map) and eval.py:13-27 (eval_kps) hand to pycocotools on the host.
// Three kernels: per image (score rank + cut, detection areas, the OKS matrix, greedy matching at every threshold and area range),
// a stable global order of the kept detections, and per (threshold, area range) the tp / fp scan, the precision envelope and the
// recall-threshold sampling.  All arithmetic in fp64, operation by operation as numpy evaluates it (contraction OFF, numpy's
// pairwise add.reduce order for the per-joint sum); tp / fp are integer counts, so precision and recall are IEEE divisions of exact
// operands.  Capacities (SP_COCO_*, simple_pose_hip.h) are enforced, never truncated to.
#include "sp_common.h"
#include "sp_oks.h"

#pragma clang fp contract(off)

namespace {

constexpr int CE_MAX_JOINTS = SP_COCO_MAX_JOINTS;
constexpr int CE_MAX_GT = SP_COCO_MAX_GT_PER_IMAGE;
constexpr int CE_MAX_DT = SP_COCO_MAX_DT_PER_IMAGE;
constexpr int CE_MAX_KEEP = SP_COCO_MAX_DETS;
constexpr int CE_MAX_THR = SP_COCO_MAX_THRS;
constexpr int CE_MAX_AREA = SP_COCO_MAX_AREAS;
constexpr int CE_MAX_REC = SP_COCO_MAX_REC_THRS;
constexpr double CE_SPACING1 = 2.220446049250313e-16;     // np.spacing(1) = 2^-52

struct CeParams {
    double var[CE_MAX_JOINTS];         // (2 sigma)^2
    double thr[CE_MAX_THR];            // iouThrs
    double area[CE_MAX_AREA][2];       // areaRng
    int J, T, A, max_dets;
};

struct CeRec {
    double thr[CE_MAX_REC];            // recThrs
    int R;
};

// (score desc, NaN last, position asc): a total order, so ranks are a permutation
__device__ __forceinline__ bool score_before(double sj, int j, double si, int i) {
    const bool nj = sj != sj, ni = si != si;
    if (nj || ni) return nj ? (ni && j < i) : true;
    return sj > si || (sj == si && j < i);
}

__device__ __forceinline__ double dt_coord(const void* xy, int f64, size_t idx) {
    return f64 ? ((const double*)xy)[idx] : (double)((const float*)xy)[idx];
}

// computeOks: one detection (row `row` of dt_xy [P,J,2]) against one ground truth
__device__ double oks_pair(const void* dt_xy, int xy_f64, size_t row, const double* __restrict__ gk /* [J][3] */, const double* __restrict__ bb,
                           double gt_area, const CeParams& prm) {
    const int J = prm.J;
    double term[CE_MAX_JOINTS];
    int k1 = 0;
    for (int j = 0; j < J; ++j) k1 += gk[j * 3 + 2] > 0 ? 1 : 0;
    const double x0 = bb[0] - bb[2], x1 = bb[0] + bb[2] * 2, y0 = bb[1] - bb[3], y1 = bb[1] + bb[3] * 2;
    const double denom = gt_area + CE_SPACING1;
    int n = 0;
    for (int j = 0; j < J; ++j) {
        const double xd = dt_coord(dt_xy, xy_f64, (row * J + j) * 2), yd = dt_coord(dt_xy, xy_f64, (row * J + j) * 2 + 1);
        double dx, dy;
        if (k1 > 0) {
            if (!(gk[j * 3 + 2] > 0)) continue;                // e = e[vg > 0]
            dx = xd - gk[j * 3];
            dy = yd - gk[j * 3 + 1];
        } else {                                               // distance to the doubled box
            dx = fmax(0.0, x0 - xd) + fmax(0.0, xd - x1);
            dy = fmax(0.0, y0 - yd) + fmax(0.0, yd - y1);
        }
        const double e = (dx * dx + dy * dy) / prm.var[j] / denom / 2;
        term[n++] = exp(-e);
    }
    return np_pairwise_sum(term, n) / (double)n;
}

// loadRes + evaluate() of one image per workgroup.  Slot k of image i (k < max_dets) is its k-th detection in score order.
__global__ __launch_bounds__(256) void coco_image_kernel(
    const int* __restrict__ gt_seg, const double* __restrict__ gt_kps, const double* __restrict__ gt_area, const double* __restrict__ gt_bbox,
    const int* __restrict__ gt_flag, const int* __restrict__ dt_seg, const int* __restrict__ dt_index, const void* __restrict__ dt_xy,
    const void* __restrict__ dt_score, int dt_flags, const CeParams prm, int n_slots, int n_gt, int* __restrict__ dt_count,
    int* __restrict__ dt_keep, double* __restrict__ dt_kscore, double* __restrict__ dt_karea, double* __restrict__ oks_out,
    int* __restrict__ dtm, unsigned char* __restrict__ dt_ig, unsigned char* __restrict__ gt_ig) {
    __shared__ int kept[CE_MAX_KEEP];
    __shared__ double karea[CE_MAX_KEEP];
    __shared__ double oks[CE_MAX_KEEP * CE_MAX_GT];
    __shared__ unsigned char ig[CE_MAX_AREA][CE_MAX_GT];
    __shared__ unsigned char gorder[CE_MAX_AREA][CE_MAX_GT];
    __shared__ unsigned char gtm[CE_MAX_THR * CE_MAX_AREA][CE_MAX_GT];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int g0 = gt_seg[img], G = gt_seg[img + 1] - g0, d0 = dt_seg[img], N = dt_seg[img + 1] - d0;
    const int J = prm.J, T = prm.T, A = prm.A, max_dets = prm.max_dets;
    const int slot0 = img * max_dets;
    const int xy_f64 = dt_flags & SP_COCO_DT_XY_F64, sc_f64 = dt_flags & SP_COCO_DT_SCORE_F64;
    for (int k = tid; k < max_dets; k += 256) {
        dt_keep[slot0 + k] = -1;
        dt_kscore[slot0 + k] = 0.0;
        dt_karea[slot0 + k] = 0.0;
    }
    for (int idx = tid; idx < A * T * max_dets; idx += 256) {
        const size_t o = (size_t)(idx / max_dets) * n_slots + slot0 + idx % max_dets;
        dtm[o] = -1;
        dt_ig[o] = 0;
    }
    __syncthreads();                                          // the fills above and the results below come from different lanes
    if (G < 0 || N < 0 || G > CE_MAX_GT || N > CE_MAX_DT) {   // uniform: nothing of this image is evaluated, the host raises
        if (tid == 0) dt_count[img] = (G < 0 || G > CE_MAX_GT) ? -2 : -1;
        return;
    }
    const int D = N < max_dets ? N : max_dets;
    // dt = sorted(dt, key=-score, stable)[:max_dets]
    for (int i = tid; i < N; i += 256) {
        const int ri = dt_index ? dt_index[d0 + i] : d0 + i;
        const double si = sc_f64 ? ((const double*)dt_score)[ri] : (double)((const float*)dt_score)[ri];
        int rank = 0;
        for (int j = 0; j < N; ++j) {
            const int rj = dt_index ? dt_index[d0 + j] : d0 + j;
            const double sj = sc_f64 ? ((const double*)dt_score)[rj] : (double)((const float*)dt_score)[rj];
            rank += score_before(sj, j, si, i) ? 1 : 0;
        }
        if (rank < D) {
            kept[rank] = ri;
            dt_keep[slot0 + rank] = ri;
            dt_kscore[slot0 + rank] = si;
        }
    }
    // _ignore per area range, and gtind = argsort(_ignore, stable)
    if (tid < A) {
        const double lo = prm.area[tid][0], hi = prm.area[tid][1];
        int n = 0;
        for (int g = 0; g < G; ++g) {
            const double ar = gt_area[g0 + g];
            const unsigned char f = ((gt_flag[g0 + g] & SP_COCO_GT_IGNORE) || ar < lo || ar > hi) ? 1 : 0;
            ig[tid][g] = f;
            gt_ig[(size_t)tid * n_gt + g0 + g] = f;
            if (!f) gorder[tid][n++] = (unsigned char)g;
        }
        for (int g = 0; g < G; ++g)
            if (ig[tid][g]) gorder[tid][n++] = (unsigned char)g;
    }
    for (int idx = tid; idx < A * T * G; idx += 256) gtm[idx / G][idx % G] = 0;
    __syncthreads();
    // loadRes: area = (max x - min x) * (max y - min y) over all joints
    if (tid < D) {
        const size_t row = kept[tid];
        double x0 = dt_coord(dt_xy, xy_f64, row * J * 2), x1 = x0, y0 = dt_coord(dt_xy, xy_f64, row * J * 2 + 1), y1 = y0;
        for (int j = 1; j < J; ++j) {
            const double x = dt_coord(dt_xy, xy_f64, (row * J + j) * 2), y = dt_coord(dt_xy, xy_f64, (row * J + j) * 2 + 1);
            x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1;
            y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
        }
        const double ar = (x1 - x0) * (y1 - y0);
        karea[tid] = ar;
        dt_karea[slot0 + tid] = ar;
    }
    // computeOks: one lane per (detection, ground truth)
    for (int pair = tid; pair < D * G; pair += 256) {
        const int d = pair / G, g = pair % G;
        const double o = oks_pair(dt_xy, xy_f64, (size_t)kept[d], gt_kps + (size_t)(g0 + g) * J * 3, gt_bbox + (size_t)(g0 + g) * 4, gt_area[g0 + g], prm);
        oks[d * CE_MAX_GT + g] = o;
        oks_out[(size_t)g0 * max_dets + pair] = o;
    }
    __syncthreads();
    // evaluateImg: one lane per (area range, threshold), sequential over detections and ground truths
    if (tid < A * T) {
        const int a = tid / T;
        const double t = prm.thr[tid % T], lo = prm.area[a][0], hi = prm.area[a][1];
        const double start = t < 1 - 1e-10 ? t : 1 - 1e-10;
        for (int d = 0; d < D; ++d) {
            double best = start;
            int m = -1;
            for (int gi = 0; gi < G; ++gi) {
                const int g = gorder[a][gi];
                if (gtm[tid][g] && !(gt_flag[g0 + g] & SP_COCO_GT_CROWD)) continue;
                if (m > -1 && !ig[a][m] && ig[a][g]) break;
                if (oks[d * CE_MAX_GT + g] < best) continue;
                best = oks[d * CE_MAX_GT + g];
                m = g;
            }
            const size_t o = (size_t)tid * n_slots + slot0 + d;
            if (m == -1) {
                dt_ig[o] = (karea[d] < lo || karea[d] > hi) ? 1 : 0;
            } else {
                dt_ig[o] = ig[a][m];
                dtm[o] = g0 + m;
                gtm[tid][m] = 1;
            }
        }
    }
    if (tid == 0) dt_count[img] = D;
}

__device__ __forceinline__ bool slot_valid(const int* __restrict__ dt_count, int max_dets, int n_slots, int s) {
    return s < n_slots && (s % max_dets) < dt_count[s / max_dets];
}

// accumulate(): inds = argsort(-dtScores, kind='mergesort') over the kept detections of all images in image order, as a tiled rank by
// counting: key = (kept first, score desc, slot asc).  sorted_slot[rank] = slot; the kept detections fill ranks [0, K).
__global__ __launch_bounds__(256) void coco_rank_kernel(const int* __restrict__ dt_count, const double* __restrict__ dt_kscore, int max_dets,
                                                        int n_slots, int* __restrict__ sorted_slot) {
    __shared__ double s_sc[256];
    __shared__ unsigned char s_ok[256];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    const bool vi = slot_valid(dt_count, max_dets, n_slots, i);
    const double si = vi ? dt_kscore[i] : 0.0;
    int rank = 0;
    for (int base = 0; base < n_slots; base += 256) {
        const int j = base + tid;
        const bool vj = slot_valid(dt_count, max_dets, n_slots, j);
        s_ok[tid] = vj ? 1 : 0;
        s_sc[tid] = vj ? dt_kscore[j] : 0.0;
        __syncthreads();
        const int lim = n_slots - base < 256 ? n_slots - base : 256;
        for (int jj = 0; jj < lim; ++jj) {
            const bool okj = s_ok[jj] != 0;
            const bool before = okj != vi ? okj : (okj ? score_before(s_sc[jj], base + jj, si, i) : base + jj < i);
            rank += before ? 1 : 0;
        }
        __syncthreads();
    }
    if (i < n_slots) sorted_slot[rank] = i;
}

// accumulate() of one (area range, threshold) per workgroup: tp / fp scan, rc, pr, the envelope from the right, searchsorted sampling.
// precision [T, R, A], recall [T, A]; entries stay -1 when the range has no non-ignored ground truth.
__global__ __launch_bounds__(256) void coco_curve_kernel(const int* __restrict__ dt_count, const int* __restrict__ dtm,
                                                         const unsigned char* __restrict__ dt_ig, const unsigned char* __restrict__ gt_ig,
                                                         const int* __restrict__ sorted_slot, int images, int n_gt, int n_slots, int T, int A,
                                                         const CeRec rec, int* __restrict__ ws_tp, double* __restrict__ ws_pr,
                                                         double* __restrict__ precision, double* __restrict__ recall) {
    __shared__ int lds4[4];
    __shared__ int s_red[2];
    __shared__ double s_max[256];
    const int at = blockIdx.x, a = at / T, t = at % T, tid = threadIdx.x, R = rec.R;
    if (tid == 0) s_red[0] = s_red[1] = 0;
    __syncthreads();
    int k = 0, np = 0;
    for (int i = tid; i < images; i += 256) k += dt_count[i] > 0 ? dt_count[i] : 0;
    for (int g = tid; g < n_gt; g += 256) np += gt_ig[(size_t)a * n_gt + g] ? 0 : 1;
    atomicAdd(&s_red[0], k);
    atomicAdd(&s_red[1], np);
    __syncthreads();
    const int K = s_red[0], npig = s_red[1];
    for (int r = tid; r < R; r += 256) precision[((size_t)t * R + r) * A + a] = -1.0;
    if (tid == 0) recall[t * A + a] = -1.0;
    if (npig == 0) return;                                    // uniform
    int* tp = ws_tp + (size_t)at * n_slots;
    double* pr = ws_pr + (size_t)at * n_slots;
    int carry_tp = 0, carry_fp = 0;
    for (int base = 0; base < K; base += 256) {
        const int i = base + tid;
        int f_tp = 0, f_fp = 0;
        if (i < K) {
            const size_t o = (size_t)at * n_slots + sorted_slot[i];
            const bool matched = dtm[o] >= 0, ignored = dt_ig[o] != 0;
            f_tp = (matched && !ignored) ? 1 : 0;
            f_fp = (!matched && !ignored) ? 1 : 0;
        }
        int tot_tp, tot_fp;
        const int c_tp = carry_tp + sp_block_scan256(f_tp, lds4, tot_tp) + f_tp;
        const int c_fp = carry_fp + sp_block_scan256(f_fp, lds4, tot_fp) + f_fp;
        if (i < K) {
            tp[i] = c_tp;
            pr[i] = (double)c_tp / ((double)c_fp + (double)c_tp + CE_SPACING1);
        }
        carry_tp += tot_tp;
        carry_fp += tot_fp;
    }
    __syncthreads();
    // for i in range(nd - 1, 0, -1): if pr[i] > pr[i - 1]: pr[i - 1] = pr[i]   (a running maximum from the right: exact in any grouping)
    double carry = -1.0;
    for (int base = K > 0 ? (K - 1) / 256 * 256 : -1; base >= 0; base -= 256) {
        const int i = base + tid;
        s_max[tid] = i < K ? pr[i] : -1.0;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const double o = tid + off < 256 ? s_max[tid + off] : -1.0;
            __syncthreads();
            if (o > s_max[tid]) s_max[tid] = o;
            __syncthreads();
        }
        const double v = s_max[tid] > carry ? s_max[tid] : carry;
        if (i < K) pr[i] = v;
        carry = s_max[0] > carry ? s_max[0] : carry;
        __syncthreads();
    }
    if (tid == 0) recall[t * A + a] = K > 0 ? (double)carry_tp / (double)npig : 0.0;
    // inds = np.searchsorted(rc, recThrs, side='left'); q[ri] = pr[pi], 0 once pi runs off the end
    for (int r = tid; r < R; r += 256) {
        const double want = rec.thr[r];
        int lo = 0, hi = K;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((double)tp[mid] / (double)npig < want) lo = mid + 1; else hi = mid;
        }
        precision[((size_t)t * R + r) * A + a] = lo < K ? pr[lo] : 0.0;
    }
}

}  // namespace

extern "C" int sp_coco_kp_eval_images(const int32_t* gt_seg, const double* gt_kps, const double* gt_area, const double* gt_bbox,
                                      const int32_t* gt_flag, const int32_t* dt_seg, const int32_t* dt_index, const void* dt_xy,
                                      const void* dt_score, int dt_flags, int images, int n_gt, int max_gt, int max_dt, int joints,
                                      const double* sigmas_host, int max_dets, const double* iou_thrs_host, int n_thrs,
                                      const double* area_rng_host, int n_areas, int32_t* dt_count, int32_t* dt_keep, double* dt_kscore,
                                      double* dt_karea, double* oks, int32_t* dtm, unsigned char* dt_ignore, unsigned char* gt_ignore,
                                      void* stream) {
    SP_REQUIRE(gt_seg && dt_seg && dt_count && dt_keep && dt_kscore && dt_karea && dtm && dt_ignore, "sp_coco_kp_eval_images: null pointer");
    SP_REQUIRE(iou_thrs_host && area_rng_host, "sp_coco_kp_eval_images: null threshold / area table");
    SP_REQUIRE(images > 0 && n_gt >= 0 && max_gt >= 0 && max_dt >= 0, "sp_coco_kp_eval_images: images=%d n_gt=%d max_gt=%d max_dt=%d", images, n_gt,
               max_gt, max_dt);
    SP_REQUIRE(n_gt == 0 || (gt_kps && gt_area && gt_bbox && gt_flag && gt_ignore && oks), "sp_coco_kp_eval_images: null ground-truth pointer");
    SP_REQUIRE(max_dt == 0 || (dt_xy && dt_score), "sp_coco_kp_eval_images: null detection pointer");
    SP_REQUIRE(joints > 0 && joints <= CE_MAX_JOINTS, "sp_coco_kp_eval_images: joints=%d (1..%d)", joints, CE_MAX_JOINTS);
    SP_REQUIRE(sigmas_host || joints == 17, "sp_coco_kp_eval_images: the default sigmas are COCO's 17; pass sigmas for %d joints", joints);
    SP_REQUIRE(max_dets > 0 && max_dets <= CE_MAX_KEEP, "sp_coco_kp_eval_images: max_dets=%d (1..%d)", max_dets, CE_MAX_KEEP);
    SP_REQUIRE(n_thrs > 0 && n_thrs <= CE_MAX_THR && n_areas > 0 && n_areas <= CE_MAX_AREA, "sp_coco_kp_eval_images: n_thrs=%d (1..%d) n_areas=%d (1..%d)",
               n_thrs, CE_MAX_THR, n_areas, CE_MAX_AREA);
    SP_REQUIRE(max_gt <= CE_MAX_GT, "sp_coco_kp_eval_images: %d ground truths in one image (limit %d)", max_gt, CE_MAX_GT);
    SP_REQUIRE(max_dt <= CE_MAX_DT, "sp_coco_kp_eval_images: %d detections in one image (limit %d)", max_dt, CE_MAX_DT);
    SP_REQUIRE((long long)images * max_dets <= 0x7fffffffLL / (CE_MAX_THR * CE_MAX_AREA), "sp_coco_kp_eval_images: %d images x %d slots overflow", images,
               max_dets);
    CeParams prm;
    for (int j = 0; j < CE_MAX_JOINTS; ++j) prm.var[j] = 1.0;
    for (int j = 0; j < joints; ++j) {
        const double s = sigmas_host ? sigmas_host[j] : sp_coco_sigma10(j) / 10.0;
        prm.var[j] = (s * 2) * (s * 2);                        // vars = (sigmas * 2) ** 2
    }
    for (int t = 0; t < CE_MAX_THR; ++t) prm.thr[t] = t < n_thrs ? iou_thrs_host[t] : 0.0;
    for (int a = 0; a < CE_MAX_AREA; ++a) {
        prm.area[a][0] = a < n_areas ? area_rng_host[a * 2] : 0.0;
        prm.area[a][1] = a < n_areas ? area_rng_host[a * 2 + 1] : 0.0;
    }
    prm.J = joints; prm.T = n_thrs; prm.A = n_areas; prm.max_dets = max_dets;
    hipLaunchKernelGGL(coco_image_kernel, dim3(images), dim3(256), 0, (hipStream_t)stream, gt_seg, gt_kps, gt_area, gt_bbox, gt_flag, dt_seg,
                       dt_index, dt_xy, dt_score, dt_flags, prm, images * max_dets, n_gt, dt_count, dt_keep, dt_kscore, dt_karea, oks, dtm,
                       dt_ignore, gt_ignore);
    return sp_check_launch("coco_image_kernel");
}

extern "C" int sp_coco_kp_accumulate_workspace(int images, int max_dets, int n_thrs, int n_areas, int64_t* bytes) {
    SP_REQUIRE(bytes, "sp_coco_kp_accumulate_workspace: null pointer");
    SP_REQUIRE(images > 0 && max_dets > 0 && max_dets <= CE_MAX_KEEP && n_thrs > 0 && n_thrs <= CE_MAX_THR && n_areas > 0 && n_areas <= CE_MAX_AREA,
               "sp_coco_kp_accumulate_workspace: images=%d max_dets=%d n_thrs=%d n_areas=%d", images, max_dets, n_thrs, n_areas);
    const int64_t slots = (int64_t)images * max_dets;
    // sorted_slot int32 [slots] (padded to 8 bytes), then per (area, threshold) pr double [slots] and tp int32 [slots]
    *bytes = (slots * 4 + 7) / 8 * 8 + (int64_t)n_thrs * n_areas * slots * 12;
    return SP_OK;
}

extern "C" int sp_coco_kp_accumulate(const int32_t* dt_count, const double* dt_kscore, const int32_t* dtm, const unsigned char* dt_ignore,
                                     const unsigned char* gt_ignore, int images, int n_gt, int max_dets, int n_thrs, int n_areas,
                                     const double* rec_thrs_host, int n_rec, void* workspace, int64_t workspace_bytes, double* precision,
                                     double* recall, void* stream) {
    SP_REQUIRE(dt_count && dt_kscore && dtm && dt_ignore && workspace && precision && recall && rec_thrs_host, "sp_coco_kp_accumulate: null pointer");
    SP_REQUIRE(n_gt >= 0 && (n_gt == 0 || gt_ignore), "sp_coco_kp_accumulate: n_gt=%d / null gt_ignore", n_gt);
    SP_REQUIRE(n_rec > 0 && n_rec <= CE_MAX_REC, "sp_coco_kp_accumulate: n_rec=%d (1..%d)", n_rec, CE_MAX_REC);
    int64_t need = 0;
    if (sp_coco_kp_accumulate_workspace(images, max_dets, n_thrs, n_areas, &need) != SP_OK) return SP_EINVAL;
    SP_REQUIRE(workspace_bytes >= need, "sp_coco_kp_accumulate: workspace %lld bytes, need %lld", (long long)workspace_bytes, (long long)need);
    SP_REQUIRE((long long)images * max_dets <= 0x7fffffffLL / (CE_MAX_THR * CE_MAX_AREA), "sp_coco_kp_accumulate: %d images x %d slots overflow", images,
               max_dets);
    const int slots = images * max_dets;
    CeRec rec;
    for (int r = 0; r < CE_MAX_REC; ++r) rec.thr[r] = r < n_rec ? rec_thrs_host[r] : 0.0;
    rec.R = n_rec;
    int* sorted_slot = (int*)workspace;
    double* ws_pr = (double*)((char*)workspace + ((int64_t)slots * 4 + 7) / 8 * 8);
    int* ws_tp = (int*)(ws_pr + (int64_t)n_thrs * n_areas * slots);
    hipLaunchKernelGGL(coco_rank_kernel, dim3(sp_ceil_div(slots, 256)), dim3(256), 0, (hipStream_t)stream, dt_count, dt_kscore, max_dets, slots,
                       sorted_slot);
    int rc = sp_check_launch("coco_rank_kernel");
    if (rc != SP_OK) return rc;
    hipLaunchKernelGGL(coco_curve_kernel, dim3(n_thrs * n_areas), dim3(256), 0, (hipStream_t)stream, dt_count, dtm, dt_ignore, gt_ignore, sorted_slot,
                       images, n_gt, slots, n_thrs, n_areas, rec, ws_tp, ws_pr, precision, recall);
    return sp_check_launch("coco_curve_kernel");
}
