// track.hip - persons across video frames on the device: the association of one frame's kept poses with the persistent tracks
// (sp_track_associate) and the next frame's boxes from the tracks' last poses (sp_track_boxes), so that a tracked frame stays one
// stream of launches (capturable as one graph) and the detector can be left out of most frames.  The reference has no tracker; the
// rules are restated for the CPU in tests/track_ref.py.
// Similarity: oks_iou of the track's last pose and the candidate pose - sp_oks.h's oks_one, the function nms.hip calls - fp64,
// contraction OFF for the whole file.  The track state (slots <= 256) lives in device memory the caller owns between frames.
// sp_track_smooth: the One-Euro filter per track and joint on the frame's kept poses (the rules in sp_smooth.h, restated for the CPU in
// tests/smooth_ref.py); its state lives next to the tracks', keyed by slot.
// Every kernel works on `images` streams at once (sp_track_*_images): the state arrays are stream-major, image s owns block s of each, and
// the launch count does not depend on `images`.  The single-image entries are images = 1 calls of the same kernels.
#include "sp_common.h"
#include "sp_oks.h"
#include "sp_smooth.h"

#include <stdint.h>

#pragma clang fp contract(off)

namespace {

constexpr int TRK_NT = 256;
constexpr int TRK_MAX_SLOTS = 256;               // one thread per slot in the match and box kernels
constexpr int TRK_MAX_IMAGES = 256;

struct TrackState {                              // of image 0; image s owns block s of every array (track_state_of)
    int* id;                                     // [slots] 0 = free
    int* age;                                    // [slots] frames the track was seen in
    int* miss;                                   // [slots] frames since it was last seen
    double* kps;                                 // [slots, J, 3] its last pose
    double* area;                                // [slots]
    float* conf;                                 // [slots] detector confidence carried along
    int* next_id;                                // [1]
};

struct FramePoses {
    const double* kps;                           // [rows, J, 3]
    const double* area;                          // [rows]
    const float* box;                            // [rows, 5]: column 4 = detector confidence
    const int* keep;                             // global row indices in pick order
    const int* keep_count;
    const int* seg;
    int rows;
};

// image s's kept poses: n (clamped to the slots and to the keep list's end) and the offset of its keep list
__device__ __forceinline__ int frame_poses(const FramePoses& f, int s, int slots, int& lo) {
    lo = f.seg[s];
    if (lo < 0 || lo > f.rows) { lo = 0; return 0; }
    int n = f.keep_count[s];
    n = n < 0 ? 0 : n;
    n = n > slots ? slots : n;
    return n > f.rows - lo ? f.rows - lo : n;
}

__device__ __forceinline__ TrackState track_state_of(const TrackState& st, int s, int slots, int J) {
    const size_t o = (size_t)s * slots;
    return {st.id + o, st.age ? st.age + o : nullptr, st.miss + o, st.kps + o * J * 3, st.area ? st.area + o : nullptr, st.conf + o,
            st.next_id ? st.next_id + s : nullptr};
}

// S[s, t, p] for every (slot, pose) pair of every image (blockIdx.y), one thread per pair: oks_iou of a live track's last pose and kept pose p; -1 where there is no
// live track or no pose (never read by the matcher).  Per pair: 2 x J x 24 B read (L2 resident), J exp.  Image 0's workgroups also zero
// track_id [rows] for the match kernel, whose workgroups (one per image) each write their own image's rows only.
__global__ __launch_bounds__(TRK_NT) void track_similarity_kernel(const FramePoses f, const TrackState st0, int slots, int J, const NmsVar var,
                                                                  double* __restrict__ S0, int* __restrict__ track_id) {
    const int img = blockIdx.y;
    const int i = blockIdx.x * TRK_NT + threadIdx.x;
    if (img == 0)
        for (int r = i; r < f.rows; r += gridDim.x * TRK_NT) track_id[r] = 0;
    if (i >= slots * slots) return;
    const TrackState st = track_state_of(st0, img, slots, J);
    double* __restrict__ S = S0 + (size_t)img * slots * slots;
    const int t = i / slots, p = i - t * slots;
    int lo;
    const int n = frame_poses(f, img, slots, lo);
    double s = -1.0;
    if (p < n && st.id[t] != 0) {
        const int row = f.keep[lo + p];
        if (row >= 0 && row < f.rows)
            s = oks_one(st.kps + (size_t)t * J * 3, f.kps + (size_t)row * J * 3, st.area[t], f.area[row], var, J, -1.0);
        else
            s = __longlong_as_double(0x7ff8000000000000ll);            // a row outside the frame never matches
    }
    S[i] = s;
}

// (S descending, slot ascending): the order in which the block picks among the slots' best pairs
__device__ __forceinline__ bool pair_before(double sa, int ta, double sb, int tb) { return sa > sb || (sa == sb && ta < tb); }

// the best still-free pose of one track: (S descending, pose ascending) over S >= thre; NaN fails the comparison and never matches
__device__ __forceinline__ void best_free_pose(const double* __restrict__ Srow, int n, double thre, const int* pose_slot, double& bs, int& bp) {
    bs = -1.0; bp = -1;
    for (int p = 0; p < n; ++p) {
        const double s = Srow[p];
        if (pose_slot[p] < 0 && s >= thre && (bp < 0 || s > bs)) { bs = s; bp = p; }
    }
}

// Greedy matching, births, evictions, ageing and the ids of the frame: ONE workgroup per image, thread t owns slot t.
// Matching visits the pairs in (S descending, slot ascending, pose ascending) order: every round the block takes the first pair of that
// order among the slots' own best free pairs, and only the slots whose best pose was just taken rescan their row - the same matches as
// one sorted walk, a total order that does not depend on thread scheduling.
__global__ __launch_bounds__(TRK_NT) void track_match_kernel(const FramePoses f, const TrackState st0, int slots, int J, double match_thre,
                                                             int max_age, const double* __restrict__ S0, int* __restrict__ track_id) {
    __shared__ int pose_slot[TRK_MAX_SLOTS];      // pose p -> the slot it ends up in (-1 until then)
    __shared__ int upose[TRK_MAX_SLOTS];          // the u-th unmatched pose, in pick order
    __shared__ int s_free[TRK_MAX_SLOTS];         // slot free at frame start
    __shared__ int s_evict[TRK_MAX_SLOTS];        // live and unmatched: may be evicted
    __shared__ int s_miss[TRK_MAX_SLOTS];
    __shared__ double w_s[4];
    __shared__ int w_t[4], w_p[4];
    __shared__ int scan[4];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const TrackState st = track_state_of(st0, img, slots, J);
    const double* __restrict__ S = S0 + (size_t)img * slots * slots;
    int lo;
    const int n = frame_poses(f, img, slots, lo);
    const bool mine = tid < slots;
    const int id0 = mine ? st.id[tid] : 0;
    const bool live = mine && id0 != 0;
    const int miss0 = live ? st.miss[tid] : 0;
    pose_slot[tid] = -1;
    __syncthreads();

    // ---- 2. greedy matching --------------------------------------------------------------------------------------------------------
    int my_pose = -1;                              // the pose this slot matched
    double bs = -1.0;
    int bp = -1;
    if (live) best_free_pose(S + (size_t)tid * slots, n, match_thre, pose_slot, bs, bp);
    for (int round = 0; round < n; ++round) {      // at most one match per pose
        double cs = bp >= 0 ? bs : -1.0;
        int ct = bp >= 0 ? tid : TRK_MAX_SLOTS, cp = bp;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double os = __shfl_xor(cs, off, 64);
            const int ot = __shfl_xor(ct, off, 64), op = __shfl_xor(cp, off, 64);
            if (op >= 0 && (cp < 0 || pair_before(os, ot, cs, ct))) { cs = os; ct = ot; cp = op; }
        }
        if (lane == 0) { w_s[wave] = cs; w_t[wave] = ct; w_p[wave] = cp; }
        __syncthreads();
        cs = w_s[0]; ct = w_t[0]; cp = w_p[0];
        for (int w = 1; w < 4; ++w)
            if (w_p[w] >= 0 && (cp < 0 || pair_before(w_s[w], w_t[w], cs, ct))) { cs = w_s[w]; ct = w_t[w]; cp = w_p[w]; }
        if (cp < 0) break;                         // uniform: every thread read the same four candidates
        if (tid == ct) { my_pose = cp; pose_slot[cp] = tid; bp = -1; }
        __syncthreads();                           // pose_slot[cp] visible; w_* free for the next round
        if (bp == cp) best_free_pose(S + (size_t)tid * slots, n, match_thre, pose_slot, bs, bp);
    }
    __syncthreads();

    // ---- 4. births: unmatched poses in pick order take the free slots in slot order, then the unmatched tracks by (miss descending, slot) ----
    const bool evictable = live && my_pose < 0;
    s_free[tid] = mine && !live;
    s_evict[tid] = evictable;
    s_miss[tid] = miss0;
    int n_unmatched;
    const bool pose_unmatched = tid < n && pose_slot[tid] < 0;
    const int u = sp_block_scan256(pose_unmatched ? 1 : 0, scan, n_unmatched);
    if (pose_unmatched) upose[u] = tid;
    __syncthreads();
    int n_free = 0, rank = 0;
    for (int t = 0; t < slots; ++t) {
        n_free += s_free[t];
        if (mine && !live) rank += (s_free[t] && t < tid) ? 1 : 0;
        else if (evictable) rank += (s_evict[t] && (s_miss[t] > miss0 || (s_miss[t] == miss0 && t < tid))) ? 1 : 0;
    }
    const int pos = (mine && !live) ? rank : (evictable ? n_free + rank : TRK_MAX_SLOTS);
    const int next0 = st.next_id[0];
    const bool born = pos < n_unmatched;
    if (born) { my_pose = upose[pos]; pose_slot[my_pose] = tid; }
    __syncthreads();

    // ---- 3. / 4. / 5. the slot's new state -------------------------------------------------------------------------------------------
    int new_id = id0;
    if (mine) {
        if (born) {
            new_id = next0 + pos;
            st.id[tid] = new_id; st.age[tid] = 1; st.miss[tid] = 0;
        } else if (my_pose >= 0) {
            st.age[tid] = st.age[tid] + 1; st.miss[tid] = 0;
        } else if (live) {
            if (miss0 + 1 > max_age) { st.id[tid] = 0; st.age[tid] = 0; st.miss[tid] = 0; new_id = 0; }
            else st.miss[tid] = miss0 + 1;
        }
        if (my_pose >= 0) {
            const int row = f.keep[lo + my_pose];
            if (row >= 0 && row < f.rows) {        // (a row outside the frame matched nothing; born from one, the slot keeps its old pose)
                st.area[tid] = f.area[row];
                st.conf[tid] = f.box[(size_t)row * 5 + 4];
                track_id[row] = new_id;            // 6.
            }
        }
    }
    if (tid == 0) st.next_id[0] = next0 + n_unmatched;
    // the poses themselves: slots x J x 3 doubles, the block copies them together
    const int J3 = J * 3;
    for (int i = tid; i < n * J3; i += TRK_NT) {
        const int p = i / J3, e = i - p * J3, t = pose_slot[p], row = f.keep[lo + p];
        if (t >= 0 && row >= 0 && row < f.rows) st.kps[(size_t)t * J3 + e] = f.kps[(size_t)row * J3 + e];
    }
}

// Boxes of the tracks seen in the last frame, in slot order, as detector rows (x1, y1, x2, y2, conf, cls): fp32 from the key points cast
// to fp32.  One workgroup per image, thread t owns slot t; rows from the count up to `slots` are zeroed.
__global__ __launch_bounds__(TRK_NT) void track_boxes_kernel(const TrackState st0, int slots, int J, float vis, float expand, float cls, float img_w,
                                                             float img_h, int max_det, float* __restrict__ det0, int* __restrict__ counts) {
    __shared__ int scan[4];
    const int img = blockIdx.x, tid = threadIdx.x;
    const TrackState st = track_state_of(st0, img, slots, J);
    float* __restrict__ det = det0 + (size_t)img * max_det * 6;
    const bool on = tid < slots && st.id[tid] != 0 && st.miss[tid] == 0;
    int total;
    const int k = sp_block_scan256(on ? 1 : 0, scan, total);
    if (on) {
        const double* q = st.kps + (size_t)tid * J * 3;
        int n_vis = 0;
        for (int j = 0; j < J; ++j) n_vis += (float)q[j * 3 + 2] > vis ? 1 : 0;
        const bool all = n_vis < 2;
        const float inf = __int_as_float(0x7f800000);
        float x1 = inf, y1 = inf, x2 = -inf, y2 = -inf;
        for (int j = 0; j < J; ++j) {
            const float x = (float)q[j * 3], y = (float)q[j * 3 + 1], c = (float)q[j * 3 + 2];
            if (!(all || c > vis)) continue;
            if (x < x1) x1 = x;
            if (x > x2) x2 = x;
            if (y < y1) y1 = y;
            if (y > y2) y2 = y;
        }
        const float cx = (x1 + x2) * 0.5f, cy = (y1 + y2) * 0.5f;
        float w = (x2 - x1) * expand, h = (y2 - y1) * expand;
        if (!(w >= 1.f)) w = 1.f;                  // also what a NaN extent becomes
        if (!(h >= 1.f)) h = 1.f;
        const float hw = w * 0.5f, hh = h * 0.5f;
        float b[4] = {cx - hw, cy - hh, cx + hw, cy + hh};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float hi = (i & 1) ? img_h : img_w;
            b[i] = b[i] > 0.f ? b[i] : 0.f;        // NaN -> 0
            b[i] = b[i] < hi ? b[i] : hi;
        }
        float* d = det + (size_t)k * 6;
        d[0] = b[0]; d[1] = b[1]; d[2] = b[2]; d[3] = b[3]; d[4] = st.conf[tid]; d[5] = cls;
    }
    for (int i = total * 6 + tid; i < slots * 6; i += TRK_NT) det[i] = 0.f;
    if (tid == 0) counts[img] = total;
}

constexpr int SMOOTH_NT = 64;

struct SmoothState {                             // of image 0; image s owns block s of every array
    int* id;                                     // [slots] the track id the slot's filters belong to
    double* x;                                   // [slots, J, 2] filtered position
    double* dx;                                  // [slots, J, 2] filtered speed
    double* t;                                   // [slots, J] time of the last accepted sample
    int* n;                                      // [slots, J] samples accepted, 0 = uninitialised
};

// One 64-lane workgroup per row, lane = joint.  The row is copied; when an image kept it (the lowest such image owns it) and it has a track
// id, the workgroup finds the id's slot among that image's tracks (lowest slot with t_id == id), takes the slot over when its filters
// belonged to another id, and every lane filters its joint with that image's time.  Rows of one image carry distinct ids
// (sp_track_associate), so no two workgroups share a slot.  44 B of state per joint in and out.
__global__ __launch_bounds__(SMOOTH_NT) void track_smooth_kernel(const FramePoses f, int images, const int* __restrict__ track_id,
                                                                 const int* __restrict__ t_id0, int slots, int J, const double* __restrict__ now_dev,
                                                                 const sp_smooth_params prm, const SmoothState st0, double* __restrict__ out) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const double* src = f.kps + (size_t)row * J * 3;
    double* dst = out + (size_t)row * J * 3;
    int img = TRK_MAX_IMAGES;
    for (int s = 0; s < images; ++s) {
        int lo;
        const int n = frame_poses(f, s, slots, lo);
        for (int p = lane; p < n; p += SMOOTH_NT)
            if (f.keep[lo + p] == row && s < img) img = s;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int oi = __shfl_xor(img, off, 64);
        img = oi < img ? oi : img;
    }
    const bool kept = img < images;                // uniform
    const int* __restrict__ t_id = t_id0 + (size_t)(kept ? img : 0) * slots;
    const int id = track_id[row];
    int slot = TRK_MAX_SLOTS;
    for (int t = lane; t < slots; t += SMOOTH_NT)
        if (t_id[t] == id && t < slot) slot = t;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int os = __shfl_xor(slot, off, 64);
        slot = os < slot ? os : slot;
    }
    if (!kept || id <= 0 || slot >= slots) {       // uniform: the raw row
        for (int i = lane; i < J * 3; i += SMOOTH_NT) dst[i] = src[i];
        return;
    }
    const size_t so = (size_t)img * slots;
    const SmoothState st = {st0.id + so, st0.x + so * J * 2, st0.dx + so * J * 2, st0.t + so * J, st0.n + so * J};
    const bool fresh = st.id[slot] != id;
    __syncthreads();                               // every lane has read the slot's owner
    if (fresh && lane == 0) st.id[slot] = id;
    if (lane >= J) return;
    const size_t sj = (size_t)slot * J + lane;
    double xh[2] = {st.x[sj * 2], st.x[sj * 2 + 1]}, dxh[2] = {st.dx[sj * 2], st.dx[sj * 2 + 1]}, tl = st.t[sj], o[3];
    int nj = fresh ? 0 : st.n[sj];
    const bool accepted = sp_smooth_joint(prm, src[lane * 3], src[lane * 3 + 1], src[lane * 3 + 2], now_dev[img],
                                          sp_smooth_size(f.box + (size_t)row * 5), xh, dxh, &tl, &nj, o);
    dst[lane * 3] = o[0]; dst[lane * 3 + 1] = o[1]; dst[lane * 3 + 2] = o[2];
    if (accepted) {
        st.x[sj * 2] = xh[0]; st.x[sj * 2 + 1] = xh[1];
        st.dx[sj * 2] = dxh[0]; st.dx[sj * 2 + 1] = dxh[1];
        st.t[sj] = tl;
    }
    if (accepted || fresh) st.n[sj] = nj;
}

}  // namespace

// The three entries and their *_images forms share these: `who` names the entry in every message.
static int track_associate(const char* who, const double* kps, const double* area, const float* box, const int32_t* keep, const int32_t* keep_count,
                           const int32_t* seg, int images, int rows, int joints, const double* sigmas_host, double match_thre, int max_age, int slots,
                           int32_t* t_id, int32_t* t_age, int32_t* t_miss, double* t_kps, double* t_area, float* t_conf, int32_t* next_id,
                           double* similarity, int32_t* track_id, void* stream) {
    SP_REQUIRE(kps && area && box && keep && keep_count && seg && t_id && t_age && t_miss && t_kps && t_area && t_conf && next_id && similarity &&
               track_id, "%s: null pointer", who);
    SP_REQUIRE(images >= 1 && images <= TRK_MAX_IMAGES, "%s: images %d (1..%d)", who, images, TRK_MAX_IMAGES);
    SP_REQUIRE(slots >= 1 && slots <= TRK_MAX_SLOTS, "%s: slots %d (1..%d)", who, slots, TRK_MAX_SLOTS);
    SP_REQUIRE(joints >= 1 && joints <= NMS_MAX_JOINTS, "%s: joints %d (1..%d)", who, joints, NMS_MAX_JOINTS);
    SP_REQUIRE(sigmas_host || joints == 17, "%s: the default sigmas are COCO's 17; pass sigmas for %d joints", who, joints);
    SP_REQUIRE(rows >= 1 && rows <= SP_MAX_ROWS, "%s: rows %d (1..%d, the OKS-NMS group limit)", who, rows, SP_MAX_ROWS);
    SP_REQUIRE(max_age >= 0, "%s: max_age %d", who, max_age);
    NmsVar var;
    sp_oks_fill_var(var, sigmas_host, joints);
    const FramePoses f = {kps, area, box, keep, keep_count, seg, rows};
    const TrackState st = {t_id, t_age, t_miss, t_kps, t_area, t_conf, next_id};
    hipLaunchKernelGGL(track_similarity_kernel, dim3(sp_ceil_div((long long)slots * slots, TRK_NT), images), dim3(TRK_NT), 0, (hipStream_t)stream,
                       f, st, slots, joints, var, similarity, track_id);
    const int rc = sp_check_launch("track_similarity_kernel");
    if (rc != SP_OK) return rc;
    hipLaunchKernelGGL(track_match_kernel, dim3(images), dim3(TRK_NT), 0, (hipStream_t)stream, f, st, slots, joints, match_thre, max_age,
                       similarity, track_id);
    return sp_check_launch("track_match_kernel");
}

static int track_boxes(const char* who, const int32_t* t_id, const int32_t* t_miss, const double* t_kps, const float* t_conf, int images, int slots,
                       int joints, float in_vis_thre, float box_expand, float cls, int img_w, int img_h, int max_det, float* det, int32_t* counts,
                       void* stream) {
    SP_REQUIRE(t_id && t_miss && t_kps && t_conf && det && counts, "%s: null pointer", who);
    SP_REQUIRE(images >= 1 && images <= TRK_MAX_IMAGES, "%s: images %d (1..%d)", who, images, TRK_MAX_IMAGES);
    SP_REQUIRE(slots >= 1 && slots <= TRK_MAX_SLOTS, "%s: slots %d (1..%d)", who, slots, TRK_MAX_SLOTS);
    SP_REQUIRE(joints >= 1 && joints <= NMS_MAX_JOINTS, "%s: joints %d (1..%d)", who, joints, NMS_MAX_JOINTS);
    SP_REQUIRE(max_det >= slots, "%s: max_det %d holds fewer rows than the %d slots", who, max_det, slots);
    SP_REQUIRE(img_w >= 1 && img_h >= 1 && img_w <= 32767 && img_h <= 32767, "%s: image %dx%d", who, img_w, img_h);
    SP_REQUIRE(box_expand > 0.f, "%s: box_expand %g", who, (double)box_expand);
    const TrackState st = {const_cast<int32_t*>(t_id), nullptr, const_cast<int32_t*>(t_miss), const_cast<double*>(t_kps), nullptr,
                           const_cast<float*>(t_conf), nullptr};
    hipLaunchKernelGGL(track_boxes_kernel, dim3(images), dim3(TRK_NT), 0, (hipStream_t)stream, st, slots, joints, in_vis_thre, box_expand, cls,
                       (float)img_w, (float)img_h, max_det, det, counts);
    return sp_check_launch("track_boxes_kernel");
}

static bool smooth_finite(double v) { return v - v == 0.0; }

static int track_smooth(const char* who, const double* kps, const float* box, const int32_t* track_id, const int32_t* keep,
                        const int32_t* keep_count, const int32_t* seg, int images, int rows, int joints, const int32_t* t_id, int slots,
                        const double* now_dev, double min_cutoff, double beta, double d_cutoff, double max_gap, double in_vis_thre, int32_t* s_id,
                        double* s_x, double* s_dx, double* s_t, int32_t* s_n, double* kps_smooth, void* stream) {
    SP_REQUIRE(kps && box && track_id && keep && keep_count && seg && t_id && now_dev && s_id && s_x && s_dx && s_t && s_n && kps_smooth,
               "%s: null pointer", who);
    SP_REQUIRE(images >= 1 && images <= TRK_MAX_IMAGES, "%s: images %d (1..%d)", who, images, TRK_MAX_IMAGES);
    SP_REQUIRE(slots >= 1 && slots <= TRK_MAX_SLOTS, "%s: slots %d (1..%d)", who, slots, TRK_MAX_SLOTS);
    SP_REQUIRE(joints >= 1 && joints <= SMOOTH_NT, "%s: joints %d (1..%d)", who, joints, SMOOTH_NT);
    SP_REQUIRE(rows >= 1, "%s: rows %d", who, rows);
    SP_REQUIRE(smooth_finite(min_cutoff) && min_cutoff > 0.0, "%s: min_cutoff %g (finite, > 0)", who, min_cutoff);
    SP_REQUIRE(smooth_finite(beta) && beta >= 0.0, "%s: beta %g (finite, >= 0)", who, beta);
    SP_REQUIRE(smooth_finite(d_cutoff) && d_cutoff > 0.0, "%s: d_cutoff %g (finite, > 0)", who, d_cutoff);
    SP_REQUIRE(smooth_finite(max_gap) && max_gap > 0.0, "%s: max_gap %g (finite, > 0)", who, max_gap);
    SP_REQUIRE(smooth_finite(in_vis_thre), "%s: in_vis_thre %g (finite)", who, in_vis_thre);
    const FramePoses f = {kps, nullptr, box, keep, keep_count, seg, rows};
    const sp_smooth_params prm = {min_cutoff, beta, d_cutoff, max_gap, in_vis_thre};
    const SmoothState st = {s_id, s_x, s_dx, s_t, s_n};
    hipLaunchKernelGGL(track_smooth_kernel, dim3(rows), dim3(SMOOTH_NT), 0, (hipStream_t)stream, f, images, track_id, t_id, slots, joints, now_dev,
                       prm, st, kps_smooth);
    return sp_check_launch("track_smooth_kernel");
}

extern "C" int sp_track_associate(const double* kps, const double* area, const float* box, const int32_t* keep, const int32_t* keep_count,
                                  const int32_t* seg, int rows, int joints, const double* sigmas_host, double match_thre, int max_age, int slots,
                                  int32_t* t_id, int32_t* t_age, int32_t* t_miss, double* t_kps, double* t_area, float* t_conf, int32_t* next_id,
                                  double* similarity, int32_t* track_id, void* stream) {
    return track_associate("sp_track_associate", kps, area, box, keep, keep_count, seg, 1, rows, joints, sigmas_host, match_thre, max_age, slots,
                           t_id, t_age, t_miss, t_kps, t_area, t_conf, next_id, similarity, track_id, stream);
}

extern "C" int sp_track_associate_images(const double* kps, const double* area, const float* box, const int32_t* keep, const int32_t* keep_count,
                                         const int32_t* seg, int images, int rows, int joints, const double* sigmas_host, double match_thre,
                                         int max_age, int slots, int32_t* t_id, int32_t* t_age, int32_t* t_miss, double* t_kps, double* t_area,
                                         float* t_conf, int32_t* next_id, double* similarity, int32_t* track_id, void* stream) {
    return track_associate("sp_track_associate_images", kps, area, box, keep, keep_count, seg, images, rows, joints, sigmas_host, match_thre,
                           max_age, slots, t_id, t_age, t_miss, t_kps, t_area, t_conf, next_id, similarity, track_id, stream);
}

extern "C" int sp_track_boxes(const int32_t* t_id, const int32_t* t_miss, const double* t_kps, const float* t_conf, int slots, int joints,
                              float in_vis_thre, float box_expand, float cls, int img_w, int img_h, int max_det, float* det, int32_t* counts,
                              void* stream) {
    return track_boxes("sp_track_boxes", t_id, t_miss, t_kps, t_conf, 1, slots, joints, in_vis_thre, box_expand, cls, img_w, img_h, max_det, det,
                       counts, stream);
}

extern "C" int sp_track_boxes_images(const int32_t* t_id, const int32_t* t_miss, const double* t_kps, const float* t_conf, int images, int slots,
                                     int joints, float in_vis_thre, float box_expand, float cls, int img_w, int img_h, int max_det, float* det,
                                     int32_t* counts, void* stream) {
    return track_boxes("sp_track_boxes_images", t_id, t_miss, t_kps, t_conf, images, slots, joints, in_vis_thre, box_expand, cls, img_w, img_h,
                       max_det, det, counts, stream);
}

extern "C" int sp_track_smooth(const double* kps, const float* box, const int32_t* track_id, const int32_t* keep, const int32_t* keep_count,
                               const int32_t* seg, int rows, int joints, const int32_t* t_id, int slots, const double* now_dev, double min_cutoff,
                               double beta, double d_cutoff, double max_gap, double in_vis_thre, int32_t* s_id, double* s_x, double* s_dx,
                               double* s_t, int32_t* s_n, double* kps_smooth, void* stream) {
    return track_smooth("sp_track_smooth", kps, box, track_id, keep, keep_count, seg, 1, rows, joints, t_id, slots, now_dev, min_cutoff, beta,
                        d_cutoff, max_gap, in_vis_thre, s_id, s_x, s_dx, s_t, s_n, kps_smooth, stream);
}

extern "C" int sp_track_smooth_images(const double* kps, const float* box, const int32_t* track_id, const int32_t* keep, const int32_t* keep_count,
                                      const int32_t* seg, int images, int rows, int joints, const int32_t* t_id, int slots, const double* now_dev,
                                      double min_cutoff, double beta, double d_cutoff, double max_gap, double in_vis_thre, int32_t* s_id,
                                      double* s_x, double* s_dx, double* s_t, int32_t* s_n, double* kps_smooth, void* stream) {
    return track_smooth("sp_track_smooth_images", kps, box, track_id, keep, keep_count, seg, images, rows, joints, t_id, slots, now_dev, min_cutoff,
                        beta, d_cutoff, max_gap, in_vis_thre, s_id, s_x, s_dx, s_t, s_n, kps_smooth, stream);
}
