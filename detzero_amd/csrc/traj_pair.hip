// Trajectory-pair table (gfx950): what the reference's assign_track_target and TrackRecall.eval_single_seq both accumulate per
// (ground-truth trajectory, track) pair over the frames the two share, for a whole sequence in one launch.
//
// Reference:
//   tracking/detzero_track/models/tracking_modules/target_assign.py:44-75 (count / similarity matrices), :101-111 (matched rows)
//   tracking/detzero_track/utils/track_calculation.py:9-52 (get_iou_mat_dict: class mask), :84-123 (get_trajectory_similarity)
//
// One thread owns one pair and walks the frame ordinals upwards, so every sum is a sequential fp32 sum in frame order: no atomics,
// the same bytes on every run.  The per-frame value is the pair body of box_geom.h (FMA contraction off), bit-identical to
// dz_boxes_iou_bev / dz_boxes_pairwise_metric(DZ_BOXM_IOU3D).  Lanes of a wave hold consecutive tracks of one ground-truth
// trajectory; the slot tables are (n_frames, n) so that their reads are one line per wave and frame.  A frame the two
// trajectories do not share, or one where the class mask already gives 0, does no geometry.  Plain C++ only; vector stores only.
#include "common.h"

#pragma clang fp contract(off)

#include "box_geom.h"
#include "class_thr.h"

namespace dz {

constexpr int TP_THREADS = 128;
constexpr int TP_LDS_BYTES = 16 * TP_THREADS * (int)(sizeof(P2) + sizeof(float));     // rect_overlap's columns: 192 B per thread
static_assert(2 * TP_LDS_BYTES <= 160 * 1024, "two workgroups per CU");

template <int METRIC>
__device__ __forceinline__ float traj_metric(const float *A, const float *B, P2 *cp, float *ang) {
    if (METRIC == DZ_TRACK_AFF_IOU_BEV) {       // as k_track_affinity: rect_iou with the circle test in front
        const float sa = A[3] * A[4], sb = B[3] * B[4];
        const float so = footprints_near(A, B) ? rect_overlap(A, B, cp, ang, TP_THREADS) : 0.f;
        return so / fmaxf(sa + sb - so, GEO_EPS);
    }
    return pair_metric_ld<DZ_BOXM_IOU3D>(A, B, cp, ang, TP_THREADS);
}

// the masked per-frame value of rows (sa, sb): 0 where the classes differ (track_calculation.py:45-49), else the metric
template <int METRIC>
__device__ __forceinline__ float traj_value(const float *__restrict__ a_box, const float *__restrict__ b_box, int sa, int sb, int ca, int cb,
                                            int distinguish, P2 *cp, float *ang) {
    if (distinguish && ca != cb) return 0.f;
    float A[7], B[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) { A[q] = a_box[sa * 7 + q]; B[q] = b_box[sb * 7 + q]; }
    return traj_metric<METRIC>(A, B, cp, ang);
}

template <int METRIC>
__global__ __launch_bounds__(TP_THREADS) void k_traj_pair_table(const float *__restrict__ a_box, const int *__restrict__ a_cls,
                                                                const int *__restrict__ a_slot, int n_a, int a_rows,
                                                                const float *__restrict__ b_box, const int *__restrict__ b_cls,
                                                                const int *__restrict__ b_slot, int n_b, int b_rows, int n_frames,
                                                                int distinguish, ClassThr thr, float *__restrict__ sum_all,
                                                                float *__restrict__ sum_hit, int *__restrict__ n_hit, int *__restrict__ n_same) {
    __shared__ P2 cp_s[16 * TP_THREADS];
    __shared__ float ang_s[16 * TP_THREADS];
    P2 *cp = cp_s + threadIdx.x;
    float *ang = ang_s + threadIdx.x;
    const long total = (long)n_a * n_b;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int i = (int)(idx / n_b), j = (int)(idx % n_b);
        float s_all = 0.f, s_hit = 0.f;
        int hit = 0, same = 0;
        for (int f = 0; f < n_frames; ++f) {
            const int sa = a_slot[f * n_a + i], sb = b_slot[f * n_b + j];
            // -1 = absent; a slot outside its rows is never followed (the wrapper refuses it first)
            if (sa < 0 || sa >= a_rows || sb < 0 || sb >= b_rows) continue;
            const int ca = a_cls[sa];
            const float v = traj_value<METRIC>(a_box, b_box, sa, sb, ca, b_cls[sb], distinguish, cp, ang);
            ++same;
            s_all = s_all + v;
            if (v >= thr_of(thr, ca)) { ++hit; s_hit = s_hit + v; }
        }
        sum_all[idx] = s_all; sum_hit[idx] = s_hit; n_hit[idx] = hit; n_same[idx] = same;
    }
}

template <int METRIC>
__global__ __launch_bounds__(TP_THREADS) void k_traj_pair_rows(const float *__restrict__ a_box, const int *__restrict__ a_cls,
                                                               const int *__restrict__ a_slot, int n_a, int a_rows,
                                                               const float *__restrict__ b_box, const int *__restrict__ b_cls,
                                                               const int *__restrict__ b_slot, int n_b, int b_rows, int n_frames,
                                                               int distinguish, const int *__restrict__ pairs, int n_pairs,
                                                               float *__restrict__ rows) {
    __shared__ P2 cp_s[16 * TP_THREADS];
    __shared__ float ang_s[16 * TP_THREADS];
    P2 *cp = cp_s + threadIdx.x;
    float *ang = ang_s + threadIdx.x;
    const long total = (long)n_pairs * n_frames;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int p = (int)(idx / n_frames), f = (int)(idx % n_frames);
        const int i = pairs[p * 2 + 0], j = pairs[p * 2 + 1];
        float v = 0.f;
        if (i >= 0 && i < n_a && j >= 0 && j < n_b) {
            const int sa = a_slot[f * n_a + i], sb = b_slot[f * n_b + j];
            if (sa >= 0 && sa < a_rows && sb >= 0 && sb < b_rows)
                v = traj_value<METRIC>(a_box, b_box, sa, sb, a_cls[sa], b_cls[sb], distinguish, cp, ang);
        }
        rows[idx] = v;
    }
}

// the scalar arguments both entry points share
static int traj_sizes(const char *who, int n_a, int a_rows, int n_b, int b_rows, int n_frames, int metric) {
    DZ_CHECK_ARG(metric == DZ_TRACK_AFF_IOU_BEV || metric == DZ_BOXM_IOU3D, "%s: metric %d (DZ_TRACK_AFF_IOU_BEV or DZ_BOXM_IOU3D)", who, metric);
    DZ_CHECK_ARG(n_a >= 0 && n_b >= 0 && a_rows >= 0 && b_rows >= 0 && n_frames >= 0, "%s: negative size", who);
    const long lim = 1L << 31;
    DZ_CHECK_ARG((long)n_frames * n_a < lim && (long)n_frames * n_b < lim && (long)a_rows * 7 < lim && (long)b_rows * 7 < lim &&
                     (long)n_a * n_b < lim,
                 "%s: %d x %d trajectories, %d frames, %d / %d rows overflow 32-bit offsets", who, n_a, n_b, n_frames, a_rows, b_rows);
    return DZ_OK;
}
// the two sides' pointers, wanted once something is launched
static bool traj_sides_ok(const float *a_box, const int *a_cls, const int *a_slot, int a_rows, const float *b_box, const int *b_cls,
                          const int *b_slot, int b_rows, int n_frames) {
    return (n_frames == 0 || (a_slot && b_slot)) && (a_rows == 0 || (a_box && a_cls)) && (b_rows == 0 || (b_box && b_cls));
}

}  // namespace dz

using namespace dz;

extern "C" {

int dz_traj_pair_table(const float *a_box, const int *a_cls, const int *a_slot, int n_a, int a_rows, const float *b_box, const int *b_cls,
                       const int *b_slot, int n_b, int b_rows, int n_frames, int metric, int distinguish_class, const float *h_thr,
                       int n_cls, float *sum_all, float *sum_hit, int *n_hit, int *n_same, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = traj_sizes("dz_traj_pair_table", n_a, a_rows, n_b, b_rows, n_frames, metric);
    if (rc != DZ_OK) return rc;
    DZ_CHECK_ARG(n_cls >= 1 && n_cls <= DZ_TRACK_MAX_CLASSES && h_thr, "dz_traj_pair_table: %d classes (1..%d) or null thresholds", n_cls,
                 DZ_TRACK_MAX_CLASSES);
    ClassThr thr;
    for (int k = 0; k < DZ_TRACK_MAX_CLASSES; ++k) {
        thr.v[k] = k < n_cls ? h_thr[k] : h_thr[0];
        // a pair without a common box keeps count 0 only when 0 never passes
        DZ_CHECK_ARG(thr.v[k] > 0.f, "dz_traj_pair_table: threshold %d is %g; every threshold must be > 0", k, (double)thr.v[k]);
    }
    if (n_a == 0 || n_b == 0) return DZ_OK;
    DZ_CHECK_ARG(traj_sides_ok(a_box, a_cls, a_slot, a_rows, b_box, b_cls, b_slot, b_rows, n_frames) && sum_all && sum_hit && n_hit && n_same,
                 "dz_traj_pair_table: null pointer");
    const dim3 grid(stream_grid((long)n_a * n_b, TP_THREADS)), block(TP_THREADS);
    if (metric == DZ_TRACK_AFF_IOU_BEV)
        hipLaunchKernelGGL(k_traj_pair_table<DZ_TRACK_AFF_IOU_BEV>, grid, block, 0, stream, a_box, a_cls, a_slot, n_a, a_rows, b_box, b_cls,
                           b_slot, n_b, b_rows, n_frames, distinguish_class, thr, sum_all, sum_hit, n_hit, n_same);
    else
        hipLaunchKernelGGL(k_traj_pair_table<DZ_BOXM_IOU3D>, grid, block, 0, stream, a_box, a_cls, a_slot, n_a, a_rows, b_box, b_cls, b_slot,
                           n_b, b_rows, n_frames, distinguish_class, thr, sum_all, sum_hit, n_hit, n_same);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_traj_pair_rows(const float *a_box, const int *a_cls, const int *a_slot, int n_a, int a_rows, const float *b_box, const int *b_cls,
                      const int *b_slot, int n_b, int b_rows, int n_frames, int metric, int distinguish_class, const int *pairs,
                      int n_pairs, float *rows, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = traj_sizes("dz_traj_pair_rows", n_a, a_rows, n_b, b_rows, n_frames, metric);
    if (rc != DZ_OK) return rc;
    DZ_CHECK_ARG(n_pairs >= 0 && (long)n_pairs * n_frames < (1L << 31), "dz_traj_pair_rows: %d pairs x %d frames", n_pairs, n_frames);
    if (n_pairs == 0 || n_frames == 0) return DZ_OK;
    DZ_CHECK_ARG(n_a > 0 && n_b > 0, "dz_traj_pair_rows: %d pairs of %d x %d trajectories", n_pairs, n_a, n_b);
    DZ_CHECK_ARG(traj_sides_ok(a_box, a_cls, a_slot, a_rows, b_box, b_cls, b_slot, b_rows, n_frames) && pairs && rows,
                 "dz_traj_pair_rows: null pointer");
    const dim3 grid(stream_grid((long)n_pairs * n_frames, TP_THREADS)), block(TP_THREADS);
    if (metric == DZ_TRACK_AFF_IOU_BEV)
        hipLaunchKernelGGL(k_traj_pair_rows<DZ_TRACK_AFF_IOU_BEV>, grid, block, 0, stream, a_box, a_cls, a_slot, n_a, a_rows, b_box, b_cls,
                           b_slot, n_b, b_rows, n_frames, distinguish_class, pairs, n_pairs, rows);
    else
        hipLaunchKernelGGL(k_traj_pair_rows<DZ_BOXM_IOU3D>, grid, block, 0, stream, a_box, a_cls, a_slot, n_a, a_rows, b_box, b_cls, b_slot,
                           n_b, b_rows, n_frames, distinguish_class, pairs, n_pairs, rows);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

}  // extern "C"
