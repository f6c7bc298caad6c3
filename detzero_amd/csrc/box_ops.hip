// Box ops next to the head post stage (gfx950): fused pair matrices of the tracker's association metrics (convex-hull
// "union" area, 3-D IoU, 3-D GIoU), the same metrics on paired boxes, the refining models' recall table and axis-aligned NMS.
//
// Reference:
//   utils/detzero_utils/ops/iou3d_nms/iou3d_nms_utils.py:74-151,173-187 (boxes_iou3d_gpu, boxes_giou3d_gpu, nms_normal_gpu)
//   utils/detzero_utils/ops/iou3d_nms/src/iou3d_nms_kernel.cu:235-326,352-368 (box_union: see rect_hull_area), :433-491 (iou_normal)
//   tracking/detzero_track/models/tracking_modules/data_association/distance.py:44-161 (the callers)
//   refining/detzero_refine/models/geometry_refine_model.py:98-141, position_refine_model.py:100-133 (the recall records' per-track
//   `boxes_iou3d_gpu(a, b).diag()` loops: k_paired_metric, k_track_recall_iou3d)
//
// Parity notes: fp32, the reference's operation order, FMA contraction disabled - the 3-D IoU is bit-identical to the torch
// composition around dz_boxes_overlap_bev that it replaces, and the axis-aligned predicate (+, -, *, /, fmaxf, fminf only) is
// bit-reproducible on any IEEE machine.
#include "common.h"

#pragma clang fp contract(off)

#include "box_geom.h"

namespace dz {

constexpr int METRIC_THREADS = 128;

// One pair, the final value (box_geom.h: pair_metric_ld, shared with track.hip's affinity kernel): the body shared by the matrix
// kernel and the paired kernels below, so that a paired result is element (i, i) of the matrix bit for bit.
template <int METRIC>
__device__ __forceinline__ float pair_metric(const float *A, const float *B, P2 *cp, float *ang) {
    return pair_metric_ld<METRIC>(A, B, cp, ang, METRIC_THREADS);
}

// one thread per (i, j) pair, the final value in one pass
template <int METRIC>
__global__ __launch_bounds__(METRIC_THREADS) void k_pairwise_metric(const float *__restrict__ a, int na, const float *__restrict__ b, int nb,
                                                                    float *__restrict__ out) {
    // rect_overlap's vertex list [16][threads] and, after it, the hull stack [9][threads] share the thread's LDS column
    __shared__ P2 cp_s[(METRIC == DZ_BOXM_UNION_BEV ? 9 : 16) * METRIC_THREADS];
    __shared__ float ang_s[METRIC == DZ_BOXM_UNION_BEV ? 1 : 16 * METRIC_THREADS];
    P2 *cp = cp_s + threadIdx.x;
    const long total = (long)na * nb;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int i = (int)(idx / nb), j = (int)(idx % nb);
        float A[7], B[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) { A[q] = a[i * 7 + q]; B[q] = b[j * 7 + q]; }
        out[idx] = pair_metric<METRIC>(A, B, cp, ang_s + threadIdx.x);
    }
}

// ------------------------------------------------------------------------------------------
// paired metric and the refiner's recall table
// ------------------------------------------------------------------------------------------
// out[i] = metric(a[i], b[i]): the diagonal of k_pairwise_metric without the matrix.  The refining models' recall records
// (refining/detzero_refine/models/geometry_refine_model.py:114-122, position_refine_model.py:106-114) build a T x T matrix per
// track and side and keep `.diag()`.
template <int METRIC>
__global__ __launch_bounds__(METRIC_THREADS) void k_paired_metric(const float *__restrict__ a, const float *__restrict__ b, int n,
                                                                  float *__restrict__ out) {
    __shared__ P2 cp_s[(METRIC == DZ_BOXM_UNION_BEV ? 9 : 16) * METRIC_THREADS];
    __shared__ float ang_s[METRIC == DZ_BOXM_UNION_BEV ? 1 : 16 * METRIC_THREADS];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {      // n * 7 < 2^31 (entry point)
        float A[7], B[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) { A[q] = a[i * 7 + q]; B[q] = b[i * 7 + q]; }
        out[i] = pair_metric<METRIC>(A, B, cp_s + threadIdx.x, ang_s + threadIdx.x);
    }
}

// Recall table of one batch of tracks in one launch: replaces the per-track loop of geometry_refine_model.py:98-141 and
// position_refine_model.py:100-133 (two T x T boxes_iou3d_gpu matrices cut to their diagonals and five or more .item() per track).
// One thread per (track, row); a group covers 128 rows of ONE track, so its counters belong to one line of `counts`
// (batch, 2, n_thr + 1): [b][s][0] = counted rows, [b][s][1 + k] = counted rows with iou > thr[k]; s = 0 input side (in, gt),
// s = 1 output side (out, gt).  Per counter a __ballot + popcount per wave, the two waves' words added through LDS, one
// integer atomicAdd per (group, counter): integer adds commute, the table is the same on every run.  Rows outside the mask
// or the track's length are never read as boxes; their iou_in / iou_out entries are 0.
constexpr int RECALL_MAX_THR = 8;
struct RecallThr { float v[RECALL_MAX_THR]; };

__global__ __launch_bounds__(METRIC_THREADS) void k_track_recall_iou3d(const float *__restrict__ boxes_in, const float *__restrict__ boxes_out,
                                                                       const float *__restrict__ boxes_gt, const unsigned char *__restrict__ mask,
                                                                       const int *__restrict__ d_len, int t_cap, int groups_per_track,
                                                                       RecallThr thr, int n_thr, float *__restrict__ iou_in,
                                                                       float *__restrict__ iou_out, int *__restrict__ counts) {
    __shared__ P2 cp_s[16 * METRIC_THREADS];
    __shared__ float ang_s[16 * METRIC_THREADS];
    __shared__ int wave_cnt[METRIC_THREADS / 64][2 * (RECALL_MAX_THR + 1)];
    const int b = blockIdx.x / groups_per_track;
    const int row = (blockIdx.x % groups_per_track) * METRIC_THREADS + threadIdx.x;
    const int len = max(min(d_len[b], t_cap), 0);
    const int at = b * t_cap + row;                       // batch * t_cap * 7 < 2^31 (entry point)
    const bool counted = row < len && mask[at] != 0;
    float v_in = 0.f, v_out = 0.f;
    if (counted) {
        float A[7], B[7], G[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) { A[q] = boxes_in[at * 7 + q]; B[q] = boxes_out[at * 7 + q]; G[q] = boxes_gt[at * 7 + q]; }
        v_in = pair_metric<DZ_BOXM_IOU3D>(A, G, cp_s + threadIdx.x, ang_s + threadIdx.x);
        v_out = pair_metric<DZ_BOXM_IOU3D>(B, G, cp_s + threadIdx.x, ang_s + threadIdx.x);
    }
    if (row < t_cap) {
        if (iou_in) iou_in[at] = v_in;
        if (iou_out) iou_out[at] = v_out;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per_side = n_thr + 1;
    const int n_counted = __popcll(__ballot(counted));
    if (lane == 0) { wave_cnt[wave][0] = n_counted; wave_cnt[wave][per_side] = n_counted; }
#pragma unroll
    for (int k = 0; k < RECALL_MAX_THR; ++k) {            // constant indices into thr.v after unrolling
        if (k < n_thr) {                                  // (uniform)
            const int c_in = __popcll(__ballot(counted && v_in > thr.v[k]));
            const int c_out = __popcll(__ballot(counted && v_out > thr.v[k]));
            if (lane == 0) { wave_cnt[wave][1 + k] = c_in; wave_cnt[wave][per_side + 1 + k] = c_out; }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * per_side) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < METRIC_THREADS / 64; ++w) sum += wave_cnt[w][threadIdx.x];
        if (sum) atomicAdd(counts + b * 2 * per_side + threadIdx.x, sum);
    }
}

// ------------------------------------------------------------------------------------------
// axis-aligned NMS
// ------------------------------------------------------------------------------------------
// iou3d_nms_kernel.cu:433-444; the heading is ignored
__device__ __forceinline__ float iou_normal(const float *a, const float *b) {
    const float left = fmaxf(a[0] - a[3] / 2, b[0] - b[3] / 2), right = fminf(a[0] + a[3] / 2, b[0] + b[3] / 2);
    const float top = fmaxf(a[1] - a[4] / 2, b[1] - b[4] / 2), bottom = fminf(a[1] + a[4] / 2, b[1] + b[4] / 2);
    const float width = fmaxf(right - left, 0.f), height = fmaxf(bottom - top, 0.f);
    const float inter = width * height;
    const float sa = a[3] * a[4], sb = b[3] * b[4];
    return inter / fmaxf(sa + sb - inter, GEO_EPS);
}

// k_nms_mask's layout and ragged d_n handling: mask[i][cb] bit j: iou_normal(box i, box cb*64+j) > thr, only for j > i; one
// wavefront per (16 rows, 64 columns).  A lane owns a column box and walks the rows; __ballot packs the word, lane r keeps row r's.
// The reference fills the lower triangle too (:455); the sweep never reads those bits for a decision.
constexpr int NMSN_ROWS_PER_WAVE = 16;
__global__ __launch_bounds__(64) void k_nms_normal_mask(const float *__restrict__ boxes, const int *__restrict__ d_n, int n_cap, float thr,
                                                        unsigned long long *__restrict__ mask, int col_blocks) {
    // batch item = blockIdx.z: boxes (B,n_cap,7), d_n (B), mask (B,n_cap,col_blocks)
    boxes += (size_t)blockIdx.z * n_cap * 7;
    mask += (size_t)blockIdx.z * n_cap * col_blocks;
    const int n = d_n ? min(d_n[blockIdx.z], n_cap) : n_cap;
    const int cb = blockIdx.x;
    const int rb = blockIdx.y / (64 / NMSN_ROWS_PER_WAVE), part = blockIdx.y % (64 / NMSN_ROWS_PER_WAVE);
    const int row0 = rb * 64 + part * NMSN_ROWS_PER_WAVE;
    if (row0 >= n) return;
    const int t = threadIdx.x;
    const int rows = min(NMSN_ROWS_PER_WAVE, n - row0);
    const int col = cb * 64 + t;
    unsigned long long word = 0ull;
    if (cb >= rb && cb * 64 < n) {        // (lower triangle / beyond n: nothing can be suppressed there, the words are 0)
        float B[7];
        const bool col_ok = col < n;
#pragma unroll
        for (int q = 0; q < 7; ++q) B[q] = col_ok ? boxes[col * 7 + q] : 0.f;
        for (int i = 0; i < rows; ++i) {
            const int row = row0 + i;
            float A[7];       // wave-uniform -> scalar loads
#pragma unroll
            for (int q = 0; q < 7; ++q) A[q] = boxes[row * 7 + q];
            const unsigned long long m = __ballot(col_ok && col > row && iou_normal(A, B) > thr);
            if (t == i) word = m;
        }
    }
    if (t < rows) mask[(size_t)(row0 + t) * col_blocks + cb] = word;
}

template <int METRIC>
static int launch_metric(const float *a, int na, const float *b, int nb, float *out, hipStream_t stream) {
    hipLaunchKernelGGL(k_pairwise_metric<METRIC>, dim3(stream_grid((long)na * nb, METRIC_THREADS)), dim3(METRIC_THREADS), 0, stream, a, na,
                       b, nb, out);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

template <int METRIC>
static int launch_paired(const float *a, const float *b, int n, float *out, hipStream_t stream) {
    hipLaunchKernelGGL(k_paired_metric<METRIC>, dim3(stream_grid(n, METRIC_THREADS)), dim3(METRIC_THREADS), 0, stream, a, b, n, out);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

}  // namespace dz

using namespace dz;

extern "C" {

int dz_boxes_pairwise_metric(const float *a, int na, const float *b, int nb, int metric, float *out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(na >= 0 && nb >= 0, "dz_boxes_pairwise_metric: negative size");
    if (metric < DZ_BOXM_UNION_BEV || metric > DZ_BOXM_GIOU3D_EXACT) {
        set_error("dz_boxes_pairwise_metric: unknown metric %d", metric);
        return DZ_ERR_UNSUPPORTED;
    }
    if (na == 0 || nb == 0) return DZ_OK;
    DZ_CHECK_ARG(a && b && out, "dz_boxes_pairwise_metric: null pointer");
    switch (metric) {
        case DZ_BOXM_UNION_BEV: return launch_metric<DZ_BOXM_UNION_BEV>(a, na, b, nb, out, stream);
        case DZ_BOXM_IOU3D: return launch_metric<DZ_BOXM_IOU3D>(a, na, b, nb, out, stream);
        case DZ_BOXM_GIOU3D: return launch_metric<DZ_BOXM_GIOU3D>(a, na, b, nb, out, stream);
        default: return launch_metric<DZ_BOXM_GIOU3D_EXACT>(a, na, b, nb, out, stream);
    }
}

int dz_boxes_paired_metric(const float *a, const float *b, int n, int metric, float *out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n >= 0, "dz_boxes_paired_metric: negative size");
    if (metric < DZ_BOXM_UNION_BEV || metric > DZ_BOXM_GIOU3D_EXACT) {
        set_error("dz_boxes_paired_metric: unknown metric %d", metric);
        return DZ_ERR_UNSUPPORTED;
    }
    if ((long)n * 7 >= (1L << 31)) {
        set_error("dz_boxes_paired_metric: %d boxes overflow 32-bit offsets", n);
        return DZ_ERR_UNSUPPORTED;
    }
    if (n == 0) return DZ_OK;
    DZ_CHECK_ARG(a && b && out, "dz_boxes_paired_metric: null pointer");
    switch (metric) {
        case DZ_BOXM_UNION_BEV: return launch_paired<DZ_BOXM_UNION_BEV>(a, b, n, out, stream);
        case DZ_BOXM_IOU3D: return launch_paired<DZ_BOXM_IOU3D>(a, b, n, out, stream);
        case DZ_BOXM_GIOU3D: return launch_paired<DZ_BOXM_GIOU3D>(a, b, n, out, stream);
        default: return launch_paired<DZ_BOXM_GIOU3D_EXACT>(a, b, n, out, stream);
    }
}

int dz_track_recall_iou3d(const float *boxes_in, const float *boxes_out, const float *boxes_gt, const unsigned char *mask, const int *d_len,
                          int batch, int t_cap, const double *h_thresholds, int n_thr, float *iou_in, float *iou_out, int *counts,
                          void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(batch >= 0 && t_cap >= 0, "dz_track_recall_iou3d: negative size");
    if (n_thr < 1 || n_thr > RECALL_MAX_THR) {
        set_error("dz_track_recall_iou3d: %d thresholds (1..%d)", n_thr, RECALL_MAX_THR);
        return DZ_ERR_UNSUPPORTED;
    }
    if ((long)batch * t_cap * 7 >= (1L << 31)) {        // also bounds the grid and the table: groups <= batch * t_cap, 18 counters < 7 * 128 floats
        set_error("dz_track_recall_iou3d: batch %d x t_cap %d overflows 32-bit offsets", batch, t_cap);
        return DZ_ERR_UNSUPPORTED;
    }
    DZ_CHECK_ARG(h_thresholds, "dz_track_recall_iou3d: null thresholds");
    if (batch == 0) return DZ_OK;
    DZ_CHECK_ARG(counts, "dz_track_recall_iou3d: null counts");
    if ((long)batch * 2 * (n_thr + 1) >= (1L << 31)) {
        set_error("dz_track_recall_iou3d: batch %d overflows the count table's 32-bit offsets", batch);
        return DZ_ERR_UNSUPPORTED;
    }
    const int rc = fill_u32(counts, 0u, (size_t)batch * 2 * (n_thr + 1), stream);
    if (rc != DZ_OK || t_cap == 0) return rc;
    DZ_CHECK_ARG(boxes_in && boxes_out && boxes_gt && mask && d_len, "dz_track_recall_iou3d: null pointer");
    RecallThr thr = {};
    for (int k = 0; k < n_thr; ++k) thr.v[k] = (float)h_thresholds[k];      // torch compares an fp32 tensor with a Python scalar in fp32
    const int groups_per_track = ceil_div(t_cap, METRIC_THREADS);
    hipLaunchKernelGGL(k_track_recall_iou3d, dim3((unsigned)batch * groups_per_track), dim3(METRIC_THREADS), 0, stream, boxes_in, boxes_out,
                       boxes_gt, mask, d_len, t_cap, groups_per_track, thr, n_thr, iou_in, iou_out, counts);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_nms_normal_batched(const float *boxes, const int *d_n, int batch, int n_cap, float thresh, int post_max, int *keep,
                          int *d_num_keep, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(keep && d_num_keep && n_cap >= 0 && post_max >= 0 && batch >= 0, "dz_nms_normal: bad argument");
    if (batch == 0) return DZ_OK;
    if (n_cap == 0) return fill_u32(d_num_keep, 0u, (size_t)batch, stream);
    DZ_CHECK_ARG(boxes && ws, "dz_nms_normal: null pointer");
    DZ_CHECK_ARG(n_cap <= 4096, "dz_nms_normal: n_cap %d > 4096 (NMS_PRE_MAXSIZE of the reference configs)", n_cap);
    DZ_CHECK_ARG(batch <= 65535, "dz_nms_normal: batch %d > 65535", batch);
    if (ws_bytes < (size_t)batch * dz_nms_workspace_bytes(n_cap)) { set_error("dz_nms_normal: workspace too small"); return DZ_ERR_WORKSPACE; }
    const int cb = (n_cap + 63) / 64;
    unsigned long long *mask = (unsigned long long *)ws;
    hipLaunchKernelGGL(k_nms_normal_mask, dim3(cb, cb * (64 / NMSN_ROWS_PER_WAVE), batch), dim3(64), 0, stream, boxes, d_n, n_cap, thresh,
                       mask, cb);
    return nms_sweep(mask, d_n, batch, n_cap, cb, post_max, keep, d_num_keep, stream);
}

int dz_nms_normal(const float *boxes, const int *d_n, int n_cap, float thresh, int post_max, int *keep, int *d_num_keep,
                  void *ws, size_t ws_bytes, void *stream_) {
    return dz_nms_normal_batched(boxes, d_n, 1, n_cap, thresh, post_max, keep, d_num_keep, ws, ws_bytes, stream_);
}

}  // extern "C"
