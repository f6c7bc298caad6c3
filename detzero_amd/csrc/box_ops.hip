// Box ops next to the head post stage (gfx950): fused pair matrices of the tracker's association metrics (convex-hull
// "union" area, 3-D IoU, 3-D GIoU) and axis-aligned NMS.
//
// Reference:
//   utils/detzero_utils/ops/iou3d_nms/iou3d_nms_utils.py:74-151,173-187 (boxes_iou3d_gpu, boxes_giou3d_gpu, nms_normal_gpu)
//   utils/detzero_utils/ops/iou3d_nms/src/iou3d_nms_kernel.cu:235-326,352-368 (box_union: see rect_hull_area), :433-491 (iou_normal)
//   tracking/detzero_track/models/tracking_modules/data_association/distance.py:44-161 (the callers)
//
// Parity notes: fp32, the reference's operation order, FMA contraction disabled - the 3-D IoU is bit-identical to the torch
// composition around dz_boxes_overlap_bev that it replaces, and the axis-aligned predicate (+, -, *, /, fmaxf, fminf only) is
// bit-reproducible on any IEEE machine.
#include "common.h"

#pragma clang fp contract(off)

#include "box_geom.h"

namespace dz {

constexpr int METRIC_THREADS = 128;

// true when the circumscribed circles of the two footprints are at most 5 cm apart (k_nms_mask's test): beyond that
// rect_overlap finds no vertex (its corner test has a 1 cm margin) and returns exactly +0
__device__ __forceinline__ bool footprints_near(const float *A, const float *B) {
    const float dx = A[0] - B[0], dy = A[1] - B[1];
    const float reach = sqrtf(0.25f * (A[3] * A[3] + A[4] * A[4])) + sqrtf(0.25f * (B[3] * B[3] + B[4] * B[4])) + 0.05f;
    return dx * dx + dy * dy <= reach * reach;
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
        if (METRIC == DZ_BOXM_UNION_BEV) {
            out[idx] = rect_hull_area(A, B, cp, METRIC_THREADS);
            continue;
        }
        // iou3d_nms_utils.py:86-105 / :122-150, operation for operation
        const float a_max = A[2] + A[5] / 2, a_min = A[2] - A[5] / 2;
        const float b_max = B[2] + B[5] / 2, b_min = B[2] - B[5] / 2;
        const float bev = footprints_near(A, B) ? rect_overlap(A, B, cp, ang_s + threadIdx.x, METRIC_THREADS) : 0.f;
        const float oh = fmaxf(fminf(a_max, b_max) - fmaxf(a_min, b_min), 0.f);
        const float o3 = bev * oh;
        const float va = (A[3] * A[4]) * A[5], vb = (B[3] * B[4]) * B[5];
        const float u3 = fmaxf((va + vb) - o3, 1e-6f);
        if (METRIC == DZ_BOXM_IOU3D) {
            out[idx] = o3 / u3;
            continue;
        }
        // the reference's enclosing height is min(tops) - min(bottoms) (:139 `max_of_max = torch.min(...)`); EXACT = max(tops) - min(bottoms)
        const float top = METRIC == DZ_BOXM_GIOU3D_EXACT ? fmaxf(a_max, b_max) : fminf(a_max, b_max);
        const float uh = fmaxf(top - fminf(a_min, b_min), 0.f);
        const float c3 = fmaxf(rect_hull_area(A, B, cp, METRIC_THREADS) * uh, 1e-6f);
        out[idx] = o3 / u3 - (c3 - u3) / c3;
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
