// Tracking module (gfx950): the per-track and per-pair arithmetic of the reference's CPU tracker on a device-resident track table.
//
// Reference:
//   tracking/detzero_track/models/tracking_modules/kalman_filter/kalman_filter.py:10-58 (constructor), :85-108 (predict), :110-146 (update)
//   tracking/detzero_track/models/tracking_modules/data_association/data_association.py:36-60 (one_stage), distance.py:9-23 (GNN masking)
//   tracking/detzero_track/models/tracking_modules/track_manager.py:262-310 (overlap_track_merge), :198-214 (info / death)
//
// One table = one sequence; the host keeps the reference's control flow (frame order, stage index lists, linear_sum_assignment) and
// sees cost matrices and a track count only.  Everything is fp32 as in the reference (its arrays are float32 when the detections
// are), FMA contraction off: the pair metrics are the bodies of box_geom.h and so agree with dz_boxes_iou_bev /
// dz_boxes_pairwise_metric bit for bit.  Plain C++ only; every store is a vector store.
// The AB3DMOT filter (kalman_filter/ab3dmot.py) is the second set of per-track kernels below: float64 state in a companion table
// (dz_track_ab3d), bodies in track_ab3dmot.h; affinity and merge are the same kernels for both filters (they read the float32 box).
#include "common.h"

#pragma clang fp contract(off)

#include "track_body.h"
#include "track_ab3dmot.h"

namespace dz {

constexpr int TRK_THREADS = 128;
constexpr int MERGE_MAX_TRACKS = 32768;
constexpr int MERGE_MAX_WORDS = MERGE_MAX_TRACKS / 64;

// The bodies of the kernels below are in track_body.h (shared with the sequence kernels of track_seq.hip).
__global__ __launch_bounds__(TRK_THREADS) void k_track_predict(dz_track_table t, int n, int gate_class) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    track_predict_body(t, i, gate_class);
}

template <int METRIC>
__global__ __launch_bounds__(TRK_THREADS) void k_track_affinity(const float *__restrict__ tbox, const int *__restrict__ tcls, int n_tab,
                                                                const int *__restrict__ ext, int n_ext, const int *__restrict__ row_idx,
                                                                int nr, const int *__restrict__ det, int n_det,
                                                                const int *__restrict__ col_idx, int nc, int distinguish, ClassThr thr,
                                                                float *__restrict__ out) {
    __shared__ P2 cp_s[16 * TRK_THREADS];
    __shared__ float ang_s[16 * TRK_THREADS];
    P2 *cp = cp_s + threadIdx.x;
    float *ang = ang_s + threadIdx.x;
    const long total = (long)nr * nc;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int r = (int)(idx / nc), c = (int)(idx % nc);
        out[idx] = track_cost_body<METRIC>(tbox, tcls, n_tab, ext, n_ext, row_idx[r], det, n_det, col_idx[c], distinguish, thr, cp, ang,
                                           TRK_THREADS);
    }
}

__global__ __launch_bounds__(TRK_THREADS) void k_track_update(dz_track_table t, int n, const int *__restrict__ det, int n_det,
                                                              const int *__restrict__ match, int m, float r_meas) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int i = match[k * 3 + 0], di = match[k * 3 + 1], stage = match[k * 3 + 2];
    if (i < 0 || i >= n || di < 0 || di >= n_det) return;
    track_update_body(t, i, det + di * ROW, stage, r_meas);
}

__global__ __launch_bounds__(TRK_THREADS) void k_track_spawn(dz_track_table t, int n, const int *__restrict__ src, int n_src,
                                                             const int *__restrict__ src_idx, const int *__restrict__ ids, int m, float p0,
                                                             float p1, float q0, float q1, float dt) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int si = src_idx[k];
    const bool ok = si >= 0 && si < n_src;      // (an index outside the buffer gives an all-zero track; the wrapper refuses it first)
    track_spawn_body(t, n + k, src + (ok ? si : 0) * ROW, ok, ids[k], p0, p1, q0, q1, dt);
}

__global__ __launch_bounds__(TRK_THREADS) void k_track_log(dz_track_table t, int n, int frame, int *__restrict__ log) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    track_log_body(t, i, frame, log + (long)i * ROW);
}

__global__ __launch_bounds__(64) void k_track_merge_bits(const float *__restrict__ box, const int *__restrict__ cls, int n, ClassThr thr,
                                                         unsigned long long *__restrict__ bits, int words, int *__restrict__ busy) {
    __shared__ P2 cp_s[16 * 64];
    __shared__ float ang_s[16 * 64];
    const int cb = blockIdx.x, row0 = blockIdx.y * MERGE_ROWS_PER_WAVE;
    if (row0 >= n) return;
    const int lane = threadIdx.x;
    track_merge_bits_body(box, cls, n, thr, bits, words, busy, cb, row0, lane, cp_s + lane, ang_s + lane);
}

__global__ __launch_bounds__(64) void k_track_merge_sweep(const unsigned long long *__restrict__ bits, int words, const int *__restrict__ busy,
                                                          const int *__restrict__ id, int n, int *__restrict__ removed) {
    __shared__ unsigned long long cleared[MERGE_MAX_WORDS], dep[MERGE_MAX_WORDS];
    track_merge_sweep_body<1>(bits, words, busy, id, n, removed, cleared, dep, nullptr);
}

// One workgroup: 256 rows at a time, exclusive scan of the keep flags, survivors copied in order.  A table is a few thousand rows
// of 72 words; the copy is not worth a second launch.
__global__ __launch_bounds__(256) void k_track_compact(dz_track_table s, int n, const int *__restrict__ removed, int death_age,
                                                       dz_track_table d, int *__restrict__ d_count) {
    __shared__ uint32_t scan_s[4];
    uint32_t base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const bool keep = i < n && track_keep_body(s, i, removed, death_age);
        uint32_t total;
        const uint32_t at = base + block_excl_scan_256(keep ? 1u : 0u, scan_s, total);
        if (keep) track_copy_body(s, i, d, (int)at);
        base += total;
    }
    if (threadIdx.x == 0) *d_count = (int)base;
}

// ---- the AB3DMOT filter (bodies: track_ab3dmot.h), one thread per track ----
__global__ __launch_bounds__(TRK_THREADS) void k_track_ab3d_predict(dz_track_table t, dz_track_ab3d a, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ab3d_predict_body(t, a, i);
}

__global__ __launch_bounds__(TRK_THREADS) void k_track_ab3d_update(dz_track_table t, dz_track_ab3d a, int n, const int *__restrict__ det,
                                                                   const double *__restrict__ det64, int n_det,
                                                                   const int *__restrict__ match, int m) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int i = match[k * 3 + 0], di = match[k * 3 + 1];
    if (i < 0 || i >= n || di < 0 || di >= n_det) return;
    ab3d_update_body(t, a, i, det + di * ROW, det64 + (long)di * AB_NZ);
}

__global__ __launch_bounds__(TRK_THREADS) void k_track_ab3d_spawn(dz_track_table t, dz_track_ab3d a, int n, const int *__restrict__ src,
                                                                  const double *__restrict__ src64, int n_src,
                                                                  const int *__restrict__ src_idx, const int *__restrict__ ids, int m) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int si = src_idx[k];
    const bool ok = si >= 0 && si < n_src;
    ab3d_spawn_body(t, a, n + k, src + (ok ? si : 0) * ROW, src64 + (long)(ok ? si : 0) * AB_NZ, ok, ids[k]);
}

__global__ __launch_bounds__(TRK_THREADS) void k_track_ab3d_log(dz_track_table t, dz_track_ab3d a, int n, int frame, int frame_id,
                                                                int birth_age, int death_age, int *__restrict__ log,
                                                                double *__restrict__ log64) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ab3d_log_body(t, a, i, frame, frame_id, birth_age, death_age, log + (long)i * ROW, log64 + (long)i * 9);
}

__global__ __launch_bounds__(256) void k_track_ab3d_compact(dz_track_table s, dz_track_ab3d as, int n, const int *__restrict__ removed,
                                                            int death_age, dz_track_table d, dz_track_ab3d ad, int *__restrict__ d_count) {
    __shared__ uint32_t scan_s[4];
    uint32_t base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const bool keep = i < n && track_keep_body(s, i, removed, death_age);
        uint32_t total;
        const uint32_t at = base + block_excl_scan_256(keep ? 1u : 0u, scan_s, total);
        if (keep) ab3d_copy_body(s, as, i, d, ad, (int)at);
        base += total;
    }
    if (threadIdx.x == 0) *d_count = (int)base;
}

static bool table_ok(const dz_track_table *t, long rows) {
    return t && rows <= t->cap && t->x && t->P && t->Q && t->dt && t->box && t->cls && t->score && t->update_score && t->num_points && t->hit && t->miss && t->id;
}
static bool ab3d_ok(const dz_track_ab3d *a, long rows) {
    return a && rows <= a->stride && a->x && a->P && a->box && a->work && a->hits;
}
// rows * 25 floats (P, Q) is the widest offset of a table, rows * ROW words that of a row buffer
static bool offsets_ok(const char *who, long table_rows, long buffer_rows) {
    if (table_rows * 25 >= (1L << 31) || buffer_rows * ROW >= (1L << 31)) {
        set_error("%s: %ld table rows / %ld buffer rows overflow 32-bit offsets", who, table_rows, buffer_rows);
        return false;
    }
    return true;
}
static int class_thr(const char *who, const float *h_thr, int n_cls, ClassThr &thr) {
    if (n_cls < 1 || n_cls > DZ_TRACK_MAX_CLASSES) {
        set_error("%s: %d classes (1..%d)", who, n_cls, DZ_TRACK_MAX_CLASSES);
        return DZ_ERR_UNSUPPORTED;
    }
    DZ_CHECK_ARG(h_thr, "%s: null thresholds", who);
    for (int k = 0; k < DZ_TRACK_MAX_CLASSES; ++k) thr.v[k] = k < n_cls ? h_thr[k] : h_thr[0];
    return DZ_OK;
}

}  // namespace dz

using namespace dz;

extern "C" {

int dz_track_predict(const dz_track_table *t, int n, int gate_class, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n >= 0, "dz_track_predict: negative size");
    if (!offsets_ok("dz_track_predict", n, 0)) return DZ_ERR_UNSUPPORTED;
    if (n == 0) return DZ_OK;
    DZ_CHECK_ARG(table_ok(t, n), "dz_track_predict: null pointer or n > cap");
    hipLaunchKernelGGL(k_track_predict, dim3(ceil_div(n, TRK_THREADS)), dim3(TRK_THREADS), 0, stream, *t, n, gate_class);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_track_affinity(const dz_track_table *t, int n, const int *ext, int n_ext, const int *row_idx, int nr, const int *det, int n_det,
                      const int *col_idx, int nc, int metric, int distinguish_class, const float *h_thr, int n_cls, float *out,
                      void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n >= 0 && n_ext >= 0 && nr >= 0 && n_det >= 0 && nc >= 0, "dz_track_affinity: negative size");
    if (metric != DZ_TRACK_AFF_IOU_BEV && metric != DZ_BOXM_IOU3D && metric != DZ_BOXM_GIOU3D) {
        set_error("dz_track_affinity: unknown metric %d", metric);
        return DZ_ERR_UNSUPPORTED;
    }
    ClassThr thr;
    const int rc = class_thr("dz_track_affinity", h_thr, n_cls, thr);
    if (rc != DZ_OK) return rc;
    if (!offsets_ok("dz_track_affinity", n, n_ext > n_det ? n_ext : n_det)) return DZ_ERR_UNSUPPORTED;
    if (nr == 0 || nc == 0) return DZ_OK;
    DZ_CHECK_ARG(row_idx && col_idx && det && out && (n == 0 || (t && t->box && t->cls && n <= t->cap)) && (n_ext == 0 || ext),
                 "dz_track_affinity: null pointer");
    const float *tbox = n ? t->box : nullptr;
    const int *tcls = n ? t->cls : nullptr;
    const dim3 grid(stream_grid((long)nr * nc, TRK_THREADS)), block(TRK_THREADS);
    switch (metric) {
        case DZ_TRACK_AFF_IOU_BEV:
            hipLaunchKernelGGL(k_track_affinity<DZ_TRACK_AFF_IOU_BEV>, grid, block, 0, stream, tbox, tcls, n, ext, n_ext, row_idx, nr, det,
                               n_det, col_idx, nc, distinguish_class, thr, out);
            break;
        case DZ_BOXM_IOU3D:
            hipLaunchKernelGGL(k_track_affinity<DZ_BOXM_IOU3D>, grid, block, 0, stream, tbox, tcls, n, ext, n_ext, row_idx, nr, det, n_det,
                               col_idx, nc, distinguish_class, thr, out);
            break;
        default:
            hipLaunchKernelGGL(k_track_affinity<DZ_BOXM_GIOU3D>, grid, block, 0, stream, tbox, tcls, n, ext, n_ext, row_idx, nr, det, n_det,
                               col_idx, nc, distinguish_class, thr, out);
    }
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_track_update(const dz_track_table *t, int n, const int *det, int n_det, const int *match, int m, float r, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n >= 0 && n_det >= 0 && m >= 0, "dz_track_update: negative size");
    if (!offsets_ok("dz_track_update", n > m ? n : m, n_det)) return DZ_ERR_UNSUPPORTED;
    if (m == 0) return DZ_OK;
    DZ_CHECK_ARG(table_ok(t, n) && det && match, "dz_track_update: null pointer or n > cap");
    hipLaunchKernelGGL(k_track_update, dim3(ceil_div(m, TRK_THREADS)), dim3(TRK_THREADS), 0, stream, *t, n, det, n_det, match, m, r);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_track_spawn(const dz_track_table *t, int n, const int *src, int n_src, const int *src_idx, const int *ids, int m, float p0,
                   float p1, float q0, float q1, float dt, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n >= 0 && n_src >= 0 && m >= 0, "dz_track_spawn: negative size");
    if (!offsets_ok("dz_track_spawn", (long)n + m, n_src)) return DZ_ERR_UNSUPPORTED;
    if (m == 0) return DZ_OK;
    DZ_CHECK_ARG(table_ok(t, (long)n + m) && src && src_idx && ids, "dz_track_spawn: null pointer or n + m > cap");
    hipLaunchKernelGGL(k_track_spawn, dim3(ceil_div(m, TRK_THREADS)), dim3(TRK_THREADS), 0, stream, *t, n, src, n_src, src_idx, ids, m, p0,
                       p1, q0, q1, dt);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

size_t dz_track_merge_workspace_bytes(int n) {
    if (n <= 0) return 256;
    const size_t words = (size_t)(n + 63) / 64;
    return align_up((size_t)n * words * sizeof(unsigned long long), 256) + align_up((size_t)n * sizeof(int), 256);
}

int dz_track_merge(const dz_track_table *t, int n, const float *h_thr, int n_cls, int *removed, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n >= 0, "dz_track_merge: negative size");
    ClassThr thr;
    int rc = class_thr("dz_track_merge", h_thr, n_cls, thr);
    if (rc != DZ_OK) return rc;
    for (int k = 0; k < n_cls; ++k)
        if (!(h_thr[k] > 0.f)) {
            set_error("dz_track_merge: threshold %d is %g; the sweep needs thresholds > 0", k, (double)h_thr[k]);
            return DZ_ERR_UNSUPPORTED;
        }
    if (n > MERGE_MAX_TRACKS) {
        set_error("dz_track_merge: %d tracks (<= %d)", n, MERGE_MAX_TRACKS);
        return DZ_ERR_UNSUPPORTED;
    }
    if (n == 0) return DZ_OK;
    DZ_CHECK_ARG(table_ok(t, n) && removed && ws, "dz_track_merge: null pointer or n > cap");
    if (ws_bytes < dz_track_merge_workspace_bytes(n)) { set_error("dz_track_merge: workspace too small"); return DZ_ERR_WORKSPACE; }
    const int words = (n + 63) / 64;
    unsigned long long *bits = (unsigned long long *)ws;
    int *busy = (int *)((char *)ws + align_up((size_t)n * words * sizeof(unsigned long long), 256));
    rc = fill_u32(busy, 0u, (size_t)n, stream);
    if (rc != DZ_OK) return rc;
    hipLaunchKernelGGL(k_track_merge_bits, dim3(words, ceil_div(n, MERGE_ROWS_PER_WAVE)), dim3(64), 0, stream, t->box, t->cls, n, thr, bits,
                       words, busy);
    DZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_track_merge_sweep, dim3(1), dim3(64), 0, stream, bits, words, busy, t->id, n, removed);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_track_compact(const dz_track_table *src, int n, const int *removed, int death_age, const dz_track_table *dst, int *d_count,
                     void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n >= 0, "dz_track_compact: negative size");
    if (!offsets_ok("dz_track_compact", n, 0)) return DZ_ERR_UNSUPPORTED;
    DZ_CHECK_ARG(d_count, "dz_track_compact: null count");
    if (n == 0) return fill_u32(d_count, 0u, 1, stream);
    DZ_CHECK_ARG(table_ok(src, n) && table_ok(dst, n) && src->x != dst->x, "dz_track_compact: null pointer, n > cap or dst == src");
    hipLaunchKernelGGL(k_track_compact, dim3(1), dim3(256), 0, stream, *src, n, removed, death_age, *dst, d_count);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_track_log(const dz_track_table *t, int n, int frame, int *log, long log_n, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n >= 0 && log_n >= 0, "dz_track_log: negative size");
    if (!offsets_ok("dz_track_log", n, log_n + n)) return DZ_ERR_UNSUPPORTED;
    if (n == 0) return DZ_OK;
    DZ_CHECK_ARG(table_ok(t, n) && log, "dz_track_log: null pointer or n > cap");
    hipLaunchKernelGGL(k_track_log, dim3(ceil_div(n, TRK_THREADS)), dim3(TRK_THREADS), 0, stream, *t, n, frame, log + log_n * ROW);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_track_ab3d_predict(const dz_track_table *t, const dz_track_ab3d *a, int n, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n >= 0, "dz_track_ab3d_predict: negative size");
    if (!offsets_ok("dz_track_ab3d_predict", n, 0)) return DZ_ERR_UNSUPPORTED;
    if (n == 0) return DZ_OK;
    DZ_CHECK_ARG(table_ok(t, n) && ab3d_ok(a, n), "dz_track_ab3d_predict: null pointer or n > cap / stride");
    hipLaunchKernelGGL(k_track_ab3d_predict, dim3(ceil_div(n, TRK_THREADS)), dim3(TRK_THREADS), 0, stream, *t, *a, n);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_track_ab3d_update(const dz_track_table *t, const dz_track_ab3d *a, int n, const int *det, const double *det64, int n_det,
                         const int *match, int m, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n >= 0 && n_det >= 0 && m >= 0, "dz_track_ab3d_update: negative size");
    if (!offsets_ok("dz_track_ab3d_update", n > m ? n : m, n_det)) return DZ_ERR_UNSUPPORTED;
    if (m == 0) return DZ_OK;
    DZ_CHECK_ARG(table_ok(t, n) && ab3d_ok(a, n) && det && det64 && match, "dz_track_ab3d_update: null pointer or n > cap / stride");
    hipLaunchKernelGGL(k_track_ab3d_update, dim3(ceil_div(m, TRK_THREADS)), dim3(TRK_THREADS), 0, stream, *t, *a, n, det, det64, n_det, match,
                       m);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_track_ab3d_spawn(const dz_track_table *t, const dz_track_ab3d *a, int n, const int *src, const double *src64, int n_src,
                        const int *src_idx, const int *ids, int m, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n >= 0 && n_src >= 0 && m >= 0, "dz_track_ab3d_spawn: negative size");
    if (!offsets_ok("dz_track_ab3d_spawn", (long)n + m, n_src)) return DZ_ERR_UNSUPPORTED;
    if (m == 0) return DZ_OK;
    DZ_CHECK_ARG(table_ok(t, (long)n + m) && ab3d_ok(a, (long)n + m) && src && src64 && src_idx && ids,
                 "dz_track_ab3d_spawn: null pointer or n + m > cap / stride");
    hipLaunchKernelGGL(k_track_ab3d_spawn, dim3(ceil_div(m, TRK_THREADS)), dim3(TRK_THREADS), 0, stream, *t, *a, n, src, src64, n_src, src_idx,
                       ids, m);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_track_ab3d_compact(const dz_track_table *src, const dz_track_ab3d *asrc, int n, const int *removed, int death_age,
                          const dz_track_table *dst, const dz_track_ab3d *adst, int *d_count, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n >= 0, "dz_track_ab3d_compact: negative size");
    if (!offsets_ok("dz_track_ab3d_compact", n, 0)) return DZ_ERR_UNSUPPORTED;
    DZ_CHECK_ARG(d_count, "dz_track_ab3d_compact: null count");
    if (n == 0) return fill_u32(d_count, 0u, 1, stream);
    DZ_CHECK_ARG(table_ok(src, n) && table_ok(dst, n) && src->x != dst->x && ab3d_ok(asrc, n) && ab3d_ok(adst, n) && asrc->x != adst->x,
                 "dz_track_ab3d_compact: null pointer, n > cap / stride or dst == src");
    hipLaunchKernelGGL(k_track_ab3d_compact, dim3(1), dim3(256), 0, stream, *src, *asrc, n, removed, death_age, *dst, *adst, d_count);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_track_ab3d_log(const dz_track_table *t, const dz_track_ab3d *a, int n, int frame, int frame_id, int birth_age, int death_age,
                      int *log, double *log64, long log_n, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n >= 0 && log_n >= 0, "dz_track_ab3d_log: negative size");
    if (!offsets_ok("dz_track_ab3d_log", n, log_n + n)) return DZ_ERR_UNSUPPORTED;
    if (n == 0) return DZ_OK;
    DZ_CHECK_ARG(table_ok(t, n) && ab3d_ok(a, n) && log && log64, "dz_track_ab3d_log: null pointer or n > cap / stride");
    hipLaunchKernelGGL(k_track_ab3d_log, dim3(ceil_div(n, TRK_THREADS)), dim3(TRK_THREADS), 0, stream, *t, *a, n, frame, frame_id, birth_age,
                       death_age, log + log_n * ROW, log64 + log_n * 9);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

}  // extern "C"
