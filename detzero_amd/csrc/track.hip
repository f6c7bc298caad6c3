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
#include "common.h"

#pragma clang fp contract(off)

#include "box_geom.h"
#include "class_thr.h"

namespace dz {

constexpr int TRK_THREADS = 128;
constexpr int ROW = DZ_TRACK_ROW_WORDS;
constexpr int ROW_SCORE = 9, ROW_HIT = 10, ROW_NPTS = 11, ROW_ID = 12, ROW_CLS = 13, ROW_FRAME = 14;
constexpr int MERGE_ROWS_PER_WAVE = 16;
constexpr int MERGE_MAX_TRACKS = 32768;
constexpr int MERGE_MAX_WORDS = MERGE_MAX_TRACKS / 64;

// ------------------------------------------------------------------------------------------
// predict
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRK_THREADS) void k_track_predict(dz_track_table t, int n, int gate_class) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float *x = t.x + i * 5, *P = t.P + i * 25, *Q = t.Q + i * 25, *box = t.box + i * 9;
    const float dt = t.dt[i];
    float vx = x[3], vy = x[4];
    if (t.cls[i] == gate_class) {       // kalman_filter.py:92-95
        const float speed = sqrtf(vx * vx + vy * vy);
        if (speed <= fmaxf(fmaxf(box[3], box[4]), box[5]) / 2.f) { vx = 0.f; vy = 0.f; }
    }
    // x = F x with F = I + dt at (0,3), (1,4)
    const float x0 = x[0] + dt * vx, x1 = x[1] + dt * vy, x2 = x[2];
    x[0] = x0; x[1] = x1; x[3] = vx; x[4] = vy;
    // P = F P F^T + Q, Q *= 1.5
    float p[25], q[25];
#pragma unroll
    for (int k = 0; k < 25; ++k) { p[k] = P[k]; q[k] = Q[k]; }
#pragma unroll
    for (int c = 0; c < 5; ++c) {       // F P: rows 0, 1
        p[0 * 5 + c] = p[0 * 5 + c] + dt * p[3 * 5 + c];
        p[1 * 5 + c] = p[1 * 5 + c] + dt * p[4 * 5 + c];
    }
#pragma unroll
    for (int r = 0; r < 5; ++r) {       // (F P) F^T: columns 0, 1
        p[r * 5 + 0] = p[r * 5 + 0] + dt * p[r * 5 + 3];
        p[r * 5 + 1] = p[r * 5 + 1] + dt * p[r * 5 + 4];
    }
#pragma unroll
    for (int k = 0; k < 25; ++k) { P[k] = p[k] + q[k]; Q[k] = q[k] * 1.5f; }
    t.miss[i] += 1;
    t.hit[i] = 0;
    box[0] = x0; box[1] = x1; box[2] = x2; box[7] = vx; box[8] = vy;       // 3:7 = size, heading: unchanged
}

// ------------------------------------------------------------------------------------------
// affinity -> cost
// ------------------------------------------------------------------------------------------
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
        const int ri = row_idx[r], ci = col_idx[c];
        const bool row_tab = ri >= 0;
        const int re = -ri - 1;
        // an index outside its buffer is never followed: the pair cannot match
        if ((row_tab ? ri >= n_tab : re >= n_ext) || ci < 0 || ci >= n_det) { out[idx] = 5000.f; continue; }
        float A[7], B[7];
        int ca;
        if (row_tab) {
#pragma unroll
            for (int q = 0; q < 7; ++q) A[q] = tbox[ri * 9 + q];
            ca = tcls[ri];
        } else {
            const int *e = ext + re * ROW;
#pragma unroll
            for (int q = 0; q < 7; ++q) A[q] = __int_as_float(e[q]);
            ca = e[ROW_CLS];
        }
        const int *d = det + ci * ROW;
#pragma unroll
        for (int q = 0; q < 7; ++q) B[q] = __int_as_float(d[q]);
        const int cb = d[ROW_CLS];
        float aff;
        if (METRIC == DZ_TRACK_AFF_IOU_BEV) {       // rect_iou (box_geom.h) with the circle test in front: far pairs overlap by exactly +0
            const float sa = A[3] * A[4], sb = B[3] * B[4];
            const float so = footprints_near(A, B) ? rect_overlap(A, B, cp, ang, TRK_THREADS) : 0.f;
            aff = so / fmaxf(sa + sb - so, GEO_EPS);
        } else {
            aff = pair_metric_ld<METRIC == DZ_TRACK_AFF_IOU_BEV ? DZ_BOXM_IOU3D : METRIC>(A, B, cp, ang, TRK_THREADS);
        }
        if (distinguish && ca != cb) aff = 0.f;             // data_association.py:49-51
        if (aff < thr_of(thr, ca)) aff = 0.f;               // :54-55
        float cost = 1.0f - aff;                            // :57
        if (cost >= 1.f) cost = 5000.f;                     // distance.py:22
        out[idx] = cost;
    }
}

// ------------------------------------------------------------------------------------------
// update / spawn / log
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRK_THREADS) void k_track_update(dz_track_table t, int n, const int *__restrict__ det, int n_det,
                                                              const int *__restrict__ match, int m, float r_meas) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int i = match[k * 3 + 0], di = match[k * 3 + 1], stage = match[k * 3 + 2];
    if (i < 0 || i >= n || di < 0 || di >= n_det) return;
    const int *d = det + di * ROW;
    t.miss[i] = 0;
    t.score[i] = __int_as_float(d[ROW_SCORE]);
    t.num_points[i] = d[ROW_NPTS];
    if (stage != 0) { t.hit[i] = 2; return; }             // kalman_filter.py:120-122
    t.hit[i] = 1;
    t.cls[i] = d[ROW_CLS];
    t.update_score[i] = fmaxf(__int_as_float(d[ROW_SCORE]), 0.03f);
    float *x = t.x + i * 5, *P = t.P + i * 25, *box = t.box + i * 9;
    float p[25];
#pragma unroll
    for (int q = 0; q < 25; ++q) p[q] = P[q];
    float z[3], res[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { z[a] = __int_as_float(d[a]); res[a] = z[a] - x[a]; }
    // S = H P H^T + R, general 3x3 inverse by cofactors.  Q grows by 1.5 per predicted frame for every track, matched or not, so S
    // reaches 1e20 after a hundred frames and the cofactors' products would leave fp32: S is scaled by the power of two of its
    // largest entry first (exact) and the inverse scaled back.
    float sm[9] = {p[0] + r_meas, p[1], p[2], p[5], p[6] + r_meas, p[7], p[10], p[11], p[12] + r_meas};
    float big = 0.f;
#pragma unroll
    for (int q = 0; q < 9; ++q) big = fmaxf(big, fabsf(sm[q]));
    const int expo = big > 0.f && big <= 3.0e38f ? ilogbf(big) : 0;
#pragma unroll
    for (int q = 0; q < 9; ++q) sm[q] = ldexpf(sm[q], -expo);
    const float s00 = sm[0], s01 = sm[1], s02 = sm[2], s10 = sm[3], s11 = sm[4], s12 = sm[5], s20 = sm[6], s21 = sm[7], s22 = sm[8];
    const float c00 = s11 * s22 - s12 * s21, c01 = s12 * s20 - s10 * s22, c02 = s10 * s21 - s11 * s20;
    const float det3 = s00 * c00 + s01 * c01 + s02 * c02;
    float inv[9];
    inv[0] = c00 / det3; inv[1] = (s02 * s21 - s01 * s22) / det3; inv[2] = (s01 * s12 - s02 * s11) / det3;
    inv[3] = c01 / det3; inv[4] = (s00 * s22 - s02 * s20) / det3; inv[5] = (s02 * s10 - s00 * s12) / det3;
    inv[6] = c02 / det3; inv[7] = (s01 * s20 - s00 * s21) / det3; inv[8] = (s00 * s11 - s01 * s10) / det3;
#pragma unroll
    for (int q = 0; q < 9; ++q) inv[q] = ldexpf(inv[q], -expo);
    float K[15];        // K = P H^T S^-1 (5x3)
#pragma unroll
    for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) K[a * 3 + b] = p[a * 5 + 0] * inv[0 * 3 + b] + p[a * 5 + 1] * inv[1 * 3 + b] + p[a * 5 + 2] * inv[2 * 3 + b];
    float xn[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) xn[a] = x[a] + (K[a * 3 + 0] * res[0] + K[a * 3 + 1] * res[1] + K[a * 3 + 2] * res[2]);
#pragma unroll
    for (int a = 0; a < 5; ++a)         // P -= K (H P): rows 0..2 of the OLD P
#pragma unroll
        for (int b = 0; b < 5; ++b)
            P[a * 5 + b] = p[a * 5 + b] - (K[a * 3 + 0] * p[0 * 5 + b] + K[a * 3 + 1] * p[1 * 5 + b] + K[a * 3 + 2] * p[2 * 5 + b]);
    x[0] = z[0]; x[1] = z[1]; x[2] = z[2]; x[3] = xn[3]; x[4] = xn[4];       // :141
#pragma unroll
    for (int q = 0; q < 7; ++q) box[q] = __int_as_float(d[q]);
    box[7] = xn[3]; box[8] = xn[4];
}

__global__ __launch_bounds__(TRK_THREADS) void k_track_spawn(dz_track_table t, int n, const int *__restrict__ src, int n_src,
                                                             const int *__restrict__ src_idx, const int *__restrict__ ids, int m, float p0,
                                                             float p1, float q0, float q1, float dt) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int i = n + k;
    const int si = src_idx[k];
    const bool ok = si >= 0 && si < n_src;      // (an index outside the buffer gives an all-zero track; the wrapper refuses it first)
    const int *s = src + (ok ? si : 0) * ROW;
    float *x = t.x + i * 5, *P = t.P + i * 25, *Q = t.Q + i * 25, *box = t.box + i * 9;
#pragma unroll
    for (int q = 0; q < 7; ++q) box[q] = ok ? __int_as_float(s[q]) : 0.f;
    box[7] = 0.f; box[8] = 0.f;
    x[0] = box[0]; x[1] = box[1]; x[2] = box[2]; x[3] = 0.f; x[4] = 0.f;
#pragma unroll
    for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            P[a * 5 + b] = a == b ? (a < 3 ? p0 : p1) : 0.f;
            Q[a * 5 + b] = a == b ? (a < 3 ? q0 : q1) : 0.f;
        }
    t.dt[i] = dt;
    t.cls[i] = ok ? s[ROW_CLS] : 0;
    const float score = ok ? __int_as_float(s[ROW_SCORE]) : 0.f;
    t.score[i] = score;
    t.update_score[i] = score;
    t.num_points[i] = ok ? s[ROW_NPTS] : 0;
    t.hit[i] = 1;
    t.miss[i] = 0;
    t.id[i] = ids[k];
}

__global__ __launch_bounds__(TRK_THREADS) void k_track_log(dz_track_table t, int n, int frame, int *__restrict__ log) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int *o = log + (long)i * ROW;
#pragma unroll
    for (int q = 0; q < 9; ++q) o[q] = __float_as_int(t.box[i * 9 + q]);
    o[ROW_SCORE] = __float_as_int(t.score[i]);
    o[ROW_HIT] = t.hit[i];
    o[ROW_NPTS] = t.num_points[i];
    o[ROW_ID] = t.id[i];
    o[ROW_CLS] = t.cls[i];
    o[ROW_FRAME] = frame;
    o[15] = 0;
}

// ------------------------------------------------------------------------------------------
// merge
// ------------------------------------------------------------------------------------------
// bits[i][cb] bit j: track cb*64+j belongs to row i's overlapped set.  One wavefront per (16 rows, 64 columns) as k_nms_mask: a lane
// owns a column box, the wave walks its rows, __ballot packs the word.  busy[i] = 1 when row i or column i holds a bit off the
// diagonal: every other track is alone in its set, nobody's set contains it, and the sweep never has to look at it.
__global__ __launch_bounds__(64) void k_track_merge_bits(const float *__restrict__ box, const int *__restrict__ cls, int n, ClassThr thr,
                                                         unsigned long long *__restrict__ bits, int words, int *__restrict__ busy) {
    __shared__ P2 cp_s[16 * 64];
    __shared__ float ang_s[16 * 64];
    const int cb = blockIdx.x, row0 = blockIdx.y * MERGE_ROWS_PER_WAVE;
    if (row0 >= n) return;
    const int lane = threadIdx.x;
    const int rows = min(MERGE_ROWS_PER_WAVE, n - row0);
    const int col = cb * 64 + lane;
    const bool col_ok = col < n;
    float B[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) B[q] = col_ok ? box[col * 9 + q] : 0.f;
    const int clsb = col_ok ? cls[col] : -1;
    unsigned long long word = 0ull;
    bool col_busy = false;
    for (int i = 0; i < rows; ++i) {
        const int row = row0 + i;
        float A[7];       // wave-uniform
#pragma unroll
        for (int q = 0; q < 7; ++q) A[q] = box[row * 9 + q];
        const int clsa = cls[row];
        bool in_set = false;
        if (col_ok && clsa == clsb && footprints_near(A, B)) {      // track_manager.py:279-281, :293-294
            const float area = A[3] * A[4];
            const float ratio = rect_overlap(A, B, cp_s + lane, ang_s + lane, 64) / (area + 1e-9f);
            in_set = ratio >= thr_of(thr, clsa);
        }
        const unsigned long long m = __ballot(in_set);
        if (lane == i) word = m;
        const bool off_diag = in_set && col != row;
        col_busy = col_busy || off_diag;
        if (__ballot(off_diag) != 0ull && lane == 0) busy[row] = 1;
    }
    if (col_busy) busy[col] = 1;
    if (lane < rows) bits[(size_t)(row0 + lane) * words + cb] = word;
}

// The reference's greedy sweep (track_manager.py:283-303), one wavefront.  cleared = the columns set to 0 so far = keep + deprecated
// sets (every set's columns are cleared when it is formed), so "i in keep or deprecated" is one bit test and a set is a row of
// `bits` without the cleared columns; its lowest id can then never be a deprecated track, which is the reference's
// "best_idx in deprecate_index_set" case that does nothing.
__global__ __launch_bounds__(64) void k_track_merge_sweep(const unsigned long long *__restrict__ bits, int words, const int *__restrict__ busy,
                                                          const int *__restrict__ id, int n, int *__restrict__ removed) {
    __shared__ unsigned long long cleared[MERGE_MAX_WORDS], dep[MERGE_MAX_WORDS];
    const int lane = threadIdx.x;
    for (int w = lane; w < words; w += 64) { cleared[w] = 0ull; dep[w] = 0ull; }
    __syncthreads();
    for (int c = 0; c < words; ++c) {
        const int mine = c * 64 + lane;
        unsigned long long todo = __ballot(mine < n && busy[mine] != 0);
        while (todo) {          // wave-uniform
            const int b = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int i = c * 64 + b;
            if ((cleared[c] >> b) & 1ull) continue;
            unsigned long long best = ~0ull;      // (id, index), lowest first
            for (int w = lane; w < words; w += 64) {
                unsigned long long set = bits[(size_t)i * words + w] & ~cleared[w];
                while (set) {
                    const int j = w * 64 + __ffsll((long long)set) - 1;
                    set &= set - 1;
                    const unsigned long long key = ((unsigned long long)((unsigned)id[j] ^ 0x80000000u) << 32) | (unsigned)j;
                    best = key < best ? key : best;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(best, off, 64);
                best = o < best ? o : best;
            }
            if (best != ~0ull) {
                const int keep = (int)(best & 0xFFFFFFFFull);
                for (int w = lane; w < words; w += 64) {
                    const unsigned long long set = bits[(size_t)i * words + w] & ~cleared[w];
                    cleared[w] |= set;
                    dep[w] |= (keep >> 6) == w ? set & ~(1ull << (keep & 63)) : set;
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) removed[i] = (int)((dep[i >> 6] >> (i & 63)) & 1ull);
}

// ------------------------------------------------------------------------------------------
// compact
// ------------------------------------------------------------------------------------------
// One workgroup: 256 rows at a time, exclusive scan of the keep flags, survivors copied in order.  A table is a few thousand rows
// of 72 words; the copy is not worth a second launch.
__global__ __launch_bounds__(256) void k_track_compact(dz_track_table s, int n, const int *__restrict__ removed, int death_age,
                                                       dz_track_table d, int *__restrict__ d_count) {
    __shared__ uint32_t scan_s[4];
    uint32_t base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + threadIdx.x;
        bool keep = i < n;
        if (keep && removed && removed[i] != 0) keep = false;
        if (keep && death_age != -1 && s.miss[i] >= death_age) keep = false;       // track_manager.py:212-214
        uint32_t total;
        const uint32_t at = base + block_excl_scan_256(keep ? 1u : 0u, scan_s, total);
        if (keep) {
            const int o = (int)at;
#pragma unroll
            for (int q = 0; q < 5; ++q) d.x[o * 5 + q] = s.x[i * 5 + q];
#pragma unroll
            for (int q = 0; q < 25; ++q) { d.P[o * 25 + q] = s.P[i * 25 + q]; d.Q[o * 25 + q] = s.Q[i * 25 + q]; }
#pragma unroll
            for (int q = 0; q < 9; ++q) d.box[o * 9 + q] = s.box[i * 9 + q];
            d.dt[o] = s.dt[i]; d.cls[o] = s.cls[i]; d.score[o] = s.score[i]; d.update_score[o] = s.update_score[i];
            d.num_points[o] = s.num_points[i]; d.hit[o] = s.hit[i]; d.miss[o] = s.miss[i]; d.id[o] = s.id[i];
        }
        base += total;
    }
    if (threadIdx.x == 0) *d_count = (int)base;
}

static bool table_ok(const dz_track_table *t, long rows) {
    return t && rows <= t->cap && t->x && t->P && t->Q && t->dt && t->box && t->cls && t->score && t->update_score && t->num_points && t->hit && t->miss && t->id;
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

}  // extern "C"
