// Per-track and per-pair bodies of the tracking module, shared by the per-op kernels (track.hip: one launch per op and frame)
// and the sequence kernels (track_seq.hip: one workgroup walks a whole pass).  Both call these functions, so the two paths
// compute the same bytes.  Include after `#pragma clang fp contract(off)`, as box_geom.h.
//
// Reference:
//   tracking/detzero_track/models/tracking_modules/kalman_filter/kalman_filter.py:10-58 (constructor), :85-108 (predict), :110-146 (update)
//   tracking/detzero_track/models/tracking_modules/data_association/data_association.py:36-60 (one_stage), distance.py:9-23 (GNN masking)
//   tracking/detzero_track/models/tracking_modules/track_manager.py:262-310 (overlap_track_merge), :198-214 (info / death)
#pragma once
#include "common.h"
#include "box_geom.h"
#include "class_thr.h"

namespace dz {

constexpr int ROW = DZ_TRACK_ROW_WORDS;
constexpr int ROW_SCORE = 9, ROW_HIT = 10, ROW_NPTS = 11, ROW_ID = 12, ROW_CLS = 13, ROW_FRAME = 14;
constexpr int MERGE_ROWS_PER_WAVE = 16;

// ------------------------------------------------------------------------------------------
// predict: track i
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void track_predict_body(const dz_track_table &t, int i, int gate_class) {
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
// affinity -> cost of one (row, column) pair.  ri >= 0: table row, ri < 0: row -ri - 1 of `ext`; ci: row of `det`.
// cp / ang: this thread's slots of the 16 * ld scratch entries of rect_overlap.
// ------------------------------------------------------------------------------------------
template <int METRIC>
__device__ __forceinline__ float track_cost_body(const float *__restrict__ tbox, const int *__restrict__ tcls, int n_tab,
                                                 const int *__restrict__ ext, int n_ext, int ri, const int *__restrict__ det, int n_det, int ci,
                                                 int distinguish, const ClassThr &thr, P2 *cp, float *ang, int ld) {
    const bool row_tab = ri >= 0;
    const int re = -ri - 1;
    // an index outside its buffer is never followed: the pair cannot match
    if ((row_tab ? ri >= n_tab : re >= n_ext) || ci < 0 || ci >= n_det) return 5000.f;
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
        const float so = footprints_near(A, B) ? rect_overlap(A, B, cp, ang, ld) : 0.f;
        aff = so / fmaxf(sa + sb - so, GEO_EPS);
    } else {
        aff = pair_metric_ld<METRIC == DZ_TRACK_AFF_IOU_BEV ? DZ_BOXM_IOU3D : METRIC>(A, B, cp, ang, ld);
    }
    if (distinguish && ca != cb) aff = 0.f;             // data_association.py:49-51
    if (aff < thr_of(thr, ca)) aff = 0.f;               // :54-55
    float cost = 1.0f - aff;                            // :57
    if (cost >= 1.f) cost = 5000.f;                     // distance.py:22
    return cost;
}

// ------------------------------------------------------------------------------------------
// update: track i from detection row d
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void track_update_body(const dz_track_table &t, int i, const int *__restrict__ d, int stage, float r_meas) {
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

// ------------------------------------------------------------------------------------------
// spawn: table row i from source row s (ok = the source index was inside its buffer; else an all-zero track)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void track_spawn_body(const dz_track_table &t, int i, const int *__restrict__ s, bool ok, int id, float p0, float p1,
                                                 float q0, float q1, float dt) {
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
    t.id[i] = id;
}

// ------------------------------------------------------------------------------------------
// log: info() of track i into row o
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void track_log_body(const dz_track_table &t, int i, int frame, int *__restrict__ o) {
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
// Wave code (no workgroup barrier): cp / ang = this lane's slots of the wave's own 16 * 64 scratch entries.
__device__ __forceinline__ void track_merge_bits_body(const float *__restrict__ box, const int *__restrict__ cls, int n, const ClassThr &thr,
                                                      unsigned long long *__restrict__ bits, int words, int *__restrict__ busy, int cb, int row0,
                                                      int lane, P2 *cp, float *ang) {
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
            const float ratio = rect_overlap(A, B, cp, ang, 64) / (area + 1e-9f);
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

// The reference's greedy sweep (track_manager.py:283-303) by a workgroup of WAVES wavefronts whose every thread calls it.
// cleared = the columns set to 0 so far = keep + deprecated sets (every set's columns are cleared when it is formed), so "i in keep
// or deprecated" is one bit test and a set is a row of `bits` without the cleared columns; its lowest id can then never be a
// deprecated track, which is the reference's "best_idx in deprecate_index_set" case that does nothing.
// cleared / dep: LDS, `words` entries each; red: LDS, WAVES entries (read for WAVES > 1 only).  Every branch around a barrier
// depends on `busy` and on `cleared` after a barrier: the same in every thread.
template <int WAVES>
__device__ __forceinline__ void track_merge_sweep_body(const unsigned long long *__restrict__ bits, int words, const int *__restrict__ busy,
                                                       const int *__restrict__ id, int n, int *__restrict__ removed, unsigned long long *cleared,
                                                       unsigned long long *dep, unsigned long long *red) {
    constexpr int T = WAVES * 64;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int w = tid; w < words; w += T) { cleared[w] = 0ull; dep[w] = 0ull; }
    __syncthreads();
    for (int c = 0; c < words; ++c) {
        const int mine = c * 64 + lane;
        unsigned long long todo = __ballot(mine < n && busy[mine] != 0);
        while (todo) {          // workgroup-uniform; at most 64 rounds
            const int b = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int i = c * 64 + b;
            if ((cleared[c] >> b) & 1ull) continue;
            unsigned long long best = ~0ull;      // (id, index), lowest first
            for (int w = tid; w < words; w += T) {
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
            if (WAVES > 1) {
                if (lane == 0) red[tid >> 6] = best;
                __syncthreads();
#pragma unroll
                for (int w = 0; w < WAVES; ++w) best = red[w] < best ? red[w] : best;
            }
            if (best != ~0ull) {
                const int keep = (int)(best & 0xFFFFFFFFull);
                for (int w = tid; w < words; w += T) {
                    const unsigned long long set = bits[(size_t)i * words + w] & ~cleared[w];
                    cleared[w] |= set;
                    dep[w] |= (keep >> 6) == w ? set & ~(1ull << (keep & 63)) : set;
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += T) removed[i] = (int)((dep[i >> 6] >> (i & 63)) & 1ull);
}

// ------------------------------------------------------------------------------------------
// compact: survivor row i of table s becomes row o of table d (another table)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool track_keep_body(const dz_track_table &s, int i, const int *__restrict__ removed, int death_age) {
    if (removed && removed[i] != 0) return false;
    if (death_age != -1 && s.miss[i] >= death_age) return false;       // track_manager.py:212-214
    return true;
}
__device__ __forceinline__ void track_copy_body(const dz_track_table &s, int i, const dz_track_table &d, int o) {
#pragma unroll
    for (int q = 0; q < 5; ++q) d.x[o * 5 + q] = s.x[i * 5 + q];
#pragma unroll
    for (int q = 0; q < 25; ++q) { d.P[o * 25 + q] = s.P[i * 25 + q]; d.Q[o * 25 + q] = s.Q[i * 25 + q]; }
#pragma unroll
    for (int q = 0; q < 9; ++q) d.box[o * 9 + q] = s.box[i * 9 + q];
    d.dt[o] = s.dt[i]; d.cls[o] = s.cls[i]; d.score[o] = s.score[i]; d.update_score[o] = s.update_score[i];
    d.num_points[o] = s.num_points[i]; d.hit[o] = s.hit[i]; d.miss[o] = s.miss[i]; d.id[o] = s.id[i];
}

}  // namespace dz
