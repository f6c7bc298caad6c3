// Per-track bodies of the AB3DMOT filter, float64, shared by the per-op kernels (track.hip) and the sequence kernels
// (track_seq.hip) exactly as track_body.h is: both call these functions, so the two paths compute the same bytes.  Include after
// `#pragma clang fp contract(off)`.
//
// Reference:
//   tracking/detzero_track/models/tracking_modules/kalman_filter/ab3dmot.py:13-86 (constructor), :88-109 (predict), :111-149 (update)
//   filterpy.kalman.KalmanFilter(dim_x=10, dim_z=7): predict (x = F x, P = F P F^T + Q), update (Joseph form)
//   tracking/detzero_track/models/tracking_modules/track_manager.py:201-214 (the output rule and death)
//
// One thread per track.  The companion table (dz_track_ab3d) is laid out with the track index fastest, so the lanes of a wave touch
// consecutive doubles.  No thread holds a matrix in a private array under a run-time index: P stays in the table, K and
// (I - K H) P in the track's slab of `work`; what is kept in registers (the Cholesky factor of S, one row of K, one row of M) is
// indexed by unrolled loops only.  The structure of F and H is used: F P F^T is three row adds and three column adds, H P H^T the
// leading 7 x 7 block, P H^T the first seven columns.
#pragma once
#include "track_body.h"

namespace dz {

constexpr int AB_NX = 10, AB_NZ = 7;
constexpr int AB_K = 0, AB_M = AB_NX * AB_NZ;           // offsets of K (10,7) and M = (I - K H) P (10,10) in a track's work slab
static_assert(AB_M + AB_NX * AB_NX == DZ_TRACK_AB3D_WORK, "work slab");
constexpr double AB_PI = 3.141592653589793;              // np.pi
constexpr double AB_2PI = AB_PI * 2;                     // np.pi * 2
constexpr double AB_PI_2 = AB_PI / 2.0;                  // np.pi / 2.0
constexpr double AB_3PI_2 = AB_PI * 3 / 2.0;             // np.pi * 3 / 2.0

__device__ __forceinline__ double ab3d_wrap(double th) {         // ab3dmot.py:95-96
    if (th >= AB_PI) th -= AB_2PI;
    if (th < -AB_PI) th += AB_2PI;
    return th;
}

// box = x[0:9] into the float64 box and its float32 rounding (what the affinity and the merge read)
__device__ __forceinline__ void ab3d_box_from_state(const dz_track_table &t, const dz_track_ab3d &a, int i) {
    const long s = a.stride;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        const double v = a.x[q * s + i];
        a.box[q * s + i] = v;
        t.box[i * 9 + q] = (float)v;
    }
}

// ------------------------------------------------------------------------------------------
// predict: track i
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void ab3d_predict_body(const dz_track_table &t, const dz_track_ab3d &a, int i) {
    const long s = a.stride;
    double *x = a.x + i, *P = a.P + i;
    // x = F x
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k * s] = x[k * s] + x[(7 + k) * s];
    // F P: rows 0..2 += rows 7..9
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < AB_NX; ++c) P[(k * AB_NX + c) * s] = P[(k * AB_NX + c) * s] + P[((7 + k) * AB_NX + c) * s];
    // (F P) F^T: columns 0..2 += columns 7..9
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < AB_NX; ++r) P[(r * AB_NX + k) * s] = P[(r * AB_NX + k) * s] + P[(r * AB_NX + 7 + k) * s];
    // + Q = diag(1 x7, 0.01 x3)
#pragma unroll
    for (int k = 0; k < AB_NX; ++k) P[(k * AB_NX + k) * s] = P[(k * AB_NX + k) * s] + (k < 7 ? 1.0 : 0.01);
    x[6 * s] = ab3d_wrap(x[6 * s]);
    t.miss[i] += 1;
    t.hit[i] = 0;
    ab3d_box_from_state(t, a, i);
}

// ------------------------------------------------------------------------------------------
// update: track i from detection row d with the measurement z7 (7 doubles)
// ------------------------------------------------------------------------------------------
#define AB_L(r, c) L[(r) * ((r) + 1) / 2 + (c)]
__device__ __forceinline__ void ab3d_update_body(const dz_track_table &t, const dz_track_ab3d &a, int i, const int *__restrict__ d,
                                                 const double *__restrict__ z7) {
    const long s = a.stride;
    t.hit[i] = 1;
    t.miss[i] = 0;
    a.hits[i] += 1;
    t.score[i] = __int_as_float(d[ROW_SCORE]);
    t.cls[i] = d[ROW_CLS];
    double *x = a.x + i, *P = a.P + i, *W = a.work + i;

    // ---- orientation correction (ab3dmot.py:122-139) ----
    double th = ab3d_wrap(x[6 * s]);
    const double zt = ab3d_wrap(z7[6]);
    const double gap = fabs(zt - th);
    if (gap > AB_PI_2 && gap < AB_3PI_2) {
        th += AB_PI;
        if (th > AB_PI) th -= AB_2PI;
        if (th < -AB_PI) th += AB_2PI;
    }
    if (fabs(zt - th) >= AB_3PI_2) {
        if (zt > 0) th += AB_2PI;
        else th -= AB_2PI;
    }
    x[6 * s] = th;

    // ---- y = z - H x ----
    double y[AB_NZ];
#pragma unroll
    for (int c = 0; c < AB_NZ; ++c) y[c] = (c == 6 ? zt : z7[c]) - x[c * s];

    // ---- S = H P H^T + R = the leading 7 x 7 block + I, symmetric positive definite: S = L L^T (lower triangle of P read) ----
    double L[AB_NZ * (AB_NZ + 1) / 2];
#pragma unroll
    for (int r = 0; r < AB_NZ; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) AB_L(r, c) = P[(r * AB_NX + c) * s] + (r == c ? 1.0 : 0.0);
#pragma unroll
    for (int j = 0; j < AB_NZ; ++j) {
        double dj = AB_L(j, j);
#pragma unroll
        for (int k = 0; k < j; ++k) dj -= AB_L(j, k) * AB_L(j, k);
        dj = sqrt(dj);
        AB_L(j, j) = dj;
#pragma unroll
        for (int r = j + 1; r < AB_NZ; ++r) {
            double v = AB_L(r, j);
#pragma unroll
            for (int k = 0; k < j; ++k) v -= AB_L(r, k) * AB_L(j, k);
            AB_L(r, j) = v / dj;
        }
    }

    // ---- K = P H^T S^-1: row r of K solves S k = (row r of P H^T)^T; x += K y ----
    for (int r = 0; r < AB_NX; ++r) {
        double k[AB_NZ];
#pragma unroll
        for (int c = 0; c < AB_NZ; ++c) k[c] = P[(r * AB_NX + c) * s];
#pragma unroll
        for (int p = 0; p < AB_NZ; ++p) {                   // L w = p
            double v = k[p];
#pragma unroll
            for (int c = 0; c < p; ++c) v -= AB_L(p, c) * k[c];
            k[p] = v / AB_L(p, p);
        }
#pragma unroll
        for (int p = AB_NZ - 1; p >= 0; --p) {              // L^T k = w
            double v = k[p];
#pragma unroll
            for (int c = p + 1; c < AB_NZ; ++c) v -= AB_L(c, p) * k[c];
            k[p] = v / AB_L(p, p);
        }
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < AB_NZ; ++c) {
            W[(AB_K + r * AB_NZ + c) * s] = k[c];
            acc += k[c] * y[c];
        }
        x[r * s] = x[r * s] + acc;
    }

    // ---- M = (I - K H) P ----
    for (int r = 0; r < AB_NX; ++r) {
        double ik[AB_NZ];       // row r of I - K H, columns 0..6 (columns 7..9 are the identity's)
#pragma unroll
        for (int c = 0; c < AB_NZ; ++c) ik[c] = (r == c ? 1.0 : 0.0) - W[(AB_K + r * AB_NZ + c) * s];
        for (int b = 0; b < AB_NX; ++b) {
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < AB_NZ; ++c) acc += ik[c] * P[(c * AB_NX + b) * s];
            if (r >= AB_NZ) acc += P[(r * AB_NX + b) * s];
            W[(AB_M + r * AB_NX + b) * s] = acc;
        }
    }
    // ---- P = M (I - K H)^T + K R K^T, R = I ----
    for (int r = 0; r < AB_NX; ++r) {
        double m[AB_NZ], kr[AB_NZ];
#pragma unroll
        for (int c = 0; c < AB_NZ; ++c) { m[c] = W[(AB_M + r * AB_NX + c) * s]; kr[c] = W[(AB_K + r * AB_NZ + c) * s]; }
        for (int b = 0; b < AB_NX; ++b) {
            double acc = 0.0, kk = 0.0;
#pragma unroll
            for (int c = 0; c < AB_NZ; ++c) {
                const double kb = W[(AB_K + b * AB_NZ + c) * s];
                acc += m[c] * ((b == c ? 1.0 : 0.0) - kb);
                kk += kr[c] * kb;
            }
            if (b >= AB_NZ) acc += W[(AB_M + r * AB_NX + b) * s];
            P[(r * AB_NX + b) * s] = acc + kk;
        }
    }
    x[6 * s] = ab3d_wrap(x[6 * s]);
    ab3d_box_from_state(t, a, i);
}
#undef AB_L

// ------------------------------------------------------------------------------------------
// spawn: table row i from source row src with the measurement z7 (ok = the source index was inside its buffer; else an all-zero track)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void ab3d_spawn_body(const dz_track_table &t, const dz_track_ab3d &a, int i, const int *__restrict__ src,
                                                const double *__restrict__ z7, bool ok, int id) {
    const long s = a.stride;
#pragma unroll
    for (int k = 0; k < AB_NX; ++k) a.x[k * s + i] = ok && k < AB_NZ ? z7[k] : 0.0;
#pragma unroll
    for (int r = 0; r < AB_NX; ++r)
#pragma unroll
        for (int c = 0; c < AB_NX; ++c) a.P[(r * AB_NX + c) * s + i] = r == c ? (r < 7 ? 10.0 : 10000.0) : 0.0;
    // the birth row's box is the reference's float32 self.bbox: the detection rounded to float32, two zero columns
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        const float v = ok && q < 7 ? __int_as_float(src[q]) : 0.f;
        t.box[i * 9 + q] = v;
        a.box[q * s + i] = (double)v;
    }
    a.hits[i] = 1;
    t.cls[i] = ok ? src[ROW_CLS] : 0;
    const float score = ok ? __int_as_float(src[ROW_SCORE]) : 0.f;
    t.score[i] = score;
    t.update_score[i] = score;
    t.num_points[i] = -1;           // ab3dmot.py:18, never written again
    t.hit[i] = 1;
    t.miss[i] = 0;
    t.id[i] = id;
}

// ------------------------------------------------------------------------------------------
// log: info() of track i into row o / o64, with the output rule (track_manager.py:202-205) in word 15
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void ab3d_log_body(const dz_track_table &t, const dz_track_ab3d &a, int i, int frame, int frame_id, int birth_age,
                                              int death_age, int *__restrict__ o, double *__restrict__ o64) {
    track_log_body(t, i, frame, o);
    const long s = a.stride;
#pragma unroll
    for (int q = 0; q < 9; ++q) o64[q] = a.box[q * s + i];
    const int hits = a.hits[i], miss = t.miss[i];
    const bool out = (hits >= birth_age || frame_id < birth_age) && miss < death_age;
    const bool birth = hits == 1 && t.hit[i] == 1;      // never updated, not predicted since the constructor
    o[15] = (out ? 0 : DZ_TRACK_AB3D_ROW_DROP) | (birth ? DZ_TRACK_AB3D_ROW_BIRTH : 0);
}

// ------------------------------------------------------------------------------------------
// compact: survivor row i of (s, as) becomes row o of (d, ad)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void ab3d_copy_body(const dz_track_table &s, const dz_track_ab3d &as, int i, const dz_track_table &d,
                                               const dz_track_ab3d &ad, int o) {
    track_copy_body(s, i, d, o);
    const long ss = as.stride, ds = ad.stride;
#pragma unroll
    for (int k = 0; k < AB_NX; ++k) ad.x[k * ds + o] = as.x[k * ss + i];
    for (int k = 0; k < AB_NX * AB_NX; ++k) ad.P[k * ds + o] = as.P[k * ss + i];
#pragma unroll
    for (int q = 0; q < 9; ++q) ad.box[q * ds + o] = as.box[q * ss + i];
    ad.hits[o] = as.hits[i];
}

__device__ __forceinline__ dz_track_ab3d ab3d_slice(const dz_track_ab3d &a, long at) {
    dz_track_ab3d o = a;
    o.x += at; o.P += at; o.box += at; o.work += at; o.hits += at;
    return o;
}

}  // namespace dz
