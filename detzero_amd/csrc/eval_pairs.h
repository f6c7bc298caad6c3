// What the detection and the tracking metrics define alike, stated once for eval_match.hip and mot_chain.hip:
// the 101 score cutoffs, the thresholded pair weight w = IoU >= thr ? IoU : 0 with its per-thread LDS columns, the range check of
// a problem descriptor's first words, and the wave sum of 64-bit counters.  Both files call these functions, so AP and MOTA agree
// about which predictions a cutoff holds and about every weight.  Include after `#pragma clang fp contract(off)` and box_geom.h, as
// track_body.h.  Plain C++ only.
#pragma once
#include "common.h"
#include "box_geom.h"

namespace dz {

typedef unsigned long long u64;

constexpr int EVAL_K = DZ_EVAL_CUTOFFS;
constexpr double EVAL_FIXED_ONE = 4294967296.0;         // the tables' HA and COST columns are fixed point with 32 fraction bits

// c_k = float32(k * 0.01), k = 0..99, and 1.0
__host__ __device__ inline float eval_cutoff(int k) { return k >= 100 ? 1.0f : (float)((double)k * 0.01); }

// the highest cutoff a score reaches, -1 = none (a NaN reaches none)
__host__ __device__ inline int eval_cut_index(float score) {
    int k = -1;
    for (int q = 0; q < EVAL_K; ++q) k = score >= eval_cutoff(q) ? q : k;
    return k;
}

// rect_overlap's columns of a workgroup of THREADS threads: 16 P2 + 16 float per thread = 192 bytes = 24 doubles
template <int THREADS>
struct EvalPairLds {
    static constexpr int DOUBLES = 24 * THREADS;
    __device__ static __forceinline__ P2 *cp(double *lds, int tid) { return (P2 *)lds + tid; }
    __device__ static __forceinline__ float *ang(double *lds, int tid) { return (float *)((P2 *)lds + 16 * THREADS) + tid; }
};

// w[i * ng + j] = the thresholded IoU of prediction i and ground truth j, one thread per pair; np * ng <= 2048 * 2048
template <int THREADS>
__device__ __forceinline__ void eval_pair_weights(const float *pb, int np, const float *gb, int ng, int box_type, float thr, double *lds,
                                                  float *w) {
    const int tid = threadIdx.x;
    P2 *cp = EvalPairLds<THREADS>::cp(lds, tid);
    float *ang = EvalPairLds<THREADS>::ang(lds, tid);
    const int total = np * ng;
    for (int idx = tid; idx < total; idx += THREADS) {
        const int i = idx / ng, j = idx - i * ng;
        float A[7], B[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) { A[q] = pb[(size_t)i * 7 + q]; B[q] = gb[(size_t)j * 7 + q]; }
        const float iou = box_type == DZ_EVAL_BOX_BEV ? rect_iou(A, B, cp, ang, THREADS) : pair_metric_ld<DZ_BOXM_IOU3D>(A, B, cp, ang, THREADS);
        w[idx] = iou >= thr ? iou : 0.f;                // (NaN: 0)
    }
}

// cut[i] = eval_cut_index(ps[i])
template <int THREADS>
__device__ __forceinline__ void eval_pred_cuts(const float *ps, int np, int *cut) {
    for (int i = threadIdx.x; i < np; i += THREADS) cut[i] = eval_cut_index(ps[i]);
}

// the first words of a problem descriptor stay inside the box buffers and the solver's limit, and name an object type
__device__ __forceinline__ bool eval_desc_ok(long long p0, long long P, long long g0, long long G, long long type, long long n_pred,
                                             long long n_gt) {
    return p0 >= 0 && P >= 0 && g0 >= 0 && G >= 0 && P + G <= DZ_LSA_MAX_DIM && p0 <= n_pred && P <= n_pred - p0 && g0 <= n_gt &&
           G <= n_gt - g0 && type >= 0 && type <= 4;
}

// the sum of v over the 64 lanes, in every lane
__device__ __forceinline__ u64 eval_wave_sum(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

}  // namespace dz
