// The workgroup form of lsa.h's context: WAVES wavefronts of 64, every thread of the workgroup calls every member.
#pragma once
#include "common.h"
#include "lsa.h"

namespace dz {

template <int WAVES>
struct LsaWgCtx {
    int tid, n;
    double *rv;     // (WAVES) LDS
    int *rk;        // (WAVES) LDS
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ void argmin(double &v, int &k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(v, off, 64);
            const int ok = __shfl_xor(k, off, 64);
            if (ov < v || (ov == v && ok < k)) { v = ov; k = ok; }
        }
        if ((tid & 63) == 0) { rv[tid >> 6] = v; rk[tid >> 6] = k; }
        __syncthreads();
        v = rv[0]; k = rk[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            const double ov = rv[w];
            const int ok = rk[w];
            if (ov < v || (ov == v && ok < k)) { v = ov; k = ok; }
        }
        __syncthreads();
    }
    __device__ __forceinline__ int excl_scan(int flag, int &total) {
        const int lane = tid & 63, wid = tid >> 6;
        int incl = flag;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        if (lane == 63) rk[wid] = incl;
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const int s = rk[w];
            if (w < wid) before += s;
            tot += s;
        }
        __syncthreads();
        total = tot;
        return before + incl - flag;
    }
};

}  // namespace dz
