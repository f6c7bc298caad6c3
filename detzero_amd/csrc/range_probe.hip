// Range probe of stored activations (gfx950): per-tensor peak, fp16-pair saturation count, non-finite count.
// The fp16-pair arithmetic (hgemm.h) is only as safe as the power-of-two pre-scale chosen for a checkpoint: MathF16::split clamps
// to +-65504 silently.  A probe is one streaming read of a tensor (or of a channel slice of its rows) that ADDS to a device record
//   slot[0] peak       max |v| over the finite elements, as the bits of a non-negative fp32 (integer max == fp32 max there);
//                      v = the element (fp32 storage) or M::join(hi, lo) (pair16 storage)
//   slot[1] saturated  fp16 pairs: elements whose hi half is +-65504 (0x7BFF) - what the clamp of split / split2 leaves behind
//   slot[2] nonfinite  elements that are inf / NaN (pairs: either half has an all-ones exponent); they do not enter the peak
//   slot[3] elements   elements looked at = rows read x c
// with device-scope atomics (max / add), so probes of several launches, frame groups and streams accumulate into one record; no
// host synchronisation, no allocation: a probe is an ordinary node of a captured graph.
//
// Work item = one group of 8 channels of one row = 32 bytes in either storage (pair16: 16 B of hi + 16 B of lo; fp32: 8 floats),
// two 16-byte loads.  Persistent grid (8 workgroups per CU), grid-stride loop whose (row, group) pair is advanced without a
// division, 64-bit byte offsets.  Reduction: registers -> wave (shuffles) -> workgroup (LDS) -> one set of atomics per workgroup.
#include "hgemm.h"

namespace dz {

constexpr int PROBE_THREADS = 256;

// STORAGE: 0 = fp32, 1 = fp16 pairs, 2 = bf16 pairs
template <int STORAGE>
__device__ __forceinline__ void probe_group(uint4 a, uint4 b, unsigned int &peak, unsigned int &sat, unsigned int &bad) {
    const unsigned int aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
    if constexpr (STORAGE == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned int u = aw[e] & 0x7FFFFFFFu, v = bw[e] & 0x7FFFFFFFu;
            const bool ub = u >= 0x7F800000u, vb = v >= 0x7F800000u;
            bad += (ub ? 1u : 0u) + (vb ? 1u : 0u);
            peak = max(peak, max(ub ? 0u : u, vb ? 0u : v));
        }
    } else {
        using M = typename std::conditional<STORAGE == 1, MathF16, MathBF16>::type;
        constexpr unsigned int EXP = STORAGE == 1 ? 0x7C00u : 0x7F80u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {                    // the two 16-bit halves of a word are two channels
                const unsigned int h = s ? (aw[e] >> 16) : (aw[e] & 0xFFFFu), l = s ? (bw[e] >> 16) : (bw[e] & 0xFFFFu);
                const bool nf = (h & EXP) == EXP || (l & EXP) == EXP;
                if constexpr (STORAGE == 1) sat += (h & 0x7FFFu) == 0x7BFFu ? 1u : 0u;
                bad += nf ? 1u : 0u;
                const unsigned int v = __float_as_uint(M::join(h, l)) & 0x7FFFFFFFu;
                peak = max(peak, nf ? 0u : v);
            }
        }
    }
}

template <int STORAGE>
__global__ __launch_bounds__(PROBE_THREADS) void k_range_probe(const unsigned char *__restrict__ x, long rows, const int *__restrict__ d_rows,
                                                                long row_bytes, long slice_off_bytes, int groups,
                                                                unsigned long long *__restrict__ slot) {
    __shared__ unsigned int red[PROBE_THREADS / 64][3];
    long n = rows;
    if (d_rows) {
        const long dn = (long)*d_rows;
        n = dn < 0 ? 0 : (dn < rows ? dn : rows);
    }
    const long total = n * groups;
    // (row, group) of this thread's first item and of the grid stride, so that the loop advances the pair without dividing
    const long step = (long)gridDim.x * PROBE_THREADS, first = (long)blockIdx.x * PROBE_THREADS + threadIdx.x;
    const long step_r = step / groups;
    const int step_g = (int)(step - step_r * groups);
    long r = first / groups;
    int g = (int)(first - r * groups);
    unsigned int peak = 0u, sat = 0u, bad = 0u;
    for (long idx = first; idx < total; idx += step) {
        const uint4 *p = reinterpret_cast<const uint4 *>(x + r * row_bytes + slice_off_bytes + (long)g * 32);
        const uint4 a = p[0], b = p[1];
        probe_group<STORAGE>(a, b, peak, sat, bad);
        r += step_r;
        g += step_g;
        if (g >= groups) { g -= groups; ++r; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        peak = max(peak, (unsigned int)__shfl_xor((int)peak, off, 64));
        sat += (unsigned int)__shfl_xor((int)sat, off, 64);
        bad += (unsigned int)__shfl_xor((int)bad, off, 64);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[wid][0] = peak; red[wid][1] = sat; red[wid][2] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0ull, b = 0ull;
        unsigned int pk = 0u;
#pragma unroll
        for (int w = 0; w < PROBE_THREADS / 64; ++w) { pk = max(pk, red[w][0]); s += red[w][1]; b += red[w][2]; }
        if (pk) atomicMax(slot + 0, (unsigned long long)pk);
        if (s) atomicAdd(slot + 1, s);
        if (b) atomicAdd(slot + 2, b);
        if (blockIdx.x == 0 && n > 0) atomicAdd(slot + 3, (unsigned long long)n * 8ull * (unsigned long long)groups);
    }
}

}  // namespace dz

using namespace dz;

extern "C" {

int dz_range_probe(const float *x, long rows, const int *d_rows, int row_stride_words, int c_off, int c, int math, unsigned long long *slot,
                   void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(rows >= 0 && row_stride_words > 0 && row_stride_words % 4 == 0, "dz_range_probe: bad sizes (rows %ld, row stride %d words)", rows,
                 row_stride_words);
    DZ_CHECK_ARG(c >= 8 && c % 8 == 0 && c_off >= 0 && c_off % 8 == 0 && (long)c_off + c <= row_stride_words,
                 "dz_range_probe: channel slice [%d, %d + %d) of %d-word rows (both multiples of 8, inside the row)", c_off, c_off, c, row_stride_words);
    DZ_CHECK_ARG(math == DZ_MATH_F32 || math == DZ_MATH_F16X2 || math == DZ_MATH_BF16X2 || math == DZ_MATH_F16, "dz_range_probe: unknown math %d", math);
    DZ_CHECK_ARG(slot, "dz_range_probe: null slot");
    if (rows == 0) return DZ_OK;
    DZ_CHECK_ARG(x && ((uintptr_t)x & 15) == 0, "dz_range_probe: null or unaligned tensor (16-byte loads)");
    const int groups = c / 8;
    long blocks = (rows * groups + PROBE_THREADS - 1) / PROBE_THREADS;
    const long cap = (long)device_cus() * 8;
    const dim3 grid((unsigned int)(blocks < cap ? blocks : cap));
    const unsigned char *xb = reinterpret_cast<const unsigned char *>(x);
    const long row_bytes = (long)row_stride_words * 4, off = (long)c_off * 4;
    if (math == DZ_MATH_F32)
        hipLaunchKernelGGL(k_range_probe<0>, grid, dim3(PROBE_THREADS), 0, stream, xb, rows, d_rows, row_bytes, off, groups, slot);
    else if (math == DZ_MATH_BF16X2)
        hipLaunchKernelGGL(k_range_probe<2>, grid, dim3(PROBE_THREADS), 0, stream, xb, rows, d_rows, row_bytes, off, groups, slot);
    else
        hipLaunchKernelGGL(k_range_probe<1>, grid, dim3(PROBE_THREADS), 0, stream, xb, rows, d_rows, row_bytes, off, groups, slot);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_range_reset(unsigned long long *table, int n_slots, void *stream_) {
    DZ_CHECK_ARG(n_slots >= 0 && (table || n_slots == 0), "dz_range_reset: bad argument");
    if (n_slots == 0) return DZ_OK;
    return fill_u32(table, 0u, (size_t)n_slots * 8, (hipStream_t)stream_);
}

}  // extern "C"
