// CenterHead targets and losses on the device (gfx950).
//
// Reference: detection/detzero_det/models/centerpoint_modules/center_head.py:107-313 (assign_target_of_single_head, _iou_target,
// get_loss), utils/loss_utils.py:143-243 (neg_loss_cornernet, _reg_loss), utils/centernet_utils.py:11-71 (gaussian_radius,
// gaussian2D, draw_gaussian_to_heatmap).  include/detzero_hip.h and DESIGN.md 7p state the contracts.
//
// Targets, two launches:
//   k_cht_clear   the heat map and the count record;
//   k_cht_assign  one workgroup per frame: the boxes of the head get their slot by a block scan in gt_boxes order, one thread per
//                 box writes its slot, then one wave per slot splats the Gaussian with integer atomicMax.
// Losses, three launches (four with the optional heat-map mask):
//   k_chl_dense   one thread per cell: the focal term of every class and, in the same pass, the cell's whole gradient row, staged in
//                 LDS so that the 48-byte rows leave as full 16-byte vectors; float64 partial sums per workgroup;
//   k_chl_slots   one workgroup per frame: L1 and IoU terms per slot, the gradient of the slots of a cell added by one thread;
//   k_chl_final   the partials in index order -> the record.
// No floating-point atomics anywhere: every float sum has a fixed order.  Plain C++ only; every store is a vector store.
#include <limits.h>

#include "common.h"

#pragma clang fp contract(off)

#include "box_geom.h"

namespace dz {

constexpr int HL_THREADS = 256;
constexpr int HL_WAVES = HL_THREADS / 64;
constexpr int HL_MAX_OBJS = DZ_HEAD_LOSS_MAX_OBJS;
constexpr int HL_MAX_CLASSES = DZ_HEAD_LOSS_MAX_CLASSES;
constexpr int HL_MAX_BLOCKS = 1024;                 // workgroups (and partial sums) of the dense pass
constexpr int HL_COMP = 9;                          // eight regression components and the IoU term
constexpr uint32_t HL_ONE_BITS = 0x3f800000u;       // 1.0f

// ------------------------------------------------------------------------------------------
// targets
// ------------------------------------------------------------------------------------------
struct ChtArgs {
    const float *gt;
    int B, M, ncls, n_classes, H, W, nmax, min_radius;
    int cls_map[HL_MAX_CLASSES + 1];                // [0] = 0 (padding rows)
    float stride, r0x, r0y, vsx, vsy;
    float om, op, om1, m2mo, a16mo;                 // (1 - o), (1 + o), (o - 1), -2 o, 16 o as the reference's float32 scalars
    float *heat, *tb;
    long long *inds, *masks;
    int *rec;
};

__global__ __launch_bounds__(HL_THREADS) void k_cht_clear(uint32_t *__restrict__ heat, long long nwords, int *__restrict__ rec) {
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += step) heat[i] = 0u;
    if (blockIdx.x == 0 && threadIdx.x < 2) rec[threadIdx.x] = 0;
}

// torch.clamp(v, 0, hi): NaN goes through
__device__ __forceinline__ float hl_clamp(float v, float hi) { return v != v ? v : fminf(fmaxf(v, 0.f), hi); }
// torch.min: NaN wins
__device__ __forceinline__ float hl_min(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fminf(a, b); }

// centernet_utils.py:11-37 with height = h, width = w: every operation rounded to float32 on its own, in the reference's order
__device__ __forceinline__ float hl_gaussian_radius(float h, float w, const ChtArgs &a) {
    const float s = __fadd_rn(h, w);
    const float c1 = __fdiv_rn(__fmul_rn(__fmul_rn(w, h), a.om), a.op);
    const float sq1 = __fsqrt_rn(__fsub_rn(__fmul_rn(s, s), __fmul_rn(4.f, c1)));
    const float r1 = __fdiv_rn(__fadd_rn(s, sq1), 2.f);
    const float b2 = __fmul_rn(2.f, s);
    const float c2 = __fmul_rn(__fmul_rn(a.om, w), h);
    const float sq2 = __fsqrt_rn(__fsub_rn(__fmul_rn(b2, b2), __fmul_rn(16.f, c2)));
    const float r2 = __fdiv_rn(__fadd_rn(b2, sq2), 2.f);
    const float b3 = __fmul_rn(a.m2mo, s);
    const float c3 = __fmul_rn(__fmul_rn(a.om1, w), h);
    const float sq3 = __fsqrt_rn(__fsub_rn(__fmul_rn(b3, b3), __fmul_rn(a.a16mo, c3)));
    const float r3 = __fdiv_rn(__fadd_rn(b3, sq3), 2.f);
    return hl_min(hl_min(r1, r2), r3);
}

__global__ __launch_bounds__(HL_THREADS) void k_cht_assign(ChtArgs a) {
    __shared__ int4 slot_s[HL_MAX_OBJS];                // x, y, radius (-1: no splat), class (0-based) of every slot of the frame
    __shared__ uint32_t scan_s[HL_WAVES];
    __shared__ int cnt_s[2];                            // new cells equal to 1, masks set
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, b = blockIdx.x;
    const float *gt = a.gt + (size_t)b * a.M * 8;
    float *tb = a.tb + (size_t)b * a.nmax * 8;
    long long *inds = a.inds + (size_t)b * a.nmax, *masks = a.masks + (size_t)b * a.nmax;
    for (int i = tid; i < a.nmax * 8; i += HL_THREADS) tb[i] = 0.f;
    for (int i = tid; i < a.nmax; i += HL_THREADS) { inds[i] = 0; masks[i] = 0; }
    if (tid < 2) cnt_s[tid] = 0;
    __syncthreads();

    int base = 0, n_ok = 0;                             // boxes of this head before the chunk (alike in every thread)
    for (int m0 = 0; m0 < a.M; m0 += HL_THREADS) {
        const int m = m0 + tid;
        int hc = 0;
        if (m < a.M) {
            const float c = gt[(size_t)m * 8 + 7];
            const int ci = (c >= 1.f && c < (float)(a.n_classes + 1)) ? (int)c : 0;
            hc = a.cls_map[ci];
        }
        uint32_t total;
        const int k = base + (int)block_excl_scan_256(hc > 0 ? 1u : 0u, scan_s, total);
        base += (int)total;
        if (hc <= 0 || k >= a.nmax) continue;
        const float *g = gt + (size_t)m * 8;
        // center_head.py:124-138
        const float cx = hl_clamp(__fdiv_rn(__fdiv_rn(__fsub_rn(g[0], a.r0x), a.vsx), a.stride), (float)a.W - 0.5f);
        const float cy = hl_clamp(__fdiv_rn(__fdiv_rn(__fsub_rn(g[1], a.r0y), a.vsy), a.stride), (float)a.H - 0.5f);
        const float sx = __fdiv_rn(__fdiv_rn(g[3], a.vsx), a.stride), sy = __fdiv_rn(__fdiv_rn(g[4], a.vsy), a.stride);
        if (sx <= 0.f || sy <= 0.f || cx != cx || cy != cy) {       // :141-145 (a NaN centre fails the reference's range test)
            slot_s[k] = make_int4(0, 0, -1, 0);
            continue;
        }
        const float rf = hl_gaussian_radius(sx, sy, a);
        const int ri = (rf == rf && fabsf(rf) < 2147483648.f) ? (int)rf : INT_MIN;       // .int() of a NaN or an overflow
        const int xi = (int)cx, yi = (int)cy;
        slot_s[k] = make_int4(xi, yi, ri > a.min_radius ? ri : a.min_radius, hc - 1);
        inds[k] = (long long)yi * a.W + xi;
        masks[k] = 1;
        ++n_ok;
        float4 lo, hi;
        lo.x = __fsub_rn(cx, (float)xi); lo.y = __fsub_rn(cy, (float)yi); lo.z = g[2]; lo.w = (float)log((double)g[3]);
        hi.x = (float)log((double)g[4]); hi.y = (float)log((double)g[5]); hi.z = (float)cos((double)g[6]); hi.w = (float)sin((double)g[6]);
        ((float4 *)tb)[k * 2] = lo;
        ((float4 *)tb)[k * 2 + 1] = hi;
    }
    __syncthreads();

    // the splat (centernet_utils.py:40-71): one wave per slot, the lanes over the clipped window
    const int n_slots = base < a.nmax ? base : a.nmax;
    int n_pos = 0;
    for (int k = wid; k < n_slots; k += HL_WAVES) {
        const int4 s = slot_s[k];
        if (s.z < 0) continue;
        const int x = s.x, y = s.y, r = s.z;
        const int left = x < r ? x : r, right = a.W - x < r + 1 ? a.W - x : r + 1;
        const int top = y < r ? y : r, bottom = a.H - y < r + 1 ? a.H - y : r + 1;
        const int fw = left + right, fh = top + bottom;                 // >= 1 each: the centre cell is inside the map
        const double sigma = (2.0 * (double)r + 1.0) / 6.0, den = 2.0 * sigma * sigma;
        uint32_t *plane = (uint32_t *)(a.heat + ((size_t)b * a.ncls + s.w) * a.H * a.W);
        for (int i = lane; i < fw * fh; i += 64) {
            const int jy = i / fw, jx = i - jy * fw;
            const double ox = (double)(jx - left), oy = (double)(jy - top);
            double v = exp(-(ox * ox + oy * oy) / den);
            if (v < 2.220446049250313e-16) v = 0.0;                     // eps * max, max = 1 at the centre
            const uint32_t bits = __float_as_uint((float)v);
            if (bits == 0u) continue;
            const uint32_t old = atomicMax(plane + (size_t)(y - top + jy) * a.W + (x - left + jx), bits);
            n_pos += (bits == HL_ONE_BITS && old != HL_ONE_BITS) ? 1 : 0;       // the one thread that makes a cell 1 counts it
        }
    }
    if (n_pos) atomicAdd(&cnt_s[0], n_pos);
    if (n_ok) atomicAdd(&cnt_s[1], n_ok);
    __syncthreads();
    if (tid < 2 && cnt_s[tid]) atomicAdd(a.rec + tid, cnt_s[tid]);     // integers: the order does not show
}

// ------------------------------------------------------------------------------------------
// losses
// ------------------------------------------------------------------------------------------
struct ChlArgs {
    const float *head, *heat, *tb, *hm_mask;
    const long long *inds, *masks;
    const int *rec;
    int B, H, W, ncls, nmax, n_blocks;
    double cls_w, loc_w, iou_w, code_w[8];
    float stride, r0x, r0y, vsx, vsy;
    double *part_dense, *part_cnt, *part_slot;          // (n_blocks, 2), (n_blocks), (B, HL_COMP)
    int *num_ws;                                        // (1): the sum of masks when the caller has no record
    double *out_rec;
    float *grad;
};

// sum over the workgroup in a fixed tree: xor shuffles inside a wave, then the waves in index order (result in thread 0)
__device__ __forceinline__ double hl_block_sum(double v, double *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();                                    // red is free again
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < HL_WAVES; ++w) s += red[w];
    return s;
}

// num_pos of the call (a.rec) or, with a mask or without a record, the call's own count
__device__ __forceinline__ double hl_num_pos(const ChlArgs &a) {
    if (a.rec && !a.hm_mask) return (double)a.rec[0];
    double np = 0.0;
    for (int i = 0; i < a.n_blocks; ++i) np += a.part_cnt[i];
    return np;
}
__device__ __forceinline__ double hl_inv_num(const ChlArgs &a) {
    const int num = a.rec ? a.rec[1] : a.num_ws[0];
    return 1.0 / (double)(num > 1 ? num : 1);
}

// the (masked) positive count of neg_loss_cornernet (loss_utils.py:153,163-169) and the sum of masks; only launched with a mask or
// without a record
__global__ __launch_bounds__(HL_THREADS) void k_chl_count(ChlArgs a) {
    __shared__ double red_s[HL_WAVES];
    __shared__ int num_s;
    const int tid = threadIdx.x, HW = a.H * a.W;
    const long long cells = (long long)a.B * HW;
    if (blockIdx.x == 0) {                              // (uniform per workgroup)
        if (tid == 0) num_s = 0;
        __syncthreads();
        int nm = 0;
        for (int i = tid; i < a.B * a.nmax; i += HL_THREADS) nm += a.masks[i] != 0 ? 1 : 0;
        if (nm) atomicAdd(&num_s, nm);
        __syncthreads();
        if (tid == 0) a.num_ws[0] = num_s;
    }
    double n = 0.0;
    for (long long cell = (long long)blockIdx.x * HL_THREADS + tid; cell < cells; cell += (long long)gridDim.x * HL_THREADS) {
        const int b = (int)(cell / HW), pix = (int)(cell - (long long)b * HW);
        const double m = a.hm_mask ? (double)a.hm_mask[cell] : 1.0;
        for (int c = 0; c < a.ncls; ++c)
            if (a.heat[((size_t)b * a.ncls + c) * HW + pix] == 1.f) n += m;
    }
    n = hl_block_sum(n, red_s);
    if (tid == 0) a.part_cnt[blockIdx.x] = n;
}

__global__ __launch_bounds__(HL_THREADS) void k_chl_dense(ChlArgs a) {
    __shared__ float4 row_s[HL_THREADS * 3];            // the tile's gradient rows
    __shared__ double red_s[HL_WAVES];
    __shared__ double scale_s;
    const int tid = threadIdx.x, HW = a.H * a.W;
    const long long cells = (long long)a.B * HW;
    if (tid == 0) {
        const double np = hl_num_pos(a);
        scale_s = a.cls_w / (np == 0.0 ? 1.0 : np);
    }
    __syncthreads();
    const double scale = scale_s;
    const double LO = (double)1e-4f, HI = (double)(float)(1.0 - 1e-4);      // center_head.py:263 on a float32 tensor
    double pos = 0.0, neg = 0.0;
    for (long long t0 = (long long)blockIdx.x * HL_THREADS; t0 < cells; t0 += (long long)gridDim.x * HL_THREADS) {
        const long long cell = t0 + tid;
        float gx[3] = {0.f, 0.f, 0.f};
        if (cell < cells) {
            const int b = (int)(cell / HW), pix = (int)(cell - (long long)b * HW);
            const double m = a.hm_mask ? (double)a.hm_mask[cell] : 1.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c >= a.ncls) continue;
                const double x = (double)a.head[cell * 12 + 9 + c];
                const float g = a.heat[((size_t)b * a.ncls + c) * HW + pix];
                const double sg = 1.0 / (1.0 + exp(-x));
                const bool clamped = sg < LO || sg > HI;
                const double p = sg < LO ? LO : (sg > HI ? HI : sg), q = 1.0 - p;
                double dp = 0.0;                        // d (term) / d p
                if (g == 1.f) {                         // loss_utils.py:153,160
                    const double lg = log(p);
                    pos += lg * q * q * m;
                    dp = q * q / p - 2.0 * q * lg;
                } else if (g < 1.f) {                   // :154-156,161
                    const double og = 1.0 - (double)g, w = (og * og) * (og * og), lg = log(q);
                    neg += lg * p * p * w * m;
                    dp = (2.0 * p * lg - p * p / q) * w;
                }
                gx[c] = clamped ? 0.f : (float)(-scale * m * dp * (p * q));
            }
        }
        if (a.grad) {
            __syncthreads();                            // the previous tile has left row_s
            row_s[tid * 3 + 0] = make_float4(0.f, 0.f, 0.f, 0.f);
            row_s[tid * 3 + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
            row_s[tid * 3 + 2] = make_float4(0.f, gx[0], gx[1], gx[2]);
            __syncthreads();
            const long long left = cells - t0;
            const int nvec = (int)(left < HL_THREADS ? left : HL_THREADS) * 3;
            float4 *dst = (float4 *)(a.grad + t0 * 12);
            for (int i = tid; i < nvec; i += HL_THREADS) dst[i] = row_s[i];
        }
    }
    pos = hl_block_sum(pos, red_s);
    neg = hl_block_sum(neg, red_s);
    if (tid == 0) { a.part_dense[blockIdx.x * 2] = pos; a.part_dense[blockIdx.x * 2 + 1] = neg; }
}

__global__ __launch_bounds__(HL_THREADS) void k_chl_slots(ChlArgs a) {
    __shared__ double lds_s[24 * HL_THREADS];           // rect_overlap's vertex and angle columns (16 P2 + 16 float per thread)
    __shared__ int ind_s[HL_MAX_OBJS];                  // the cell of a slot, -1 = masked out
    __shared__ int sgn_s[HL_MAX_OBJS];                  // 2 bits per component: 1 = +1, 2 = -1
    __shared__ double red_s[HL_WAVES];
    const int tid = threadIdx.x, b = blockIdx.x, HW = a.H * a.W;
    const float *head = a.head + (size_t)b * HW * 12, *tb = a.tb + (size_t)b * a.nmax * 8;
    for (int k = tid; k < a.nmax; k += HL_THREADS) {
        const long long ind = a.inds[(size_t)b * a.nmax + k];
        ind_s[k] = (a.masks[(size_t)b * a.nmax + k] != 0 && ind >= 0 && ind < HW) ? (int)ind : -1;
        sgn_s[k] = 0;
    }
    __syncthreads();
    P2 *cp = (P2 *)lds_s + tid;
    float *ang = (float *)((P2 *)lds_s + 16 * HL_THREADS) + tid;
    double acc[HL_COMP];
#pragma unroll
    for (int q = 0; q < HL_COMP; ++q) acc[q] = 0.0;
    for (int k = tid; k < a.nmax; k += HL_THREADS) {
        const int ind = ind_s[k];
        if (ind < 0) continue;
        float p[9], t[8];
#pragma unroll
        for (int q = 0; q < 9; ++q) p[q] = head[(size_t)ind * 12 + q];
#pragma unroll
        for (int q = 0; q < 8; ++q) t[q] = tb[(size_t)k * 8 + q];
        int sgn = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {                   // loss_utils.py:203-210 (a NaN target is masked out)
            const double d = t[q] == t[q] ? (double)p[q] - (double)t[q] : 0.0;
            acc[q] += fabs(d);
            sgn |= (d > 0.0 ? 1 : (d < 0.0 ? 2 : 0)) << (2 * q);
        }
        if (a.iou_w > 0.0) {                            // center_head.py:164-200
            const float xs = (float)(ind % a.W), ys = (float)(ind / a.W);
            float A[7], G[7];
            A[0] = (xs + p[0]) * a.stride * a.vsx + a.r0x; A[1] = (ys + p[1]) * a.stride * a.vsy + a.r0y; A[2] = p[2];
            A[3] = expf(p[3]); A[4] = expf(p[4]); A[5] = expf(p[5]); A[6] = atan2f(p[6], p[7]);
            G[0] = (xs + t[0]) * a.stride * a.vsx + a.r0x; G[1] = (ys + t[1]) * a.stride * a.vsy + a.r0y; G[2] = t[2];
            G[3] = expf(t[3]); G[4] = expf(t[4]); G[5] = expf(t[5]); G[6] = atan2f(t[6], t[7]);
            const float iou = pair_metric_ld<DZ_BOXM_IOU3D>(A, G, cp, ang, HL_THREADS);
            const double d = iou == iou ? (double)p[8] - (double)iou : 0.0;
            acc[8] += fabs(d);
            sgn |= (d > 0.0 ? 1 : (d < 0.0 ? 2 : 0)) << 16;
        }
        sgn_s[k] = sgn;
    }
#pragma unroll
    for (int q = 0; q < HL_COMP; ++q) {
        const double s = hl_block_sum(acc[q], red_s);   // (its first barrier also orders sgn_s)
        if (tid == 0) a.part_slot[(size_t)b * HL_COMP + q] = s;
    }
    if (!a.grad) return;
    // the gradient rows: the first slot of a cell gathers the cell's slots in slot order and writes columns 0..8 once
    const double inv_num = hl_inv_num(a);
    float *grad = a.grad + (size_t)b * HW * 12;
    for (int k = tid; k < a.nmax; k += HL_THREADS) {
        const int ind = ind_s[k];
        if (ind < 0) continue;
        bool first = true;
        for (int j = 0; j < k; ++j) first = first && ind_s[j] != ind;
        if (!first) continue;
        int cnt[HL_COMP];
#pragma unroll
        for (int q = 0; q < HL_COMP; ++q) cnt[q] = 0;
        for (int j = k; j < a.nmax; ++j) {
            if (ind_s[j] != ind) continue;
            const int sgn = sgn_s[j];
#pragma unroll
            for (int q = 0; q < HL_COMP; ++q) { const int v = (sgn >> (2 * q)) & 3; cnt[q] += v == 1 ? 1 : (v == 2 ? -1 : 0); }
        }
        float4 g0, g1;
        g0.x = (float)(a.loc_w * a.code_w[0] * inv_num * cnt[0]); g0.y = (float)(a.loc_w * a.code_w[1] * inv_num * cnt[1]);
        g0.z = (float)(a.loc_w * a.code_w[2] * inv_num * cnt[2]); g0.w = (float)(a.loc_w * a.code_w[3] * inv_num * cnt[3]);
        g1.x = (float)(a.loc_w * a.code_w[4] * inv_num * cnt[4]); g1.y = (float)(a.loc_w * a.code_w[5] * inv_num * cnt[5]);
        g1.z = (float)(a.loc_w * a.code_w[6] * inv_num * cnt[6]); g1.w = (float)(a.loc_w * a.code_w[7] * inv_num * cnt[7]);
        float4 *row = (float4 *)(grad + (size_t)ind * 12);
        row[0] = g0;
        row[1] = g1;
        grad[(size_t)ind * 12 + 8] = a.iou_w > 0.0 ? (float)(a.iou_w * inv_num * cnt[8]) : 0.f;
    }
}

__global__ __launch_bounds__(64) void k_chl_final(ChlArgs a) {
    __shared__ double sum_s[2 + HL_COMP];
    const int tid = threadIdx.x;
    if (tid < 2) {
        double s = 0.0;
        for (int i = 0; i < a.n_blocks; ++i) s += a.part_dense[i * 2 + tid];
        sum_s[tid] = s;
    } else if (tid < 2 + HL_COMP) {
        double s = 0.0;
        for (int b = 0; b < a.B; ++b) s += a.part_slot[(size_t)b * HL_COMP + (tid - 2)];
        sum_s[tid] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    const double np = hl_num_pos(a);
    const double hm = a.cls_w * (np == 0.0 ? -sum_s[1] : -(sum_s[0] + sum_s[1]) / np);      // loss_utils.py:174-177
    const double inv_num = hl_inv_num(a);
    double loc = 0.0;
    a.out_rec[0] = hm;
    for (int q = 0; q < 8; ++q) {
        const double c = sum_s[2 + q] * inv_num * a.code_w[q];
        a.out_rec[1 + q] = c;
        loc += c;
    }
    loc *= a.loc_w;
    const double iou = a.iou_w > 0.0 ? sum_s[2 + 8] * inv_num : 0.0;
    a.out_rec[9] = loc;
    a.out_rec[10] = iou;
    a.out_rec[11] = hm + loc + (a.iou_w > 0.0 ? a.iou_w * iou : 0.0);
}

static int hl_dense_blocks(int batch, int feat_h, int feat_w) {
    const long long tiles = ((long long)batch * feat_h * feat_w + HL_THREADS - 1) / HL_THREADS;
    return (int)(tiles < 1 ? 1 : (tiles > HL_MAX_BLOCKS ? HL_MAX_BLOCKS : tiles));
}

static bool hl_shape_ok(int batch, int feat_h, int feat_w, int ncls) {
    return batch > 0 && feat_h > 0 && feat_w > 0 && (long long)batch * ncls * feat_h * feat_w < (1LL << 31);
}

}  // namespace dz

using namespace dz;

extern "C" {

int dz_centerhead_targets(const float *gt_boxes, int batch, int max_boxes, int gt_cols, const int *cls_table, int n_classes, int ncls,
                          int feat_h, int feat_w, double stride, const double *range_xy, const double *voxel_xy, int nmax,
                          double gaussian_overlap, int min_radius, float *heatmap, float *target_boxes, long long *inds, long long *masks,
                          int *rec, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (gt_cols != 8) {
        set_error("dz_centerhead_targets: gt_boxes with %d columns (8: a `vel` head is not supported)", gt_cols);
        return DZ_ERR_UNSUPPORTED;
    }
    DZ_CHECK_ARG(cls_table && range_xy && voxel_xy && heatmap && target_boxes && inds && masks && rec, "dz_centerhead_targets: null pointer");
    DZ_CHECK_ARG(gt_boxes || max_boxes == 0, "dz_centerhead_targets: null gt_boxes");
    DZ_CHECK_ARG(max_boxes >= 0 && max_boxes < (1 << 24), "dz_centerhead_targets: %d boxes per frame", max_boxes);
    DZ_CHECK_ARG(ncls >= 1 && ncls <= 3, "dz_centerhead_targets: %d classes in the head (1..3)", ncls);
    DZ_CHECK_ARG(n_classes >= 1 && n_classes <= HL_MAX_CLASSES, "dz_centerhead_targets: %d classes (1..%d)", n_classes, HL_MAX_CLASSES);
    DZ_CHECK_ARG(nmax >= 1 && nmax <= HL_MAX_OBJS, "dz_centerhead_targets: NUM_MAX_OBJS %d (1..%d)", nmax, HL_MAX_OBJS);
    DZ_CHECK_ARG(hl_shape_ok(batch, feat_h, feat_w, ncls), "dz_centerhead_targets: map %d x %d x %d x %d", batch, ncls, feat_h, feat_w);
    DZ_CHECK_ARG(stride > 0 && voxel_xy[0] > 0 && voxel_xy[1] > 0, "dz_centerhead_targets: stride / voxel size must be positive");
    ChtArgs a;
    a.gt = gt_boxes; a.B = batch; a.M = max_boxes; a.ncls = ncls; a.n_classes = n_classes; a.H = feat_h; a.W = feat_w; a.nmax = nmax;
    a.min_radius = min_radius;
    for (int i = 0; i <= HL_MAX_CLASSES; ++i) a.cls_map[i] = 0;
    for (int i = 0; i < n_classes; ++i) {
        DZ_CHECK_ARG(cls_table[i] >= 0 && cls_table[i] <= ncls, "dz_centerhead_targets: cls_table[%d] = %d (0..%d)", i, cls_table[i], ncls);
        a.cls_map[i + 1] = cls_table[i];
    }
    a.stride = (float)stride; a.r0x = (float)range_xy[0]; a.r0y = (float)range_xy[1]; a.vsx = (float)voxel_xy[0]; a.vsy = (float)voxel_xy[1];
    const double o = gaussian_overlap;
    a.om = (float)(1.0 - o); a.op = (float)(1.0 + o); a.om1 = (float)(o - 1.0); a.m2mo = (float)(-2.0 * o); a.a16mo = (float)(4.0 * (4.0 * o));
    a.heat = heatmap; a.tb = target_boxes; a.inds = inds; a.masks = masks; a.rec = rec;
    const long long nwords = (long long)batch * ncls * feat_h * feat_w;
    hipLaunchKernelGGL(k_cht_clear, dim3(stream_grid(nwords, HL_THREADS)), dim3(HL_THREADS), 0, stream, (uint32_t *)heatmap, nwords, rec);
    DZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cht_assign, dim3(batch), dim3(HL_THREADS), 0, stream, a);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

size_t dz_centerhead_loss_ws_bytes(int batch, int feat_h, int feat_w) {
    if (!hl_shape_ok(batch, feat_h, feat_w, 1)) return 0;
    return align_up(((size_t)hl_dense_blocks(batch, feat_h, feat_w) * 3 + (size_t)batch * HL_COMP + 1) * sizeof(double), 256);
}

int dz_centerhead_loss(const float *head, const float *heatmap, const float *target_boxes, const long long *inds, const long long *masks,
                       const int *rec, const float *hm_mask, int batch, int feat_h, int feat_w, int ncls, int nmax, const double *weights,
                       double stride, const double *range_xy, const double *voxel_xy, double *out_rec, float *grad_head, void *ws,
                       size_t ws_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(head && heatmap && target_boxes && inds && masks && weights && range_xy && voxel_xy && out_rec && ws,
                 "dz_centerhead_loss: null pointer");
    DZ_CHECK_ARG(ncls >= 1 && ncls <= 3, "dz_centerhead_loss: %d classes in the head (1..3)", ncls);
    DZ_CHECK_ARG(nmax >= 1 && nmax <= HL_MAX_OBJS, "dz_centerhead_loss: NUM_MAX_OBJS %d (1..%d)", nmax, HL_MAX_OBJS);
    DZ_CHECK_ARG(hl_shape_ok(batch, feat_h, feat_w, ncls), "dz_centerhead_loss: map %d x %d x %d x %d", batch, ncls, feat_h, feat_w);
    DZ_CHECK_ARG(((uintptr_t)grad_head & 15) == 0 && ((uintptr_t)target_boxes & 15) == 0, "dz_centerhead_loss: buffers must be 16-byte aligned");
    if (ws_bytes < dz_centerhead_loss_ws_bytes(batch, feat_h, feat_w)) {
        set_error("dz_centerhead_loss: workspace of %zu bytes, %zu needed", ws_bytes, dz_centerhead_loss_ws_bytes(batch, feat_h, feat_w));
        return DZ_ERR_WORKSPACE;
    }
    ChlArgs a;
    a.head = head; a.heat = heatmap; a.tb = target_boxes; a.hm_mask = hm_mask; a.inds = inds; a.masks = masks; a.rec = rec;
    a.B = batch; a.H = feat_h; a.W = feat_w; a.ncls = ncls; a.nmax = nmax; a.n_blocks = hl_dense_blocks(batch, feat_h, feat_w);
    a.cls_w = weights[0]; a.loc_w = weights[1]; a.iou_w = weights[10];
    for (int q = 0; q < 8; ++q) a.code_w[q] = weights[2 + q];
    a.stride = (float)stride; a.r0x = (float)range_xy[0]; a.r0y = (float)range_xy[1]; a.vsx = (float)voxel_xy[0]; a.vsy = (float)voxel_xy[1];
    a.part_dense = (double *)ws; a.part_cnt = a.part_dense + (size_t)a.n_blocks * 2; a.part_slot = a.part_cnt + a.n_blocks;
    a.num_ws = (int *)(a.part_slot + (size_t)batch * HL_COMP);
    a.out_rec = out_rec; a.grad = grad_head;
    if (hm_mask || !rec) {
        hipLaunchKernelGGL(k_chl_count, dim3(a.n_blocks), dim3(HL_THREADS), 0, stream, a);
        DZ_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_chl_dense, dim3(a.n_blocks), dim3(HL_THREADS), 0, stream, a);
    DZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_chl_slots, dim3(batch), dim3(HL_THREADS), 0, stream, a);
    DZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_chl_final, dim3(1), dim3(64), 0, stream, a);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

}  // extern "C"
