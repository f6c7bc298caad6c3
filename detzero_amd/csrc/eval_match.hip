// Detection matching for AP / APH at every score cutoff (gfx950): one workgroup per (frame, shard) problem.
//
// Reference: detection/detzero_det/datasets/waymo/waymo_eval_detection.py:87-134 (the configuration: Hungarian matching, IoU
// thresholds per type, 101 score cutoffs, difficulty levels 1 and 2).  The metric core behind that file is not part of the
// reference; include/detzero_hip.h and DESIGN.md 7n state the protocol this kernel computes.
//
// Three phases per problem, P predictions (descending score) x G ground truths:
//   1. weights: one thread per pair, the thresholded IoU into the problem's workspace slice, and each prediction's highest cutoff
//      (eval_pairs.h, shared with k_mot_weights);
//   2. solve: lsa_assign_prefix over G + P columns - column j < G costs 1 - w, the P others cost 1 ("unmatched") - so rows <= columns
//      always holds; the per-column vectors reuse phase 1's LDS when G + P <= 1024, else they live in the slice;
//   3. (inside 2, after each row) at a cutoff boundary the workgroup counts the valid pairs of the current prefix and adds them to
//      every cutoff that holds exactly that many predictions.
// Every loop is bounded by the problem size or by the 101 cutoffs.  Plain C++ only; every store is a vector store.
#include "common.h"

#pragma clang fp contract(off)

#include "box_geom.h"
#include "eval_pairs.h"
#include "lsa_wg.h"

namespace dz {

constexpr int EVM_THREADS = 256;
constexpr int EVM_WAVES = EVM_THREADS / 64;
constexpr int EVM_LDS_DIM = 1024;                                   // columns whose vectors fit phase 1's LDS (40 bytes each)
constexpr int EVM_LDS_DOUBLES = EvalPairLds<EVM_THREADS>::DOUBLES;  // 48 KiB
constexpr int EVM_K = EVAL_K;
constexpr int EVM_SLOT = 2 * EVM_K * 4;                             // int64 words of one shard (or one problem's slot)
static_assert(5 * EVM_LDS_DIM <= EVM_LDS_DOUBLES, "the solver's LDS vectors reuse the pair columns");

struct EvmArgs {
    const float *pred_box, *pred_score, *gt_box;
    const int *gt_diff;
    const long long *desc;
    long long n_pred, n_gt, ws_bytes;
    int n_shards, box_type, scheme;
    float thr[5];
    u64 *table, *slots;
    int *status;
    char *ws;
};

// bytes of the three parts of a slice: weights (P, G) f32, the predictions' cutoff index (P) i32, the solver's vectors
__host__ __device__ inline size_t evm_weight_bytes(int P, int G) { return ((size_t)P * G * sizeof(float) + 15) / 16 * 16; }
__host__ __device__ inline size_t evm_cut_bytes(int P) { return ((size_t)P * sizeof(int) + 15) / 16 * 16; }
__host__ __device__ inline size_t evm_slice_bytes(int P, int G) {
    if (P <= 0) return 0;                               // nothing to solve: the slice is not touched
    return evm_weight_bytes(P, G) + evm_cut_bytes(P) + (P + G > EVM_LDS_DIM ? lsa_work_bytes(P, P + G) : 0);
}

struct EvmCost {
    const float *w;
    int G;
    __device__ __forceinline__ double operator()(int i, int j) const { return j < G ? 1.0 - (double)w[(size_t)i * G + j] : 1.0; }
};

// adds one (level, cutoff) entry; zero terms are skipped (most false-positive and true-positive terms of the high cutoffs are)
__device__ __forceinline__ void evm_add(u64 *entry, int scheme, u64 tp, u64 fp, u64 fn, u64 ha) {
    if (scheme == DZ_EVAL_ACC_ATOMIC) {
        if (tp) atomicAdd(entry + 0, tp);
        if (fp) atomicAdd(entry + 1, fp);
        if (fn) atomicAdd(entry + 2, fn);
        if (ha) atomicAdd(entry + 3, ha);
    } else {                                    // the problem's own slot: this workgroup alone writes it, a cutoff by one thread at a time
        entry[0] += tp; entry[1] += fp; entry[2] += fn; entry[3] += ha;
    }
}

struct EvmEmit {
    const float *w, *pred_box, *gt_box;       // of the problem
    const int *gt_diff, *cut;                 // cut[r]: highest cutoff the score of row r reaches, -1 = none
    int P, G, g1, g2, scheme;                 // g1 / g2: ground truths of difficulty <= 1 / <= 2
    u64 *out;                                 // (2, 101, 4) of the shard, or the problem's slot
    u64 *acc;                                 // (5) LDS: |M|, TP_1, TP_2, HA_1, HA_2

    template <class Ctx>
    __device__ void operator()(Ctx &cx, int rows_done, const int *col4row) {
        const int hi = cut[rows_done - 1];
        const int lo = rows_done < P ? cut[rows_done] : -1;       // cutoffs lo < k <= hi hold exactly rows_done predictions
        if (hi <= lo) return;                                     // (alike in every thread)
        if (cx.tid < 5) acc[cx.tid] = 0;
        cx.sync();
        u64 m = 0, tp1 = 0, tp2 = 0, ha1 = 0, ha2 = 0;
        for (int r = cx.tid; r < rows_done; r += cx.n) {
            const int g = col4row[r];
            if (g < 0 || g >= G || !(w[(size_t)r * G + g] > 0.f)) continue;
            double d = (double)pred_box[(size_t)r * 7 + 6] - (double)gt_box[(size_t)g * 7 + 6];
            d -= 6.283185307179586 * floor((d + 3.141592653589793) / 6.283185307179586);
            double acc_h = 1.0 - fabs(d) / 3.141592653589793;
            acc_h = acc_h >= 0.0 && acc_h <= 1.0 ? acc_h : 0.0;  // (a NaN heading adds nothing)
            const u64 h = (u64)llrint(acc_h * EVAL_FIXED_ONE);
            const int diff = gt_diff[g];
            ++m;
            if (diff <= 1) { ++tp1; ha1 += h; }
            if (diff <= 2) { ++tp2; ha2 += h; }
        }
        m = eval_wave_sum(m); tp1 = eval_wave_sum(tp1); tp2 = eval_wave_sum(tp2); ha1 = eval_wave_sum(ha1); ha2 = eval_wave_sum(ha2);
        if ((cx.tid & 63) == 0) {
            atomicAdd(acc + 0, m); atomicAdd(acc + 1, tp1); atomicAdd(acc + 2, tp2); atomicAdd(acc + 3, ha1); atomicAdd(acc + 4, ha2);
        }
        cx.sync();
        const u64 fp = (u64)rows_done - acc[0];
        const int k_lo = lo < -1 ? 0 : lo + 1, k_hi = hi > EVM_K - 1 ? EVM_K - 1 : hi;
        for (int k = k_lo + cx.tid; k <= k_hi; k += cx.n) {
            evm_add(out + (size_t)(0 * EVM_K + k) * 4, scheme, acc[1], fp, (u64)g1 - acc[1], acc[3]);
            evm_add(out + (size_t)(1 * EVM_K + k) * 4, scheme, acc[2], fp, (u64)g2 - acc[2], acc[4]);
        }
        cx.sync();                                                // acc is free again
    }
};

__global__ __launch_bounds__(EVM_THREADS) void k_eval_match(EvmArgs a) {
    __shared__ double lds_s[EVM_LDS_DOUBLES];           // phase 1: rect_overlap's vertex and angle columns; phase 2: the solver's vectors
    __shared__ double rv_s[EVM_WAVES];
    __shared__ int rk_s[EVM_WAVES];
    __shared__ u64 acc_s[5];
    __shared__ int word_s[3];                           // the solver's word, ground truths of level 1 / level 2
    const int tid = threadIdx.x;
    const long long *d = a.desc + (size_t)blockIdx.x * DZ_EVAL_DESC_WORDS;
    const long long p0 = d[0], P = d[1], g0 = d[2], G = d[3], shard = d[4], type = d[5], ws_off = d[6];
    // a descriptor that leaves its buffers is not followed (uniform: every thread reads the same words)
    bool ok = eval_desc_ok(p0, P, g0, G, type, a.n_pred, a.n_gt) && shard >= 0 && shard < a.n_shards && ws_off >= 0 && (ws_off & 15) == 0 &&
              ws_off <= a.ws_bytes;
    if (ok) ok = (long long)evm_slice_bytes((int)P, (int)G) <= a.ws_bytes - ws_off;
    if (!ok) {
        if (tid == 0) atomicOr(a.status, DZ_EVAL_ST_DESC);
        return;
    }
    const int np = (int)P, ng = (int)G;
    const float *pb = a.pred_box + (size_t)p0 * 7, *ps = a.pred_score + p0, *gb = a.gt_box + (size_t)g0 * 7;
    const int *gd = a.gt_diff + g0;
    char *slice = a.ws + ws_off;
    float *w = (float *)slice;
    int *cut = (int *)(slice + evm_weight_bytes(np, ng));
    u64 *out = a.scheme == DZ_EVAL_ACC_ATOMIC ? a.table + (size_t)shard * EVM_SLOT : a.slots + (size_t)blockIdx.x * EVM_SLOT;

    // phase 1
    if (tid < 3) word_s[tid] = 0;
    __syncthreads();
    {
        eval_pair_weights<EVM_THREADS>(pb, np, gb, ng, a.box_type, a.thr[type], lds_s, w);
        eval_pred_cuts<EVM_THREADS>(ps, np, cut);
        int n1 = 0, n2 = 0;
        for (int j = tid; j < ng; j += EVM_THREADS) { n1 += gd[j] <= 1; n2 += gd[j] <= 2; }
        if (n1) atomicAdd(&word_s[1], n1);
        if (n2) atomicAdd(&word_s[2], n2);
    }
    __syncthreads();                                    // the slice's weights and cut[], the LDS columns are free

    // cutoffs no prediction reaches: every ground truth is missed
    const int g1 = word_s[1], g2 = word_s[2];
    {
        int first = np > 0 ? cut[0] + 1 : 0;
        first = first < 0 ? 0 : first;
        for (int k = first + tid; k < EVM_K; k += EVM_THREADS) {
            evm_add(out + (size_t)(0 * EVM_K + k) * 4, a.scheme, 0, 0, (u64)g1, 0);
            evm_add(out + (size_t)(1 * EVM_K + k) * 4, a.scheme, 0, 0, (u64)g2, 0);
        }
    }
    if (np == 0) return;

    // phases 2 and 3
    const int C = ng + np;
    const bool in_lds = C <= EVM_LDS_DIM;
    void *base = in_lds ? (void *)lds_s : (void *)(slice + evm_weight_bytes(np, ng) + evm_cut_bytes(np));
    const LsaWork work = lsa_work_at(base, np, C);
    LsaWgCtx<EVM_WAVES> cx{tid, EVM_THREADS, rv_s, rk_s};
    const EvmCost cost{w, ng};
    EvmEmit emit{w, pb, gb, gd, cut, np, ng, g1, g2, a.scheme, out, acc_s};
    const int st = lsa_assign_prefix(cx, cost, np, C, work, &word_s[0], emit);
    if (st != LSA_OK && tid == 0) atomicOr(a.status, DZ_EVAL_ST_SOLVER);
}

// table[s][e] += the slots of the problems of shard s, in problem order (integers: the order does not show in the result)
__global__ __launch_bounds__(256) void k_eval_reduce(const long long *__restrict__ desc, int n_problems, int n_shards,
                                                     const u64 *__restrict__ slots, u64 *__restrict__ table) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_shards * EVM_SLOT) return;
    const int s = idx / EVM_SLOT, e = idx - s * EVM_SLOT;
    u64 sum = 0;
    for (int p = 0; p < n_problems; ++p)
        if (desc[(size_t)p * DZ_EVAL_DESC_WORDS + 4] == s) sum += slots[(size_t)p * EVM_SLOT + e];
    table[idx] += sum;
}

}  // namespace dz

using namespace dz;

extern "C" {

size_t dz_eval_match_ws_bytes(int n_pred, int n_gt) {
    if (n_pred <= 0 || n_gt < 0 || (long long)n_pred + n_gt > DZ_LSA_MAX_DIM) return 0;
    return align_up(evm_slice_bytes(n_pred, n_gt), 256);
}

int dz_eval_match_counts(const float *pred_box, const float *pred_score, long long n_pred, const float *gt_box, const int *gt_difficulty,
                         long long n_gt, const long long *desc, int n_problems, int max_dim, int n_shards, int box_type, const float *iou_thr,
                         int scheme, long long *table, long long *slots, int *status, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n_problems >= 0 && n_pred >= 0 && n_gt >= 0 && max_dim >= 0 && n_shards >= 0, "dz_eval_match_counts: negative size");
    DZ_CHECK_ARG(box_type == DZ_EVAL_BOX_3D || box_type == DZ_EVAL_BOX_BEV, "dz_eval_match_counts: box_type %d", box_type);
    DZ_CHECK_ARG(scheme == DZ_EVAL_ACC_ATOMIC || scheme == DZ_EVAL_ACC_SLOTS, "dz_eval_match_counts: scheme %d", scheme);
    if (max_dim > DZ_LSA_MAX_DIM) {
        set_error("dz_eval_match_counts: a problem of %d predictions + ground truths (<= %d)", max_dim, DZ_LSA_MAX_DIM);
        return DZ_ERR_UNSUPPORTED;
    }
    if (n_pred >= (1LL << 31) / 7 || n_gt >= (1LL << 31) / 7 || (long long)n_shards * EVM_SLOT >= (1LL << 31)) {
        set_error("dz_eval_match_counts: %lld predictions / %lld ground truths / %d shards in one call", n_pred, n_gt, n_shards);
        return DZ_ERR_UNSUPPORTED;
    }
    if (n_problems == 0) return DZ_OK;
    DZ_CHECK_ARG(desc && iou_thr && table && status && n_shards > 0, "dz_eval_match_counts: null pointer");
    DZ_CHECK_ARG(((pred_box && pred_score) || n_pred == 0) && ((gt_box && gt_difficulty) || n_gt == 0), "dz_eval_match_counts: null boxes");
    DZ_CHECK_ARG(ws || ws_bytes == 0, "dz_eval_match_counts: null workspace of %zu bytes", ws_bytes);
    DZ_CHECK_ARG(slots || scheme == DZ_EVAL_ACC_ATOMIC, "dz_eval_match_counts: the slot scheme needs slots");
    EvmArgs a;
    a.pred_box = pred_box; a.pred_score = pred_score; a.gt_box = gt_box; a.gt_diff = gt_difficulty; a.desc = desc;
    a.n_pred = n_pred; a.n_gt = n_gt; a.ws_bytes = (long long)ws_bytes;
    a.n_shards = n_shards; a.box_type = box_type; a.scheme = scheme;
    for (int t = 0; t < 5; ++t) a.thr[t] = iou_thr[t];
    a.table = (u64 *)table; a.slots = (u64 *)slots; a.status = status; a.ws = (char *)ws;
    if (scheme == DZ_EVAL_ACC_SLOTS)
        DZ_HIP(hipMemsetAsync(slots, 0, (size_t)n_problems * EVM_SLOT * sizeof(u64), stream));
    hipLaunchKernelGGL(k_eval_match, dim3(n_problems), dim3(EVM_THREADS), 0, stream, a);
    DZ_LAUNCH_CHECK();
    if (scheme == DZ_EVAL_ACC_SLOTS) {
        const int total = n_shards * EVM_SLOT;
        hipLaunchKernelGGL(k_eval_reduce, dim3((total + 255) / 256), dim3(256), 0, stream, desc, n_problems, n_shards, (const u64 *)slots,
                           (u64 *)table);
        DZ_LAUNCH_CHECK();
    }
    return DZ_OK;
}

}  // extern "C"
