// Tracking metrics (MOTA / MOTP at every score cutoff, gfx950): the weights of every (frame, shard) problem, then one workgroup per
// chain (sequence, shard, cutoff) that walks the sequence's frames in order.
//
// Reference: evaluator/waymo_eval_tracking.py:103-137 (the configuration: Hungarian matching, IoU thresholds per type, 101 score
// cutoffs, difficulty levels 1 and 2).  The metric core behind that file is not part of the reference; include/detzero_hip.h and
// DESIGN.md 7o state the protocol these kernels compute.
//
// k_mot_weights: one workgroup per problem, one thread per pair - the thresholded IoU and each prediction's highest cutoff, by the
// functions of eval_pairs.h that phase 1 of k_eval_match calls too.  The weights serve all cutoffs.
//
// k_mot_chain<WAVES>: workgroup (chain descriptor c, cutoff k), WAVES * 64 threads.
//   pass 0  every descriptor and id of the chain is range-checked before anything is followed; the same pass finds whether a
//           prediction of the chain has its highest cutoff exactly at k and the highest one below k: cutoffs between two such values
//           hold the same predictions in every frame, so only the upper one runs and it adds its counts to all of them.
//   frames  carry (the pairs of `last` that are present and still overlap), compaction of the rest, lsa_reset / lsa_augment_row over
//           the remaining rows and columns, update of `last`, counts into per-thread 64-bit registers.
//   end     one reduction, then 64-bit integer atomics (zero terms skipped) on the entries of every cutoff the chain stands for.
// `last` (both directions) and the id -> row table of the current frame live in the chain's workspace slice; the per-frame lists
// and the solver's vectors live in LDS when the chain's largest P + G is <= MOT_LDS_DIM, else in the slice too.
// Every loop is bounded by a frame count, a problem size or 101.  Plain C++ only; every store is a vector store.
#include "common.h"

#pragma clang fp contract(off)

#include "box_geom.h"
#include "eval_pairs.h"
#include "lsa_wg.h"

namespace dz {

constexpr int MOTW_THREADS = 256;
constexpr int MOT_K = EVAL_K;
constexpr int MOT_LDS_DIM = DZ_MOT_LDS_DIM;                         // P + G of a frame whose lists and solver vectors fit LDS
constexpr int MOT_LIST_INTS = 4;                                    // per unit of P + G: colmatch / remC (G), rowflag / remR (P), twice over
constexpr int MOT_WORK_BYTES = 40;                                  // per column: lsa_work_bytes(r, c) <= 40 c for r <= c
constexpr int MOT_LDS_BYTES = MOT_LDS_DIM * (MOT_WORK_BYTES + MOT_LIST_INTS * 4);
constexpr int MOT_SLOT = 2 * MOT_K * DZ_MOT_COUNTS;                 // int64 words of one shard

// bytes of one cutoff's part of a chain slice: last (gt -> pred, pred -> gt), the id -> row table, and beyond the LDS bound the
// per-frame lists and the solver's vectors
__host__ __device__ inline size_t mot_last_bytes(long long n_pid, long long n_gid) {
    return ((size_t)(n_gid + 2 * n_pid) * sizeof(int) + 15) / 16 * 16;
}
__host__ __device__ inline size_t mot_cut_slice_bytes(long long n_pid, long long n_gid, long long max_dim) {
    return mot_last_bytes(n_pid, n_gid) + (max_dim > MOT_LDS_DIM ? (size_t)max_dim * (MOT_WORK_BYTES + MOT_LIST_INTS * 4) : 0);
}

struct MotwArgs {
    const float *pred_box, *pred_score, *gt_box;
    const long long *pdesc;
    long long n_pred, n_gt, w_len;
    int box_type;
    float thr[5];
    float *weights;
    int *cut, *status;
};

__global__ __launch_bounds__(MOTW_THREADS) void k_mot_weights(MotwArgs a) {
    __shared__ double lds_s[EvalPairLds<MOTW_THREADS>::DOUBLES];        // rect_overlap's vertex and angle columns: 48 KiB
    const int tid = threadIdx.x;
    const long long *d = a.pdesc + (size_t)blockIdx.x * DZ_MOT_PDESC_WORDS;
    const long long p0 = d[0], P = d[1], g0 = d[2], G = d[3], type = d[4], w_off = d[5];
    // a descriptor that leaves its buffers is not followed (uniform: every thread reads the same words)
    const bool ok = eval_desc_ok(p0, P, g0, G, type, a.n_pred, a.n_gt) && w_off >= 0 && w_off <= a.w_len && P * G <= a.w_len - w_off;
    if (!ok) {
        if (tid == 0) atomicOr(a.status, DZ_EVAL_ST_DESC);
        return;
    }
    const int np = (int)P, ng = (int)G;
    eval_pair_weights<MOTW_THREADS>(a.pred_box + (size_t)p0 * 7, np, a.gt_box + (size_t)g0 * 7, ng, a.box_type, a.thr[type], lds_s,
                                    a.weights + w_off);
    eval_pred_cuts<MOTW_THREADS>(a.pred_score + p0, np, a.cut + p0);
}

struct MotArgs {
    const float *weights;
    const int *cut, *pred_id, *gt_id, *gt_diff;
    const long long *pdesc, *cdesc, *frames;
    long long w_len, n_pred, n_gt, n_frames, ws_bytes;
    int n_problems, n_shards, merge;
    u64 *table;
    int *status;
    char *ws;
};

// the remaining rows x (the remaining columns, then one "unmatched" column per row)
struct MotCost {
    const float *w;
    const int *rem_r, *rem_c;
    int G, cg;
    __device__ __forceinline__ double operator()(int i, int j) const {
        return j < cg ? 1.0 - (double)w[(size_t)rem_r[i] * G + rem_c[j]] : 1.0;
    }
};

// in tid order: out[..] = the x < n with flag(x), count returned (the same in every thread); ends on a sync
template <class Ctx, class Flag>
__device__ __forceinline__ int mot_compact(Ctx &cx, int n, int *out, const Flag &flag) {
    int count = 0;
    for (int x0 = 0; x0 < n; x0 += cx.n) {
        const int x = x0 + cx.tid;
        const int f = x < n && flag(x) ? 1 : 0;
        int total;
        const int at = count + cx.excl_scan(f, total);
        if (f) out[at] = x;
        count += total;
    }
    cx.sync();
    return count;
}

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_mot_chain(MotArgs a) {
    constexpr int NT = WAVES * 64;
    __shared__ double lds_s[MOT_LDS_BYTES / 8];         // the solver's vectors, then the four per-frame lists
    __shared__ double rv_s[WAVES];
    __shared__ int rk_s[WAVES];
    __shared__ u64 acc_s[9];
    __shared__ int word_s[4];                           // the solver's word, bad descriptor, a prediction at k, the highest cutoff below k
    const int tid = threadIdx.x;
    const int chain = blockIdx.x / MOT_K, k = blockIdx.x - chain * MOT_K;
    const long long *c = a.cdesc + (size_t)chain * DZ_MOT_CDESC_WORDS;
    const long long f0 = c[0], nf = c[1], shard = c[2], n_pid = c[3], n_gid = c[4], max_dim = c[5], ws_off = c[6];
    bool ok = f0 >= 0 && nf >= 0 && f0 <= a.n_frames && nf <= a.n_frames - f0 && shard >= 0 && shard < a.n_shards && n_pid >= 0 &&
              n_pid <= a.n_pred && n_gid >= 0 && n_gid <= a.n_gt && max_dim >= 0 && max_dim <= DZ_LSA_MAX_DIM && ws_off >= 0 &&
              (ws_off & 15) == 0 && ws_off <= a.ws_bytes;
    if (ok) ok = (long long)(mot_cut_slice_bytes(n_pid, n_gid, max_dim) * MOT_K) <= a.ws_bytes - ws_off;
    if (!ok) {
        if (tid == 0) atomicOr(a.status, DZ_EVAL_ST_DESC);
        return;
    }
    if (tid < 9) acc_s[tid] = 0;
    if (tid < 4) word_s[tid] = tid == 3 ? -1 : 0;
    __syncthreads();

    // pass 0: the chain's descriptors and ids, and where k stands among the cutoffs its predictions reach
    const long long *fr = a.frames + f0;
    {
        int bad = 0, at_k = 0, below = -1;
        for (int t = 0; t < (int)nf; ++t) {
            const long long pr = fr[t];
            if (pr < 0 || pr >= a.n_problems) { bad = 1; break; }                                    // (uniform)
            const long long *d = a.pdesc + (size_t)pr * DZ_MOT_PDESC_WORDS;
            const long long p0 = d[0], P = d[1], g0 = d[2], G = d[3], type = d[4], w_off = d[5];
            if (!(eval_desc_ok(p0, P, g0, G, type, a.n_pred, a.n_gt) && P + G <= max_dim && w_off >= 0 && w_off <= a.w_len &&
                  P * G <= a.w_len - w_off)) { bad = 1; break; }
            for (int r = tid; r < (int)P; r += NT) {
                const int id = a.pred_id[p0 + r], ck = a.cut[p0 + r];
                bad |= id < 0 || id >= n_pid;
                at_k |= ck == k;
                below = ck < k && ck > below ? ck : below;
            }
            for (int g = tid; g < (int)G; g += NT) { const int id = a.gt_id[g0 + g]; bad |= id < 0 || id >= n_gid; }
        }
        if (bad) atomicOr(&word_s[1], 1);
        if (at_k) atomicOr(&word_s[2], 1);
        if (below >= 0) atomicMax(&word_s[3], below);
    }
    __syncthreads();
    if (word_s[1]) {
        if (tid == 0) atomicOr(a.status, DZ_EVAL_ST_DESC);
        return;
    }
    // merged: the chain of k runs when a prediction reaches exactly k (or k is the last cutoff) and stands for every cutoff above the
    // next lower such value; unmerged (tests): every cutoff runs for itself
    if (a.merge && !word_s[2] && k != MOT_K - 1) return;
    const int k_lo = a.merge ? word_s[3] + 1 : k;

    char *slice = a.ws + ws_off + mot_cut_slice_bytes(n_pid, n_gid, max_dim) * (size_t)k;
    int *g2p = (int *)slice, *p2g = g2p + n_gid, *row_of = p2g + n_pid;
    char *big = max_dim > MOT_LDS_DIM ? slice + mot_last_bytes(n_pid, n_gid) : (char *)lds_s;
    const int md = max_dim > MOT_LDS_DIM ? (int)max_dim : MOT_LDS_DIM;
    int *colmatch = (int *)(big + (size_t)md * MOT_WORK_BYTES), *rowflag = colmatch + md, *rem_c = rowflag + md, *rem_r = rem_c + md;
    for (int i = tid; i < (int)(n_gid + 2 * n_pid); i += NT) g2p[i] = -1;
    __syncthreads();

    LsaWgCtx<WAVES> cx{tid, NT, rv_s, rk_s};
    u64 m = 0, tp1 = 0, tp2 = 0, mm1 = 0, mm2 = 0, c1 = 0, c2 = 0, n1 = 0, n2 = 0, n_in = 0;
    int solver = LSA_OK;
    for (int t = 0; t < (int)nf && solver == LSA_OK; ++t) {
        const long long *d = a.pdesc + (size_t)fr[t] * DZ_MOT_PDESC_WORDS;
        const int p0 = (int)d[0], P = (int)d[1], g0 = (int)d[2], G = (int)d[3];
        const float *w = a.weights + d[5];
        const int *cut = a.cut + p0, *pid = a.pred_id + p0, *gid = a.gt_id + g0, *gd = a.gt_diff + g0;
        // the frame's predictions of this cutoff, by id
        for (int r = tid; r < P; r += NT) {
            const bool in = cut[r] >= k;
            rowflag[r] = in ? 1 : 0;                    // 1: in the pool, 0: out of it (below the cutoff, or carried)
            if (in) { row_of[pid[r]] = r; ++n_in; }
        }
        for (int g = tid; g < G; g += NT) colmatch[g] = -1;
        __syncthreads();
        // carry: `last` is a partial bijection, so no two ground truths name the same row
        for (int g = tid; g < G; g += NT) {
            const int q = g2p[gid[g]];
            if (q < 0) continue;
            const int r = row_of[q];
            if (r >= 0 && w[(size_t)r * G + g] > 0.f) { colmatch[g] = r; rowflag[r] = 0; }
        }
        __syncthreads();
        const int nr = mot_compact(cx, P, rem_r, [&](int r) { return rowflag[r] != 0; });
        const int cg = mot_compact(cx, G, rem_c, [&](int g) { return colmatch[g] < 0; });
        if (nr > 0 && cg > 0) {
            const int C = cg + nr;
            const LsaWork work = lsa_work_at(big, nr, C);
            const MotCost cost{w, rem_r, rem_c, G, cg};
            lsa_reset(cx, nr, C, work);
            for (int cur = 0; cur < nr && solver == LSA_OK; ++cur) solver = lsa_augment_row(cx, cost, cur, C, work, &word_s[0]);
            if (solver == LSA_OK) {
                // the new pairs, judged against `last` as the frame found it; their ground truths' former partners let go
                for (int i = tid; i < nr; i += NT) {
                    const int j = work.col4row[i];
                    if (j < 0 || j >= cg) continue;
                    const int r = rem_r[i], g = rem_c[j];
                    if (!(w[(size_t)r * G + g] > 0.f)) continue;
                    colmatch[g] = r;
                    const int old = g2p[gid[g]];
                    if (old >= 0 && old != pid[r]) { mm1 += gd[g] <= 1; mm2 += gd[g] <= 2; p2g[old] = -1; }
                }
                __syncthreads();
                // their predictions' former partners let go (not a mismatch)
                for (int i = tid; i < nr; i += NT) {
                    const int j = work.col4row[i];
                    if (j < 0 || j >= cg) continue;
                    const int r = rem_r[i], g = rem_c[j];
                    if (!(w[(size_t)r * G + g] > 0.f)) continue;
                    const int og = p2g[pid[r]];
                    if (og >= 0) g2p[og] = -1;
                }
                __syncthreads();
                for (int i = tid; i < nr; i += NT) {
                    const int j = work.col4row[i];
                    if (j < 0 || j >= cg) continue;
                    const int r = rem_r[i], g = rem_c[j];
                    if (!(w[(size_t)r * G + g] > 0.f)) continue;
                    g2p[gid[g]] = pid[r];
                    p2g[pid[r]] = gid[g];
                }
            }
        }
        // counts of the frame: the kept and the new pairs
        for (int g = tid; g < G; g += NT) {
            const int df = gd[g], r = colmatch[g];
            n1 += df <= 1; n2 += df <= 2;
            if (r < 0) continue;
            const u64 cst = (u64)llrint((1.0 - (double)w[(size_t)r * G + g]) * EVAL_FIXED_ONE);
            ++m;
            if (df <= 1) { ++tp1; c1 += cst; }
            if (df <= 2) { ++tp2; c2 += cst; }
        }
        for (int r = tid; r < P; r += NT)
            if (cut[r] >= k) row_of[pid[r]] = -1;
        __syncthreads();
    }
    if (solver != LSA_OK) {                             // (the same in every thread) nothing of a failed chain is added
        if (tid == 0) atomicOr(a.status, DZ_EVAL_ST_SOLVER);
        return;
    }
    u64 v[9] = {tp1, tp2, n_in - m, n1 - tp1, n2 - tp2, mm1, mm2, c1, c2};     // (FP, MISS: per-thread parts, whole after the sum mod 2^64)
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        v[q] = eval_wave_sum(v[q]);
        if ((tid & 63) == 0 && v[q]) atomicAdd(&acc_s[q], v[q]);
    }
    __syncthreads();
    // [TP, FP, MISS, MISMATCH, COST] of level 1, then of level 2, for every cutoff this chain stands for
    u64 *out = a.table + (size_t)shard * MOT_SLOT;
    const int span = (k - k_lo + 1) * 2 * DZ_MOT_COUNTS;                        // <= 1010
    for (int idx = tid; idx < span; idx += NT) {
        const int kk = k_lo + idx / (2 * DZ_MOT_COUNTS), e = idx % (2 * DZ_MOT_COUNTS), lv = e / DZ_MOT_COUNTS, q = e - lv * DZ_MOT_COUNTS;
        const u64 val = q == 0 ? acc_s[lv] : q == 1 ? acc_s[2] : q == 2 ? acc_s[3 + lv] : q == 3 ? acc_s[5 + lv] : acc_s[7 + lv];
        if (val) atomicAdd(out + ((size_t)lv * MOT_K + kk) * DZ_MOT_COUNTS + q, val);
    }
}

}  // namespace dz

using namespace dz;

extern "C" {

size_t dz_mot_chain_ws_bytes(long long n_pred_ids, long long n_gt_ids, int max_dim) {
    if (n_pred_ids < 0 || n_gt_ids < 0 || max_dim < 0 || max_dim > DZ_LSA_MAX_DIM) return 0;
    return align_up(mot_cut_slice_bytes(n_pred_ids, n_gt_ids, max_dim) * MOT_K, 256);
}

int dz_mot_weights(const float *pred_box, const float *pred_score, long long n_pred, const float *gt_box, long long n_gt, const long long *pdesc,
                   int n_problems, int max_dim, int box_type, const float *iou_thr, float *weights, long long w_len, int *cut, int *status,
                   void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n_problems >= 0 && n_pred >= 0 && n_gt >= 0 && max_dim >= 0 && w_len >= 0, "dz_mot_weights: negative size");
    DZ_CHECK_ARG(box_type == DZ_EVAL_BOX_3D || box_type == DZ_EVAL_BOX_BEV, "dz_mot_weights: box_type %d", box_type);
    if (max_dim > DZ_LSA_MAX_DIM) {
        set_error("dz_mot_weights: a problem of %d predictions + ground truths (<= %d)", max_dim, DZ_LSA_MAX_DIM);
        return DZ_ERR_UNSUPPORTED;
    }
    if (n_pred >= (1LL << 31) / 7 || n_gt >= (1LL << 31) / 7) {
        set_error("dz_mot_weights: %lld predictions / %lld ground truths in one call", n_pred, n_gt);
        return DZ_ERR_UNSUPPORTED;
    }
    if (n_problems == 0) return DZ_OK;
    DZ_CHECK_ARG(pdesc && iou_thr && status, "dz_mot_weights: null pointer");
    DZ_CHECK_ARG(((pred_box && pred_score && cut) || n_pred == 0) && (gt_box || n_gt == 0) && (weights || w_len == 0), "dz_mot_weights: null buffer");
    MotwArgs a;
    a.pred_box = pred_box; a.pred_score = pred_score; a.gt_box = gt_box; a.pdesc = pdesc;
    a.n_pred = n_pred; a.n_gt = n_gt; a.w_len = w_len; a.box_type = box_type;
    for (int t = 0; t < 5; ++t) a.thr[t] = iou_thr[t];
    a.weights = weights; a.cut = cut; a.status = status;
    hipLaunchKernelGGL(k_mot_weights, dim3(n_problems), dim3(MOTW_THREADS), 0, stream, a);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_mot_chain_counts(const float *weights, long long w_len, const int *cut, const int *pred_id, long long n_pred, const int *gt_id,
                        const int *gt_difficulty, long long n_gt, const long long *pdesc, int n_problems, const long long *cdesc, int n_chains,
                        const long long *frames, long long n_frames, int max_dim, int n_shards, int mapping, int merge, long long *table,
                        int *status, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n_problems >= 0 && n_chains >= 0 && n_pred >= 0 && n_gt >= 0 && n_frames >= 0 && max_dim >= 0 && n_shards >= 0 && w_len >= 0,
                 "dz_mot_chain_counts: negative size");
    DZ_CHECK_ARG(mapping == DZ_MOT_MAP_WAVE || mapping == DZ_MOT_MAP_WORKGROUP, "dz_mot_chain_counts: mapping %d", mapping);
    if (max_dim > DZ_LSA_MAX_DIM) {
        set_error("dz_mot_chain_counts: a frame of %d predictions + ground truths (<= %d)", max_dim, DZ_LSA_MAX_DIM);
        return DZ_ERR_UNSUPPORTED;
    }
    if (n_pred >= (1LL << 31) || n_gt >= (1LL << 31) || n_frames >= (1LL << 31) || (long long)n_chains * MOT_K >= (1LL << 31) ||
        (long long)n_shards * MOT_SLOT >= (1LL << 31)) {       // (the kernel's frame, row and column counters are int)
        set_error("dz_mot_chain_counts: %lld predictions / %lld ground truths / %lld frames / %d chains / %d shards in one call", n_pred, n_gt,
                  n_frames, n_chains, n_shards);
        return DZ_ERR_UNSUPPORTED;
    }
    if (n_chains == 0) return DZ_OK;
    DZ_CHECK_ARG(cdesc && table && status && n_shards > 0, "dz_mot_chain_counts: null pointer");
    DZ_CHECK_ARG((pdesc || n_problems == 0) && (frames || n_frames == 0) && (weights || w_len == 0), "dz_mot_chain_counts: null descriptors");
    DZ_CHECK_ARG(((cut && pred_id) || n_pred == 0) && ((gt_id && gt_difficulty) || n_gt == 0), "dz_mot_chain_counts: null ids");
    DZ_CHECK_ARG(ws || ws_bytes == 0, "dz_mot_chain_counts: null workspace of %zu bytes", ws_bytes);
    MotArgs a;
    a.weights = weights; a.cut = cut; a.pred_id = pred_id; a.gt_id = gt_id; a.gt_diff = gt_difficulty;
    a.pdesc = pdesc; a.cdesc = cdesc; a.frames = frames;
    a.w_len = w_len; a.n_pred = n_pred; a.n_gt = n_gt; a.n_frames = n_frames; a.ws_bytes = (long long)ws_bytes;
    a.n_problems = n_problems; a.n_shards = n_shards; a.merge = merge ? 1 : 0;
    a.table = (u64 *)table; a.status = status; a.ws = (char *)ws;
    if (mapping == DZ_MOT_MAP_WAVE)
        hipLaunchKernelGGL(k_mot_chain<1>, dim3(n_chains * MOT_K), dim3(64), 0, stream, a);
    else
        hipLaunchKernelGGL(k_mot_chain<4>, dim3(n_chains * MOT_K), dim3(256), 0, stream, a);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

}  // extern "C"
