// Tracking module, a pass of a sequence as one workgroup (gfx950): grid = sequences, each workgroup walks its sequence's frames in
// order and does per frame what TrackManager.online_track_module / reverse_tracking_module (track_models.py) do through the seven
// per-op entry points of track.hip - with the assignment on the device (lsa.h), so a pass needs no host decision.
//
// Reference:
//   tracking/detzero_track/models/tracking_modules/track_manager.py:145-260 (the two per-frame modules)
//   tracking/detzero_track/models/tracking_modules/data_association/data_association.py:9-155 (one_stage / two_stage / only_two_stage)
//   .../data_association/distance.py:9-41 (GNN_assignment)
//
// The per-track and per-pair arithmetic is track_body.h, the same functions the per-op kernels call; the assignment is lsa.h.
// Barriers: every __syncthreads() below is reached by all threads of the workgroup - the trip counts and branches around them
// depend on the sequence's descriptors, on `n` / counts that every thread computes alike from workgroup scans, and on words
// read after a barrier.  No loop waits on memory: frames, tracks, detections and lsa.h's bounds limit every one.
// Plain C++ only; every store is a vector store.
#include "common.h"

#pragma clang fp contract(off)

#include "track_body.h"
#include "track_ab3dmot.h"
#include "lsa_wg.h"

namespace dz {

constexpr int SEQ_THREADS = 128;
constexpr int SEQ_WAVES = SEQ_THREADS / 64;
constexpr int SEQ_LSA_LDS_DIM = 512;                        // 40 bytes per column -> 20 KiB; larger problems use the workspace slice
constexpr int SEQ_LSA_LDS_DOUBLES = 5 * SEQ_LSA_LDS_DIM;
constexpr int SEQ_MAX_WORDS = DZ_TRACK_SEQ_MAX_TRACKS / 64;
constexpr float SEQ_REVERSE_DT = -0.1f;                     // track_manager.py:258
constexpr int OVF_TRACKS = DZ_TRACK_SEQ_OVF_TRACKS, OVF_LOG = DZ_TRACK_SEQ_OVF_LOG, OVF_LSA = DZ_TRACK_SEQ_OVF_LSA,
              OVF_DESC = DZ_TRACK_SEQ_OVF_DESC;
// LDS: rect_overlap scratch 16 * 128 * (8 + 4) = 24 KiB, assignment vectors 20 KiB, sweep sets 2 * 64 * 8 = 1 KiB: 45 KiB of 64.

struct SeqClassThr { ClassThr first, second, merge; };

// One sequence's slice of the workspace.
struct SeqWs {
    float *cost;                // (row_cap, det_cap)
    unsigned long long *bits;   // (track_cap, ceil(track_cap / 64))
    void *lsa;                  // lsa_work_bytes(row_cap, det_cap)
    int *row_sel, *r2c, *rows_free;                         // (row_cap)
    int *col_sel, *cols_free, *first_free, *spawn_list;     // (det_cap)
    int *mdet, *mstage, *removed, *busy;                    // (track_cap)
    int *counts;                                            // (4)
};
static __host__ __device__ inline size_t seq_align(size_t x, size_t a) { return (x + a - 1) / a * a; }
static __host__ __device__ inline size_t seq_ws_bytes_one(int track_cap, int row_cap, int det_cap) {
    const size_t words = (size_t)(track_cap + 63) / 64;
    size_t b = seq_align((size_t)row_cap * det_cap * sizeof(float), 256);
    b += seq_align((size_t)track_cap * words * sizeof(unsigned long long), 256);
    b += seq_align(lsa_work_bytes(row_cap, det_cap), 256);
    b += seq_align(((size_t)3 * row_cap + (size_t)4 * det_cap + (size_t)4 * track_cap + 4) * sizeof(int), 256);
    return b;
}
__device__ __forceinline__ SeqWs seq_ws_at(char *base, int track_cap, int row_cap, int det_cap) {
    const size_t words = (size_t)(track_cap + 63) / 64;
    SeqWs w;
    w.cost = (float *)base;
    base += seq_align((size_t)row_cap * det_cap * sizeof(float), 256);
    w.bits = (unsigned long long *)base;
    base += seq_align((size_t)track_cap * words * sizeof(unsigned long long), 256);
    w.lsa = (void *)base;
    base += seq_align(lsa_work_bytes(row_cap, det_cap), 256);
    int *q = (int *)base;
    w.row_sel = q; q += row_cap;
    w.r2c = q; q += row_cap;
    w.rows_free = q; q += row_cap;
    w.col_sel = q; q += det_cap;
    w.cols_free = q; q += det_cap;
    w.first_free = q; q += det_cap;
    w.spawn_list = q; q += det_cap;
    w.mdet = q; q += track_cap;
    w.mstage = q; q += track_cap;
    w.removed = q; q += track_cap;
    w.busy = q; q += track_cap;
    w.counts = q;
    return w;
}
__device__ __forceinline__ dz_track_table table_slice(const dz_track_table &t, long at, int cap) {
    dz_track_table s;
    s.x = t.x + at * 5; s.P = t.P + at * 25; s.Q = t.Q + at * 25; s.dt = t.dt + at; s.box = t.box + at * 9; s.cls = t.cls + at;
    s.score = t.score + at; s.update_score = t.update_score + at; s.num_points = t.num_points + at; s.hit = t.hit + at; s.miss = t.miss + at;
    s.id = t.id + at; s.cap = cap;
    return s;
}

// The LDS of a workgroup and what every step needs.
struct SeqCtx {
    LsaWgCtx<SEQ_WAVES> cx;
    P2 *cp_s;           // (16 * SEQ_THREADS)
    float *ang_s;       // (16 * SEQ_THREADS)
    double *lsa_s;      // (SEQ_LSA_LDS_DOUBLES)
    unsigned long long *cleared, *dep, *red;
    SeqWs w;
};

// out[0..count) = the i in [0, n) with pred(i), ascending (np.flatnonzero); count is returned to every thread.
template <class Pred>
__device__ __forceinline__ int seq_flatnonzero(SeqCtx &c, int n, Pred pred, int *out) {
    int count = 0;
    for (int i0 = 0; i0 < n; i0 += SEQ_THREADS) {
        const int i = i0 + c.cx.tid;
        const int flag = i < n && pred(i) ? 1 : 0;
        int total;
        const int at = count + c.cx.excl_scan(flag, total);
        if (flag) out[at] = i;
        count += total;
    }
    __syncthreads();
    return count;
}

// one_stage + GNN_assignment on rows row_sel[0..nr) x columns col_sel[0..nc): r2c / rows_free / cols_free / counts.  -> status
template <int METRIC>
__device__ __forceinline__ int seq_associate(SeqCtx &c, const dz_track_table &t, int n, const int *ext, int n_ext, const int *det, int n_det,
                                             int nr, int nc, int distinguish, const ClassThr &thr) {
    const int total = nr * nc;
    for (int idx = c.cx.tid; idx < total; idx += SEQ_THREADS) {
        const int r = idx / nc, col = idx % nc;
        c.w.cost[idx] = track_cost_body<METRIC>(t.box, t.cls, n, ext, n_ext, c.w.row_sel[r], det, n_det, c.w.col_sel[col], distinguish, thr,
                                                c.cp_s + c.cx.tid, c.ang_s + c.cx.tid, SEQ_THREADS);
    }
    __syncthreads();
    const bool in_lds = nr <= SEQ_LSA_LDS_DIM && nc <= SEQ_LSA_LDS_DIM;
    const LsaWork work = lsa_work_at(in_lds ? (void *)c.lsa_s : c.w.lsa, nr, nc);
    return lsa_assign(c.cx, c.w.cost, nr, nc, 1.0, work, c.w.r2c, c.w.rows_free, c.w.cols_free, c.w.counts);
}

// overlap_track_merge's verdicts for rows [0, n) of table a: removed[] (dz_track_merge's two kernels as two phases)
__device__ __forceinline__ void seq_merge(SeqCtx &c, const dz_track_table &a, int n, const ClassThr &thr) {
    const int tid = c.cx.tid, lane = tid & 63, wave = tid >> 6;
    const int words = (n + 63) / 64;
    for (int i = tid; i < n; i += SEQ_THREADS) c.w.busy[i] = 0;
    __syncthreads();
    const int tiles = words * ((n + MERGE_ROWS_PER_WAVE - 1) / MERGE_ROWS_PER_WAVE);
    for (int tile = wave; tile < tiles; tile += SEQ_WAVES)          // wave code: no workgroup barrier inside
        track_merge_bits_body(a.box, a.cls, n, thr, c.w.bits, words, c.w.busy, tile % words, (tile / words) * MERGE_ROWS_PER_WAVE, lane,
                              c.cp_s + wave * 16 * 64 + lane, c.ang_s + wave * 16 * 64 + lane);
    __syncthreads();
    track_merge_sweep_body<SEQ_WAVES>(c.w.bits, words, c.w.busy, a.id, n, c.w.removed, c.cleared, c.dep, c.red);
    __syncthreads();
}

// dz_track_compact's (AB3D: dz_track_ab3d_compact's) loop on a -> b; returns the new count (the caller swaps the tables)
template <bool AB3D>
__device__ __forceinline__ int seq_compact(SeqCtx &c, const dz_track_table &a, const dz_track_table &b, const dz_track_ab3d &fa,
                                           const dz_track_ab3d &fb, int n, const int *removed, int death_age) {
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += SEQ_THREADS) {
        const int i = i0 + c.cx.tid;
        const bool keep = i < n && track_keep_body(a, i, removed, death_age);
        int total;
        const int at = base + c.cx.excl_scan(keep ? 1 : 0, total);
        if (keep) {
            if (AB3D) ab3d_copy_body(a, fa, i, b, fb, at);
            else track_copy_body(a, i, b, at);
        }
        base += total;
    }
    __syncthreads();
    return base;
}

struct SeqArgs {
    dz_track_seq_params p;
    dz_track_seq_io io;
    SeqClassThr thr;
    dz_track_table tables;
    int *log, *log_count, *overflow;
    char *ws;
    size_t ws_one;
};

// AB3D: the filter is AB3DMOT (track_ab3dmot.h) - its bodies at the five per-track call sites (predict, update, spawn, the two
// removals' copy, log); the association, the merge verdicts and every capacity check are the same code.  Forward pass only.
template <bool REVERSE, int METRIC, bool AB3D>
__device__ __forceinline__ void seq_pass(const SeqArgs &g) {
    __shared__ P2 cp_s[16 * SEQ_THREADS];
    __shared__ float ang_s[16 * SEQ_THREADS];
    __shared__ double lsa_s[SEQ_LSA_LDS_DOUBLES];
    __shared__ unsigned long long cleared_s[SEQ_MAX_WORDS], dep_s[SEQ_MAX_WORDS], red_s[SEQ_WAVES];
    __shared__ double rv_s[SEQ_WAVES];
    __shared__ int rk_s[SEQ_WAVES];

    const int s = blockIdx.x, tid = threadIdx.x;
    const dz_track_seq_params &p = g.p;
    const dz_track_seq_io &io = g.io;
    const int TC = io.track_cap, RC = io.row_cap, DC = io.det_cap;
    SeqCtx c;
    c.cx = LsaWgCtx<SEQ_WAVES>{tid, SEQ_THREADS, rv_s, rk_s};
    c.cp_s = cp_s; c.ang_s = ang_s; c.lsa_s = lsa_s; c.cleared = cleared_s; c.dep = dep_s; c.red = red_s;
    c.w = seq_ws_at(g.ws + (size_t)s * g.ws_one, TC, RC, DC);
    dz_track_table a = table_slice(g.tables, (long)s * 2 * TC, TC), b = table_slice(g.tables, (long)s * 2 * TC + TC, TC);
    int *log = g.log + (size_t)s * io.log_cap * ROW;
    dz_track_ab3d fa = {}, fb = {};
    double *log64 = nullptr;
    if constexpr (AB3D) {
        fa = ab3d_slice(io.ab3d, (long)s * 2 * TC);
        fb = ab3d_slice(io.ab3d, (long)s * 2 * TC + TC);
        log64 = io.log64 + (size_t)s * io.log_cap * 9;
    }

    int n = 0, log_n = 0, id_count = p.init_track_id, ovf = 0;
    const int f0 = io.seq_frame[s], f1 = io.seq_frame[s + 1];
    if (f0 < 0 || f1 < f0 || f1 > io.n_frames) ovf = OVF_DESC;
    const int frames = ovf ? 0 : f1 - f0;
    const int *ext = nullptr;
    int n_ext = 0;
    if (REVERSE) {
        ext = io.ext + (size_t)s * io.ext_cap * ROW;
        n_ext = min(max(io.ext_count[s], 0), io.ext_cap);
    }

    for (int k = 0; k < frames && ovf == 0; ++k) {
        const int ordinal = REVERSE ? frames - 1 - k : k;
        const int gf = f0 + ordinal;
        const int d0 = io.frame_row[gf], d1 = io.frame_row[gf + 1];
        if (d0 < 0 || d1 < d0 || d1 > io.n_det_rows || d1 - d0 > DC) { ovf = OVF_DESC; break; }
        const int D = d1 - d0;
        const int *det = io.det + (size_t)d0 * ROW;
        const int *flags = io.det_flags + d0;

        // ---- predict -----------------------------------------------------------------------------------------------
        for (int i = tid; i < n; i += SEQ_THREADS) {
            if (AB3D) ab3d_predict_body(a, fa, i);
            else track_predict_body(a, i, p.gate_class);
        }
        for (int i = tid; i < n; i += SEQ_THREADS) { c.w.mdet[i] = -1; c.w.mstage[i] = 0; }
        __syncthreads();

        // ---- association -------------------------------------------------------------------------------------------
        int n_spawn = 0;            // forward: entries of spawn_list
        int status = LSA_OK;
        if (!REVERSE) {
            if (!p.two_stage) {
                for (int i = tid; i < n; i += SEQ_THREADS) c.w.row_sel[i] = i;
                for (int j = tid; j < D; j += SEQ_THREADS) c.w.col_sel[j] = j;
                __syncthreads();
                status = seq_associate<METRIC>(c, a, n, nullptr, 0, det, D, n, D, p.distinguish_class, g.thr.first);
                if (status == LSA_OK) {
                    for (int i = tid; i < n; i += SEQ_THREADS) c.w.mdet[i] = c.w.r2c[i];
                    n_spawn = c.w.counts[2];
                    for (int j = tid; j < n_spawn; j += SEQ_THREADS) c.w.spawn_list[j] = c.w.cols_free[j];
                }
            } else if (n == 0) {
                n_spawn = seq_flatnonzero(c, D, [&](int j) { return (flags[j] & 2) != 0; }, c.w.spawn_list);
            } else {
                for (int i = tid; i < n; i += SEQ_THREADS) c.w.row_sel[i] = i;
                const int da = seq_flatnonzero(c, D, [&](int j) { return (flags[j] & 1) != 0; }, c.w.col_sel);
                status = seq_associate<METRIC>(c, a, n, nullptr, 0, det, D, n, da, p.distinguish_class, g.thr.first);
                if (status == LSA_OK) {
                    const int rows_free = c.w.counts[1], cols_free = c.w.counts[2];
                    for (int i = tid; i < n; i += SEQ_THREADS) { const int col = c.w.r2c[i]; c.w.mdet[i] = col >= 0 ? c.w.col_sel[col] : -1; }
                    for (int j = tid; j < cols_free; j += SEQ_THREADS) c.w.first_free[j] = c.w.col_sel[c.w.cols_free[j]];
                    for (int i = tid; i < rows_free; i += SEQ_THREADS) c.w.row_sel[i] = c.w.rows_free[i];      // ascending already
                    __syncthreads();
                    const int db = seq_flatnonzero(c, D, [&](int j) { return (flags[j] & 1) == 0; }, c.w.col_sel);
                    status = seq_associate<METRIC>(c, a, n, nullptr, 0, det, D, rows_free, db, p.distinguish_class, g.thr.second);
                    if (status == LSA_OK) {
                        for (int i = tid; i < rows_free; i += SEQ_THREADS) {
                            const int col = c.w.r2c[i];
                            if (col >= 0) { c.w.mdet[c.w.row_sel[i]] = c.w.col_sel[col]; c.w.mstage[c.w.row_sel[i]] = 1; }
                        }
                        // the second stage's unmatched detections never spawn (data_association.py:121-123)
                        int count = 0;
                        for (int j0 = 0; j0 < cols_free; j0 += SEQ_THREADS) {
                            const int j = j0 + tid;
                            const int dj = j < cols_free ? c.w.first_free[j] : 0;
                            const int flag = j < cols_free && (flags[dj] & 2) != 0 ? 1 : 0;
                            int total;
                            const int at = count + c.cx.excl_scan(flag, total);
                            if (flag) c.w.spawn_list[at] = dj;
                            count += total;
                        }
                        n_spawn = count;
                    }
                }
            }
        } else {
            const int g0 = io.going_at[gf], g1 = io.going_at[gf + 1];
            if (g0 < 0 || g1 < g0 || g1 > io.n_going || n + (g1 - g0) > RC) { ovf = OVF_DESC; break; }
            const int nr = n + (g1 - g0);
            if (nr > 0) {
                for (int i = tid; i < n; i += SEQ_THREADS) c.w.row_sel[i] = i;
                for (int i = tid; i < g1 - g0; i += SEQ_THREADS) c.w.row_sel[n + i] = -io.going_idx[g0 + i] - 1;
                const int db = seq_flatnonzero(c, D, [&](int j) { return (flags[j] & 1) == 0; }, c.w.col_sel);
                status = seq_associate<METRIC>(c, a, n, ext, n_ext, det, D, nr, db, p.distinguish_class, g.thr.second);
                if (status == LSA_OK)
                    for (int i = tid; i < n; i += SEQ_THREADS) {
                        const int col = c.w.r2c[i];
                        c.w.mdet[i] = col >= 0 ? c.w.col_sel[col] : -1;
                        c.w.mstage[i] = 1;
                    }
            }
        }
        if (status != LSA_OK) { ovf = OVF_LSA; break; }
        __syncthreads();

        // ---- update, forward spawn ---------------------------------------------------------------------------------
        for (int i = tid; i < n; i += SEQ_THREADS) {
            const int di = c.w.mdet[i];
            if (di >= 0 && di < D) {
                if (AB3D) ab3d_update_body(a, fa, i, det + di * ROW, io.det64 + ((size_t)d0 + di) * AB_NZ);
                else track_update_body(a, i, det + di * ROW, c.w.mstage[i], p.r);
            }
        }
        if (!REVERSE) {
            if (n + n_spawn > TC) { ovf = OVF_TRACKS; break; }
            for (int j = tid; j < n_spawn; j += SEQ_THREADS) {
                const int si = c.w.spawn_list[j];
                const bool ok = si >= 0 && si < D;
                if (AB3D) ab3d_spawn_body(a, fa, n + j, det + (ok ? si : 0) * ROW, io.det64 + ((size_t)d0 + (ok ? si : 0)) * AB_NZ, ok, id_count + j);
                else track_spawn_body(a, n + j, det + (ok ? si : 0) * ROW, ok, id_count + j, p.p0, p.p1, p.q0, p.q1, p.dt);
            }
            n += n_spawn;
            id_count += n_spawn;
        }
        __syncthreads();

        // ---- merge, log --------------------------------------------------------------------------------------------
        if (p.merge_enable && n > 0) {
            seq_merge(c, a, n, g.thr.merge);
            n = seq_compact<AB3D>(c, a, b, fa, fb, n, c.w.removed, -1);
            const dz_track_table t = a; a = b; b = t;
            if constexpr (AB3D) { const dz_track_ab3d ft = fa; fa = fb; fb = ft; }
        }
        if (log_n + n > io.log_cap) { ovf = OVF_LOG; break; }
        for (int i = tid; i < n; i += SEQ_THREADS) {
            if (AB3D) ab3d_log_body(a, fa, i, ordinal, io.frame_id[gf], p.birth_age, p.death_age, log + (size_t)(log_n + i) * ROW,
                                    log64 + (size_t)(log_n + i) * 9);
            else track_log_body(a, i, ordinal, log + (size_t)(log_n + i) * ROW);
        }
        log_n += n;

        if (!REVERSE) {
            if (p.death_age != -1 && n > 0) {
                __syncthreads();
                n = seq_compact<AB3D>(c, a, b, fa, fb, n, nullptr, p.death_age);
                const dz_track_table t = a; a = b; b = t;
                if constexpr (AB3D) { const dz_track_ab3d ft = fa; fa = fb; fb = ft; }
            }
        } else {
            // the forward tracks that start at this frame become reverse tracks (track_manager.py:247-260)
            const int s0 = io.start_at[gf], s1 = io.start_at[gf + 1];
            if (s0 < 0 || s1 < s0 || s1 > io.n_start) { ovf = OVF_DESC; break; }
            const int m = s1 - s0;
            if (n + m > TC) { ovf = OVF_TRACKS; break; }
            for (int j = tid; j < m; j += SEQ_THREADS) {
                const int si = io.start_idx[s0 + j];
                const bool ok = si >= 0 && si < n_ext;
                const int *src = ext + (size_t)(ok ? si : 0) * ROW;
                track_spawn_body(a, n + j, src, ok, ok ? src[ROW_ID] : -1, p.p0, p.p1, p.q0, p.q1, SEQ_REVERSE_DT);
            }
            n += m;
        }
        __syncthreads();
    }
    if (tid == 0) { g.log_count[s] = log_n; g.overflow[s] = ovf; }
}

template <int METRIC>
__global__ __launch_bounds__(SEQ_THREADS) void k_track_seq_forward(SeqArgs g) { seq_pass<false, METRIC, false>(g); }
template <int METRIC>
__global__ __launch_bounds__(SEQ_THREADS) void k_track_seq_reverse(SeqArgs g) { seq_pass<true, METRIC, false>(g); }
template <int METRIC>
__global__ __launch_bounds__(SEQ_THREADS) void k_track_seq_forward_ab3d(SeqArgs g) { seq_pass<false, METRIC, true>(g); }

}  // namespace dz

using namespace dz;

extern "C" {

size_t dz_track_seq_ws_bytes(int n_seq, int track_cap, int row_cap, int det_cap) {
    if (n_seq <= 0 || track_cap <= 0 || row_cap <= 0 || det_cap <= 0) return 256;
    return (size_t)n_seq * seq_ws_bytes_one(track_cap, row_cap, det_cap);
}

int dz_track_seq_pass(const dz_track_seq_params *p, const dz_track_seq_io *io, int reverse, const dz_track_table *tables, int *log,
                      int *log_count, int *overflow, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(p && io, "dz_track_seq_pass: null parameters");
    DZ_CHECK_ARG(io->n_seq >= 0 && io->n_frames >= 0 && io->n_det_rows >= 0 && io->log_cap >= 0, "dz_track_seq_pass: negative size");
    if (p->n_cls < 1 || p->n_cls > DZ_TRACK_MAX_CLASSES) {
        set_error("dz_track_seq_pass: %d classes (1..%d)", p->n_cls, DZ_TRACK_MAX_CLASSES);
        return DZ_ERR_UNSUPPORTED;
    }
    if (p->metric != DZ_TRACK_AFF_IOU_BEV && p->metric != DZ_BOXM_IOU3D && p->metric != DZ_BOXM_GIOU3D) {
        set_error("dz_track_seq_pass: unknown metric %d", p->metric);
        return DZ_ERR_UNSUPPORTED;
    }
    if (io->track_cap < 1 || io->track_cap > DZ_TRACK_SEQ_MAX_TRACKS || io->det_cap < 1 || io->det_cap > DZ_TRACK_SEQ_MAX_DET ||
        io->row_cap < io->track_cap || io->row_cap > 2 * DZ_TRACK_SEQ_MAX_TRACKS) {
        set_error("dz_track_seq_pass: capacities %d tracks (1..%d), %d detections per frame (1..%d), %d assignment rows (tracks..%d)",
                  io->track_cap, DZ_TRACK_SEQ_MAX_TRACKS, io->det_cap, DZ_TRACK_SEQ_MAX_DET, io->row_cap, 2 * DZ_TRACK_SEQ_MAX_TRACKS);
        return DZ_ERR_UNSUPPORTED;
    }
    if ((long)io->n_seq * 2 * io->track_cap * 25 >= (1L << 31) || (long)io->n_det_rows * ROW >= (1L << 31) ||
        (long)io->n_seq * io->log_cap * ROW >= (1L << 40) || (long)io->log_cap * ROW >= (1L << 31) ||
        (reverse && (long)io->ext_cap * ROW >= (1L << 31))) {
        set_error("dz_track_seq_pass: %d sequences x %d tracks / %d detection rows / %d log rows overflow 32-bit offsets", io->n_seq,
                  io->track_cap, io->n_det_rows, io->log_cap);
        return DZ_ERR_UNSUPPORTED;
    }
    if (p->merge_enable)
        for (int k = 0; k < p->n_cls; ++k)
            if (!(p->thr_merge[k] > 0.f)) {
                set_error("dz_track_seq_pass: merge threshold %d is %g; the sweep needs thresholds > 0", k, (double)p->thr_merge[k]);
                return DZ_ERR_UNSUPPORTED;
            }
    const bool ab3d = p->filter == DZ_TRACK_FILTER_AB3DMOT;
    if ((p->filter != DZ_TRACK_FILTER_KALMAN && !ab3d) || (ab3d && reverse)) {
        set_error("dz_track_seq_pass: filter %d%s (0 = KalmanFilter, 1 = AB3DMOT on the forward pass)", p->filter, reverse ? ", reverse pass" : "");
        return DZ_ERR_UNSUPPORTED;
    }
    if (io->n_seq == 0) return DZ_OK;
    DZ_CHECK_ARG(io->frame_row && io->seq_frame && log_count && overflow && ws && (log || io->log_cap == 0) &&
                     (io->n_det_rows == 0 || (io->det && io->det_flags)),
                 "dz_track_seq_pass: null pointer");
    DZ_CHECK_ARG(tables && tables->cap >= (long)io->n_seq * 2 * io->track_cap && tables->x && tables->P && tables->Q && tables->dt && tables->box &&
                     tables->cls && tables->score && tables->update_score && tables->num_points && tables->hit && tables->miss && tables->id,
                 "dz_track_seq_pass: the table needs 2 x track_cap rows per sequence");
    if (ab3d)
        DZ_CHECK_ARG(io->frame_id && (io->log64 || io->log_cap == 0) && (io->n_det_rows == 0 || io->det64) && io->ab3d.x && io->ab3d.P &&
                         io->ab3d.box && io->ab3d.work && io->ab3d.hits && io->ab3d.stride >= (long)io->n_seq * 2 * io->track_cap,
                     "dz_track_seq_pass: AB3DMOT needs det64, frame_id, log64 and a companion of 2 x track_cap rows per sequence");
    if (reverse)
        DZ_CHECK_ARG(io->ext_cap >= 0 && io->n_going >= 0 && io->n_start >= 0 && io->ext_count && io->going_at && io->start_at &&
                         (io->ext || io->ext_cap == 0) && (io->going_idx || io->n_going == 0) && (io->start_idx || io->n_start == 0),
                     "dz_track_seq_pass: null pointer or negative size among the reverse pass's lists");
    if (ws_bytes < dz_track_seq_ws_bytes(io->n_seq, io->track_cap, io->row_cap, io->det_cap)) {
        set_error("dz_track_seq_pass: workspace too small");
        return DZ_ERR_WORKSPACE;
    }
    SeqArgs g;
    g.p = *p;
    g.io = *io;
    for (int k = 0; k < DZ_TRACK_MAX_CLASSES; ++k) {
        g.thr.first.v[k] = p->thr_first[k < p->n_cls ? k : 0];
        g.thr.second.v[k] = p->thr_second[k < p->n_cls ? k : 0];
        g.thr.merge.v[k] = p->thr_merge[k < p->n_cls ? k : 0];
    }
    g.tables = *tables;
    g.log = log; g.log_count = log_count; g.overflow = overflow;
    g.ws = (char *)ws;
    g.ws_one = seq_ws_bytes_one(io->track_cap, io->row_cap, io->det_cap);
    const dim3 grid(io->n_seq), block(SEQ_THREADS);
#define DZ_SEQ_LAUNCH(M)                                                                                   \
    do {                                                                                                   \
        if (ab3d) hipLaunchKernelGGL(k_track_seq_forward_ab3d<M>, grid, block, 0, stream, g);              \
        else if (reverse) hipLaunchKernelGGL(k_track_seq_reverse<M>, grid, block, 0, stream, g);           \
        else hipLaunchKernelGGL(k_track_seq_forward<M>, grid, block, 0, stream, g);                        \
    } while (0)
    switch (p->metric) {
        case DZ_TRACK_AFF_IOU_BEV: DZ_SEQ_LAUNCH(DZ_TRACK_AFF_IOU_BEV); break;
        case DZ_BOXM_IOU3D: DZ_SEQ_LAUNCH(DZ_BOXM_IOU3D); break;
        default: DZ_SEQ_LAUNCH(DZ_BOXM_GIOU3D);
    }
#undef DZ_SEQ_LAUNCH
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

}  // extern "C"
