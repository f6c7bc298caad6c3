// Linear sum assignment with GNN_assignment's masking (distance.py:9-41), written once for the host and the device.
//
// The solver is the shortest-augmenting-path algorithm of scipy.optimize.linear_sum_assignment (rectangular_lsap: Crouse 2016):
// dual variables and path lengths are double, the fp32 costs are widened to double as scipy does with a float32 matrix, the
// problem is transposed when it has more rows than columns.  Around it sits what GNN_assignment does: a cost >= threshold counts as
// 5000, and after the assignment a pair whose cost is not < threshold is dropped.
//
// The code is cooperative: `Ctx` says how many threads run it (cx.n), which one this is (cx.tid) and how they meet:
//   cx.sync()                  every thread arrives (a workgroup barrier; nothing on the host)
//   cx.argmin(value, key)      in/out: the lexicographic minimum of (value, key) over all threads, the same in every thread;
//                              it meets every thread (a sync) before it returns
//   cx.excl_scan(flag, total)  exclusive prefix of `flag` over the threads in tid order, total = the sum
// Every thread makes the same calls in the same order: all branches around them depend on values every thread holds alike.
// HostCtx below is the one-thread form; csrc/lsa.hip has the workgroup form.  This header includes nothing of HIP.
//
// The row step is a function of its own (lsa_augment_row) with two drivers: lsa_assign, GNN_assignment as described above, and
// lsa_assign_prefix, which takes the cost as a functor, never transposes and shows its caller the assignment after every row
// (csrc/eval_match.hip reads the matching of every score cutoff off one solve that way).
//
// Bounds (no loop here waits on data): at most R = min(rows, cols) augmentations, at most C = max(rows, cols) column scans per
// augmentation (a scan marks one more column), at most R steps back along a path.  A problem that would pass one of them, or that
// has no finite column left (a NaN cost), stops with a status and all of its rows unmatched.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define DZ_LSA_HD __host__ __device__
#else
#define DZ_LSA_HD
#endif

namespace dz {

constexpr int LSA_OK = 0;
constexpr int LSA_INFEASIBLE = 1;       // no finite reduced cost among the unscanned columns (NaN costs)
constexpr int LSA_BOUND = 2;            // a loop bound derived from the problem size was reached
constexpr int LSA_BAD_PROBLEM = 3;      // (batch kernel) a descriptor outside its buffers or limits
constexpr double LSA_MASKED = 5000.0;   // distance.py:22
constexpr double LSA_INF = 1.0e300;     // above every path length: R * 5000 at the most
constexpr int LSA_KEY_ASSIGNED = 1 << 30;

// The per-column and per-row vectors of one problem: C = max(rows, cols), R = min(rows, cols).
struct LsaWork {
    double *v;       // (C) column duals
    double *spc;     // (C) shortest path costs of the current augmentation
    double *u;       // (R) row duals
    int *path;       // (C) row from which a column was reached; afterwards: column -> row of the ORIGINAL problem
    int *row4col;    // (C)
    int *scanned;    // (C) == augmentation number + 1: the column is in SC
    int *col4row;    // (R)
};
DZ_LSA_HD inline size_t lsa_work_bytes(int rows, int cols) {
    const size_t c = rows > cols ? rows : cols, r = rows > cols ? cols : rows;
    return ((2 * c + r) * sizeof(double) + (3 * c + r) * sizeof(int) + 15) / 16 * 16;
}
// `base` is 8-byte aligned
DZ_LSA_HD inline LsaWork lsa_work_at(void *base, int rows, int cols) {
    const size_t c = rows > cols ? rows : cols, r = rows > cols ? cols : rows;
    LsaWork w;
    w.v = (double *)base;
    w.spc = w.v + c;
    w.u = w.spc + c;
    w.path = (int *)(w.u + r);
    w.row4col = w.path + c;
    w.scanned = w.row4col + c;
    w.col4row = w.scanned + c;
    return w;
}

struct LsaHostCtx {
    int tid = 0, n = 1;
    void sync() {}
    void argmin(double &, int &) {}
    int excl_scan(int flag, int &total) { total = flag; return 0; }
};

// Solver-space cost of (row i, column j) of the R x C problem: the original matrix, transposed when rows > cols.
DZ_LSA_HD inline double lsa_cost_at(const float *cost, int cols, bool transposed, int i, int j, double threshold) {
    const double c = (double)(transposed ? cost[(size_t)j * cols + i] : cost[(size_t)i * cols + j]);
    return c >= threshold ? LSA_MASKED : c;
}

// The same cost as a functor (row, column) -> double of the solver's R x C problem: what lsa_assign hands to lsa_augment_row.
struct LsaMatrixCost {
    const float *cost;
    int cols;
    bool transposed;
    double threshold;
    DZ_LSA_HD double operator()(int i, int j) const { return lsa_cost_at(cost, cols, transposed, i, j, threshold); }
};

// Zero duals, nothing assigned: the state before row 0 enters.  Ends on a sync.
template <class Ctx>
DZ_LSA_HD void lsa_reset(Ctx &cx, int R, int C, LsaWork w) {
    for (int j = cx.tid; j < C; j += cx.n) { w.v[j] = 0.0; w.row4col[j] = -1; w.scanned[j] = 0; }
    for (int i = cx.tid; i < R; i += cx.n) { w.u[i] = 0.0; w.col4row[i] = -1; }
    cx.sync();
}

// One augmentation: row `cur` enters an optimal assignment of rows 0..cur-1 (rows >= cur are unassigned) over C columns, and an
// optimal assignment of rows 0..cur is left in w.col4row / w.row4col.  cost_of(i, j) is the solver-space cost.  `word` is one int
// every thread can read and thread 0 writes (the path walk's verdict goes through it).  Returns the status, the same in every
// thread; the last thing every thread did is a sync.
template <class Ctx, class Cost>
DZ_LSA_HD int lsa_augment_row(Ctx &cx, const Cost &cost_of, int cur, int C, LsaWork w, int *word) {
    const int mark = cur + 1;
    for (int j = cx.tid; j < C; j += cx.n) w.spc[j] = LSA_INF;
    cx.sync();
    int i = cur, sink = -1;
    double min_val = 0.0;
    for (int step = 0; step < C; ++step) {
        const double ui = w.u[i];
        double best = LSA_INF;
        int key = 0x7FFFFFFF;
        for (int j = cx.tid; j < C; j += cx.n) {        // a thread owns its columns: spc / path are written by the owner only
            if (w.scanned[j] == mark) continue;
            const double r = min_val + cost_of(i, j) - ui - w.v[j];
            double s = w.spc[j];
            if (r < s) { w.path[j] = i; w.spc[j] = r; s = r; }
            const int k = j | (w.row4col[j] == -1 ? 0 : LSA_KEY_ASSIGNED);      // among equals: a free column first (scipy), then the lowest
            if (s < best || (s == best && k < key)) { best = s; key = k; }
        }
        cx.argmin(best, key);
        if (!(best < LSA_INF)) return LSA_INFEASIBLE;
        min_val = best;
        const int j = key & (LSA_KEY_ASSIGNED - 1);
        const int owner = w.row4col[j];                 // (written between augmentations only)
        if (cx.tid == 0) w.scanned[j] = mark;           // argmin met every thread after its scan: nobody reads scanned[] now
        cx.sync();
        if (owner == -1) { sink = j; break; }
        i = owner;
    }
    if (sink < 0) return LSA_BOUND;
    // duals: SR = {cur} and the owners of the scanned columns, SC = the scanned columns (the sink's term is zero)
    for (int j = cx.tid; j < C; j += cx.n) {
        if (w.scanned[j] != mark) continue;
        const double d = min_val - w.spc[j];
        if (j != sink) w.u[w.row4col[j]] += d;          // col4row[that row] == j: one column per row
        w.v[j] -= d;
    }
    cx.sync();
    if (cx.tid == 0) {
        w.u[cur] += min_val;
        int j = sink, done = 0;
        for (int k = 0; k <= cur; ++k) {                // the path holds at most cur + 1 rows
            const int r = w.path[j];
            w.row4col[j] = r;
            const int prev = w.col4row[r];
            w.col4row[r] = j;
            j = prev;
            if (r == cur) { done = 1; break; }
        }
        *word = done ? LSA_OK : LSA_BOUND;
    }
    cx.sync();
    const int status = *word;
    cx.sync();
    return status;
}

// Rows enter in order and the caller looks at every prefix: after row n - 1 the state is an optimal assignment of rows 0..n-1
// (the invariant of the shortest-augmenting-path method), so one solve passes through the optimum of every leading row set.
// cost_of(row, col) -> double; never transposed: the caller guarantees rows <= cols, and `w` is lsa_work_at(base, rows, cols).
// After each row on_prefix(cx, rows_done, col4row) is called from every thread, behind a sync; col4row[0..rows_done) is then
// that prefix's assignment (every row has a column).  on_prefix may sync, alike in every thread, and must not write `w`.
// Returns the status, the same in every thread; rows after a failed one are not entered.
template <class Ctx, class Cost, class OnPrefix>
DZ_LSA_HD int lsa_assign_prefix(Ctx &cx, const Cost &cost_of, int rows, int cols, LsaWork w, int *word, OnPrefix &on_prefix) {
    lsa_reset(cx, rows, cols, w);
    int status = LSA_OK;
    for (int cur = 0; cur < rows && status == LSA_OK; ++cur) {
        status = lsa_augment_row(cx, cost_of, cur, cols, w, word);
        if (status == LSA_OK) on_prefix(cx, cur + 1, (const int *)w.col4row);
    }
    return status;
}

// cost (rows, cols) fp32 row-major.  Outputs: row_to_col (rows) = matched column or -1; unmatched_rows (rows) / unmatched_cols
// (cols): ascending lists, their lengths in counts[1] / counts[2]; counts[0] = matched pairs; counts[3] = status.
// Returns the status (the same in every thread).
template <class Ctx>
DZ_LSA_HD int lsa_assign(Ctx &cx, const float *cost, int rows, int cols, double threshold, LsaWork w, int *row_to_col,
                         int *unmatched_rows, int *unmatched_cols, int *counts) {
    const bool transposed = rows > cols;
    const int R = transposed ? cols : rows, C = transposed ? rows : cols;
    int status = LSA_OK;
    const LsaMatrixCost cost_of{cost, cols, transposed, threshold};

    for (int i = cx.tid; i < rows; i += cx.n) row_to_col[i] = -1;
    lsa_reset(cx, R, C, w);

    for (int cur = 0; cur < R && status == LSA_OK; ++cur) status = lsa_augment_row(cx, cost_of, cur, C, w, counts + 3);

    // GNN_assignment's filter, in the original orientation; path becomes column -> row
    for (int j = cx.tid; j < cols; j += cx.n) w.path[j] = -1;
    cx.sync();
    if (status == LSA_OK) {
        for (int i = cx.tid; i < R; i += cx.n) {
            const int j = w.col4row[i];
            if (j < 0) continue;
            const int r = transposed ? j : i, c = transposed ? i : j;
            if ((double)cost[(size_t)r * cols + c] < threshold) { row_to_col[r] = c; w.path[c] = r; }
        }
    }
    cx.sync();
    int n_rows_free = 0, n_cols_free = 0;
    for (int i0 = 0; i0 < rows; i0 += cx.n) {
        const int i = i0 + cx.tid;
        const int flag = i < rows && row_to_col[i] < 0 ? 1 : 0;
        int total;
        const int at = n_rows_free + cx.excl_scan(flag, total);
        if (flag) unmatched_rows[at] = i;
        n_rows_free += total;
    }
    for (int j0 = 0; j0 < cols; j0 += cx.n) {
        const int j = j0 + cx.tid;
        const int flag = j < cols && w.path[j] < 0 ? 1 : 0;
        int total;
        const int at = n_cols_free + cx.excl_scan(flag, total);
        if (flag) unmatched_cols[at] = j;
        n_cols_free += total;
    }
    if (cx.tid == 0) {
        counts[0] = rows - n_rows_free;
        counts[1] = n_rows_free;
        counts[2] = n_cols_free;
        counts[3] = status;
    }
    cx.sync();
    return status;
}

}  // namespace dz
