// Batched linear sum assignment (gfx950): one workgroup per problem runs the cooperative core of lsa.h.
//
// Reference: tracking/detzero_track/models/tracking_modules/data_association/distance.py:9-41 (GNN_assignment) around
// scipy.optimize.linear_sum_assignment.  Costs stay in global memory (a step reads one row, or one column of a transposed problem);
// the per-column vectors of a problem with max(rows, cols) <= LSA_LDS_DIM live in LDS, larger ones in the problem's slice of the
// caller's workspace.  Every loop of the core is bounded by the problem size (lsa.h); the kernel has no loop of its own.
// Plain C++ only; every store is a vector store.
#include "common.h"
#include "lsa_wg.h"

namespace dz {

constexpr int LSA_THREADS = 256;
constexpr int LSA_WAVES = LSA_THREADS / 64;
constexpr int LSA_LDS_DIM = 1024;                                   // 40 bytes per column: 40 KiB of the 64 KiB a kernel gets by default
constexpr int LSA_LDS_DOUBLES = 5 * LSA_LDS_DIM;                    // == lsa_work_bytes(LSA_LDS_DIM, LSA_LDS_DIM) / 8
constexpr int LSA_DESC_WORDS = DZ_LSA_DESC_WORDS;

struct LsaBuffers {
    long long cost_len, rows_len, cols_len, ws_bytes;       // elements of cost, of row_to_col / unmatched_rows, of unmatched_cols; bytes of ws
};

__global__ __launch_bounds__(LSA_THREADS) void k_lsa_batch(const float *__restrict__ cost, const long long *__restrict__ desc, double threshold,
                                                           LsaBuffers len, int *__restrict__ row_to_col, int *__restrict__ unmatched_rows,
                                                           int *__restrict__ unmatched_cols, int *__restrict__ counts, char *__restrict__ ws) {
    __shared__ double work_s[LSA_LDS_DOUBLES];
    __shared__ double rv_s[LSA_WAVES];
    __shared__ int rk_s[LSA_WAVES];
    const long long *d = desc + (size_t)blockIdx.x * LSA_DESC_WORDS;
    const long long rows = d[0], cols = d[1], cost_off = d[2], row_off = d[3], col_off = d[4], ws_off = d[5];
    int *cnt = counts + (size_t)blockIdx.x * 4;
    // a descriptor that leaves its buffers is not followed (uniform: every thread reads the same words)
    bool ok = rows >= 0 && cols >= 0 && rows <= DZ_LSA_MAX_DIM && cols <= DZ_LSA_MAX_DIM && cost_off >= 0 && row_off >= 0 && col_off >= 0 &&
              cost_off + rows * cols <= len.cost_len && row_off + rows <= len.rows_len && col_off + cols <= len.cols_len;
    const bool in_lds = rows <= LSA_LDS_DIM && cols <= LSA_LDS_DIM;
    if (ok && !in_lds)
        ok = ws_off >= 0 && (ws_off & 15) == 0 && ws_off + (long long)lsa_work_bytes((int)rows, (int)cols) <= len.ws_bytes;
    if (!ok) {
        if (threadIdx.x == 0) { cnt[0] = 0; cnt[1] = 0; cnt[2] = 0; cnt[3] = LSA_BAD_PROBLEM; }
        return;
    }
    LsaWgCtx<LSA_WAVES> cx{(int)threadIdx.x, LSA_THREADS, rv_s, rk_s};
    const LsaWork w = lsa_work_at(in_lds ? (void *)work_s : (void *)(ws + ws_off), (int)rows, (int)cols);
    lsa_assign(cx, cost + cost_off, (int)rows, (int)cols, threshold, w, row_to_col + row_off, unmatched_rows + row_off, unmatched_cols + col_off,
               cnt);
}

}  // namespace dz

using namespace dz;

extern "C" {

size_t dz_lsa_ws_bytes(int rows, int cols) {
    if (rows <= 0 || cols <= 0 || (rows <= LSA_LDS_DIM && cols <= LSA_LDS_DIM)) return 0;
    return align_up(lsa_work_bytes(rows, cols), 256);
}

int dz_lsa_batch(const float *cost, long long cost_len, const long long *desc, int n_problems, int max_rows, int max_cols, double threshold,
                 int *row_to_col, int *unmatched_rows, long long rows_len, int *unmatched_cols, long long cols_len, int *counts, void *ws,
                 size_t ws_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n_problems >= 0 && max_rows >= 0 && max_cols >= 0 && cost_len >= 0 && rows_len >= 0 && cols_len >= 0, "dz_lsa_batch: negative size");
    if (max_rows > DZ_LSA_MAX_DIM || max_cols > DZ_LSA_MAX_DIM) {
        set_error("dz_lsa_batch: %d x %d problems (each side <= %d)", max_rows, max_cols, DZ_LSA_MAX_DIM);
        return DZ_ERR_UNSUPPORTED;
    }
    if (cost_len >= (1LL << 40) || rows_len >= (1LL << 31) || cols_len >= (1LL << 31)) {
        set_error("dz_lsa_batch: %lld costs / %lld rows / %lld columns in one call", cost_len, rows_len, cols_len);
        return DZ_ERR_UNSUPPORTED;
    }
    if (n_problems == 0) return DZ_OK;
    DZ_CHECK_ARG(desc && counts && (cost || cost_len == 0) && ((row_to_col && unmatched_rows) || rows_len == 0) && (unmatched_cols || cols_len == 0),
                 "dz_lsa_batch: null pointer");
    DZ_CHECK_ARG(ws || ws_bytes == 0, "dz_lsa_batch: null workspace of %zu bytes", ws_bytes);
    // the workspace is checked per problem, by the kernel: the descriptors (and with them each slice's offset and size) are on the device
    const LsaBuffers len{cost_len, rows_len, cols_len, (long long)ws_bytes};
    hipLaunchKernelGGL(k_lsa_batch, dim3(n_problems), dim3(LSA_THREADS), 0, stream, cost, desc, threshold, len, row_to_col, unmatched_rows,
                       unmatched_cols, counts, (char *)ws);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

}  // extern "C"
