// Stand-alone host program around csrc/lsa.h (tests/test_lsa_host.py compiles and runs it): the one-thread form of the code the
// device runs cooperatively.
//
//   lsa_host_main <problems> <results>
// problems: int32 count, then per problem int32 rows, int32 cols, float64 threshold, rows * cols float32 costs (row-major).
// results:  per problem int32 counts[4] (matched, unmatched rows, unmatched cols, status), rows int32 row_to_col,
//           rows int32 unmatched rows (the first counts[1] hold the list), cols int32 unmatched columns (the first counts[2]).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lsa.h"

static bool read_all(FILE *f, void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }
static bool write_all(FILE *f, const void *src, size_t bytes) { return bytes == 0 || fwrite(src, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <problems> <results>\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]); return 2; }
    int32_t count = 0;
    if (!read_all(in, &count, sizeof(count)) || count < 0) { fprintf(stderr, "bad header\n"); return 2; }
    for (int32_t p = 0; p < count; ++p) {
        int32_t dims[2];
        double threshold;
        if (!read_all(in, dims, sizeof(dims)) || !read_all(in, &threshold, sizeof(threshold)) || dims[0] < 0 || dims[1] < 0) {
            fprintf(stderr, "problem %d: bad header\n", p);
            return 2;
        }
        const int rows = dims[0], cols = dims[1];
        std::vector<float> cost((size_t)rows * cols);
        if (!read_all(in, cost.data(), cost.size() * sizeof(float))) { fprintf(stderr, "problem %d: short matrix\n", p); return 2; }
        std::vector<double> work(dz::lsa_work_bytes(rows, cols) / sizeof(double) + 1);
        std::vector<int32_t> row_to_col(rows), rows_free(rows), cols_free(cols);
        int32_t counts[4] = {0, 0, 0, 0};
        dz::LsaHostCtx cx;
        dz::lsa_assign(cx, cost.data(), rows, cols, threshold, dz::lsa_work_at(work.data(), rows, cols), row_to_col.data(), rows_free.data(),
                       cols_free.data(), counts);
        if (!write_all(out, counts, sizeof(counts)) || !write_all(out, row_to_col.data(), rows * sizeof(int32_t)) ||
            !write_all(out, rows_free.data(), rows * sizeof(int32_t)) || !write_all(out, cols_free.data(), cols * sizeof(int32_t))) {
            fprintf(stderr, "problem %d: write failed\n", p);
            return 2;
        }
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
