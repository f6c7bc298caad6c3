// Stand-alone host program around csrc/lsa.h's prefix driver (tests/test_eval_match_host.py compiles and runs it): the one-thread
// form of the solve csrc/eval_match.hip makes per problem.
//
//   eval_match_host_main <problems> <results>
// problems: int32 count, then per problem int32 P, int32 G, P * G float32 weights (row-major, >= 0, already thresholded).
// The solve has G + P columns: column j < G costs 1 - w, the others cost 1 ("unmatched").
// results:  per problem int32 status, then for every prefix n = 1..P the n int32 of its rows: the matched ground truth of a
//           valid pair (w > 0), else -1.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lsa.h"

static bool read_all(FILE *f, void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

struct Cost {
    const float *w;
    int G;
    double operator()(int i, int j) const { return j < G ? 1.0 - (double)w[(size_t)i * G + j] : 1.0; }
};

struct Record {
    const float *w;
    int G;
    std::vector<int32_t> *out;
    void operator()(dz::LsaHostCtx &, int rows_done, const int *col4row) {
        for (int r = 0; r < rows_done; ++r) {
            const int j = col4row[r];
            out->push_back(j >= 0 && j < G && w[(size_t)r * G + j] > 0.f ? j : -1);
        }
    }
};

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <problems> <results>\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]); return 2; }
    int32_t count = 0;
    if (!read_all(in, &count, sizeof(count)) || count < 0) { fprintf(stderr, "bad header\n"); return 2; }
    for (int32_t p = 0; p < count; ++p) {
        int32_t dims[2];
        if (!read_all(in, dims, sizeof(dims)) || dims[0] < 0 || dims[1] < 0) { fprintf(stderr, "problem %d: bad header\n", p); return 2; }
        const int P = dims[0], G = dims[1], C = G + P;
        std::vector<float> w((size_t)P * G);
        if (!read_all(in, w.data(), w.size() * sizeof(float))) { fprintf(stderr, "problem %d: short matrix\n", p); return 2; }
        std::vector<double> work(dz::lsa_work_bytes(P, C) / sizeof(double) + 1);
        std::vector<int32_t> res(1, 0);
        int word = 0;
        dz::LsaHostCtx cx;
        const Cost cost{w.data(), G};
        Record rec{w.data(), G, &res};
        res[0] = dz::lsa_assign_prefix(cx, cost, P, C, dz::lsa_work_at(work.data(), P, C), &word, rec);
        if (fwrite(res.data(), sizeof(int32_t), res.size(), out) != res.size()) { fprintf(stderr, "problem %d: write failed\n", p); return 2; }
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
