// Segmented object crop over many frames (daemon/prepare_object_data.py:241-273,310 driven over a whole sequence).
//
// dz_crop_points_in_boxes (head_post.hip) serves one frame: a T x M bitmap, its scan, a guessed capacity and one sync per frame.
// Here the points of F frames lie back to back, every frame brings its own boxes, and two passes over the same geometry replace the
// bitmap:
//   count  one workgroup = one chunk of SEQ_CHUNK consecutive points of ONE frame (a chunk never straddles a frame).  The frame's boxes
//          are staged 64 at a time in LDS with cos / sin (pib_test.h, as k_points_in_boxes_bits does), one 64-bit __ballot and one
//          __popcll per wave and box, the waves' counts summed through LDS: one integer per (box, chunk).  The table is laid out row by
//          row in RANK order (row rank[b] = the chunks of box b's frame), so a flat exclusive prefix over it is every (box, chunk)'s write
//          position in output order, and the prefix at the row starts is the per-segment offset.
//   fill   same geometry, same test.  A (box, chunk) whose count is 0 is skipped without the test (nearly all of them: a box covers a
//          few square metres of a frame).  A kept point's row = prefix + counts of the earlier waves of the chunk + kept lanes below.
// No atomics, no bitmap, no capacity: the host reads the total once and allocates exactly.  Within a segment the points ascend (the
// order of `pts[mask[i]]`), and the bytes are the same on every run.
#include "common.h"
#include "pib_test.h"

namespace dz {

constexpr int SEQ_CHUNK = 256;               // points per chunk = threads per workgroup (4 waves, one point per lane)
constexpr int SEQ_WAVES = SEQ_CHUNK / 64;

struct SeqCropGeom {
    const float *xyz;                        // (m,3)
    const int *pt_off;                       // (nf+1) first point of every frame
    const float *boxes;                      // (nb,7) frame-major
    const int *box_off;                      // (nf+1) first box of every frame
    const int *rank;                         // (nb) output segment of box b
    const int *row_off;                      // (nb+1) first table entry of every segment (rank order)
    const int *chunk_frame;                  // (n_chunks) frame of every chunk
    const int *chunk_first;                  // (nf+1) first chunk of every frame
    int m, nb, nf, n_entries;
};

// what one workgroup works on; every index that came from memory is clamped to its array before it is followed
struct SeqChunk {
    int lc, b_lo, b_hi;
    bool valid;                              // this lane holds a point
    long i;                                  // its index
    float x, y, z;
};

__device__ __forceinline__ bool seq_chunk_setup(const SeqCropGeom &g, SeqChunk &c) {
    const int f = g.chunk_frame[blockIdx.x];
    if ((unsigned)f >= (unsigned)g.nf) return false;
    c.lc = (int)blockIdx.x - g.chunk_first[f];
    if (c.lc < 0) return false;
    const int p_lo = max(g.pt_off[f], 0), p_hi = min(g.pt_off[f + 1], g.m);
    c.b_lo = max(g.box_off[f], 0);
    c.b_hi = min(g.box_off[f + 1], g.nb);
    c.i = (long)p_lo + (long)c.lc * SEQ_CHUNK + threadIdx.x;
    c.valid = c.i < (long)p_hi;
    c.x = c.y = c.z = 0.f;
    if (c.valid) { c.x = g.xyz[c.i * 3]; c.y = g.xyz[c.i * 3 + 1]; c.z = g.xyz[c.i * 3 + 2]; }
    return true;
}

// table entry of (box b, this chunk), or -1 when rank / row_off do not name one
__device__ __forceinline__ int seq_entry(const SeqCropGeom &g, int b, int lc) {
    const int r = g.rank[b];
    if ((unsigned)r >= (unsigned)g.nb) return -1;
    const long e = (long)g.row_off[r] + lc;
    return (e >= 0 && e < (long)g.row_off[r + 1] && e < (long)g.n_entries) ? (int)e : -1;
}

__global__ __launch_bounds__(SEQ_CHUNK) void k_seq_crop_count(SeqCropGeom g, int *__restrict__ counts) {
    __shared__ float sb[PIB_STAGE_BOXES * PIB_BOX_FLOATS];
    __shared__ int wc[SEQ_WAVES][PIB_STAGE_BOXES];
    SeqChunk c;
    if (!seq_chunk_setup(g, c)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = c.b_lo; base < c.b_hi; base += PIB_STAGE_BOXES) {
        const int nb = min(PIB_STAGE_BOXES, c.b_hi - base);
        __syncthreads();
        if ((int)threadIdx.x < nb) pib_stage_box(g.boxes + (size_t)(base + threadIdx.x) * 7, sb + threadIdx.x * PIB_BOX_FLOATS);
        __syncthreads();
        for (int k = 0; k < nb; ++k) {
            const bool in = c.valid && pib_inside(c.x, c.y, c.z, sb + k * PIB_BOX_FLOATS);
            const unsigned long long bits = __ballot(in);
            if (lane == 0) wc[wave][k] = __popcll(bits);
        }
        __syncthreads();
        if ((int)threadIdx.x < nb) {
            const int e = seq_entry(g, base + threadIdx.x, c.lc);
            int s = 0;
#pragma unroll
            for (int w = 0; w < SEQ_WAVES; ++w) s += wc[w][threadIdx.x];
            if (e >= 0) counts[e] = s;
        }
    }
}

__global__ __launch_bounds__(SEQ_CHUNK) void k_seq_crop_fill(SeqCropGeom g, const int *__restrict__ counts, const int *__restrict__ prefix,
                                                             const uint32_t *__restrict__ payload, int words, uint32_t *__restrict__ out,
                                                             int *__restrict__ out_index, int total) {
    __shared__ float sb[PIB_STAGE_BOXES * PIB_BOX_FLOATS];
    __shared__ int scnt[PIB_STAGE_BOXES], spre[PIB_STAGE_BOXES];
    __shared__ int wc[2][SEQ_WAVES];
    SeqChunk c;
    if (!seq_chunk_setup(g, c)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int par = 0;
    for (int base = c.b_lo; base < c.b_hi; base += PIB_STAGE_BOXES) {
        const int nb = min(PIB_STAGE_BOXES, c.b_hi - base);
        __syncthreads();
        if ((int)threadIdx.x < nb) {
            pib_stage_box(g.boxes + (size_t)(base + threadIdx.x) * 7, sb + threadIdx.x * PIB_BOX_FLOATS);
            const int e = seq_entry(g, base + threadIdx.x, c.lc);
            scnt[threadIdx.x] = e >= 0 ? counts[e] : 0;
            spre[threadIdx.x] = e >= 0 ? prefix[e] : 0;
        }
        __syncthreads();
        for (int k = 0; k < nb; ++k) {
            if (scnt[k] == 0) continue;                              // the same for the whole workgroup
            const bool in = c.valid && pib_inside(c.x, c.y, c.z, sb + k * PIB_BOX_FLOATS);
            const unsigned long long bits = __ballot(in);
            if (lane == 0) wc[par][wave] = __popcll(bits);
            __syncthreads();                                         // wc[par] is written again two boxes on, a barrier later
            if (in) {
                int pos = spre[k] + __popcll(bits & ((1ull << lane) - 1ull));
                for (int w = 0; w < wave; ++w) pos += wc[par][w];
                if ((unsigned)pos < (unsigned)total) {
                    const uint32_t *src = payload + (size_t)c.i * words;
                    uint32_t *dst = out + (size_t)pos * words;
                    for (int w = 0; w < words; ++w) dst[w] = src[w];
                    if (out_index) out_index[pos] = (int)c.i;
                }
            }
            par ^= 1;
        }
    }
}

static int seq_crop_check(const char *who, const float *xyz, long long m, const int *pt_off, const float *boxes, long long nb, const int *box_off,
                          const int *rank, const int *row_off, int n_frames, const int *chunk_frame, const int *chunk_first, long long n_chunks,
                          long long n_entries) {
    DZ_CHECK_ARG(m >= 0 && nb >= 0 && n_frames >= 0 && n_chunks >= 0 && n_entries >= 0, "%s: negative size", who);
    DZ_CHECK_ARG(m < (1ll << 31) && nb < (1ll << 31) && n_chunks < (1ll << 31) && n_entries < (1ll << 31),
                 "%s: points, boxes, chunks or table entries reach 2^31", who);
    if (n_chunks == 0) return DZ_OK;
    DZ_CHECK_ARG(m > 0 && nb > 0 && n_frames > 0, "%s: chunks without points, boxes or frames", who);
    DZ_CHECK_ARG(xyz && pt_off && boxes && box_off && rank && row_off && chunk_frame && chunk_first, "%s: null pointer", who);
    return DZ_OK;
}

}  // namespace dz

using namespace dz;

extern "C" {

int dz_seq_crop_chunk_points(void) { return SEQ_CHUNK; }

int dz_seq_crop_count(const float *xyz, long long m, const int *pt_off, const float *boxes, long long nb, const int *box_off, const int *rank,
                      const int *row_off, int n_frames, const int *chunk_frame, const int *chunk_first, long long n_chunks, int *counts,
                      long long n_entries, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = seq_crop_check("dz_seq_crop_count", xyz, m, pt_off, boxes, nb, box_off, rank, row_off, n_frames, chunk_frame, chunk_first, n_chunks,
                            n_entries);
    if (rc || n_chunks == 0) return rc;
    DZ_CHECK_ARG(counts && n_entries > 0, "dz_seq_crop_count: chunks without a count table");
    const SeqCropGeom g{xyz, pt_off, boxes, box_off, rank, row_off, chunk_frame, chunk_first, (int)m, (int)nb, n_frames, (int)n_entries};
    hipLaunchKernelGGL(k_seq_crop_count, dim3((unsigned)n_chunks), dim3(SEQ_CHUNK), 0, stream, g, counts);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_seq_crop_fill(const float *xyz, long long m, const int *pt_off, const float *boxes, long long nb, const int *box_off, const int *rank,
                     const int *row_off, int n_frames, const int *chunk_frame, const int *chunk_first, long long n_chunks, const int *counts,
                     const int *prefix, long long n_entries, const void *payload, int payload_words, void *out, int *out_index, long long total,
                     void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = seq_crop_check("dz_seq_crop_fill", xyz, m, pt_off, boxes, nb, box_off, rank, row_off, n_frames, chunk_frame, chunk_first, n_chunks,
                            n_entries);
    if (rc) return rc;
    DZ_CHECK_ARG(payload_words >= 1, "dz_seq_crop_fill: payload_words %d", payload_words);
    DZ_CHECK_ARG(total >= 0 && total < (1ll << 31), "dz_seq_crop_fill: total rows %lld outside [0, 2^31)", total);
    if (n_chunks == 0 || total == 0) return DZ_OK;
    DZ_CHECK_ARG(counts && prefix && payload && out && n_entries > 0, "dz_seq_crop_fill: null pointer");
    const SeqCropGeom g{xyz, pt_off, boxes, box_off, rank, row_off, chunk_frame, chunk_first, (int)m, (int)nb, n_frames, (int)n_entries};
    hipLaunchKernelGGL(k_seq_crop_fill, dim3((unsigned)n_chunks), dim3(SEQ_CHUNK), 0, stream, g, counts, prefix, (const uint32_t *)payload,
                       payload_words, (uint32_t *)out, out_index, (int)total);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

}  // extern "C"
