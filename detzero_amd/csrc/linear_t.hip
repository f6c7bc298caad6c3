// Linear layers of the exact-fp32 mode on the bf16 matrix pipe (gfx950): the row GEMM of dz_linear_forward - the refiner's and the PDV
// head's Conv1d / Conv2d(1x1) / Linear + BN + ReLU layers, attention projections, FFNs and FC stacks - in the three-limb arithmetic of
// limb3.h.  fp32 rows in and out exactly as dz_linear_forward reads and writes them, no tensor format; every operand as THREE exact
// bf16 limbs (h = rn(x), m = rn(x - h), l = x - h - m, the clamp before the first rounding only), six v_mfma_f32_32x32x16_bf16 per
// product with fp32 accumulation.
// Reference call sites: refining/detzero_refine/models/modules/geometry_transformer.py:34-67, position_transformer.py:38-70,
// detection/detzero_det/models/centerpoint_modules/pdv_head.py:154-172.
//
// Skeleton: k_conv2d_t's (conv2d_t.hip) on the shared limb tile (Limb3Tile / limb3_* of limb3.h) - an output-stationary tile of BP rows
// x BC output channels, blockIdx.x = row tile, blockIdx.y = channel tile; a chunk is KC input channels.  A side: fp32 buffer loads into
// registers one chunk ahead, split ONCE per value on the way into LDS (limb3_store); B side: the limb-packed weights staged verbatim
// (rows of a channel tile past the packed ones read as zeros).  Double-buffered LDS, one barrier per chunk.
// What is this kernel's own:
//   * addressing: row r lives at x + r * x_stride - no (b, y, x) mapping, no division in the address path.  Rows at or beyond `rows`
//     use the out-of-range buffer offset: zeros come back, nothing is stored for them.  Columns cin .. x_stride - 1 are never read
//     (the buffer ends behind column cin - 1 of the last row).
//   * the epilogue: v = relu?(fma(acc + group_shift[row / group_rows][col], scale[col], shift[col])) - the per-row-group addend of the
//     PointNet concat goes in ONCE, before scale / shift, as dz_linear_forward defines it; group_shift is (row groups, cout_pad) fp32,
//     a group boundary may fall anywhere inside a tile and the last group may be ragged.  scale / shift may be NULL (1 / 0).
//   * the write contract: columns [0, cout) of rows [0, rows) only - float4 where y_stride, the column and the pointer allow it, word
//     by word otherwise; columns cout .. y_stride - 1 and everything behind the last row keep their contents.
//
// Accumulation order per output element (fixed; independent of tile, launch split and scheduling): 16-channel k-steps ascending, and per
// k-step the six terms (weight limb . input limb)
//        l.h  h.l  m.m  m.h  h.m  h.h          (smallest first: limb3_terms)
// added onto the element's ONE accumulator; dropped: m.l + l.m + l.l, at most 2^-26 of |x.w|.  No atomics; two launches agree bit for
// bit, and so do a single launch and the row chunks of dz_linear_limb3_forward.
//
// Instances (BP x BC x KC; the tiles of conv2d_t.hip, 256 threads = one wave per SIMD; registers from the compiler's resource report):
//   k_linear_t<128x128x16>  2 x 2 waves, wave tile 64 x 64:  126 + 64 registers, 57 344 B LDS   (cout_pad % 128 == 0)
//   k_linear_t<128x64x32>   4 x 1 waves, wave tile 32 x 64:   96 + 32 registers, 79 872 B LDS   (other widths above 32)
//   k_linear_t<128x32x32>   4 x 1 waves, wave tile 32 x 32:   74 + 16 registers, 66 560 B LDS   (cout_pad 16 / 32)
// Each allows 2 workgroups per CU (LDS: 160 KB; the registers allow 2 / 4 / 5 waves per SIMD).  0 bytes of scratch, no spilled VGPR
// (tests/test_linear_limb3_build.py reads the report).  With BC = 128 a 128 -> 512 layer re-reads and re-splits its input rows four
// times.  Tried on an MI355X and not kept: an input-resident form for cin = 128 - the limb rows of the row tile
// split once and kept in LDS (100 KB + the weight buffers: one workgroup per CU), the workgroup walking the channel tiles itself;
// bit-identical, and 0.63 - 0.77 x the speed of this form on 128 -> 128 / 256 / 512.
#include "hgemm.h"
#include "limb3.h"

namespace dz {

template <int BP, int BC, int KC, int WP, int WC>
struct LTTile : Limb3Tile<BP, BC, KC, WP, WC> {};

constexpr int LT_ROW_MULT = 32;         // output-channel rows of the packed weights: cout_pad rounded up to this

struct LinTArgs {
    const float *x, *w, *scale, *shift, *group_shift;
    float *y;
    unsigned int rows;                  // of this launch
    int cin, x_stride, cout, cout_pad, y_stride, group_rows, relu, wrows;
    unsigned int x_bytes, w_bytes;
};

// The epilogue: addend, scale / shift, ReLU, and the stores of the write contract
template <class T>
__device__ __forceinline__ void lt_epilogue(const LinTArgs &p, const f32x16 (&acc)[T::CT][T::PT], unsigned int row0, int n0, int wp, int wc, int l31, int kh) {
    constexpr int PT = T::PT, CT = T::CT;
    // register quad j of fragment (ct, pt) = channels ct*32 + 8 j + 4 kh .. + 3 of my row
    const bool vec = (p.y_stride & 3) == 0 && (reinterpret_cast<size_t>(p.y) & 15) == 0;       // 16-byte aligned quads
    const bool has_sc = p.scale != nullptr, has_sh = p.shift != nullptr, has_gs = p.group_shift != nullptr;
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
        const unsigned int row = row0 + wp * PT * 32 + pt * 32 + l31;
        if (row >= p.rows) continue;
        float *const orow = p.y + (size_t)row * p.y_stride;
        const float *const grow = has_gs ? p.group_shift + (size_t)(row / (unsigned int)p.group_rows) * p.cout_pad : nullptr;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            // (addend, scale and shift of the fragment are requested before the first is used: one memory round trip)
            float4 gs[4], sc[4], sh[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = n0 + wc * CT * 32 + ct * 32 + j * 8 + kh * 4;
                const bool live = col < p.cout;                // (col % 4 == 0 and cout_pad % 16 == 0: the quad lies inside the vectors)
                const float *const a = grow + col, *const s = p.scale + col, *const b = p.shift + col;
                gs[j] = has_gs && live ? make_float4(a[0], a[1], a[2], a[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
                sc[j] = has_sc && live ? make_float4(s[0], s[1], s[2], s[3]) : make_float4(1.f, 1.f, 1.f, 1.f);      // (word loads: the vectors
                sh[j] = has_sh && live ? make_float4(b[0], b[1], b[2], b[3]) : make_float4(0.f, 0.f, 0.f, 0.f);      // need no 16-byte alignment)
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = n0 + wc * CT * 32 + ct * 32 + j * 8 + kh * 4;
                if (col >= p.cout) continue;
                float a[4] = {acc[ct][pt][4 * j], acc[ct][pt][4 * j + 1], acc[ct][pt][4 * j + 2], acc[ct][pt][4 * j + 3]};
                if (has_gs) { a[0] += gs[j].x; a[1] += gs[j].y; a[2] += gs[j].z; a[3] += gs[j].w; }
                float v[4] = {fmaf(a[0], sc[j].x, sh[j].x), fmaf(a[1], sc[j].y, sh[j].y), fmaf(a[2], sc[j].z, sh[j].z), fmaf(a[3], sc[j].w, sh[j].w)};
                if (p.relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                float *const o = orow + col;
                if (vec && col + 4 <= p.cout) {
                    *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (col + e < p.cout) o[e] = v[e];
                }
            }
        }
    }
}

template <class T>
__global__ __launch_bounds__(T::THREADS) void k_linear_t(LinTArgs p) {
    constexpr int P = T::P_PER_THREAD, C = T::C_PER_THREAD, PT = T::PT, CT = T::CT, G = T::G, ROWB = T::ROWB;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *const Ps0 = smem, *const Cs0 = smem + 2 * T::PS_BYTES;      // [2][PS], [2][CS]

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wp = wid / T::WC, wc = wid % T::WC, l31 = lane & 31, kh = lane >> 5;
    const int n0 = blockIdx.y * T::BC;
    const unsigned int row0 = blockIdx.x * (unsigned int)T::BP;
    const int nchunks = p.cin / T::KC;
    const __amdgpu_buffer_rsrc_t prsrc = make_rsrc(p.x, p.x_bytes), crsrc = make_rsrc(p.w, p.w_bytes);
    const unsigned int wrow_bytes = (unsigned int)p.cin * 6u;                  // cin / 8 groups of 48 bytes

    unsigned int cvoff[C], clds[C];         // my pieces of a chunk's weight slice: rows n0 .. n0 + BC - 1 of the packed rows
    limb3_weight_pieces<T>(tid, n0, p.wrows, wrow_bytes, cvoff, clds);
    // my 8-channel groups of the input chunk: byte offset in channel slice 0, and where the group goes in an LDS buffer
    unsigned int pvoff[P], plds[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int idx = tid + i * T::THREADS;
        const int r = idx / G, g = idx % G;
        pvoff[i] = row0 + r < p.rows ? ((row0 + r) * (unsigned int)p.x_stride + (unsigned int)(g * 8)) * 4u : OOB_OFFSET;
        plds[i] = (unsigned int)(r * ROWB + g * 48);
    }
    const int poff = limb3_frag_base<T>(wp, PT, lane), coff = limb3_frag_base<T>(wc, CT, lane);

    f32x16 acc[CT][PT];
    limb3_zero<T>(acc);

    unsigned int padd = 0u, cadd = 0u;      // byte offsets of the chunk relative to pvoff / cvoff
    v4u sp[P][2], sw[C];
    auto issue = [&]() {
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const unsigned int off = pvoff[i] == OOB_OFFSET ? OOB_OFFSET : pvoff[i] + padd;
            sp[i][0] = __builtin_amdgcn_raw_buffer_load_b128(prsrc, off, 0, 0);
            sp[i][1] = __builtin_amdgcn_raw_buffer_load_b128(prsrc, off == OOB_OFFSET ? OOB_OFFSET : off + 16u, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < C; ++i) sw[i] = __builtin_amdgcn_raw_buffer_load_b128(crsrc, cvoff[i] == OOB_OFFSET ? OOB_OFFSET : cvoff[i] + cadd, 0, 0);
        padd += (unsigned int)(T::KC * 4);
        cadd += (unsigned int)(G * 48);
    };
    auto store = [&](int buf) { limb3_store<T>(Ps0 + buf * T::PS_BYTES, Cs0 + buf * T::CS_BYTES, sp, sw, plds, clds); };

    issue();                // chunk 0
    store(0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int cur = c & 1;
        const bool has1 = c + 1 < nchunks;
        if (has1) issue();  // chunk c + 1: lands in registers behind this chunk's MFMAs
        limb3_mma<T>(Ps0 + cur * T::PS_BYTES + poff, Cs0 + cur * T::CS_BYTES + coff, acc);
        if (has1) store(cur ^ 1);
        __syncthreads();
    }

    lt_epilogue<T>(p, acc, row0, n0, wp, wc, l31, kh);
}

// The instances: BP x BC x KC, the three of conv2d_t.hip (the register and LDS budgets are known there; figures in the header)
using LT_128_16 = LTTile<128, 128, 16, 2, 2>;
using LT_64_32 = LTTile<128, 64, 32, 4, 1>;
using LT_32_32 = LTTile<128, 32, 32, 4, 1>;
static_assert(2 * LT_128_16::LDS_BYTES <= 160 * 1024 && 2 * LT_64_32::LDS_BYTES <= 160 * 1024 && 2 * LT_32_32::LDS_BYTES <= 160 * 1024,
              "two workgroups per CU");

static inline int lt_wrows(int cout_pad) { return (cout_pad + LT_ROW_MULT - 1) / LT_ROW_MULT * LT_ROW_MULT; }
static inline size_t lt_w_bytes(int cin, int cout_pad) { return (size_t)lt_wrows(cout_pad) * (size_t)cin * 6; }

template <class T>
static int launch_lt(const LinTArgs &a, hipStream_t stream) {
    static PerDeviceFlags done;
    if (int rc = reserve_lds(reinterpret_cast<const void *>(&k_linear_t<T>), T::LDS_BYTES, done, "dz_linear_limb3_forward")) return rc;
    dim3 grid((unsigned int)ceil_div((long)a.rows, T::BP), (unsigned int)ceil_div(a.wrows, T::BC));
    hipLaunchKernelGGL((k_linear_t<T>), grid, dim3(T::THREADS), T::LDS_BYTES, stream, a);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

enum LTVariant { LT_NONE = 0, LT_V_128_16, LT_V_64_32, LT_V_32_32 };
using LTLaunch = int (*)(const LinTArgs &, hipStream_t);
struct LTEntry { const char *name; LTLaunch launch; };
static const LTEntry kLT[] = {
    {"none", nullptr},
    {"k_linear_t<128x128x16>", launch_lt<LT_128_16>},
    {"k_linear_t<128x64x32>", launch_lt<LT_64_32>},
    {"k_linear_t<128x32x32>", launch_lt<LT_32_32>},
};

// The field that keeps a layer off this engine, or nullptr: what dz_linear_limb3_supported answers and _forward reports
static const char *lt_refusal(int cin, int x_stride, int cout, int cout_pad, int y_stride) {
    if (cin <= 0 || cin % 32 != 0) return "cin (a multiple of 32)";
    if (cout_pad <= 0 || cout_pad % 16 != 0) return "cout_pad (a multiple of 16)";
    if (cout < 1 || cout > cout_pad) return "cout (1 .. cout_pad)";
    if (x_stride < cin || x_stride % 4 != 0) return "x_stride (at least cin, a multiple of 4)";
    if (y_stride < cout) return "y_stride (at least cout)";
    if (lt_w_bytes(cin, cout_pad) >= 0x80000000ull) return "w_limb (weights at or beyond the 2 GiB buffer-addressing limit)";
    return nullptr;
}

// The one decision of this engine: the channel width alone picks the tile
static LTVariant linear_t_select(int cin, int cout_pad) {
    if (cin <= 0 || cin % 32 != 0 || cout_pad <= 0 || cout_pad % 16 != 0 || lt_w_bytes(cin, cout_pad) >= 0x80000000ull) return LT_NONE;
    if (cout_pad % 128 == 0) return LT_V_128_16;
    if (cout_pad > 32) return LT_V_64_32;
    return LT_V_32_32;
}

}  // namespace dz

using namespace dz;

extern "C" {

int dz_linear_limb3_supported(int cin, int x_stride, int cout, int cout_pad, int y_stride) {
    return lt_refusal(cin, x_stride, cout, cout_pad, y_stride) ? 0 : 1;
}

const char *dz_linear_limb3_variant(int cin, int cout_pad) { return kLT[linear_t_select(cin, cout_pad)].name; }

int dz_linear_limb3_forward(const float *x, long rows, int cin, int x_stride, const float *w_limb, int cout, int cout_pad, const float *scale,
                            const float *shift, const float *group_shift, int group_rows, int relu, float *y, int y_stride, long max_launch_rows,
                            void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (const char *why = lt_refusal(cin, x_stride, cout, cout_pad, y_stride)) {
        set_error("dz_linear_limb3_forward: %s is not covered by the bf16x3 engine (cin %d x_stride %d cout %d cout_pad %d y_stride %d)", why, cin,
                  x_stride, cout, cout_pad, y_stride);
        return DZ_ERR_UNSUPPORTED;
    }
    DZ_CHECK_ARG(x && y && w_limb, "dz_linear_limb3_forward: null pointer (x, y or w_limb)");
    DZ_CHECK_ARG(rows >= 0, "dz_linear_limb3_forward: negative rows (%ld)", rows);
    DZ_CHECK_ARG(max_launch_rows >= 0, "dz_linear_limb3_forward: negative max_launch_rows (%ld)", max_launch_rows);
    if (rows == 0) return DZ_OK;
    if (group_rows < 1) group_rows = 1;
    // the rows are fetched through 32-bit buffer offsets: at most ~2 GiB of them per launch (dz_linear_forward's window)
    long max_rows = (long)(0x7FF00000ull / ((size_t)x_stride * sizeof(float)));
    if (max_launch_rows > 0 && max_launch_rows < max_rows) max_rows = max_launch_rows;
    if (group_shift) max_rows = max_rows / group_rows * group_rows;     // keep launches aligned to row groups
    if (max_rows < 1) {
        set_error("dz_linear_limb3_forward: one row group (group_rows %d) exceeds %s", group_rows,
                  max_launch_rows > 0 && max_launch_rows < group_rows ? "max_launch_rows" : "the 2 GiB addressing window");
        return DZ_ERR_UNSUPPORTED;
    }
    const LTLaunch launch = kLT[linear_t_select(cin, cout_pad)].launch;
    for (long r0 = 0; r0 < rows; r0 += max_rows) {
        const long n = rows - r0 < max_rows ? rows - r0 : max_rows;
        LinTArgs a;
        a.x = x + (size_t)r0 * x_stride; a.w = w_limb; a.scale = scale; a.shift = shift;
        a.group_shift = group_shift ? group_shift + (size_t)(r0 / group_rows) * cout_pad : nullptr;
        a.y = y + (size_t)r0 * y_stride;
        a.rows = (unsigned int)n; a.cin = cin; a.x_stride = x_stride; a.cout = cout; a.cout_pad = cout_pad; a.y_stride = y_stride;
        a.group_rows = group_rows; a.relu = relu; a.wrows = lt_wrows(cout_pad);
        a.x_bytes = (unsigned int)((((size_t)n - 1) * x_stride + cin) * sizeof(float));       // ends behind column cin - 1 of the last row
        a.w_bytes = (unsigned int)lt_w_bytes(cin, cout_pad);
        if (int rc = launch(a, stream)) return rc;
    }
    return DZ_OK;
}

}  // extern "C"
