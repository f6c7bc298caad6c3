// Submanifold 3 x 3 x 3 sparse convolution with the inputs of a whole z slab staged ONCE per unit ("x-run" engine), gfx950,
// EXACT fp32: fp32 rows in, v_mfma_f32_32x32x2_f32 (bitwise an fmaf chain), fp32 rows out.  The fp32 sibling of sparse_conv_x.hip;
// reference call sites: detection/detzero_det/models/centerpoint_modules/backbone3d.py:93-121 (SparseBasicBlock: two SubMConv3d +
// BatchNorm + ReLU with the residual add), :243-280 (conv2 / conv3 / conv4 of VoxelResBackBone8x).
//
// Why: in fp32 every sparse convolution ran on the gather kernel of sparse_conv.hip, which fetches one input row per (output row,
// tap) pair and stages it through registers.  Rows of a level are stored in ascending linear key, so the neighbours of UR consecutive
// output rows at one z offset are ONE contiguous range of input rows (the "window" of sparse_conv_x.hip, from the same index:
// dz_build_neighbors_packed_x / dz_spconv_x_windows); the kernel keeps a 16-channel chunk of that window resident in LDS and runs
// the nine taps of the slab from it.  An fp32 MFMA does 1/16 of the work per issue slot of a 16-bit one while a 16-channel chunk of
// an fp32 row is the same 64 bytes as a pair16 k-step, so this kernel is compute-bound and keeps NONE of the latency machinery of the
// pair16 kernel (no persistent workgroups, no tile queues, no weight ring, no counted vmcnt): the structure is deliberately plain.
//
//   unit      UR = dz_spconv_x_tile_rows consecutive output rows (positions, when the table is in tap-set order) x all COUT channels,
//             one 512-thread workgroup per unit; wave (wp, wc) owns one 32-row fragment x CT 32-channel fragments (CT x 16 accumulator
//             registers).  The windows are read per unit; the 16 queue words behind them are never touched (they stay zero).
//             LDS is sized so that TWO workgroups share a CU (<= 80 KB each): one's barrier waits, prologue and epilogue run under
//             the other's MFMAs.  Measured at 160k points x 16 frames with one workgroup per CU (windows of 896 / 640 rows) the
//             64 / 128-channel layers were 3 % / 14 % SLOWER than the gather kernel; with two, 12 % / 1.3 % faster.
//   stage     (tz, 16-channel chunk kc): the window's rows x 64 bytes -> LDS by `buffer_load_dwordx4 ... lds` (no staging registers,
//             1 KB per wave instruction), double buffered.  Slabs without a neighbour (window of 0 rows) have no stages.  A window
//             longer than RCAP rows (a unit in a sparse region next to a dense slab) is not staged: the stage runs in GATHER mode -
//             each lane fetches its neighbour row's 32 bytes of the chunk straight from global memory; same taps, same order.
//   step      the three taps of one window row ty of a stage: their weight slices (16 input channels x COUT: 16 * COUT * 4 contiguous
//             bytes of the (27, cin, cout) fp32 weights each - the layout dz_spconv_forward takes, no repacking) -> LDS the same way,
//             double buffered.  The loads of step i + 1 are issued behind the MFMAs of step i's first tap; ONE `s_waitcnt vmcnt(0)` +
//             barrier per step (the step's 24 x CT MFMAs of 64 cycles are far longer than the loads' latency).  The staged and the
//             gather form of a step are two copies of the code, so the staged one holds no wait for a compiler-tracked load.
//   rows      64-byte window rows are unpadded; 16-byte piece p of row r sits at slot p ^ ((r >> 2) & 3) (conflict-free ds_read_b128 for
//             consecutive rows); the direct loads realise the swizzle by permuting which source piece a lane fetches.  Lane (row l & 31,
//             half h = l >> 5) reads the two pieces 2 h, 2 h + 1 = channels 8 h .. 8 h + 7 of the chunk; a missing neighbour reads the
//             zero row behind the window.
//   table     the PACKED neighbour table (one word per (tz, ty) and output row = rank below the centre cell + three presence bits),
//             nine words per lane read once per unit.
//   skipping  a (fragment, tap) none of the fragment's 32 rows has a neighbour at issues no MFMAs (wave-uniform branch on a ballot).
//
// Orientation D[cout x row] = W[cout x k] . X^T[k x row]: the 32 x 32 accumulator holds, per lane, 4 consecutive output channels of one
// row per register quad -> the epilogue (out = relu?(acc * scale + shift (+ residual)), as dz_spconv_forward) stores 16 bytes per quad
// straight into the row (scale / shift / residual of a whole 32-channel fragment requested before the first use: one round trip).
// Rows at or beyond *d_m_out are never written.
//
// Accumulation order per output element (fixed; independent of the unit a row falls into, of the mode of the stage and of scheduling):
//   tz = 0..2, 16-channel chunk kc, ty = 0..2, tx = 0..2, then for s = 0..7 the two products of channels kc*16 + s and kc*16 + 8 + s,
// each one fmaf onto the running sum (absent taps add nothing).  No atomics; two launches agree bit for bit.  Against
// dz_spconv_forward (tap, then channel) the result differs by fp32 summation-order noise only.
#include <type_traits>

#include "sparse_conv_xw.h"

namespace dz {

template <int COUT_, int WP_, int WC_, int RCAP_>
struct XFCfg {
    static constexpr int COUT = COUT_, WP = WP_, WC = WC_, RCAP = RCAP_;
    static constexpr int NW = WP * WC, THREADS = 64 * NW;
    static constexpr int CT = COUT / (32 * WC);              // 32-channel fragments per wave
    static constexpr int UR = WP * 32;                       // output rows per unit
    static constexpr int SPS = 3;                            // steps per stage (tz, kc): one per window row ty
    static constexpr int WIN_BYTES = (RCAP + 1) * 64;        // + the zero row missing neighbours read
    static constexpr int TAP_BYTES = 16 * COUT * 4;          // weight slice of one tap: 16 input channels x COUT
    static constexpr int WSTEP_BYTES = 3 * TAP_BYTES;
    static constexpr int OFF_WIN = 0, OFF_W = 2 * WIN_BYTES;
    static constexpr int LDS_BYTES = OFF_W + 2 * WSTEP_BYTES;
    static constexpr int WRUNS = WSTEP_BYTES / 1024;         // 1 KB direct loads per step's weights
    static_assert(COUT % (32 * WC) == 0 && RCAP % 16 == 0 && TAP_BYTES % 1024 == 0, "shape");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
    static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");
};

template <class C>
__global__ __launch_bounds__(C::THREADS) void k_spconv_xf(SpConvXWArgs a) {
    constexpr int CT = C::CT, COUT = C::COUT, RCAP = C::RCAP, NW = C::NW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wc = wid % C::WC, l31 = lane & 31, kh = lane >> 5;
    const int m = min(*a.d_m_out, a.cap);
    if ((int)blockIdx.x * C::UR >= m) return;
    const srsrc_t crsrc = make_srsrc(a.w, a.w_bytes);
    const unsigned int in_rows = a.in_bytes / ((unsigned int)a.cin * 4u);
    XWUnit<C> u(a, smem, m, wid, lane);
    const int nsteps = u.nz * u.nk * C::SPS;

    auto issue = [&](int i) {
        if (i >= nsteps) return;
        int tz, kc, ty;
        u.stage_of(i, tz, kc, ty);
        // weights of the step's three taps: tap (tz*9 + ty*3 + tx), input channels [kc*16, kc*16 + 16), all COUT; 1 KB runs of
        // contiguous memory, copied as they are
        const unsigned int wbuf = (unsigned int)(C::OFF_W + (i & 1) * C::WSTEP_BYTES);
        for (int j = wid; j < C::WRUNS; j += NW) {
            const int tx = j / (C::TAP_BYTES / 1024), part = j % (C::TAP_BYTES / 1024);
            const unsigned int src = (unsigned int)(((tz * 9 + ty * 3 + tx) * a.cin + kc * 16) * COUT * 4 + part * 1024);
            load16_lds(wbuf + (unsigned int)j * 1024u, (unsigned int)lane * 16u, crsrc, src);
        }
        // the window of the stage, at its first step (a window beyond RCAP rows is not staged: gather mode)
        const int n = xw_pick(u.wn, tz);
        if (ty == 0 && n <= RCAP) {
            const int lo = xw_pick(u.wlo, tz);
            const int nruns = (n + 15) >> 4;
            for (int j = wid; j < nruns; j += NW) u.load_window_run(i / C::SPS, j, lo, n, kc);
        }
    };

    f32x16 acc[CT];
#pragma unroll
    for (int i = 0; i < CT; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

    issue(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // (the table words are in their registers from here on: no wait for them - and with them for the direct loads in flight - in the loop)
#pragma unroll
    for (int g = 0; g < 9; ++g) asm volatile("" : "+v"(u.pw[g]));
    __syncthreads();

    const unsigned int wcol = (unsigned int)((wc * CT * 32 + l31) * 4 + kh * 8 * COUT * 4);     // my weight column, input channel 8 kh of the chunk
    // one step: the three taps of window row ty.  GM (gather mode) is a compile-time copy of the body: with both operand paths in one
    // body the compiler's wait-count pass puts the global loads' `s_waitcnt vmcnt(0)` in front of every tap's MFMAs, which in the staged
    // mode would wait for the NEXT step's direct loads as well
    auto step = [&](int i, auto gm_t) {
        constexpr bool GM = decltype(gm_t)::value;
        int tz, kc, ty;
        u.stage_of(i, tz, kc, ty);
        const int lo = xw_pick(u.wlo, tz), n = xw_pick(u.wn, tz);
        const unsigned int(&pw)[9] = u.pw;
        const unsigned int e = tz == 0 ? (ty == 0 ? pw[0] : ty == 1 ? pw[1] : pw[2])
                             : tz == 1 ? (ty == 0 ? pw[3] : ty == 1 ? pw[4] : pw[5]) : (ty == 0 ? pw[6] : ty == 1 ? pw[7] : pw[8]);
        const int rank = (int)(e & 0x1FFFFFFFu);
        const unsigned char *const wbuf = smem + C::OFF_W + (i & 1) * C::WSTEP_BYTES + wcol;
        const unsigned char *const winb = smem + C::OFF_WIN + ((i / C::SPS) & 1) * C::WIN_BYTES;
        auto tap = [&](auto tx_t) {
            constexpr int tx = decltype(tx_t)::value;
            const int idx = rank + (tx == 0 ? -1 : tx == 1 ? 0 : (int)((e >> 30) & 1u));       // input row of the tap
            const int off = idx - lo;
            // (gather mode reads the row through a plain pointer: a rank at or past the input's rows - a level that overflowed its
            // calibrated capacity keeps such ranks in its index - has no row to read and adds nothing, as in the staged mode,
            // whose buffer loads return zeros there)
            const bool valid = ((e >> (29 + tx)) & 1u) != 0u && (GM ? (unsigned int)idx < in_rows : (unsigned int)off < (unsigned int)n);
            if (__ballot(valid) == 0ull) return;            // none of the fragment's rows has this tap
            float4 x0, x1;
            if constexpr (GM) {
                x0 = x1 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (valid) {
                    const float4 *p = reinterpret_cast<const float4 *>(a.in + (size_t)idx * a.cin + kc * 16 + kh * 8);
                    x0 = p[0];
                    x1 = p[1];
                }
            } else {
                const unsigned int ra = valid ? (unsigned int)off * 64u + (unsigned int)(((2 * kh) ^ ((off >> 2) & 3)) << 4) : (unsigned int)(RCAP * 64);
                x0 = *reinterpret_cast<const float4 *>(winb + ra);
                x1 = *reinterpret_cast<const float4 *>(winb + (ra ^ 16u));
            }
            const float xb[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
            const unsigned char *const wt = wbuf + tx * C::TAP_BYTES;
            float wv[CT][8];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int s = 0; s < 8; ++s) wv[ct][s] = *reinterpret_cast<const float *>(wt + s * COUT * 4 + ct * 128);
#pragma unroll
            for (int s = 0; s < 8; ++s)
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[ct][s], xb[s], acc[ct], 0, 0, 0);
        };
        // the next step's loads go out behind the first tap's MFMAs: no barrier is followed by address arithmetic and load issue in
        // front of a cold matrix pipe
        tap(std::integral_constant<int, 0>{});
        issue(i + 1);
        tap(std::integral_constant<int, 1>{});
        tap(std::integral_constant<int, 2>{});
    };
    for (int i = 0; i < nsteps; ++i) {
        int tz, kc, ty;
        u.stage_of(i, tz, kc, ty);
        if (xw_pick(u.wn, tz) > RCAP) step(i, std::true_type{});
        else step(i, std::false_type{});
        // the next step's loads have landed, and everyone is done with the buffers the loads issued next will overwrite
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    xw_epilogue<C>(a, acc, u.pos, m, wc, kh);
}

// unit rows = dz_spconv_x_tile_rows of the pair16 engine's shipped configurations (one index serves both arithmetics)
// RCAP: the largest window with which TWO workgroups share a CU's 160 KB of LDS (one's barrier waits, prologue and epilogue run under
// the other's MFMAs)
using XF32 = XFCfg<32, 8, 1, 512>;
using XF64 = XFCfg<64, 8, 1, 432>;
using XF128 = XFCfg<128, 4, 2, 240>;

static const XWVariant kXF[] = {{32, XF32::UR, XF32::RCAP, "k_spconv_xf<32>", launch_xw<k_spconv_xf<XF32>, XF32>},
                                 {64, XF64::UR, XF64::RCAP, "k_spconv_xf<64>", launch_xw<k_spconv_xf<XF64>, XF64>},
                                 {128, XF128::UR, XF128::RCAP, "k_spconv_xf<128>", launch_xw<k_spconv_xf<XF128>, XF128>}};

}  // namespace dz

using namespace dz;

extern "C" {

int dz_spconv_x_f32_window_rows(int cin, int cout) {
    const XWVariant *v = xw_select(kXF, cin, cout);
    return v ? v->window_rows : 0;
}

const char *dz_spconv_x_f32_variant(int cin, int cout) {
    const XWVariant *v = xw_select(kXF, cin, cout);
    return v ? v->name : "none";
}

int dz_spconv_forward_x_f32(const float *in, int in_rows, int cin, const int *nbr_packed, const int *perm, int *windows, int tile_rows,
                            int cap_out, const int *d_m_out, const float *w, const float *scale, const float *shift, const float *residual,
                            int relu, float *out, int cout, void *stream) {
    return xw_forward("dz_spconv_forward_x_f32", xw_select(kXF, cin, cout), (size_t)27 * cin * cout * sizeof(float), in, in_rows, cin, nbr_packed,
                      perm, windows, tile_rows, cap_out, d_m_out, w, scale, shift, residual, relu, out, cout, stream);
}

}  // extern "C"
