// Submanifold 3 x 3 x 3 sparse convolution of the exact-fp32 mode on the bf16 matrix pipe ("x-run" engine, gfx950): fp32 rows in,
// every operand as THREE exact bf16 limbs (limb3.h: h = rn(x), m = rn(x - h), l = x - h - m), six v_mfma_f32_32x32x16_bf16 per
// product with fp32 accumulation, fp32 rows out.  The third arithmetic of sparse_conv_x.hip (pair16) / sparse_conv_xf.hip (fp32
// MFMA); reference call sites: detection/detzero_det/models/centerpoint_modules/backbone3d.py:93-121, :243-280.
//
// Why: per (tap, 32-channel fragment) k_spconv_xf issues 8 fp32 MFMAs of 64 cycles (512 cycles) for a 16-channel chunk; the six bf16
// terms   l.h  h.l  m.m  m.h  h.m  h.h   (weight limb . input limb, smallest first - the order of conv3x3_t.hip)
// are six MFMAs of 32 cycles (192 cycles) for the same chunk.  Dropped: m.l + l.m + l.l, at most 2^-26 of |x.w|.
// Tiny values: for |x| < 2^-100 the l limb (below 2^-109 the m limb too) is a bf16 subnormal.  Measured on an MI355X: the bf16 MFMA
// KEEPS subnormal inputs - with inputs of exponent [-120, -104] against one-hot weights every output equals (h + m + l) . w bit for
// bit, none the value with those limbs flushed (test_subnormal_limbs_are_measured).  Below 2^-110 the split itself
// stops being exact (bf16's quantum there is 2^-133): the result is then within 2^-133 |w| of x . w.
//
// Everything the index decides is k_spconv_xf's, from the frame both kernels share (sparse_conv_xw.h): the unit (WP x 32 rows =
// dz_spconv_x_tile_rows), the windows and the zero row behind them, the packed table words, the epilogue and the write contract, the
// checks of the entry point.  Written out here as there: the gather-mode arm for a window longer than RCAP (same taps, same order), the
// ballot skip of (fragment, tap) pairs, the operand mapping (lane (row l & 31, half l >> 5) holds channels 8 half .. 8 half + 7 of
// the chunk = the B operand of ONE 32x32x16 k-step; D[cout x row]).
//
// Where the split happens - form (B) of the two workable ones, at every width: the fp32 window stays in LDS exactly as k_spconv_xf
// stages it (direct loads, 64 bytes per row and chunk) and the 8 values of a fragment read are split in registers: 4 x split3x2 =
// 45 VALU instructions in the generated code (+ 8-16 accumulator moves around the ballot branch), ~210-250 issue cycles per (wave,
// tap), against 192 x CT MFMA cycles.  At CT = 2 (64 and 128 channels) the matrix pipe is the longer of the two; at CT = 1 (32
// channels) the kernel is VALU-bound on paper, still 2 x below k_spconv_xf's 512.  Form (A) (limb rows in LDS, split once per
// staged value) would remove that bound at 32 channels at the price of a register-staged window (96 B per row and chunk, no direct
// loads).  Measured (16 frames of 160k points, us per launch, gather kernel / k_spconv_xf / this kernel, same
// tensors, launches interleaved): 32 ch 1185 / 877 / 672, 64 ch 1545 / 1330 / 892, 128 ch 2130 / 2100 / 1865 - every width beats
// both, so form (B) ships at all three; a width that did not would be compiled out of the selector below (XT_SHIP_*).
//
//   weights   split at plan time (ops.pack_weight_limb3(w, cout_mult=32)): per tap, output channel and group of 8 input channels
//             48 bytes = 16 B of h, 16 of m, 16 of l - already the A operand: lane (cout l & 31, half) reads 3 x 16 B.  A tap's slice
//             of a 16-channel chunk is COUT rows x 96 bytes (6 pieces), fetched straight into LDS by `buffer_load_dwordx4 ... lds`
//             (lane L of run j fetches piece j * 64 + L; 96-byte segments of rows cin * 6 bytes apart).  LDS rows are unpadded
//             (direct loads write 1 KB contiguously), so source piece p of row co sits at slot (p - ((co >> 3) & 1)) mod 6: rows
//             co .. co + 7 then cover the even (or odd) 16-byte slots of a 256-byte bank line and rows co + 8 .. co + 15 the others -
//             conflict-free ds_read_b128 for 16 consecutive output channels.
//   step      TPS taps of a stage (tz, chunk kc): 3 (a window row ty, as k_spconv_xf) at 32 / 64 channels, 1 at 128.  Limb weights
//             are 1.5 x the fp32 bytes: a 3-tap step at 128 channels is 36 KB, 72 KB double buffered, which leaves a window of 48
//             rows inside the 80 KB at which TWO workgroups share a CU (k_spconv_xf measured that this matters; with MFMA time per
//             step 2.7 x shorter it matters more).  One tap per step is 12 KB, 24 KB double buffered: RCAP = 432.
//             The loads of step i + 1 are issued behind the MFMAs of step i's first tap; one `s_waitcnt vmcnt(0)` + barrier per step.
//   LDS       2 x (RCAP + 1) x 64 (windows + zero rows) + 2 x TPS x COUT x 96 (weights) <= 80 KB:
//                  32 ch: 2 x 481 x 64 + 2 x  9216 = 80000      64 ch: 2 x 337 x 64 + 2 x 18432 = 80000
//                 128 ch: 2 x 433 x 64 + 2 x 12288 = 80000
//
// Accumulation order per output element (fixed; independent of the unit a row falls into, of the mode of the stage and of scheduling):
//   tz = 0..2, 16-channel chunk kc, ty = 0..2, tx = 0..2, and per (tap, chunk) the six terms l.h, h.l, m.m, m.h, h.m, h.h, each one
//   MFMA k-step over the chunk's 16 channels added onto the element's ONE accumulator (absent taps add nothing; a tap skipped by the
//   ballot would have added exact zeros).  No atomics; two launches agree bit for bit.
#include <type_traits>

#include "limb3.h"
#include "sparse_conv_xw.h"

namespace dz {

template <int COUT_, int WP_, int WC_, int RCAP_, int TPS_>
struct XTCfg {
    static constexpr int COUT = COUT_, WP = WP_, WC = WC_, RCAP = RCAP_, TPS = TPS_;
    static constexpr int NW = WP * WC, THREADS = 64 * NW;
    static constexpr int CT = COUT / (32 * WC);              // 32-channel fragments per wave
    static constexpr int UR = WP * 32;                       // output rows per unit
    static constexpr int SPS = 9 / TPS;                      // steps per stage (tz, kc)
    static constexpr int WIN_BYTES = (RCAP + 1) * 64;        // + the zero row missing neighbours read
    static constexpr int TAP_BYTES = COUT * 96;              // limb slice of one tap: COUT rows x 2 groups of 8 input channels x 48 B
    static constexpr int WSTEP_BYTES = TPS * TAP_BYTES;
    static constexpr int OFF_WIN = 0, OFF_W = 2 * WIN_BYTES;
    static constexpr int LDS_BYTES = OFF_W + 2 * WSTEP_BYTES;
    static constexpr int TAP_RUNS = TAP_BYTES / 1024;        // 1 KB direct loads per tap slice
    static constexpr int WRUNS = TPS * TAP_RUNS;
    static_assert(COUT % (32 * WC) == 0 && RCAP % 16 == 0 && TAP_BYTES % 1024 == 0 && (TPS == 1 || TPS == 3), "shape");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
    static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");
};

template <class C>
__global__ __launch_bounds__(C::THREADS) void k_spconv_xt(SpConvXWArgs a) {
    constexpr int CT = C::CT, COUT = C::COUT, RCAP = C::RCAP, NW = C::NW, TPS = C::TPS, SPS = C::SPS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wc = wid % C::WC, l31 = lane & 31, kh = lane >> 5;
    const int m = min(*a.d_m_out, a.cap);
    if ((int)blockIdx.x * C::UR >= m) return;
    const srsrc_t crsrc = make_srsrc(a.w, a.w_bytes);
    const unsigned int in_rows = a.in_bytes / ((unsigned int)a.cin * 4u);
    const unsigned int wrow_bytes = (unsigned int)a.cin * 6u;           // a weight row: cin / 8 groups of 48 bytes
    XWUnit<C> u(a, smem, m, wid, lane);
    const int nsteps = u.nz * u.nk * SPS;

    // step i of a stage: r = window row ty (TPS == 3) or tap ty * 3 + tx (TPS == 1)
    // (through a lambda: with u.stage_of called in place the 128-channel kernel computes i / 9 once more per step body)
    auto stage_of = [&](int i, int &tz, int &kc, int &r) { u.stage_of(i, tz, kc, r); };
    auto issue = [&](int i) {
        if (i >= nsteps) return;
        int tz, kc, r;
        stage_of(i, tz, kc, r);
        // limb weights of the step's taps: tap tz*9 + ty*3 + tx, all COUT rows, the two 48-byte groups of input channels [kc*16, kc*16 + 16).
        // Slot d = part * 64 + lane of a tap slice = (row d / 6, slot d % 6), which holds source piece (slot + ((row >> 3) & 1)) mod 6
        const unsigned int wbuf = (unsigned int)(C::OFF_W + (i & 1) * C::WSTEP_BYTES);
        const int tap0 = tz * 9 + (TPS == 3 ? r * 3 : r);
        for (int j = wid; j < C::WRUNS; j += NW) {
            const int t = j / C::TAP_RUNS, part = j - t * C::TAP_RUNS;
            const int d = part * 64 + lane, co = d / 6, q = d - co * 6;
            int p = q + ((co >> 3) & 1);
            p = p >= 6 ? p - 6 : p;
            const unsigned int voff = (unsigned int)co * wrow_bytes + (unsigned int)p * 16u;
            const unsigned int src = (unsigned int)((tap0 + t) * COUT) * wrow_bytes + (unsigned int)(kc * 96);
            load16_lds(wbuf + (unsigned int)j * 1024u, voff, crsrc, src);
        }
        // the window of the stage, at its first step (a window beyond RCAP rows is not staged: gather mode)
        const int n = xw_pick(u.wn, tz);
        if (r == 0 && n <= RCAP) {
            const int lo = xw_pick(u.wlo, tz);
            const int nruns = (n + 15) >> 4;
            for (int j = wid; j < nruns; j += NW) u.load_window_run(i / SPS, j, lo, n, kc);
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

    // my weight row of a tap slice and the slots of its three limbs (h, m, l of input channels 8 kh .. 8 kh + 7 of the chunk)
    const int rot = (l31 >> 3) & 1;
    const unsigned int wrow = (unsigned int)((wc * CT * 32 + l31) * 96);
    const unsigned int wslot_h = wrow + (unsigned int)((kh * 3 + 6 - rot) % 6) * 16u, wslot_m = wrow + (unsigned int)((kh * 3 + 7 - rot) % 6) * 16u,
                       wslot_l = wrow + (unsigned int)((kh * 3 + 8 - rot) % 6) * 16u;
    // one step: TPS taps.  GM (gather mode) is a compile-time copy of the body: with both operand paths in one body the compiler's
    // wait-count pass puts the global loads' `s_waitcnt vmcnt(0)` in front of every tap's MFMAs, which in the staged mode would wait
    // for the NEXT step's direct loads as well
    auto step = [&](int i, auto gm_t) {
        constexpr bool GM = decltype(gm_t)::value;
        int tz, kc, r;
        stage_of(i, tz, kc, r);
        const int ty = TPS == 3 ? r : r / 3;
        const int lo = xw_pick(u.wlo, tz), n = xw_pick(u.wn, tz);
        const int line = tz * 3 + ty;
        unsigned int e = u.pw[0];
#pragma unroll
        for (int g = 1; g < 9; ++g) {
            e = line == g ? u.pw[g] : e;
            asm volatile("" : "+v"(e));          // (a chain of selects, not an indexed read of the table words: that would move them to scratch)
        }
        const int rank = (int)(e & 0x1FFFFFFFu);
        const unsigned char *const wbuf = smem + C::OFF_W + (i & 1) * C::WSTEP_BYTES;
        const unsigned char *const winb = smem + C::OFF_WIN + ((i / SPS) & 1) * C::WIN_BYTES;
        auto tap = [&](int t, int tx) {
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
            const unsigned char *const wt = wbuf + t * C::TAP_BYTES;
            v4u w[3][CT], x[3];                              // limb operands: h, m, l
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                w[0][ct] = *reinterpret_cast<const v4u *>(wt + ct * 32 * 96 + wslot_h);
                w[1][ct] = *reinterpret_cast<const v4u *>(wt + ct * 32 * 96 + wslot_m);
                w[2][ct] = *reinterpret_cast<const v4u *>(wt + ct * 32 * 96 + wslot_l);
            }
            // the 8 channels of my half of the chunk, split here; term-major, so consecutive MFMAs go to different accumulators
            split3x8(__builtin_bit_cast(v4u, x0), __builtin_bit_cast(v4u, x1), x[0], x[1], x[2]);
            limb3_terms([&](auto wl, auto xl) {
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[ct] = MathBF16::mma(w[wl][ct], x[xl], acc[ct]);
            });
        };
        // the next step's loads go out behind the first tap's MFMAs: no barrier is followed by address arithmetic and load issue in
        // front of a cold matrix pipe
        if constexpr (TPS == 3) {
            tap(0, 0);
            issue(i + 1);
            tap(1, 1);
            tap(2, 2);
        } else {
            tap(0, r - ty * 3);
            issue(i + 1);
        }
    };
    for (int i = 0; i < nsteps; ++i) {
        int tz, kc, r;
        stage_of(i, tz, kc, r);
        if (xw_pick(u.wn, tz) > RCAP) step(i, std::true_type{});
        else step(i, std::false_type{});
        // the next step's loads have landed, and everyone is done with the buffers the loads issued next will overwrite
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    xw_epilogue<C>(a, acc, u.pos, m, wc, kh);
}

// unit rows = dz_spconv_x_tile_rows of the pair16 engine's shipped configurations (one index serves every arithmetic)
// RCAP: the largest window with which TWO workgroups share a CU's 160 KB of LDS (the budget in the file header)
using XT32 = XTCfg<32, 8, 1, 480, 3>;
using XT64 = XTCfg<64, 8, 1, 336, 3>;
using XT128 = XTCfg<128, 4, 2, 432, 1>;

// Which widths the selector offers: a width ships only where it measured faster than BOTH existing fp32 kernels of its layer (the gather
// kernel and k_spconv_xf; DESIGN.md 2h-bis has the numbers).  A width that is off has no row below and no kernel instance; it reports
// 0 window rows and "none": the backbone keeps such a layer on k_spconv_xf.
#define XT_SHIP_32 1
#define XT_SHIP_64 1
#define XT_SHIP_128 1

static const XWVariant kXT[] = {
#if XT_SHIP_32
    {32, XT32::UR, XT32::RCAP, "k_spconv_xt<32>", launch_xw<k_spconv_xt<XT32>, XT32>},
#endif
#if XT_SHIP_64
    {64, XT64::UR, XT64::RCAP, "k_spconv_xt<64>", launch_xw<k_spconv_xt<XT64>, XT64>},
#endif
#if XT_SHIP_128
    {128, XT128::UR, XT128::RCAP, "k_spconv_xt<128>", launch_xw<k_spconv_xt<XT128>, XT128>},
#endif
};

}  // namespace dz

using namespace dz;

extern "C" {

int dz_spconv_x_limb3_window_rows(int cin, int cout) {
    const XWVariant *v = xw_select(kXT, cin, cout);
    return v ? v->window_rows : 0;
}

const char *dz_spconv_x_limb3_variant(int cin, int cout) {
    const XWVariant *v = xw_select(kXT, cin, cout);
    return v ? v->name : "none";
}

int dz_spconv_forward_x_limb3(const float *in, int in_rows, int cin, const int *nbr_packed, const int *perm, int *windows, int tile_rows,
                              int cap_out, const int *d_m_out, const float *w, const float *scale, const float *shift, const float *residual,
                              int relu, float *out, int cout, void *stream) {
    return xw_forward("dz_spconv_forward_x_limb3", xw_select(kXT, cin, cout), (size_t)27 * cout * cin * 6, in, in_rows, cin, nbr_packed, perm,
                      windows, tile_rows, cap_out, d_m_out, w, scale, shift, residual, relu, out, cout, stream);
}

}  // extern "C"
