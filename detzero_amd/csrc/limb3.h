// The three-limb arithmetic of the exact-fp32 mode's bf16x3 engines (conv3x3_t.hip, conv2d_t.hip, linear_t.hip, sparse_conv_xt.hip,
// sparse_conv_gt.hip, sparse_conv_wt.hip): any finite fp32 x is exactly
//        h = rn(x),   m = rn(x - h),   l = x - h - m                      (three bf16 values, 8 + 8 + 8 = 24 significant bits)
// with x clamped to +-bf16-max (0x7F7F) before the FIRST rounding only (the rule of MathF16::split): a finite fp32 near the top of
// the range gets no inf limb, the rest goes to m and l, and the sum stays exact.  The host mirror is ops.limb3_pack.
// Below the split: the order of the six limb products (limb3_terms) and the LDS tile of limb rows that k_spconv_gt, k_conv2d_t and
// k_linear_t stage their chunks into and multiply from (Limb3Tile and the limb3_* function templates on it).
#pragma once

#include <type_traits>

#include "hgemm.h"

namespace dz {

constexpr float T3_BF16_MAX = 3.3895313892515355e38f;            // 0x7F7F0000

// two fp32 values -> their three bf16 limbs, packed (a in the low half): split2<MathBF16> with the clamp in front and one more
// remainder step
__device__ __forceinline__ void split3x2(float a, float b, unsigned int &h, unsigned int &m, unsigned int &l) {
    const f32x2v x = {a, b};
    const f32x2v xc = {__builtin_amdgcn_fmed3f(a, -T3_BF16_MAX, T3_BF16_MAX), __builtin_amdgcn_fmed3f(b, -T3_BF16_MAX, T3_BF16_MAX)};
    h = __builtin_bit_cast(unsigned int, __builtin_convertvector(xc, b2_t));
    const f32x2v r1 = x - f32x2v{__uint_as_float(h << 16), __uint_as_float(h & 0xFFFF0000u)};
    m = __builtin_bit_cast(unsigned int, __builtin_convertvector(r1, b2_t));
    const f32x2v r2 = r1 - f32x2v{__uint_as_float(m << 16), __uint_as_float(m & 0xFFFF0000u)};
    l = __builtin_bit_cast(unsigned int, __builtin_convertvector(r2, b2_t));
}

// eight consecutive fp32 channels (two 16-byte quads, as loaded) -> one MFMA operand per limb: two channels per word, the first in
// the low half
__device__ __forceinline__ void split3x8(const v4u &x0, const v4u &x1, v4u &xh, v4u &xm, v4u &xl) {
    unsigned int h0, h1, h2, h3, m0, m1, m2, m3, l0, l1, l2, l3;
    split3x2(__uint_as_float(x0.x), __uint_as_float(x0.y), h0, m0, l0);
    split3x2(__uint_as_float(x0.z), __uint_as_float(x0.w), h1, m1, l1);
    split3x2(__uint_as_float(x1.x), __uint_as_float(x1.y), h2, m2, l2);
    split3x2(__uint_as_float(x1.z), __uint_as_float(x1.w), h3, m3, l3);
    xh = v4u{h0, h1, h2, h3};
    xm = v4u{m0, m1, m2, m3};
    xl = v4u{l0, l1, l2, l3};
}

// The six products of a bf16x3 multiplication in the order every engine adds them: term(weight limb, input limb) with limb 0 = h,
// 1 = m, 2 = l as compile-time values,
//        l.h  h.l  m.m  m.h  h.m  h.h          (smallest first; dropped: m.l + l.m + l.l, at most 2^-26 of |x.w|)
// The caller's term runs over all of its accumulators (term-major), so that consecutive MFMAs go to different accumulators.
template <class F>
__device__ __forceinline__ void limb3_terms(F &&term) {
    constexpr std::integral_constant<int, 0> H{};
    constexpr std::integral_constant<int, 1> M{};
    constexpr std::integral_constant<int, 2> L{};
    term(L, H);
    term(H, L);
    term(M, M);
    term(M, H);
    term(H, M);
    term(H, H);
}

// ---- the limb tile of k_spconv_gt / k_conv2d_t / k_linear_t: BP rows (MFMA N side) x BC output channels (MFMA M side), KC channels of one tap per
// chunk, WP x WC waves.  An LDS row is KC / 8 groups of 48 bytes (16 B of h, 16 of m, 16 of l of 8 channels: the group layout of
// conv3x3_t.hip and of the packed weights) + 16 bytes of padding; two buffers of BP input rows, two of BC weight rows.
template <int BP_, int BC_, int KC_, int WP_, int WC_>
struct Limb3Tile {
    static constexpr int BP = BP_, BC = BC_, KC = KC_, WP = WP_, WC = WC_;
    static constexpr int THREADS = 64 * WP * WC;
    static constexpr int PT = BP / (32 * WP);               // 32-row fragments per wave
    static constexpr int CT = BC / (32 * WC);               // 32-channel fragments per wave
    static constexpr int G = KC / 8;                        // 48-byte limb groups per LDS row
    static constexpr int ROWB = G * 48 + 16;                // LDS row stride
    static constexpr int P_PER_THREAD = BP * G / THREADS;   // 8-channel groups of the input chunk per thread
    static constexpr int C_PIECES = BC * G * 3;             // 16-byte pieces of a chunk's weight slice
    static constexpr int C_PER_THREAD = (C_PIECES + THREADS - 1) / THREADS;
    static constexpr int PS_BYTES = BP * ROWB, CS_BYTES = BC * ROWB;
    static constexpr int LDS_BYTES = 2 * (PS_BYTES + CS_BYTES);
    static_assert(KC == 16 || KC == 32, "KC is one or two 16-deep MFMA steps");
    static_assert(BP % (32 * WP) == 0 && BC % (32 * WC) == 0 && (BP * G) % THREADS == 0, "tile must split into 32x32 fragments and whole groups per thread");
    static_assert((ROWB / 16) % 2 == 1, "odd slot stride: conflict-free ds_read_b128");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

constexpr unsigned int LIMB3_NO_PIECE = 0xFFFFFFFFu;

// My pieces of a chunk's weight slice: packed row n0 + n of the tile's BC channels (rows at or beyond `rows` read as zeros), 16-byte
// piece q of its KC / 8 groups -> byte offset inside a (tap, channel slice) of the packed weights, byte offset in an LDS weight buffer
template <class T>
__device__ __forceinline__ void limb3_weight_pieces(int tid, int n0, int rows, unsigned int wrow_bytes, unsigned int (&cvoff)[T::C_PER_THREAD],
                                                    unsigned int (&clds)[T::C_PER_THREAD]) {
#pragma unroll
    for (int i = 0; i < T::C_PER_THREAD; ++i) {
        const int idx = tid + i * T::THREADS;
        const int n = idx / (T::G * 3), q = idx % (T::G * 3);
        const bool own = T::C_PIECES % T::THREADS == 0 || idx < T::C_PIECES;
        cvoff[i] = own && n0 + n < rows ? (unsigned int)(n0 + n) * wrow_bytes + (unsigned int)q * 16u : OOB_OFFSET;
        clds[i] = own ? (unsigned int)(n * T::ROWB + q * 16) : LIMB3_NO_PIECE;
    }
}

// Fragment address inside an LDS buffer: my row (lane & 31) of the first of the FT fragments of wave w, limb group lane >> 5 of a k-step
template <class T>
__device__ __forceinline__ int limb3_frag_base(int w, int FT, int lane) { return (w * FT * 32 + (lane & 31)) * T::ROWB + (lane >> 5) * 48; }

template <class T>
__device__ __forceinline__ void limb3_zero(f32x16 (&acc)[T::CT][T::PT]) {
#pragma unroll
    for (int i = 0; i < T::CT; ++i)
#pragma unroll
        for (int j = 0; j < T::PT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
}

// A staged chunk -> LDS: every input value is split ONCE here (sp[i]: the two quads of my i-th 8-channel group, to byte plds[i] of the
// input buffer Ps); the weight pieces sw go verbatim to bytes clds of the weight buffer Cs
template <class T>
__device__ __forceinline__ void limb3_store(unsigned char *Ps, unsigned char *Cs, const v4u (&sp)[T::P_PER_THREAD][2], const v4u (&sw)[T::C_PER_THREAD],
                                            const unsigned int (&plds)[T::P_PER_THREAD], const unsigned int (&clds)[T::C_PER_THREAD]) {
#pragma unroll
    for (int i = 0; i < T::P_PER_THREAD; ++i) {
        v4u *const d = reinterpret_cast<v4u *>(Ps + plds[i]);
        split3x8(sp[i][0], sp[i][1], d[0], d[1], d[2]);
    }
#pragma unroll
    for (int i = 0; i < T::C_PER_THREAD; ++i)
        if (T::C_PIECES % T::THREADS == 0 || clds[i] != LIMB3_NO_PIECE) *reinterpret_cast<v4u *>(Cs + clds[i]) = sw[i];
}

// The MFMAs of one chunk: Pc / Cc = the current input / weight buffer + the wave's limb3_frag_base.  Per 16-channel k-step, ascending:
// 3 x 16 B per operand fragment, then the six terms of limb3_terms over the wave's CT x PT accumulators.  (With CT = PT = 1 the six
// MFMAs are one dependent chain per wave, and only the other waves of the SIMD fill its gaps.)  Fenced, so that the loads the caller
// issued in front stay in front and its LDS writes stay behind.
template <class T>
__device__ __forceinline__ void limb3_mma(const unsigned char *Pc, const unsigned char *Cc, f32x16 (&acc)[T::CT][T::PT]) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < T::KC / 16; ++q) {
        v4u x[3][T::PT], w[3][T::CT];
#pragma unroll
        for (int pt = 0; pt < T::PT; ++pt)
#pragma unroll
            for (int s = 0; s < 3; ++s) x[s][pt] = reinterpret_cast<const v4u *>(Pc + pt * 32 * T::ROWB + q * 96)[s];
#pragma unroll
        for (int ct = 0; ct < T::CT; ++ct)
#pragma unroll
            for (int s = 0; s < 3; ++s) w[s][ct] = reinterpret_cast<const v4u *>(Cc + ct * 32 * T::ROWB + q * 96)[s];
        limb3_terms([&](auto wl, auto xl) {
#pragma unroll
            for (int ct = 0; ct < T::CT; ++ct)
#pragma unroll
                for (int pt = 0; pt < T::PT; ++pt) acc[ct][pt] = MathBF16::mma(w[wl][ct], x[xl][pt], acc[ct][pt]);
        });
    }
    __builtin_amdgcn_sched_barrier(0);
}

}  // namespace dz
