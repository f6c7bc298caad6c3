// The three-limb split of the exact-fp32 mode's bf16x3 engines (conv3x3_t.hip, sparse_conv_xt.hip): any finite fp32 x is exactly
//        h = rn(x),   m = rn(x - h),   l = x - h - m                      (three bf16 values, 8 + 8 + 8 = 24 significant bits)
// with x clamped to +-bf16-max (0x7F7F) before the FIRST rounding only (the rule of MathF16::split): a finite fp32 near the top of
// the range gets no inf limb, the rest goes to m and l, and the sum stays exact.  The host mirror is ops.limb3_pack.
#pragma once

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

}  // namespace dz
