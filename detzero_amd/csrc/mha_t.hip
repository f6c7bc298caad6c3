// Multi-head attention core of the exact-fp32 mode on the bf16 matrix pipe with three-limb operands (opt-in engine 'bf16x3' of
// ops.mha_core; the default stays k_mha_core / k_mha_block of mha.hip on the fp32 MFMA), gfx950.
//
// Reference: refining/detzero_refine/models/modules/transformer/multi_head_attention.py:207-288.  The frame is k_mha_block_h's
// (mha_h.hip): a workgroup = one (batch, head), up to 8 waves of 32 queries; keys in blocks of 64 staged once per workgroup (double
// buffered, one barrier per block); S^T tiles of 32 keys x 32 queries whose registers ARE the B operand of the second product; online
// softmax in log2 units on v_exp_f32, running maximum / sum per query, rescale only when a maximum moved.  The arithmetic is limb3.h's:
// every operand is three exact bf16 limbs h + m + l, a product the six terms of limb3_terms (A limb . B limb, smallest first), fp32
// accumulation.
//   q        times scale * log2(e) in fp32 (one rounding, as k_mha_block), split once, in registers for the whole key loop;
//   K block  -> LDS as limb rows [key][h | m | l of the 32 channels] + 16 bytes of padding (row stride 13 x 16 bytes, odd: conflict-free
//               16-byte reads); the A operand of S^T = K . Q^T is one 16-byte read per limb;
//   V block  -> LDS transposed, three planes [limb][channel][key position] with k_mha_block_h's key permutation: the A operand of
//               O^T += V^T . P^T is one 16-byte read per limb;
//   p        = exp2(s - m) in fp32, split into three limbs in the lane that holds it.
// Both products take all six terms (with only h.h + h.m + m.h in P.V the host emulation leaves the fp32 error class: DESIGN.md), k-steps
// and keys ascending, no atomics: two launches agree bit for bit.  Masked keys: the score is REPLACED by -inf (their K rows may hold
// anything); keys at or beyond lk are dead and zero in K and V.
#include "limb3.h"

namespace dz {
namespace {

constexpr int AT_KEYS = 64;                                  // keys per staged block
constexpr int AT_KROW = 3 * 64 + 16;                         // K limb row: 32 channels x 3 limbs x 2 bytes + padding
constexpr int AT_VROW = 144;                                 // V^T plane row: 64 key positions x 2 bytes + padding
constexpr int AT_KT = AT_KEYS * AT_KROW, AT_VP = 32 * AT_VROW;
constexpr int AT_BUF = AT_KT + 3 * AT_VP + AT_KEYS, AT_LDS = 2 * AT_BUF;
static_assert((AT_KROW / 16) % 2 == 1 && (AT_VROW / 16) % 2 == 1, "odd slot strides: conflict-free ds_read_b128");
static_assert(AT_BUF % 16 == 0 && AT_LDS <= 80 * 1024, "two workgroups per CU");

__device__ __forceinline__ void split3f8(const float (&x)[8], v4u (&limb)[3]) {
    const v4u a = {__float_as_uint(x[0]), __float_as_uint(x[1]), __float_as_uint(x[2]), __float_as_uint(x[3])};
    const v4u c = {__float_as_uint(x[4]), __float_as_uint(x[5]), __float_as_uint(x[6]), __float_as_uint(x[7])};
    split3x8(a, c, limb[0], limb[1], limb[2]);
}

// 4 waves per SIMD = at most 128 registers: two 8-wave workgroups per CU (the LDS allows two as well)
template <bool MASK>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_mha_block_t(
    const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v, const uint8_t *__restrict__ kpm, int lq, int lk,
    int heads, float scale, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) unsigned char sm[AT_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int hd = blockIdx.y, b = blockIdx.z;
    const int e_dim = heads * 32;
    const int qi = (blockIdx.x * (blockDim.x >> 6) + wid) * 32 + l31;
    // B operand of S^T: Q[query l31][d = 16 s + 8 h .. + 7], scaled to log2 units, as three limbs (a wave without queries holds zeros)
    v4u ql[2][3];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (qi < lq) {
            const float4 a = *reinterpret_cast<const float4 *>(q + ((size_t)b * lq + qi) * e_dim + hd * 32 + s * 16 + h * 8);
            const float4 c = *reinterpret_cast<const float4 *>(q + ((size_t)b * lq + qi) * e_dim + hd * 32 + s * 16 + h * 8 + 4);
            const float sc2 = scale * 1.44269504088896340736f;
            x[0] = a.x * sc2; x[1] = a.y * sc2; x[2] = a.z * sc2; x[3] = a.w * sc2;
            x[4] = c.x * sc2; x[5] = c.y * sc2; x[6] = c.z * sc2; x[7] = c.w * sc2;
        }
        split3f8(x, ql[s]);
    }
    f32x16 o;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    const float *kb = k + (size_t)b * lk * e_dim + hd * 32, *vb = v + (size_t)b * lk * e_dim + hd * 32;
    const uint8_t *mb = MASK ? kpm + (size_t)b * lk : nullptr;
    // staging: thread (key = tid / 4, 8-channel group tid % 4) of the first 256 threads
    const bool stager = tid < 256;
    const int skey = tid >> 2, sg = tid & 3;
    // position of a key inside its 32-key tile in the V^T planes: key = 16 t + 8 g + 4 hh + r -> 16 t + 8 hh + 4 g + r
    const int spos = (skey & 32) | (skey & 16) | ((skey & 4) << 1) | ((skey & 8) >> 1) | (skey & 3);
    // a block is staged in two halves through the same eight registers: K (and the mask byte) under the block's first tile, V under its
    // second - with K and V both in flight the kernel needs more than 128 registers, and two workgroups no longer share a CU
    v4u stg[2];
    unsigned char mst = 1;
    auto fetch = [&](const float *src, int key0, bool with_mask) {
        if (!stager) return;
        const int key = key0 + skey;
        if (key < lk) {
            const float *p = src + (size_t)key * e_dim + sg * 8;
            stg[0] = *reinterpret_cast<const v4u *>(p); stg[1] = *reinterpret_cast<const v4u *>(p + 4);
            if (with_mask) mst = (MASK && sg == 0) ? mb[key] : 0;
        } else {
            stg[0] = stg[1] = v4u{0u, 0u, 0u, 0u};
            if (with_mask) mst = 1;
        }
    };
    // every K and V value is split ONCE per workgroup, on the way into LDS
    auto stash_k = [&](int buf) {
        if (!stager) return;
        unsigned char *base = sm + buf * AT_BUF;
        v4u kl[3];
        split3x8(stg[0], stg[1], kl[0], kl[1], kl[2]);
#pragma unroll
        for (int s = 0; s < 3; ++s) *reinterpret_cast<v4u *>(base + skey * AT_KROW + s * 64 + sg * 16) = kl[s];
        if (sg == 0) base[AT_KT + 3 * AT_VP + skey] = mst;
    };
    auto stash_v = [&](int buf) {
        if (!stager) return;
        unsigned char *base = sm + buf * AT_BUF;
        const unsigned int vw[8] = {stg[0].x, stg[0].y, stg[0].z, stg[0].w, stg[1].x, stg[1].y, stg[1].z, stg[1].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {                                        // channels 2 j (low halves) and 2 j + 1 of my group
            unsigned int vl[3];
            split3x2(__uint_as_float(vw[2 * j]), __uint_as_float(vw[2 * j + 1]), vl[0], vl[1], vl[2]);
            unsigned char *row = base + AT_KT + (sg * 8 + 2 * j) * AT_VROW + spos * 2;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                *reinterpret_cast<unsigned short *>(row + s * AT_VP) = (unsigned short)(vl[s] & 0xFFFFu);
                *reinterpret_cast<unsigned short *>(row + s * AT_VP + AT_VROW) = (unsigned short)(vl[s] >> 16);
            }
        }
    };
    const int nblocks = (lk + AT_KEYS - 1) / AT_KEYS;
    fetch(kb, 0, true);
    stash_k(0);
    fetch(vb, 0, false);
    stash_v(0);
    __syncthreads();
    for (int blk = 0; blk < nblocks; ++blk) {
        const int cur = blk & 1;
        const bool more = blk + 1 < nblocks;
        const unsigned char *base = sm + cur * AT_BUF;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            if (more) fetch(mt ? vb : kb, (blk + 1) * AT_KEYS, mt == 0);          // lands under this tile's MFMAs
            // ---- S^T tile: 32 keys x 32 queries, k-steps ascending, six terms each
            f32x16 s;
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const unsigned char *kp = base + (mt * 32 + l31) * AT_KROW + (2 * st + h) * 16;
                v4u kl[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) kl[i] = *reinterpret_cast<const v4u *>(kp + i * 64);
                limb3_terms([&](auto a, auto c) { s = MathBF16::mma(kl[a], ql[st][c], s); });
            }
            // lane (query l31, half h): s[i] = score of key 8 (i / 4) + 4 h + i % 4 of the tile
            unsigned int mw[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) mw[j] = *reinterpret_cast<const unsigned int *>(base + AT_KT + 3 * AT_VP + mt * 32 + 8 * j + 4 * h);
            float p[16], tmax = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const bool dead = ((mw[i >> 2] >> (8 * (i & 3))) & 0xFFu) != 0u;
                p[i] = dead ? -INFINITY : s[i];
                tmax = fmaxf(tmax, p[i]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float m_new = fmaxf(m_run, tmax);
            float alpha = 1.f, psum = 0.f;
            if (m_new != -INFINITY) {
                alpha = __builtin_amdgcn_exp2f(m_run - m_new);               // m_run = -inf -> 0
#pragma unroll
                for (int i = 0; i < 16; ++i) { p[i] = __builtin_amdgcn_exp2f(p[i] - m_new); psum += p[i]; }
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) p[i] = 0.f;
            }
            l_run = l_run * alpha + psum;                                    // in-lane partial over this half's keys; halves summed at the end
            m_run = m_new;
            if (!__all(alpha == 1.f)) {
#pragma unroll
                for (int i = 0; i < 16; ++i) o[i] *= alpha;
            }
            // ---- O^T += V^T . P^T: k-step t <-> the lane's registers 8 t .. 8 t + 7, split where they are
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float pv[8] = {p[8 * t], p[8 * t + 1], p[8 * t + 2], p[8 * t + 3], p[8 * t + 4], p[8 * t + 5], p[8 * t + 6], p[8 * t + 7]};
                v4u pl[3], vl[3];
                split3f8(pv, pl);
                const unsigned char *vp = base + AT_KT + l31 * AT_VROW + (mt * 32 + 16 * t + 8 * h) * 2;
#pragma unroll
                for (int i = 0; i < 3; ++i) vl[i] = *reinterpret_cast<const v4u *>(vp + i * AT_VP);
                limb3_terms([&](auto a, auto c) { o = MathBF16::mma(vl[a], pl[c], o); });
            }
            if (more) {                                // the other buffer was last read before the previous barrier
                if (mt) stash_v(cur ^ 1);
                else stash_k(cur ^ 1);
            }
        }
        __syncthreads();
    }
    const float l = l_run + __shfl_xor(l_run, 32, 64);
    if (qi < lq) {
        const float inv = 1.f / l;                     // fully masked row -> NaN, as torch.softmax gives
        float *dst = out + ((size_t)b * lq + qi) * e_dim + hd * 32;
#pragma unroll
        for (int j = 0; j < 4; ++j)                    // o[i] = O^T[d = 8 (i / 4) + 4 h + i % 4][query]
            *reinterpret_cast<float4 *>(dst + 8 * j + 4 * h) = make_float4(o[4 * j] * inv, o[4 * j + 1] * inv, o[4 * j + 2] * inv, o[4 * j + 3] * inv);
    }
}

// what keeps a call off the engine, or nullptr: the answer of dz_mha_core_limb3_supported and the refusal of dz_mha_core_limb3
const char *mha_t_refusal(int batch, int lq, int lk, int heads) {
    if (!(batch >= 0 && lq >= 0 && lk >= 1 && heads >= 1 && heads <= 65535 && batch <= 65535)) return "bad sizes";
    return nullptr;
}

}  // namespace
}  // namespace dz

using namespace dz;

extern "C" {

int dz_mha_core_limb3_supported(int batch, int lq, int lk, int heads) { return mha_t_refusal(batch, lq, lk, heads) ? 0 : 1; }

int dz_mha_core_limb3(const float *q, const float *k, const float *v, const uint8_t *key_padding_mask, int batch, int lq, int lk, int heads,
                      float scale, float *out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *why = mha_t_refusal(batch, lq, lk, heads);
    DZ_CHECK_ARG(!why, "dz_mha_core_limb3: %s", why);
    if (batch == 0 || lq == 0) return DZ_OK;
    DZ_CHECK_ARG(q && k && v && out, "dz_mha_core_limb3: null pointer");
    const int qw = (lq + 31) / 32, blocks = (qw + 7) / 8;
    int nw = (qw + blocks - 1) / blocks;
    if (nw < 4) nw = 4;                                // the first 256 threads stage the key blocks
    const dim3 grid(blocks, heads, batch);
    if (key_padding_mask)
        hipLaunchKernelGGL(k_mha_block_t<true>, grid, dim3(64 * nw), 0, stream, q, k, v, key_padding_mask, lq, lk, heads, scale, out);
    else
        hipLaunchKernelGGL(k_mha_block_t<false>, grid, dim3(64 * nw), 0, stream, q, k, v, key_padding_mask, lq, lk, heads, scale, out);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

}  // extern "C"
