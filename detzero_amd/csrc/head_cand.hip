// The regression branches of the CenterHead (center, center_z, dim, rot: center_head.py:14-48) evaluated at the top-K candidate
// cells only, instead of over the whole BEV map.
//
// The decode reads columns 0:8 of the head map at the K selected cells of a frame (500 of 35,344 at the Waymo size); dense, their
// two layers - 64 -> 64 per branch 3x3 + BatchNorm + ReLU, then 64 -> 1..3 3x3 - were computed, written and read back at every cell.
// Here a workgroup takes 32 candidates of one frame and ONE branch:
//   * hidden layer: wave ty (3 waves) owns the hidden pixels (ty, 0..2) of the candidates' 3 x 3 neighbourhoods.  A 32-wide MFMA
//     fragment is "hidden pixel (ty, tx) of candidates 0..31": its operand for tap (ky, kx) is the shared-map pixel at the
//     candidate's cell + (ty + ky - 2, tx + kx - 2), 32 contiguous bytes (hi | lo of the lane's 8 channels) straight from memory;
//     the weight rows are the MFMA's other operand, straight from memory too (the 147 KB of a branch stay in L2 / L1).
//   * the hidden values are rounded to pair16 exactly as the dense epilogue stores them and kept in LDS (9 x 32 x 64 values);
//     a hidden pixel outside the image is ZERO - the dense hidden map is zero-bordered - and none of its taps is read (they would
//     leave the shared map's own border).
//   * output layer: wave 0, fragment = the 32 candidates, operand of tap t = hidden pixel t from LDS; fp32 result into columns
//     g_ooff .. of the candidate's head row.
// Every output value is accumulated in the order of k_conv3x3_h / k_conv2d_h (32-channel chunks outermost, the nine taps inside, two
// 16-deep k steps, lo.hi + hi.lo + hi.hi on v_mfma_f32_32x32x16 with the same lane -> k assignment), so it is the dense value bit for bit.
#include "hgemm.h"

namespace dz {

constexpr int HC_C = 64;                        // shared-map channels = hidden channels per branch
constexpr int HC_CAND = 32;                     // candidates per workgroup (one MFMA fragment)
constexpr int HC_THREADS = 192;                 // 3 waves: hidden rows ty = 0..2
constexpr int HC_PIX_BYTES = HC_C * 4;          // pair16 row of a pixel
constexpr int HC_HROW = HC_PIX_BYTES + 16;      // LDS row of a hidden pixel (padded: conflict-free 16-byte reads)
constexpr int HC_LDS_BYTES = 9 * HC_CAND * HC_HROW;
constexpr int HC_MAX_BRANCH = 4;

struct HcArgs {
    const unsigned char *shared;
    const unsigned long long *cand;
    const int *ncand;
    const unsigned char *w1, *w2;
    const float *s1, *b1, *s2, *b2;
    float *head;
    int h, w, k, cand_stride, w1_cout;
    int g_cout[HC_MAX_BRANCH], g_ooff[HC_MAX_BRANCH];
};

template <class M>
__global__ __launch_bounds__(HC_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_head_at_cand(HcArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hid_s[];          // [9][32][HC_HROW]
    const int tid = threadIdx.x, lane = tid & 63, ty = tid >> 6;
    const int n = lane & 31, hh = lane >> 5;
    const int g = blockIdx.y, b = blockIdx.z;
    const int hw = a.h * a.w, hp = a.h + 2, wp = a.w + 2;
    const int ncand = min(min(a.ncand[b], a.k), a.cand_stride);
    const int slot = blockIdx.x * HC_CAND + n;
    if (blockIdx.x * HC_CAND >= ncand) return;                  // (whole workgroup)
    const bool live = slot < ncand;
    int pix = 0, y = 0, x = 0;
    if (live) {
        const unsigned long long e = a.cand[(size_t)b * a.cand_stride + slot];
        const uint32_t flat = 0xFFFFFFFFu - (uint32_t)(e & 0xFFFFFFFFull);
        pix = (int)(flat % (uint32_t)hw);
        y = pix / a.w;
        x = pix - y * a.w;
    }
    // hidden pixel (ty, tx) of my candidate: image cell (y + ty - 1, x + tx - 1); tap (ky, kx) reads padded pixel (hy + ky, hx + kx)
    const int hy = y + ty - 1;
    bool ok[3];
    const unsigned char *base[3];
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) {
        const int hx = x + tx - 1;
        ok[tx] = live && hy >= 0 && hy < a.h && hx >= 0 && hx < a.w;
        base[tx] = a.shared + (ok[tx] ? (((size_t)b * hp + hy) * wp + hx) * HC_PIX_BYTES : (size_t)0);
    }
    f32x16 acc[2][3];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int tx = 0; tx < 3; ++tx)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ct][tx][e] = 0.f;
    const v4u zero4 = {0u, 0u, 0u, 0u};
    const unsigned char *const wrow = a.w1 + ((size_t)(g * HC_C + n) * HC_C) * 4;           // my weight row of tap 0, fragment 0
    const size_t w_tap = (size_t)a.w1_cout * HC_C * 4, w_ct = (size_t)32 * HC_C * 4;
    for (int kc = 0; kc < HC_C / 32; ++kc) {
#pragma unroll
        for (int s = 0; s < 9; ++s) {
            const int ky = s / 3, kx = s - ky * 3;
            const size_t toff = (size_t)(ky * wp + kx) * HC_PIX_BYTES;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int koff = kc * 128 + q * 64 + hh * 32;          // 16 bytes of hi, then 16 of lo, of my 8 channels
                v4u c_hi[2], c_lo[2], p_hi[3], p_lo[3];
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const unsigned char *wpn = wrow + s * w_tap + ct * w_ct + koff;
                    c_hi[ct] = *reinterpret_cast<const v4u *>(wpn);
                    c_lo[ct] = *reinterpret_cast<const v4u *>(wpn + 16);
                }
#pragma unroll
                for (int tx = 0; tx < 3; ++tx) {
                    p_hi[tx] = p_lo[tx] = zero4;
                    if (ok[tx]) {
                        const unsigned char *pp = base[tx] + toff + koff;
                        p_hi[tx] = *reinterpret_cast<const v4u *>(pp);
                        p_lo[tx] = *reinterpret_cast<const v4u *>(pp + 16);
                    }
                }
                // every accumulator receives lo.hi, hi.lo, hi.hi in that order, as in the dense kernels
#pragma unroll
                for (int term = 3 - M::TERMS; term < 3; ++term)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                        for (int tx = 0; tx < 3; ++tx)
                            acc[ct][tx] = M::mma(term == 0 ? c_lo[ct] : c_hi[ct], term == 1 ? p_lo[tx] : p_hi[tx], acc[ct][tx]);
            }
        }
    }
    // ---- hidden epilogue: BatchNorm, ReLU, pair16 split; accumulator register 4j + e = channel 8j + 4hh + e of the fragment
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) {
        unsigned char *const row = hid_s + ((ty * 3 + tx) * HC_CAND + n) * HC_HROW;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ch = g * HC_C + ct * 32 + 8 * j + 4 * hh;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(fmaf(acc[ct][tx][4 * j + e], a.s1[ch + e], a.b1[ch + e]), 0.f);
                uint2 hi, lo;
                split4<M>(v, hi, lo);
                if (!ok[tx]) hi = lo = make_uint2(0u, 0u);
                unsigned char *d = row + (ct * 4 + j) * 32 + hh * 8;
                *reinterpret_cast<uint2 *>(d) = hi;
                *reinterpret_cast<uint2 *>(d + 16) = lo;
            }
        }
    }
    __syncthreads();
    if (ty != 0) return;
    // ---- output layer of the branch: D[32 padded columns x 32 candidates]
    f32x16 out;
#pragma unroll
    for (int e = 0; e < 16; ++e) out[e] = 0.f;
    const unsigned char *const w2row = a.w2 + ((size_t)(g * 9 * 32 + n) * HC_C) * 4;
    for (int kc = 0; kc < HC_C / 32; ++kc) {
#pragma unroll
        for (int s = 0; s < 9; ++s) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int koff = kc * 128 + q * 64 + hh * 32;
                const unsigned char *wpn = w2row + (size_t)s * 32 * HC_C * 4 + koff;
                const v4u c_hi = *reinterpret_cast<const v4u *>(wpn), c_lo = *reinterpret_cast<const v4u *>(wpn + 16);
                const unsigned char *pp = hid_s + (s * HC_CAND + n) * HC_HROW + koff;
                const v4u p_hi = *reinterpret_cast<const v4u *>(pp), p_lo = *reinterpret_cast<const v4u *>(pp + 16);
                if constexpr (M::TERMS == 3) {
                    out = M::mma(c_lo, p_hi, out);
                    out = M::mma(c_hi, p_lo, out);
                }
                out = M::mma(c_hi, p_hi, out);
            }
        }
    }
    if (live && hh == 0) {
        float *o = a.head + ((size_t)b * hw + pix) * 12 + a.g_ooff[g];
        const int gc = a.g_cout[g];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e < gc) o[e] = fmaf(out[e], a.s2 ? a.s2[g * 32 + e] : 1.f, a.b2 ? a.b2[g * 32 + e] : 0.f);
        }
    }
}


// ---- fp32 (DZ_MATH_F32): the same decomposition on v_mfma_f32_16x16x4_f32, in the order of k_conv2d (conv2d.hip / igemm.h): taps
// outermost, 32-channel chunks inside, two 16-deep slices, step e of a slice = channel 16q + 4 (lane >> 4) + e; pixels on the
// MFMA's row side, output channels on its column side.  A workgroup takes 16 candidates and one branch; plain fp32 hidden values.
constexpr int HF_CAND = 16;
constexpr int HF_HROW = HC_C + 4;              // floats per LDS row of a hidden pixel

__global__ __launch_bounds__(HC_THREADS) void k_head_at_cand_f32(HcArgs a) {
    __shared__ __attribute__((aligned(16))) float hid_s[9 * HF_CAND * HF_HROW];
    __shared__ int pix_s[HF_CAND];             // cell of candidate c, -1: none
    __shared__ int ok_s[3][HF_CAND];           // bit tx: hidden pixel (ty, tx) of candidate c lies in the image
    const int tid = threadIdx.x, lane = tid & 63, ty = tid >> 6;
    const int r = lane & 15, g4 = lane >> 4;
    const int br = blockIdx.y, b = blockIdx.z;
    const int hw = a.h * a.w, hp = a.h + 2, wp = a.w + 2;
    const int ncand = min(min(a.ncand[b], a.k), a.cand_stride);
    if (blockIdx.x * HF_CAND >= ncand) return;                  // (whole workgroup)
    const int slot = blockIdx.x * HF_CAND + r;
    const bool live = slot < ncand;
    int pix = 0, y = 0, x = 0;
    if (live) {
        const unsigned long long e = a.cand[(size_t)b * a.cand_stride + slot];
        const uint32_t flat = 0xFFFFFFFFu - (uint32_t)(e & 0xFFFFFFFFull);
        pix = (int)(flat % (uint32_t)hw);
        y = pix / a.w;
        x = pix - y * a.w;
    }
    const int hy = y + ty - 1;
    bool ok[3];
    const float *base[3];
    int okm = 0;
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) {
        const int hx = x + tx - 1;
        ok[tx] = live && hy >= 0 && hy < a.h && hx >= 0 && hx < a.w;
        okm |= ok[tx] ? 1 << tx : 0;
        base[tx] = reinterpret_cast<const float *>(a.shared) + (ok[tx] ? (((size_t)b * hp + hy) * wp + hx) * HC_C : (size_t)0);
    }
    if (lane < HF_CAND) {
        ok_s[ty][lane] = okm;
        if (ty == 0) pix_s[lane] = live ? pix : -1;
    }
    __syncthreads();
    f32x4 acc[3][4];
#pragma unroll
    for (int tx = 0; tx < 3; ++tx)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[tx][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float *const w1 = reinterpret_cast<const float *>(a.w1) + br * HC_C + r;          // (9, 64, w1_cout): my column of fragment 0
    for (int s = 0; s < 9; ++s) {
        const int ky = s / 3, kx = s - ky * 3;
        const size_t toff = (size_t)(ky * wp + kx) * HC_C;
#pragma unroll
        for (int kq = 0; kq < HC_C / 16; ++kq) {                 // (chunk, slice) pairs in order
            const int k0 = kq * 16 + g4 * 4;
            f32x4 av[3];
#pragma unroll
            for (int tx = 0; tx < 3; ++tx) {
                av[tx] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (ok[tx]) av[tx] = *reinterpret_cast<const f32x4 *>(base[tx] + toff + k0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float bv[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) bv[nt] = w1[((size_t)s * HC_C + k0 + e) * a.w1_cout + nt * 16];
#pragma unroll
                for (int tx = 0; tx < 3; ++tx)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) acc[tx][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tx][e], bv[nt], acc[tx][nt], 0, 0, 0);
            }
        }
    }
    // accumulator element e = candidate 4 g4 + e, channel 16 nt + r
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int ch = br * HC_C + nt * 16 + r;
        const float sc = a.s1[ch], sh = a.b1[ch];
#pragma unroll
        for (int tx = 0; tx < 3; ++tx)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = 4 * g4 + e;
                const float v = fmaxf(fmaf(acc[tx][nt][e], sc, sh), 0.f);
                hid_s[((ty * 3 + tx) * HF_CAND + c) * HF_HROW + nt * 16 + r] = ((ok_s[ty][c] >> tx) & 1) ? v : 0.f;
            }
    }
    __syncthreads();
    if (ty != 0) return;
    f32x4 out = {0.f, 0.f, 0.f, 0.f};
    const float *const w2 = reinterpret_cast<const float *>(a.w2) + (size_t)br * 9 * HC_C * 16 + r;      // (groups, 9, 64, 16)
    for (int s = 0; s < 9; ++s) {
#pragma unroll
        for (int kq = 0; kq < HC_C / 16; ++kq) {
            const int k0 = kq * 16 + g4 * 4;
            const f32x4 av = *reinterpret_cast<const f32x4 *>(hid_s + (s * HF_CAND + r) * HF_HROW + k0);
#pragma unroll
            for (int e = 0; e < 4; ++e) out = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], w2[((size_t)s * HC_C + k0 + e) * 16], out, 0, 0, 0);
        }
    }
    if (r < a.g_cout[br]) {
        const float sc = a.s2 ? a.s2[br * 16 + r] : 1.f, sh = a.b2 ? a.b2[br * 16 + r] : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int px = pix_s[4 * g4 + e];
            if (px >= 0) a.head[((size_t)b * hw + px) * 12 + a.g_ooff[br] + r] = fmaf(out[e], sc, sh);
        }
    }
}

template <class M>
static int launch_head_at_cand(const HcArgs &a, int batch, int nbranch, hipStream_t stream) {
    static PerDeviceFlags lds_done;
    if (int rc_ = reserve_lds(reinterpret_cast<const void *>(&k_head_at_cand<M>), HC_LDS_BYTES, lds_done, "dz_head_at_candidates")) return rc_;
    hipLaunchKernelGGL((k_head_at_cand<M>), dim3(ceil_div(a.k, HC_CAND), nbranch, batch), dim3(HC_THREADS), HC_LDS_BYTES, stream, a);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

}  // namespace dz

using namespace dz;

extern "C" {

int dz_head_at_candidates_supported(int math, int channels) {
    return (math == DZ_MATH_F32 || math == DZ_MATH_F16X2 || math == DZ_MATH_BF16X2 || math == DZ_MATH_F16) && channels == HC_C ? 1 : 0;
}

int dz_head_at_candidates(const float *shared, int batch, int h, int w, const unsigned long long *cand, const int *d_ncand, int cand_stride,
                          int k, const float *w1, int w1_cout, const float *s1, const float *b1, const float *w2, const float *s2,
                          const float *b2, int nbranch, const int *h_g_cout, const int *h_g_ooff, float *head, int math, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(dz_head_at_candidates_supported(math, HC_C), "dz_head_at_candidates: unknown math mode %d", math);
    DZ_CHECK_ARG(batch >= 0 && batch <= 65535 && h >= 1 && w >= 1 && k >= 1 && cand_stride >= k, "dz_head_at_candidates: bad sizes");
    DZ_CHECK_ARG(nbranch >= 1 && nbranch <= HC_MAX_BRANCH && w1_cout >= nbranch * HC_C && w1_cout % 32 == 0, "dz_head_at_candidates: bad branch layout");
    DZ_CHECK_ARG(shared && cand && d_ncand && w1 && s1 && b1 && w2 && head && h_g_cout && h_g_ooff, "dz_head_at_candidates: null pointer");
    if (batch == 0) return DZ_OK;
    HcArgs a{};
    for (int g = 0; g < nbranch; ++g) {
        DZ_CHECK_ARG(h_g_cout[g] >= 1 && h_g_cout[g] <= 4 && h_g_ooff[g] >= 0 && h_g_ooff[g] + h_g_cout[g] <= 12, "dz_head_at_candidates: bad columns of branch %d", g);
        a.g_cout[g] = h_g_cout[g];
        a.g_ooff[g] = h_g_ooff[g];
    }
    a.shared = reinterpret_cast<const unsigned char *>(shared);
    a.cand = cand; a.ncand = d_ncand;
    a.w1 = reinterpret_cast<const unsigned char *>(w1); a.w2 = reinterpret_cast<const unsigned char *>(w2);
    a.s1 = s1; a.b1 = b1; a.s2 = s2; a.b2 = b2; a.head = head;
    a.h = h; a.w = w; a.k = k; a.cand_stride = cand_stride; a.w1_cout = w1_cout;
    if (math == DZ_MATH_F32) {
        hipLaunchKernelGGL(k_head_at_cand_f32, dim3(ceil_div(k, HF_CAND), nbranch, batch), dim3(HC_THREADS), 0, stream, a);
        DZ_LAUNCH_CHECK();
        return DZ_OK;
    }
    if (math == DZ_MATH_F16X2) return launch_head_at_cand<MathF16>(a, batch, nbranch, stream);
    if (math == DZ_MATH_F16) return launch_head_at_cand<MathF16H>(a, batch, nbranch, stream);
    return launch_head_at_cand<MathBF16>(a, batch, nbranch, stream);
}

}  // extern "C"
