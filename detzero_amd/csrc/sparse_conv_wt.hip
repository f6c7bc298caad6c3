// Wave-private sparse 3-D convolution of the exact-fp32 mode for the 16-channel layers (16 -> 16, 16 -> 32) on the bf16 matrix pipe
// (gfx950): fp32 rows in, every operand as THREE exact bf16 limbs (limb3.h: h = rn(x), m = rn(x - h), l = x - h - m), fp32 rows out.
// The arithmetic of sparse_conv_gt.hip on the frame of k_spconv_w (sparse_conv_w.h): wave-private 32-row tiles as two 16-row halves
// that share the A fragments, the weights of ALL taps resident in LDS, activations gathered straight into registers (no LDS staging,
// no barrier in the loop), taps skipped from the table's 32-row tile masks (MFMAs per 16-row half), the persistent XCD-aware deal of
// groups of WAVES tiles and the three-stage per-wave pipeline with hand-counted loads - all as described at the top of that file.
// Reference call sites: detection/detzero_det/models/centerpoint_modules/backbone3d.py:243-259 (conv_input, conv1, conv2's first layer).
//
// Why the frame carries over: an fp32 row of 16 channels is 64 bytes, the pair16 row k_spconv_w was laid out around.  Lane
// (n = lane & 15, kg = lane >> 4) loads the 16 bytes of channels 4 kg .. 4 kg + 3 of the row of pixel n: one gather instruction covers
// 16 whole rows.  The lane splits its four values ONCE in registers (2 x split3x2) and the six limb terms of the other bf16x3 engines
// fall into three v_mfma_f32_16x16x32_bf16, whose lane supplies 8 k values = (4 channels) x (2 limbs):
//        B1 = [x_h | x_m]   B2 = [x_l | x_h]                               (k = 8 kg + j: channel 4 kg + (j & 3), limb slot j >> 2)
//        A3 = [w_h | w_l] . B2  ->  w_h.x_l + w_l.x_h
//        A2 = [w_m | w_m] . B1  ->  w_m.x_h + w_m.x_m
//        A1 = [w_h | w_h] . B1  ->  w_h.x_h + w_h.x_m
// issued in this order (smallest terms first) onto the element's ONE accumulator; dropped: m.l + l.m + l.l, at most 2^-26 of |x.w|.
// Weights: the layer's pack_weight_limb3(w, cout_mult=32) words (the copy k_spconv_gt / k_spconv_xt read) are re-arranged on their way
// into LDS into one 24-byte unit per (tap, 16-channel output block, lane): 16 bytes [w_h | w_m] and 8 bytes w_l of the lane's four
// channels of output channel n, stored once; the three A fragments are assembled from them in registers.  Rows at or beyond cout of the
// 32 packed rows are never read.  27 x CB x 64 x 24 bytes = 41 KB (16 -> 16) / 83 KB (16 -> 32).
//
// Accumulation order per output element (fixed; independent of the tile a row falls into, the grid and scheduling): taps ascending, per
// tap the three MFMAs above.  A skipped tap would have added exact zeros.  Two launches agree bit for bit.
// Epilogue: fmaf(acc, scale, shift) (scale / shift from LDS), + fp32 residual (one 16-byte load per lane, riding behind the gathers of
// the tile's last chunk), ReLU, one 16-byte store per lane: a lane holds four consecutive channels of one row.
// Missing neighbours (-1), rows at or beyond m = min(*d_m_out, cap) and absent slots use the out-of-range buffer offset: zeros come
// back, no row is fetched.  Rows at or beyond m and everything behind cap are never written.
#include "sparse_conv_w.h"
#include "limb3.h"

namespace dz {

struct SpConvWTArgs {
    const float *in;                // fp32 rows (in_rows, 16)
    const int *nbr;                 // plain table (kvol, cap)
    const uint32_t *tile_masks;     // tap mask per 32 output rows
    const int *d_m_out;
    const float *w;                 // (kvol, 32, 2 groups x 3 x 16 B) limb words
    const float *scale, *shift, *residual;
    float *out;
    int cout, kvol, cap, relu;
    unsigned int in_bytes, nbr_bytes, mask_bytes, out_bytes;
};

constexpr int WT_CIN = 16, WT_ROWB = WT_CIN * 4, WT_WROWB = WT_CIN * 6, WT_WROWS = 32;
constexpr int wt_lds_bytes(int kvol, int cout) { return kvol * (cout / 16) * 64 * 24 + 64 * 4; }

template <int COUT, int G, int WAVES, int OCC>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(OCC))) void k_spconv_wt(SpConvWTArgs a) {
    constexpr int CB = COUT / 16;           // 16-channel output blocks
    constexpr int NI = 2 * G;               // index loads per chunk (one per 16-pixel half and slot)
    constexpr int NL = 2 * G;               // gather loads per chunk
    constexpr int NR = 2 * CB;              // residual loads of a tile (16 bytes per half and block)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    v4u *const whm_s = reinterpret_cast<v4u *>(smem_raw);                           // [kvol][CB][64] {w_h (8 B), w_m (8 B)}
    uint2 *const wl_s = reinterpret_cast<uint2 *>(whm_s + a.kvol * CB * 64);        // [kvol][CB][64] w_l (8 B)
    float *const sc_s = reinterpret_cast<float *>(wl_s + a.kvol * CB * 64);         // [32] scale, [32] shift

    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, kg = lane >> 4;
    const int m = min(*a.d_m_out, a.cap);

    // ---- weights -> LDS: unit (tap, cb, lane) = the limbs of channels 4 kg .. 4 kg + 3 of output channel 16 cb + n, from the 48-byte
    // group (16 B of h, 16 of m, 16 of l) of channels 8 (kg >> 1) .. + 7 of that row
    {
        const unsigned char *wg = reinterpret_cast<const unsigned char *>(a.w);
        const int units = a.kvol * CB * 64;
        for (int u = tid; u < units; u += 64 * WAVES) {
            const int ul = u & 63, c = ul & 15, q = ul >> 4, cb = (u >> 6) % CB, tap = (u >> 6) / CB;
            const unsigned char *src = wg + (size_t)(tap * WT_WROWS + cb * 16 + c) * WT_WROWB + (q >> 1) * 48 + (q & 1) * 8;
            const uint2 wh = *reinterpret_cast<const uint2 *>(src), wm = *reinterpret_cast<const uint2 *>(src + 16);
            whm_s[u] = v4u{wh.x, wh.y, wm.x, wm.y};
            wl_s[u] = *reinterpret_cast<const uint2 *>(src + 32);
        }
        if (tid < 32) {
            sc_s[tid] = (a.scale && tid < a.cout) ? a.scale[tid] : 1.f;
            sc_s[32 + tid] = (a.shift && tid < a.cout) ? a.shift[tid] : 0.f;
        }
    }
    __syncthreads();

    const srsrc_t prsrc = make_srsrc(a.in, a.in_bytes);
    const srsrc_t nrsrc = make_srsrc(a.nbr, a.nbr_bytes);
    const srsrc_t rrsrc = make_srsrc(a.residual ? a.residual : a.in, a.residual ? a.out_bytes : 0u);
    const unsigned int nbr_tap_bytes = (unsigned int)a.cap * 4u;
    const unsigned int kmask = (1u << a.kvol) - 1u;         // (kvol <= 27)

    // ---- this wave's tile sequence (k_spconv_w's deal): workgroup b runs on XCD b % 8; at step s the workgroups of an XCD work on
    // neighbouring groups of WAVES consecutive tiles, in runs of XRUN groups per XCD
    constexpr int XRUN = 4;
    const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3, nx = gridDim.x >> 3;
    const int ntiles_w = (m + 31) >> 5;
    int seq = -1;                           // groups of this workgroup handed out so far
    auto tile_of = [&](int s) {
        const int q = s * nx + jx;
        return ((q / XRUN) * 8 * XRUN + xcd * XRUN + q % XRUN) * WAVES + wid;
    };
    // tap masks of this wave's next 64 tiles, one per lane (ONE vector load per 64 tiles, outside the hand-counted stream)
    int mask_base = 0;
    const srsrc_t mrsrc = make_srsrc(a.tile_masks, a.mask_bytes);
    auto load_masks = [&](int base) -> unsigned int {
        const int tile = tile_of(base + lane);
        unsigned int v;
        asm volatile("buffer_load_dword %0, %1, %2, 0 offen\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(tile >= 0 && tile < ntiles_w ? (unsigned int)tile * 4u : OOB_OFFSET), "s"(mrsrc));
        return v;
    };
    unsigned int mask_vec = load_masks(0);
    unsigned int rem = 0u;
    int cur_row0 = 0, cur_live = 0;
    unsigned int cur_rowoff[2] = {OOB_OFFSET, OOB_OFFSET};   // byte offset of this lane's two rows in one tap of the table
    bool started = false;
    // next chunk of this wave's stream.  Slots past the end of a tile's tap list repeat its last tap (loaded, not multiplied)
    auto next_chunk = [&]() {
        WChunk c;
        if (rem == 0u || !started) {                       // move to the next tile
            started = true;
            ++seq;
            if (seq - mask_base == 64) {                   // (drains the load pipeline once per 64 tiles)
                mask_base += 64;
                mask_vec = load_masks(mask_base);
            }
            const int tile = tile_of(seq);
            cur_live = tile >= 0 && tile < ntiles_w;
            cur_row0 = tile * 32;
            rem = cur_live ? (unsigned int)__builtin_amdgcn_readlane((int)mask_vec, seq - mask_base) & kmask : 0u;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int row = cur_row0 + h * 16 + n;
                cur_rowoff[h] = (cur_live && row < m) ? (unsigned int)row * 4u : OOB_OFFSET;
            }
        }
        c.row0 = cur_row0;
        c.live = cur_live;
        c.taps = 0u;
        c.nslots = 0;
        int t = 0;
#pragma unroll
        for (int s = 0; s < G; ++s) {
            if (rem) { t = __ffs((int)rem) - 1; rem &= rem - 1; ++c.nslots; }
            c.taps |= (unsigned int)t << (5 * s);
        }
        c.last = (rem == 0u);
        c.rowoff[0] = cur_rowoff[0];
        c.rowoff[1] = cur_rowoff[1];
        return c;
    };

    // ---- pipeline registers
    int idx[2][G][2];                       // neighbour indices of a chunk: [slot][16-pixel half]
    v4u gat[2][G][2];                       // gathered fp32 quads of a chunk: [slot][half]
    v4u resv[2][NR];                        // residual quads of the tile whose last chunk sits in the slot
    unsigned int present[2] = {0u, 0u};     // bit 2*slot + half: that half of the tile has a neighbour at the slot's tap
    f32x4v acc[2][CB];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[h][cb][e] = 0.f;

    auto issue_idx = [&](const WChunk &c, int (&dst)[G][2]) {
#pragma unroll
        for (int s = 0; s < G; ++s) {
            const unsigned int toff = ((c.taps >> (5 * s)) & 31u) * nbr_tap_bytes;       // scalar: rides in the instruction's soffset
#pragma unroll
            for (int h = 0; h < 2; ++h)
                asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "=v"(dst[s][h]) : "v"(c.rowoff[h]), "s"(nrsrc), "s"(toff));
        }
    };
    // indices have landed (caller waited): gather the operands, remember which halves have any neighbour at all.
    // A missing neighbour is -1: (unsigned)(-1) * 64 + kg * 16 stays just below 2^32, i.e. out of range -> zeros.
    auto issue_gather = [&](const WChunk &c, int (&ix)[G][2], v4u (&dst)[G][2], unsigned int &pres) {
        pres = 0u;
#pragma unroll
        for (int s = 0; s < G; ++s) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                asm volatile("" : "+v"(ix[s][h]));
                if (__ballot(ix[s][h] >= 0) != 0ull) pres |= 1u << (2 * s + h);
                const unsigned int base = (unsigned int)ix[s][h] * (unsigned int)WT_ROWB + (unsigned int)(kg * 16);
                asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(dst[s][h]) : "v"(base), "s"(prsrc));
            }
        }
        pres &= (1u << (2 * c.nslots)) - 1u;                   // repeated slots: loaded, not multiplied
        if (!c.live) pres = 0u;
    };
    // residual rows of the chunk's tile, in the accumulators' layout (issued only behind the gathers of a tile's LAST chunk)
    auto issue_res = [&](const WChunk &c, v4u (&dst)[NR]) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = c.row0 + h * 16 + n;
            const bool rok = c.live && row < m;
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                const unsigned int off = rok ? (unsigned int)(((size_t)row * COUT + cb * 16 + 4 * kg) * 4) : OOB_OFFSET;
                asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(dst[h * CB + cb]) : "v"(off), "s"(rrsrc));
            }
        }
    };
    auto mfma_chunk = [&](const WChunk &c, v4u (&src)[G][2], unsigned int pres) {
#pragma unroll
        for (int s = 0; s < G; ++s) {
#pragma unroll
            for (int h = 0; h < 2; ++h) asm volatile("" : "+v"(src[s][h]));
            if (!((pres >> (2 * s)) & 3u)) continue;             // wave-uniform
            const int t = (int)((c.taps >> (5 * s)) & 31u);
            v4u whm[CB];
            uint2 wl[CB];
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                whm[cb] = whm_s[(t * CB + cb) * 64 + lane];
                wl[cb] = wl_s[(t * CB + cb) * 64 + lane];
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (!((pres >> (2 * s + h)) & 1u)) continue;      // wave-uniform
                const v4u x = src[s][h];
                unsigned int h0, h1, m0, m1, l0, l1;
                split3x2(__uint_as_float(x.x), __uint_as_float(x.y), h0, m0, l0);
                split3x2(__uint_as_float(x.z), __uint_as_float(x.w), h1, m1, l1);
                const v4u b1 = {h0, h1, m0, m1}, b2 = {l0, l1, h0, h1};
                // term-major: with CB = 2 consecutive MFMAs go to different accumulators
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) acc[h][cb] = MathBF16::mma16(v4u{whm[cb].x, whm[cb].y, wl[cb].x, wl[cb].y}, b2, acc[h][cb]);
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) acc[h][cb] = MathBF16::mma16(v4u{whm[cb].z, whm[cb].w, whm[cb].z, whm[cb].w}, b1, acc[h][cb]);
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) acc[h][cb] = MathBF16::mma16(v4u{whm[cb].x, whm[cb].y, whm[cb].x, whm[cb].y}, b1, acc[h][cb]);
            }
        }
    };
    // accumulator of a 16x16 fragment: pixel = lane & 15, channel = 4 * (lane >> 4) + reg
    auto epilogue = [&](const WChunk &c, v4u (&rv)[NR]) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = c.row0 + h * 16 + n;
            const bool rok = c.live && row < m;
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                const int col = cb * 16 + 4 * kg;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaf(acc[h][cb][e], sc_s[col + e], sc_s[32 + col + e]);
                if (a.residual) {
                    asm volatile("" : "+v"(rv[h * CB + cb]));
                    const v4u r = rv[h * CB + cb];
                    v[0] += __uint_as_float(r.x);
                    v[1] += __uint_as_float(r.y);
                    v[2] += __uint_as_float(r.z);
                    v[3] += __uint_as_float(r.w);
                }
                if (a.relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                if (rok) *reinterpret_cast<float4 *>(a.out + (size_t)row * COUT + col) = make_float4(v[0], v[1], v[2], v[3]);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[h][cb][e] = 0.f;
            }
        }
    };
    const bool has_res = a.residual != nullptr;
    // wait until at most NI + NL (+ NR when `extra`) younger loads are outstanding
    auto wait_for = [&](bool extra) {
        if (extra) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI + NL + NR));
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI + NL));
    };
    static_assert(NI + NL + NR <= 63, "vmcnt is a 6-bit counter");

    // ---- prologue: D0 gathers in flight, D1 indices in flight; then k_spconv_w's steady state, unrolled by two:
    //   1. indices of chunk c+2 -> idx[c & 1]              (its previous user, gather(c), has been issued)
    //   2. wait idx(c+1); gather(c+1) -> gat[(c+1) & 1]     (+ residual rows if c+1 ends its tile)
    //   3. wait gather(c) (+ its residual rows); split + MFMAs; epilogue if c ends its tile
    // younger loads at both waits: NI (indices of c+2) + NL (a chunk's gathers) [+ NR residual loads of the chunk in between]
    WChunk d0 = next_chunk(), d1 = next_chunk(), d2;
    issue_idx(d0, idx[0]);
    issue_idx(d1, idx[1]);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI));
    issue_gather(d0, idx[0], gat[0], present[0]);
    bool r0 = has_res && d0.last;           // residual loads issued behind gather(d0)
    if (r0) issue_res(d0, resv[0]);
    auto step = [&](auto par_t) {
        constexpr int A = decltype(par_t)::value, B = A ^ 1;
        d2 = next_chunk();
        issue_idx(d2, idx[A]);
        wait_for(r0);                                        // idx(d1) landed; behind it: gather(d0) [+ res(d0)], idx(d2)
        issue_gather(d1, idx[B], gat[B], present[B]);
        const bool r1 = has_res && d1.last;
        if (r1) issue_res(d1, resv[B]);
        wait_for(r1);                                        // gather(d0) [+ res(d0)] landed; behind: idx(d2), gather(d1) [+ res(d1)]
        mfma_chunk(d0, gat[A], present[A]);
        if (d0.last) epilogue(d0, resv[A]);
        d0 = d1; d1 = d2; r0 = r1;
    };
    while (d0.live) {
        step(std::integral_constant<int, 0>{});
        if (!d0.live) break;
        step(std::integral_constant<int, 1>{});
    }
    asm volatile("s_waitcnt vmcnt(0)");
}

// The instances: waves per workgroup and slots per chunk.  16 -> 16: 41 KB of weights, three workgroups of 4 waves per CU (k_spconv_w's
// shape).  16 -> 32: 83 KB, so ONE workgroup per CU, which then carries all 12 waves of the three-per-SIMD register budget.
template <int COUT, int G_, int WAVES_, int OCC_>
struct WTile {
    static constexpr int CO = COUT, G = G_, WAVES = WAVES_, OCC = OCC_;
    static constexpr int PER_CU = (4 * OCC) / WAVES > 0 ? (4 * OCC) / WAVES : 1;
    static constexpr int LDS_BYTES = wt_lds_bytes(27, COUT);
    static_assert(COUT == 16 || COUT == 32, "one or two 16-channel output blocks");
    static_assert(LDS_BYTES <= 160 * 1024 && PER_CU * LDS_BYTES <= 160 * 1024, "LDS: all 27 taps resident, PER_CU workgroups per CU");
    static_assert(64 * WAVES <= 1024, "workgroup size");
};
using WT_16_16 = WTile<16, 4, 4, 3>;
using WT_16_32 = WTile<32, 3, 12, 3>;

template <class T>
static int launch_wt(const SpConvWTArgs &a, int max_workgroups, hipStream_t stream) {
    static PerDeviceFlags lds_done;
    const void *const fn = reinterpret_cast<const void *>(&k_spconv_wt<T::CO, T::G, T::WAVES, T::OCC>);
    if (int rc = reserve_lds(fn, T::LDS_BYTES, lds_done, "dz_spconv_forward_limb3_w")) return rc;
    // persistent workgroups: as many as fit on the chip (or the caller's cap), a multiple of 8 for the XCD schedule
    int grid = device_cus() * T::PER_CU;
    const int need = ceil_div(ceil_div(a.cap, 32), T::WAVES);
    if (grid > need) grid = need;
    if (max_workgroups > 0 && grid > max_workgroups) grid = max_workgroups;
    grid = (grid + 7) & ~7;
    if (grid < 8) grid = 8;
    hipLaunchKernelGGL((k_spconv_wt<T::CO, T::G, T::WAVES, T::OCC>), dim3(grid), dim3(64 * T::WAVES), wt_lds_bytes(a.kvol, T::CO), stream, a);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

enum WTVariant { WT_NONE = 0, WT_V_16_16, WT_V_16_32 };
using WTLaunch = int (*)(const SpConvWTArgs &, int, hipStream_t);
struct WTEntry { const char *name; int tile_rows; WTLaunch launch; };
static const WTEntry kWT[] = {
    {"none", 0, nullptr},
    {"k_spconv_wt<16x16>", 32 * WT_16_16::WAVES, launch_wt<WT_16_16>},
    {"k_spconv_wt<16x32>", 32 * WT_16_32::WAVES, launch_wt<WT_16_32>},
};

// Which layers the selector offers: an instance ships only where it measured faster than k_spconv_gt on the same tensors in both rounds
// of tools/bench_spconv.py --f32-small, by more than either kernel's round-to-round spread (DESIGN.md 2h-quater has the numbers).  A
// layer that is off reports 0 rows and "none" and stays on the kernel it has.
constexpr bool WT_SHIP_16_16 = true, WT_SHIP_16_32 = true;

static WTVariant spconv_wt_select(int cin, int cout) {
    if (cin == 16 && cout == 16) return WT_SHIP_16_16 ? WT_V_16_16 : WT_NONE;
    if (cin == 16 && cout == 32) return WT_SHIP_16_32 ? WT_V_16_32 : WT_NONE;
    return WT_NONE;
}

}  // namespace dz

using namespace dz;

extern "C" {

int dz_spconv_limb3_w_tile_rows(int cin, int cout) { return kWT[spconv_wt_select(cin, cout)].tile_rows; }

const char *dz_spconv_limb3_w_variant(int cin, int cout) { return kWT[spconv_wt_select(cin, cout)].name; }

int dz_spconv_forward_limb3_w(const float *in, int in_rows, int cin, const int *nbr, const uint32_t *tile_masks, int kvol, int cap_out,
                              const int *d_m_out, const float *w_limb, const float *scale, const float *shift, const float *residual,
                              int relu, float *out, int cout, int max_workgroups, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(in && nbr && tile_masks && d_m_out && w_limb && out, "dz_spconv_forward_limb3_w: null pointer");
    DZ_CHECK_ARG(kvol >= 1 && kvol <= 27, "dz_spconv_forward_limb3_w: kvol %d not in [1,27]", kvol);
    DZ_CHECK_ARG(cap_out >= 0 && in_rows >= 0 && max_workgroups >= 0, "dz_spconv_forward_limb3_w: negative row count or workgroup cap");
    const WTVariant v = spconv_wt_select(cin, cout);
    if (v == WT_NONE) {
        set_error("dz_spconv_forward_limb3_w: unsupported channels cin=%d cout=%d", cin, cout);
        return DZ_ERR_UNSUPPORTED;
    }
    const size_t in_bytes = (size_t)in_rows * cin * sizeof(float), out_bytes = (size_t)cap_out * cout * sizeof(float);
    const size_t nbr_bytes = (size_t)kvol * cap_out * sizeof(int);
    if (in_bytes >= 0x80000000ull || out_bytes >= 0x80000000ull || nbr_bytes >= 0x80000000ull) {
        set_error("dz_spconv_forward_limb3_w: input of %zu / output of %zu / table of %zu bytes exceeds the 2 GiB buffer-addressing limit",
                  in_bytes, out_bytes, nbr_bytes);
        return DZ_ERR_UNSUPPORTED;
    }
    if (cap_out == 0) return DZ_OK;
    SpConvWTArgs a{in, nbr, tile_masks, d_m_out, w_limb, scale, shift, residual, out, cout, kvol, cap_out, relu,
                   (unsigned int)in_bytes, (unsigned int)nbr_bytes, (unsigned int)tile_masks_words(cap_out) * 4u, (unsigned int)out_bytes};
    return kWT[v].launch(a, max_workgroups, stream);
}

}  // extern "C"
