// Gather-path sparse 3-D convolution of the exact-fp32 mode on the bf16 matrix pipe (gfx950): fp32 rows in, every operand as THREE
// exact bf16 limbs (limb3.h: h = rn(x), m = rn(x - h), l = x - h - m), six v_mfma_f32_32x32x16_bf16 per product with fp32
// accumulation, fp32 rows out.  The arithmetic of sparse_conv_xt.hip on the rulebook of sparse_conv.hip / sparse_conv_h.hip: any
// plain (kvol, cap) int32 table with 1..27 taps - the submanifold table, the stride-2 tables, conv_out's three taps.
// Reference call sites: detection/detzero_det/models/centerpoint_modules/backbone3d.py:64-121, :243-280.
//
// Skeleton (k_spconv_h's): an output-stationary tile of BP rows x all (padded) output channels, the tile's tap mask from the table's
// 32-row tile_masks, taps without a neighbour in the tile skipped, chunks = (KC-channel slice, live tap) with the taps innermost,
// persistent XCD-aware tile deal, one direct store per output, no atomics.
//
// Where the split happens - form (A): every gathered value is split ONCE, on its way from the staging registers into LDS.  A thread
// owns two adjacent 16-byte pieces (8 channels) of a gathered row, runs 4 x split3x2 and writes one 48-byte group (16 B of h, 16 of
// m, 16 of l: the group layout of conv3x3_t.hip).  An LDS row is KC / 8 groups + 16 bytes of padding (208 B at KC = 32, 112 at
// KC = 16: an odd number of 16-byte slots, conflict-free ds_read_b128 over 16 consecutive rows).  The weights arrive limb-packed
// (ops.pack_weight_limb3(w, cout_mult=32): per tap and output channel cin / 8 groups of 48 bytes) and are staged verbatim into rows
// of the same stride.  A fragment read is 3 x 16 B per operand: lane (row l & 31, half l >> 5) holds the limbs of channels
// 8 half .. 8 half + 7 of a 16-channel k-step; D[cout x row], so the accumulator holds four consecutive output channels of one row
// per register quad and the epilogue stores fp32 straight from registers.
//
// Pipeline: double-buffered LDS, one barrier per chunk.  The loads of chunk c + 1 (gathered rows, weights) and the neighbour indices
// of chunk c + 2 are issued in front of chunk c's MFMAs and land in registers behind them; the split + LDS write of chunk c + 1
// follows the MFMAs.  Missing neighbours and rows at or beyond m = min(*d_m_out, cap) use the out-of-range buffer offset: zeros
// come back, no row is fetched.
//
// Accumulation order per output element (fixed; independent of the tile a row falls into and of scheduling): KC-channel slice kc
// ascending, live taps ascending, 16-channel k-step ascending, and per k-step the six terms (weight limb . input limb)
//        l.h  h.l  m.m  m.h  h.m  h.h          (smallest first, the order of conv3x3_t.hip and sparse_conv_xt.hip)
// added onto the element's ONE accumulator; dropped: m.l + l.m + l.l, at most 2^-26 of |x.w|.  A skipped tap would have added exact
// zeros.  Two launches agree bit for bit.
// Tiny values: for |x| < 2^-100 the l limb (below 2^-109 the m limb too) is a bf16 subnormal.  Measured on an MI355X: the bf16 MFMA
// KEEPS subnormal inputs - with inputs of exponent [-120, -104] against one-hot weights every output equals (h + m + l) . w bit for
// bit, none the value with those limbs flushed (test_subnormal_limbs_are_measured).  Below 2^-110 the split itself
// stops being exact (bf16's quantum there is 2^-133): the result is then within 2^-133 |w| of x . w.
#include "hgemm.h"
#include "limb3.h"

namespace dz {

struct SpConvGTArgs {
    const float *in;                // fp32 rows (in_rows, cin)
    const int *nbr;                 // plain table (kvol, cap)
    const uint32_t *tile_masks;     // tap mask per 32 output rows
    const int *d_m_out;
    const float *w;                 // (kvol, cout_pad, cin / 8, 3 x 16 B) limb words
    const float *scale, *shift, *residual;
    float *out;
    int cin, cout, cout_pad, kvol, cap, relu;
    unsigned int in_bytes, w_bytes, nbr_bytes;
};

// The tile (limb3.h): BP rows x BC output channels (= cout_pad), KC channels of one tap per chunk, WP x WC waves
template <int BP, int BC, int KC, int WP, int WC>
struct GTile : Limb3Tile<BP, BC, KC, WP, WC> {};

template <class T>
__global__ __launch_bounds__(T::THREADS) void k_spconv_gt(SpConvGTArgs a) {
    constexpr int P = T::P_PER_THREAD, C = T::C_PER_THREAD, PT = T::PT, CT = T::CT, G = T::G, ROWB = T::ROWB;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *const Ps0 = smem, *const Cs0 = smem + 2 * T::PS_BYTES;      // [2][PS], [2][CS]

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wp = wid / T::WC, wc = wid % T::WC, l31 = lane & 31, kh = lane >> 5;
    const int m = min(*a.d_m_out, a.cap);
    const int ntiles = (m + T::BP - 1) / T::BP;
    const int kchunks = a.cin / T::KC;
    const __amdgpu_buffer_rsrc_t prsrc = make_rsrc(a.in, a.in_bytes), crsrc = make_rsrc(a.w, a.w_bytes), nrsrc = make_rsrc(a.nbr, a.nbr_bytes);
    const unsigned int row_bytes = (unsigned int)a.cin * 4u, wrow_bytes = (unsigned int)a.cin * 6u;
    const unsigned int tap_bytes = (unsigned int)a.cout_pad * wrow_bytes, nbr_tap_bytes = (unsigned int)a.cap * 4u;

    unsigned int cvoff[C], clds[C];         // my pieces of a tap's weight slice: all BC = cout_pad rows of the tap
    limb3_weight_pieces<T>(tid, 0, T::BC, wrow_bytes, cvoff, clds);
    const int poff = limb3_frag_base<T>(wp, PT, lane), coff = limb3_frag_base<T>(wc, CT, lane);

    // XCD-aware persistent schedule (k_spconv_h's): workgroup b runs on XCD b % 8; tiles are dealt to the XCDs in runs of XRUN
    // consecutive (spatially sorted) row tiles, which share their gathered neighbour rows in one L2
    constexpr int XRUN = 16;
    const int xcd = blockIdx.x & 7;
    for (int t = blockIdx.x >> 3;; t += gridDim.x >> 3) {
        const int tile = ((t / XRUN) * 8 + xcd) * XRUN + t % XRUN;
        if ((t / XRUN) * 8 * XRUN >= ntiles) break;
        if (tile >= ntiles) continue;
        const int row0 = tile * T::BP;
        unsigned int taps = 0u;
#pragma unroll
        for (int i = 0; i < T::BP / 32; ++i) taps |= a.tile_masks[tile * (T::BP / 32) + i];
        taps = __builtin_amdgcn_readfirstlane(taps);
        if (a.kvol < 32) taps &= (1u << a.kvol) - 1u;

        f32x16 acc[CT][PT];
        limb3_zero<T>(acc);

        const int nchunks = __popc(taps) * kchunks;
        if (nchunks > 0) {
            // my rows of the tile in one tap of the table (byte offset), and where their groups go in an LDS buffer
            unsigned int nvoff[P], plds[P], pgrp[P];
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const int idx = tid + i * T::THREADS;
                const int r = idx / G, g = idx % G;
                nvoff[i] = row0 + r < m ? (unsigned int)(row0 + r) * 4u : OOB_OFFSET;
                plds[i] = (unsigned int)(r * ROWB + g * 48);
                pgrp[i] = (unsigned int)g * 32u;
            }
            // chunk iterator of the loads (channel slice outermost, live taps innermost: neighbouring taps gather mostly the same
            // rows) and tap iterator of the index fetches, one chunk further ahead
            unsigned int rem = taps, rem_a = taps;
            int tap = __ffs((int)rem) - 1, kc = 0, tap_a = tap;
            auto advance = [&]() {
                rem &= rem - 1;
                if (rem == 0u) { rem = taps; ++kc; }
                tap = __ffs((int)rem) - 1;
            };
            int nb[P];
            auto fetch_nbr = [&]() {
                const unsigned int toff = (unsigned int)tap_a * nbr_tap_bytes;
#pragma unroll
                for (int i = 0; i < P; ++i)
                    nb[i] = (int)__builtin_amdgcn_raw_buffer_load_b32(nrsrc, nvoff[i] == OOB_OFFSET ? OOB_OFFSET : nvoff[i] + toff, 0, 0);
                rem_a &= rem_a - 1;
                if (rem_a == 0u) rem_a = taps;          // (keeps cycling past the last chunk: those fetches are never used)
                tap_a = __ffs((int)rem_a) - 1;
            };
            v4u sp[P][2], sw[C];
            auto issue = [&]() {
                const unsigned int padd = (unsigned int)(kc * T::KC * 4);
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    const unsigned int off = (nvoff[i] != OOB_OFFSET && nb[i] >= 0) ? (unsigned int)nb[i] * row_bytes + pgrp[i] + padd : OOB_OFFSET;
                    sp[i][0] = __builtin_amdgcn_raw_buffer_load_b128(prsrc, off, 0, 0);
                    sp[i][1] = __builtin_amdgcn_raw_buffer_load_b128(prsrc, off == OOB_OFFSET ? OOB_OFFSET : off + 16u, 0, 0);
                }
                const unsigned int cadd = (unsigned int)tap * tap_bytes + (unsigned int)(kc * G * 48);
#pragma unroll
                for (int i = 0; i < C; ++i) sw[i] = __builtin_amdgcn_raw_buffer_load_b128(crsrc, cvoff[i] == OOB_OFFSET ? OOB_OFFSET : cvoff[i] + cadd, 0, 0);
            };
            auto store = [&](int buf) { limb3_store<T>(Ps0 + buf * T::PS_BYTES, Cs0 + buf * T::CS_BYTES, sp, sw, plds, clds); };

            fetch_nbr();
            issue();                // chunk 0 (waits for its indices)
            advance();
            fetch_nbr();            // indices of chunk 1
            store(0);
            __syncthreads();
            for (int c = 0; c < nchunks; ++c) {
                const int cur = c & 1;
                const bool has1 = c + 1 < nchunks;
                if (has1) {
                    issue();        // chunk c + 1
                    advance();
                    fetch_nbr();    // indices of chunk c + 2
                }
                limb3_mma<T>(Ps0 + cur * T::PS_BYTES + poff, Cs0 + cur * T::CS_BYTES + coff, acc);
                if (has1) store(cur ^ 1);
                __syncthreads();
            }
        }

        // ---- epilogue: register quad j of fragment (ct, pt) = channels ct*32 + 8 j + 4 kh .. + 3 of my row
        const bool has_sc = a.scale != nullptr, has_sh = a.shift != nullptr, has_res = a.residual != nullptr;
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
            const int row = row0 + wp * PT * 32 + pt * 32 + l31;
            const size_t rbase = (size_t)row * a.cout;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                // (all of scale / shift / residual of the fragment are requested before the first is used: one memory round trip)
                float4 sc[4], sh[4], rs[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ch = wc * CT * 32 + ct * 32 + j * 8 + kh * 4;
                    const bool live = row < m && ch < a.cout;
                    sc[j] = has_sc && live ? *reinterpret_cast<const float4 *>(a.scale + ch) : make_float4(1.f, 1.f, 1.f, 1.f);
                    sh[j] = has_sh && live ? *reinterpret_cast<const float4 *>(a.shift + ch) : make_float4(0.f, 0.f, 0.f, 0.f);
                    rs[j] = has_res && live ? *reinterpret_cast<const float4 *>(a.residual + rbase + ch) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ch = wc * CT * 32 + ct * 32 + j * 8 + kh * 4;
                    float4 v = make_float4(fmaf(acc[ct][pt][4 * j], sc[j].x, sh[j].x), fmaf(acc[ct][pt][4 * j + 1], sc[j].y, sh[j].y),
                                           fmaf(acc[ct][pt][4 * j + 2], sc[j].z, sh[j].z), fmaf(acc[ct][pt][4 * j + 3], sc[j].w, sh[j].w));
                    if (has_res) { v.x += rs[j].x; v.y += rs[j].y; v.z += rs[j].z; v.w += rs[j].w; }
                    if (a.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                    if (row < m && ch < a.cout) *reinterpret_cast<float4 *>(a.out + rbase + ch) = v;
                }
            }
        }
    }
}

// The instances: BP x BC x KC.  LDS is 1.5 x k_spconv_h's at the same tile (limb rows), so the tiles are the ones at which two
// workgroups still share a CU: 128 x 32 x 16 is 36 KB, 128 x 32 x 32 is 67 KB, 128 x 64 x 32 is 80 KB, 128 x 128 x 16 is 57 KB
using GT_32_16 = GTile<128, 32, 16, 4, 1>;
using GT_32_32 = GTile<128, 32, 32, 4, 1>;
using GT_64_32 = GTile<128, 64, 32, 4, 1>;
using GT_128_16 = GTile<128, 128, 16, 2, 2>;
static_assert(2 * GT_64_32::LDS_BYTES <= 160 * 1024 && 2 * GT_128_16::LDS_BYTES <= 160 * 1024, "two workgroups per CU");

template <class T>
static int launch_gt(const SpConvGTArgs &a, hipStream_t stream) {
    static PerDeviceFlags done;
    if (int rc = reserve_lds(reinterpret_cast<const void *>(&k_spconv_gt<T>), T::LDS_BYTES, done, "dz_spconv_forward_limb3")) return rc;
    int grid = ceil_div(a.cap, T::BP);
    if (grid > 2048) grid = 2048;
    grid = (grid + 7) & ~7;             // a multiple of 8: see the XCD schedule in the kernel
    if (grid < 8) grid = 8;
    hipLaunchKernelGGL((k_spconv_gt<T>), dim3(grid), dim3(T::THREADS), T::LDS_BYTES, stream, a);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

enum GTVariant { GT_NONE = 0, GT_V_32_16, GT_V_32_32, GT_V_64_32, GT_V_128_16 };
using GTLaunch = int (*)(const SpConvGTArgs &, hipStream_t);
struct GTEntry { const char *name; int tile_rows; GTLaunch launch; };
static const GTEntry kGT[] = {
    {"none", 0, nullptr},
    {"k_spconv_gt<128x32x16>", GT_32_16::BP, launch_gt<GT_32_16>},
    {"k_spconv_gt<128x32x32>", GT_32_32::BP, launch_gt<GT_32_32>},
    {"k_spconv_gt<128x64x32>", GT_64_32::BP, launch_gt<GT_64_32>},
    {"k_spconv_gt<128x128x16>", GT_128_16::BP, launch_gt<GT_128_16>},
};

// Which layers the selector offers: a layer ships only where the kernel measured faster than k_spconv on the same tensors in both
// rounds of tools/bench_spconv.py --f32-gather (DESIGN.md 2h-ter has the numbers).  A layer that is off reports 0 rows and "none":
// the backbone keeps it on k_spconv.
constexpr bool GT_SHIP_16_16 = true, GT_SHIP_16_32 = true, GT_SHIP_32_32 = true, GT_SHIP_32_64 = true, GT_SHIP_64_64 = true,
               GT_SHIP_64_128 = true, GT_SHIP_128_128 = true;

// The one decision of this engine: which instance runs a (cin, cout) layer (GT_NONE: none does).  The kernel volume decides nothing.
static GTVariant spconv_gt_select(int cin, int cout) {
    if (cin == 16 && cout == 16) return GT_SHIP_16_16 ? GT_V_32_16 : GT_NONE;
    if (cin == 16 && cout == 32) return GT_SHIP_16_32 ? GT_V_32_16 : GT_NONE;
    if (cin == 32 && cout == 32) return GT_SHIP_32_32 ? GT_V_32_32 : GT_NONE;
    if (cin == 32 && cout == 64) return GT_SHIP_32_64 ? GT_V_64_32 : GT_NONE;
    if (cin == 64 && cout == 64) return GT_SHIP_64_64 ? GT_V_64_32 : GT_NONE;
    if (cin == 64 && cout == 128) return GT_SHIP_64_128 ? GT_V_128_16 : GT_NONE;
    if (cin == 128 && cout == 128) return GT_SHIP_128_128 ? GT_V_128_16 : GT_NONE;
    return GT_NONE;
}

}  // namespace dz

using namespace dz;

extern "C" {

int dz_spconv_limb3_tile_rows(int cin, int cout) { return kGT[spconv_gt_select(cin, cout)].tile_rows; }

const char *dz_spconv_limb3_variant(int cin, int cout) { return kGT[spconv_gt_select(cin, cout)].name; }

int dz_spconv_forward_limb3(const float *in, int in_rows, int cin, const int *nbr, const uint32_t *tile_masks, int kvol, int cap_out,
                            const int *d_m_out, const float *w_limb, const float *scale, const float *shift, const float *residual,
                            int relu, float *out, int cout, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(in && nbr && tile_masks && d_m_out && w_limb && out, "dz_spconv_forward_limb3: null pointer");
    DZ_CHECK_ARG(kvol >= 1 && kvol <= 27, "dz_spconv_forward_limb3: kvol %d not in [1,27]", kvol);
    DZ_CHECK_ARG(cap_out >= 0 && in_rows >= 0, "dz_spconv_forward_limb3: negative row count");
    const GTVariant v = spconv_gt_select(cin, cout);
    if (v == GT_NONE) {
        set_error("dz_spconv_forward_limb3: unsupported channels cin=%d cout=%d", cin, cout);
        return DZ_ERR_UNSUPPORTED;
    }
    const int cout_pad = cout < 32 ? 32 : cout;
    const size_t in_bytes = (size_t)in_rows * cin * sizeof(float), out_bytes = (size_t)cap_out * cout * sizeof(float);
    const size_t nbr_bytes = (size_t)kvol * cap_out * sizeof(int), w_bytes = (size_t)kvol * cout_pad * cin * 6;
    if (in_bytes >= 0x80000000ull || out_bytes >= 0x80000000ull || nbr_bytes >= 0x80000000ull) {
        set_error("dz_spconv_forward_limb3: input of %zu / output of %zu / table of %zu bytes exceeds the 2 GiB buffer-addressing limit",
                  in_bytes, out_bytes, nbr_bytes);
        return DZ_ERR_UNSUPPORTED;
    }
    if (cap_out == 0) return DZ_OK;
    SpConvGTArgs a{in, nbr, tile_masks, d_m_out, w_limb, scale, shift, residual, out, cin, cout, cout_pad, kvol, cap_out, relu,
                   (unsigned int)in_bytes, (unsigned int)w_bytes, (unsigned int)nbr_bytes};
    return kGT[v].launch(a, stream);
}

}  // extern "C"
