// Sparse 3-D convolution forward on the 16-bit matrix cores with split-precision (pair16) operands: the
// output-stationary gather -> implicit GEMM -> direct store of sparse_conv.hip (same rulebook, tap skipping,
// fused BatchNorm + bias + residual + ReLU epilogue), fp32-class results at ~5x the fp32-MFMA rate (hgemm.h).
//
// Reference call sites: detection/detzero_det/models/centerpoint_modules/backbone3d.py:64-121, :243-280.
#include "hgemm.h"
#include "sparse_conv_w.h"

namespace dz {

constexpr int KVOL_MAX_H = 27;

// GN = false: the tile's slice of the neighbour table is staged in LDS and scanned for its tap mask first.
// GN = true (tile_masks given): no table in LDS and no per-tile scan - the tap mask comes precomputed and each
// thread fetches the neighbour index of the rows it gathers straight from the table, NS chunks ahead of the gather
// that uses it (a register ring, filled by EXTRA loads behind every stage's loads; see hgemm_pipeline).  Less LDS per
// workgroup = more resident workgroups for the small-channel levels, and the tile prologue disappears.
template <class T, class M, int NS, bool GN, int OCC>
__global__ __launch_bounds__(T::THREADS) __attribute__((amdgpu_waves_per_eu(OCC))) void k_spconv_h(SpConvHArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    v4u *const smem = reinterpret_cast<v4u *>(smem_raw);
    int *const nbr_s = reinterpret_cast<int *>(smem + T::LDS_U4);       // [kvol][BP]   (GN = false only)
    __shared__ unsigned int mask_s;
    __shared__ __attribute__((aligned(16))) float sc_s[T::BC], sh_s[T::BC];     // BatchNorm scale / shift of my channel tile
    constexpr int P = T::P_PER_THREAD;
    constexpr int NST = T::P_PER_THREAD + T::C_PER_THREAD;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wp = wid / T::WC, wc = wid % T::WC;
    const int m = min(*a.d_m_out, a.cap);
    const int ntiles = (m + T::BP - 1) / T::BP;
    const int kchunks = a.cin / T::KC;
    const int n0 = blockIdx.y * T::BC;          // channel tile (cout_pad may be split over blockIdx.y)
    const srsrc_t prsrc = make_srsrc(a.in, a.in_bytes);
    const srsrc_t crsrc = make_srsrc(a.w, a.w_bytes);
    const srsrc_t nrsrc = make_srsrc(a.nbr, a.nbr_bytes);
    unsigned int cvoff[T::C_PER_THREAD];
#pragma unroll
    for (int i = 0; i < T::C_PER_THREAD; ++i) {
        const int idx = tid + i * T::THREADS;
        cvoff[i] = OOB_OFFSET;
        if (T::C_PIECES % T::THREADS == 0 || idx < T::C_PIECES) {
            const int n = idx / (T::KC / 4), q = idx % (T::KC / 4);
            cvoff[i] = (unsigned int)(((n0 + n) * a.cin + q * 4) * 4);
        }
    }
    const unsigned int tap_bytes = (unsigned int)(a.cout_pad * a.cin * 4);
    const unsigned int nbr_tap_bytes = (unsigned int)a.cap * 4u;
    for (int c = tid; c < T::BC; c += T::THREADS) {
        const bool in = n0 + c < a.cout;
        sc_s[c] = (in && a.scale) ? a.scale[n0 + c] : 1.f;
        sh_s[c] = (in && a.shift) ? a.shift[n0 + c] : 0.f;
    }
    __syncthreads();

    // XCD-aware persistent schedule: workgroup b runs on XCD b % 8 (private L2 each).  Tiles are dealt to the XCDs
    // in runs of XRUN consecutive (spatially sorted) row tiles: a run shares its gathered neighbour rows in one L2,
    // while the round-robin of runs keeps the eight XCDs evenly loaded (whole contiguous eighths were measured slower:
    // tile cost follows the local point density)
    constexpr int XRUN = 16;
    const int xcd = blockIdx.x & 7;
    for (int t = blockIdx.x >> 3;; t += gridDim.x >> 3) {
        const int tile = ((t / XRUN) * 8 + xcd) * XRUN + t % XRUN;
        if ((t / XRUN) * 8 * XRUN >= ntiles) break;
        if (tile >= ntiles) continue;
        const int row0 = tile * T::BP;
        unsigned int taps;
        if constexpr (GN) {
            taps = 0u;
#pragma unroll
            for (int i = 0; i < T::BP / 32; ++i) taps |= a.tile_masks[tile * (T::BP / 32) + i];
            taps = __builtin_amdgcn_readfirstlane(taps);
        } else {
            if (tid == 0) mask_s = 0u;
            __syncthreads();
            unsigned int local = 0u;
            for (int idx = tid; idx < a.kvol * T::BP; idx += T::THREADS) {
                const int k = idx / T::BP, r = idx % T::BP;
                const int row = row0 + r;
                const int v = (row < m) ? a.nbr[(size_t)k * a.cap + row] : -1;
                nbr_s[idx] = v;
                if (v >= 0) local |= 1u << k;
            }
            if (local) atomicOr(&mask_s, local);
            __syncthreads();
            taps = mask_s;
        }

        f32x16 acc[T::CT][T::PT];
#pragma unroll
        for (int i = 0; i < T::CT; ++i)
#pragma unroll
            for (int j = 0; j < T::PT; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

        const int nchunks = __popc(taps) * kchunks;
        if (nchunks > 0) {
            unsigned int rem = taps;
            int tap = __ffs((int)rem) - 1, kc = 0;
            // chunk order: channel chunk outermost, taps innermost - neighbouring taps gather mostly the same input
            // rows, so their KC-channel slices are re-read back to back while they are still in the CU's L1
            auto advance = [&]() {
                rem &= rem - 1;
                if (rem == 0u) { rem = taps; ++kc; }
                tap = __ffs((int)rem) - 1;
            };
            if constexpr (GN) {
                // neighbour-index ring: slot s holds the indices of the chunk that will be gathered into stage s next
                int nb[NS][P];
                unsigned int nvoff[P];          // byte offset of this thread's rows in one tap of the table
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    const int idx = tid + i * T::THREADS;
                    const int row = row0 + idx / (T::KC / 4);
                    nvoff[i] = ((T::P_PIECES % T::THREADS == 0 || idx < T::P_PIECES) && row < m) ? (unsigned int)row * 4u : OOB_OFFSET;
                }
                unsigned int rem_a = taps;                  // tap iterator of the ring: NS chunks ahead of (rem, tap)
                int tap_a = __ffs((int)rem_a) - 1;
                auto fetch_nbr = [&](int (&dst)[P]) {
                    const unsigned int toff = (unsigned int)tap_a * nbr_tap_bytes;
#pragma unroll
                    for (int i = 0; i < P; ++i)
                        asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(dst[i]) : "v"(nvoff[i] == OOB_OFFSET ? OOB_OFFSET : nvoff[i] + toff), "s"(nrsrc));
                    rem_a &= rem_a - 1;
                    if (rem_a == 0u) rem_a = taps;          // keeps cycling past the last chunk: those fetches are never used
                    tap_a = __ffs((int)rem_a) - 1;
                };
#pragma unroll
                for (int s = 0; s < NS; ++s) fetch_nbr(nb[s]);
                asm volatile("s_waitcnt vmcnt(0)");
#pragma unroll
                for (int s = 0; s < NS; ++s)
#pragma unroll
                    for (int i = 0; i < P; ++i) asm volatile("" : "+v"(nb[s][i]));
                auto issue = [&](HStage<T> &st, auto s_t) {
                    constexpr int S = decltype(s_t)::value;
                    // the fetch into slot S was issued NS calls ago, right behind that call's stage loads
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 1) * (NST + P)));
                    unsigned int pvoff[P];
#pragma unroll
                    for (int i = 0; i < P; ++i) {
                        asm volatile("" : "+v"(nb[S][i]));
                        const int q = (tid + i * T::THREADS) % (T::KC / 4);
                        const int rb = nb[S][i];
                        pvoff[i] = (nvoff[i] != OOB_OFFSET && rb >= 0) ? (unsigned int)rb * (unsigned int)(a.cin * 4) + (unsigned int)(q * 16) : OOB_OFFSET;
                    }
                    load_hstage<T>(st, prsrc, pvoff, (unsigned int)(kc * T::KC * 4), crsrc, cvoff,
                                   (unsigned int)tap * tap_bytes + (unsigned int)(kc * T::KC * 4));
                    fetch_nbr(nb[S]);
                };
                hgemm_pipeline<T, M, NS, P, (T::THREADS == 512)>(nchunks, smem, issue, advance, acc, wp, wc, lane, tid);
            } else {
                auto issue = [&](HStage<T> &st, auto) {
                    unsigned int pvoff[P];
#pragma unroll
                    for (int i = 0; i < P; ++i) {
                        const int idx = tid + i * T::THREADS;
                        pvoff[i] = OOB_OFFSET;
                        if (T::P_PIECES % T::THREADS == 0 || idx < T::P_PIECES) {
                            const int rr = idx / (T::KC / 4), q = idx % (T::KC / 4);
                            const int rb = nbr_s[tap * T::BP + rr];
                            pvoff[i] = rb >= 0 ? (unsigned int)rb * (unsigned int)(a.cin * 4) + (unsigned int)(q * 16) : OOB_OFFSET;
                        }
                    }
                    load_hstage<T>(st, prsrc, pvoff, (unsigned int)(kc * T::KC * 4), crsrc, cvoff,
                                   (unsigned int)tap * tap_bytes + (unsigned int)(kc * T::KC * 4));
                };
                hgemm_pipeline<T, M, NS>(nchunks, smem, issue, advance, acc, wp, wc, lane, tid);
            }
        }

        // epilogue through the (now idle) tile buffers: see store_tile_pair16
        store_tile_pair16<T, M>(acc, smem_raw, sc_s, sh_s, n0, a.cout, a.relu != 0, reinterpret_cast<const unsigned char *>(a.residual),
                                reinterpret_cast<unsigned char *>(a.out), wp, wc, lane, wid, [&](int lr) {
                                    const int row = row0 + lr;
                                    return row < m ? (size_t)row * a.cout * 4 : ~size_t(0);
                                });
        __syncthreads();      // the next tile's first stage (and, without the ring, its table slice) overwrites the buffers
    }
}


template <class M, class T, int NS, bool GN, int OCC>
static int launch_spconv_h(const SpConvHArgs &a, hipStream_t stream) {
    constexpr int LDS = T::LDS_BYTES + (GN ? 0 : KVOL_MAX_H * T::BP * 4);
    static PerDeviceFlags lds_done;
    if (int rc_ = reserve_lds(reinterpret_cast<const void *>(&k_spconv_h<T, M, NS, GN, OCC>), LDS, lds_done, "dz_spconv_forward_split")) return rc_;
    int grid = ceil_div(a.cap, T::BP);
    if (grid > 2048) grid = 2048;
    grid = (grid + 7) & ~7;            // a multiple of 8: see the XCD schedule in the kernel
    if (grid < 8) grid = 8;
    hipLaunchKernelGGL((k_spconv_h<T, M, NS, GN, OCC>), dim3(grid, a.cout_pad / T::BC), dim3(T::THREADS), LDS, stream, a);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

// Variants of the split path: the wave-private small-channel kernels (sparse_conv_w.h) on the plain (SH_W_*) and on the packed (SH_WP_*)
// table, and the BP x BC x KC tiles of k_spconv_h with their arm - RING: tile masks given, neighbour indices through the register
// ring; LDS: the table slice staged in LDS.  The 128-row tiles have the LDS arm only: with tile masks their layers run on k_spconv_w.
enum SpHVariant { SH_NONE = 0, SH_W_16_16, SH_W_16_32, SH_W_32_32, SH_WP_16_16, SH_WP_16_32, SH_WP_32_32, SH_128_32_16_LDS, SH_128_32_32_LDS,
                  SH_256_64_RING, SH_256_64_LDS, SH_256_128_RING, SH_256_128_LDS };

// What a variant is called (`arm`: with the arm of a k_spconv_h tile) and what launches it, per split mode.
using SpHLaunch = int (*)(const SpConvHArgs &, hipStream_t);
struct SpHEntry { const char *name, *arm; SpHLaunch launch[3]; };      // launch[math - 1]
#define DZ_BY_MATH(fn, ...) {fn<MathF16, __VA_ARGS__>, fn<MathBF16, __VA_ARGS__>, fn<MathF16H, __VA_ARGS__>}
// (template arguments behind the shape: k_spconv_w - taps per chunk, waves, waves per SIMD, packed table; k_spconv_h - register
// stages, ring arm, waves per SIMD the register allocation leaves room for)
static const SpHEntry kSpH[] = {
    {"none", "none", {nullptr, nullptr, nullptr}},
    {"k_spconv_w<16x16>", "k_spconv_w<16x16>", DZ_BY_MATH(launch_spconv_w, 16, 16, 4, 4, 3, false)},
    {"k_spconv_w<16x32>", "k_spconv_w<16x32>", DZ_BY_MATH(launch_spconv_w, 16, 32, 3, 6, 3, false)},
    {"k_spconv_w<32x32>", "k_spconv_w<32x32>", DZ_BY_MATH(launch_spconv_w, 32, 32, 2, 12, 3, false)},
    {"k_spconv_w<16x16>", "k_spconv_w<16x16>", DZ_BY_MATH(launch_spconv_w, 16, 16, 4, 6, 3, true)},
    {"k_spconv_w<16x32>", "k_spconv_w<16x32>", DZ_BY_MATH(launch_spconv_w, 16, 32, 3, 6, 3, true)},
    {"k_spconv_w<32x32>", "k_spconv_w<32x32>", DZ_BY_MATH(launch_spconv_w, 32, 32, 2, 12, 3, true)},
    {"k_spconv_h<128x32x16>", "k_spconv_h<128x32x16> lds", DZ_BY_MATH(launch_spconv_h, HTile<128, 32, 16, 4, 1>, 4, false, 4)},
    {"k_spconv_h<128x32x32>", "k_spconv_h<128x32x32> lds", DZ_BY_MATH(launch_spconv_h, HTile<128, 32, 32, 4, 1>, 3, false, 1)},
    {"k_spconv_h<256x64x32>", "k_spconv_h<256x64x32> ring", DZ_BY_MATH(launch_spconv_h, HTile<256, 64, 32, 4, 2>, 3, true, 2)},
    {"k_spconv_h<256x64x32>", "k_spconv_h<256x64x32> lds", DZ_BY_MATH(launch_spconv_h, HTile<256, 64, 32, 4, 2>, 3, false, 2)},
    {"k_spconv_h<256x128x32>", "k_spconv_h<256x128x32> ring", DZ_BY_MATH(launch_spconv_h, HTile<256, 128, 32, 4, 2>, 2, true, 2)},
    {"k_spconv_h<256x128x32>", "k_spconv_h<256x128x32> lds", DZ_BY_MATH(launch_spconv_h, HTile<256, 128, 32, 4, 2>, 2, false, 2)},
};
#undef DZ_BY_MATH
static_assert(sizeof(kSpH) / sizeof(kSpH[0]) == SH_256_128_LDS + 1, "one entry per variant");

// The one decision of the split path: which instance and arm runs a layer (SH_NONE: none does).  packed: the table is the packed one
// of dz_spconv_forward_split_packed; masks: a plain table that comes with tile masks and lies inside the 2 GiB window of a buffer
// descriptor.  dz_spconv_forward_split[_packed] launch what it returns and the dz_spconv_variant_split* functions report it.
// (The kernel volume decides nothing: every variant takes 1..27 taps.)
static SpHVariant spconv_h_select(int cin, int cout, bool packed, bool masks) {
    if (packed || (masks && cout <= 32)) {
        if (cin == 16 && cout == 16) return packed ? SH_WP_16_16 : SH_W_16_16;
        if (cin == 16 && cout == 32) return packed ? SH_WP_16_32 : SH_W_16_32;
        if (cin == 32 && cout == 32) return packed ? SH_WP_32_32 : SH_W_32_32;
        if (packed) return SH_NONE;
    }
    if (cin == 16 && cout <= 32) return SH_128_32_16_LDS;
    if (cin == 32 && cout <= 32) return SH_128_32_32_LDS;
    if ((cin == 32 || cin == 64) && cout == 64) return masks ? SH_256_64_RING : SH_256_64_LDS;
    if ((cin == 64 || cin == 128) && cout == 128) return masks ? SH_256_128_RING : SH_256_128_LDS;
    return SH_NONE;
}

}  // namespace dz

using namespace dz;

extern "C" {

int dz_spconv_forward_split(const float *in, int in_rows, int cin, const int *nbr, const uint32_t *tile_masks, int kvol, int cap_out,
                            const int *d_m_out, const float *w, const float *scale, const float *shift, const float *residual,
                            int relu, float *out, int cout, int math, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(in && nbr && d_m_out && w && out, "dz_spconv_forward_split: null pointer");
    DZ_CHECK_ARG(kvol >= 1 && kvol <= KVOL_MAX_H, "dz_spconv_forward_split: kvol %d not in [1,27]", kvol);
    DZ_CHECK_ARG(math == DZ_MATH_F16X2 || math == DZ_MATH_BF16X2 || math == DZ_MATH_F16, "dz_spconv_forward_split: math %d is not a split mode", math);
    DZ_CHECK_ARG(cout % 8 == 0 && cin % 8 == 0, "dz_spconv_forward_split: channels must be multiples of the 8-channel pair16 group");
    if (cap_out == 0) return DZ_OK;
    const int cout_pad = cout < 32 ? 32 : cout;
    const size_t in_bytes = (size_t)in_rows * cin * sizeof(float);
    const size_t w_bytes = (size_t)kvol * cout_pad * cin * sizeof(float);
    if (in_rows < 0 || in_bytes >= 0x80000000ull) {
        set_error("dz_spconv_forward_split: input of %zu bytes exceeds the 2 GiB buffer-addressing limit", in_bytes);
        return DZ_ERR_UNSUPPORTED;
    }
    // the table is addressed through a buffer descriptor when it fits its 2 GiB window (else: staged through LDS)
    const size_t nbr_bytes = (size_t)kvol * cap_out * sizeof(int);
    SpConvHArgs a{in, nbr, tile_masks, d_m_out, w, scale, shift, residual, out, cin, cout, cout_pad, kvol, cap_out, relu,
                  (unsigned int)in_bytes, (unsigned int)w_bytes, nbr_bytes < 0x80000000ull ? (unsigned int)nbr_bytes : 0u,
                  tile_masks ? (unsigned int)tile_masks_words(cap_out) * 4u : 0u};
    const SpHVariant v = spconv_h_select(cin, cout, false, a.tile_masks && a.nbr_bytes);
    if (v == SH_NONE) {
        set_error("dz_spconv_forward_split: unsupported channels cin=%d cout=%d", cin, cout);
        return DZ_ERR_UNSUPPORTED;
    }
    return kSpH[v].launch[math - 1](a, stream);
}

int dz_spconv_forward_split_packed(const float *in, int in_rows, int cin, const int *nbr_packed, const uint32_t *tile_masks, int cap_out,
                                   const int *d_m_out, const float *w, const float *scale, const float *shift, const float *residual,
                                   int relu, float *out, int cout, int math, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(in && nbr_packed && tile_masks && d_m_out && w && out, "dz_spconv_forward_split_packed: null pointer");
    DZ_CHECK_ARG(math == DZ_MATH_F16X2 || math == DZ_MATH_BF16X2 || math == DZ_MATH_F16, "dz_spconv_forward_split_packed: math %d is not a split mode", math);
    if (cap_out == 0) return DZ_OK;
    const int kvol = 27, cout_pad = 32;
    const size_t in_bytes = (size_t)in_rows * cin * sizeof(float);
    const size_t w_bytes = (size_t)kvol * cout_pad * cin * sizeof(float);
    const size_t nbr_bytes = (size_t)9 * cap_out * sizeof(int);
    if (in_rows < 0 || in_bytes >= 0x80000000ull || nbr_bytes >= 0x80000000ull) {
        set_error("dz_spconv_forward_split_packed: input of %zu / table of %zu bytes exceeds the 2 GiB buffer-addressing limit", in_bytes, nbr_bytes);
        return DZ_ERR_UNSUPPORTED;
    }
    SpConvHArgs a{in, nbr_packed, tile_masks, d_m_out, w, scale, shift, residual, out, cin, cout, cout_pad, kvol, cap_out, relu,
                  (unsigned int)in_bytes, (unsigned int)w_bytes, (unsigned int)nbr_bytes, (unsigned int)tile_masks_words(cap_out) * 4u};
    const SpHVariant v = spconv_h_select(cin, cout, true, true);
    if (v == SH_NONE) {
        set_error("dz_spconv_forward_split_packed: %d -> %d channels (the packed table feeds the 16 -> 16, 16 -> 32 and 32 -> 32 kernels)", cin, cout);
        return DZ_ERR_UNSUPPORTED;
    }
    return kSpH[v].launch[math - 1](a, stream);
}

const char *dz_spconv_variant_split(int cin, int cout) {
    return kSpH[spconv_h_select(cin, cout, false, true)].name;        // (dz_build_neighbors always writes the table's tile masks)
}

const char *dz_spconv_variant_split_packed(int cin, int cout) {
    return kSpH[spconv_h_select(cin, cout, true, true)].name;
}

const char *dz_spconv_variant_split_arm(int cin, int cout, int kvol, int has_tile_masks, size_t nbr_bytes) {
    (void)kvol;
    return kSpH[spconv_h_select(cin, cout, false, has_tile_masks && nbr_bytes > 0 && nbr_bytes < 0x80000000ull)].arm;
}

}  // extern "C"
