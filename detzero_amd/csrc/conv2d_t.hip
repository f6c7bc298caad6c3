// Generic dense BEV convolution of the exact-fp32 mode on the bf16 matrix pipe (gfx950): the layers conv3x3_t.hip does not take - 3 x 3
// with stride 2, the 1 x 1 deblock phases (output stride 1 or 2), the head's grouped output layer - and any plain layer as well.
// fp32 images in and out exactly as k_conv2d (conv2d.hip) reads and writes them, no tensor format; every operand as THREE exact bf16
// limbs (limb3.h: h = rn(x), m = rn(x - h), l = x - h - m, the clamp before the first rounding only), six v_mfma_f32_32x32x16_bf16
// per product with fp32 accumulation.
// Reference call sites: detection/detzero_det/models/centerpoint_modules/backbone2d.py:33-120, center_head.py:14-48.
//
// Skeleton (k_spconv_gt's, sparse_conv_gt.hip, with computed addresses instead of a neighbour table): an output-stationary tile of
// BP output pixels x BC output channels; rows m = (b, y, x) over batch * ho * wo, the input pixel of tap (0, 0) and the output pixel
// exactly k_conv2d's mapping; blockIdx.x = row tile, blockIdx.y = (group, channel tile).  A chunk is one tap x KC channels.
// A side: fp32 buffer loads into registers one chunk ahead; a thread owns two adjacent 16-byte pieces (8 channels) of a row, runs
// 4 x split3x2 ONCE per value on its way into LDS and writes one 48-byte group (16 B of h, 16 of m, 16 of l).  Rows at or beyond
// m_total use the out-of-range buffer offset: zeros come back, nothing is stored for them.  B side: the weights arrive limb-packed
// (ops.pack_weight_limb3 on (groups * taps, cin, cout_pad) with cout_mult = 32: per (group, tap) round_up(cout_pad, 32) output-channel
// rows of cin / 8 groups of 48 bytes) and are staged verbatim; rows of a channel tile past the packed ones read as zeros.
// An LDS row is KC / 8 groups + 16 bytes of padding (208 B at KC = 32, 112 at KC = 16: an odd number of 16-byte slots, conflict-free
// ds_read_b128 over 16 consecutive rows).  Double-buffered LDS, one barrier per chunk.  A fragment read is 3 x 16 B per operand: lane
// (row l & 31, half l >> 5) holds the limbs of channels 8 half .. 8 half + 7 of a 16-channel k-step; D[cout x pixel], so a register
// quad of the accumulator is four consecutive output channels of one pixel and the epilogue stores fp32 straight from registers -
// as float4 where the output row allows it (out_cstride and the channel offset multiples of 4, the quad inside g_cout), word by word
// otherwise (the head map has 12 columns).
//
// Accumulation order per output element (fixed; independent of the tile a pixel falls into and of scheduling): taps ascending
// (ky, then kx: the OUTER loop), KC-channel slices ascending inside a tap, 16-channel k-steps ascending inside a slice, and per k-step
// the six terms (weight limb . input limb)
//        l.h  h.l  m.m  m.h  h.m  h.h          (smallest first, the order of conv3x3_t.hip and sparse_conv_gt.hip)
// added onto the element's ONE accumulator; dropped: m.l + l.m + l.l, at most 2^-26 of |x.w|.  Two launches agree bit for bit.
// (KC is a multiple of 16 and slices follow each other inside a tap, so the order is "taps, then channels in steps of 16" for every
// instance.)  Tiny values: as in conv3x3_t.hip - the bf16 MFMA keeps subnormal limbs (measured).
//
// Instances (BP x BC x KC, waves; VGPRs + AGPRs from the compiler's resource report; every workgroup is 256 threads = one wave per SIMD):
//   k_conv2d_t<128x128x16>  2 x 2 waves, wave tile 64 x 64:  108 + 64 registers, 57 344 B LDS   (cout_pad % 128 == 0: the 256-channel layers)
//   k_conv2d_t<128x64x32>   4 x 1 waves, wave tile 32 x 64:   87 + 32 registers, 79 872 B LDS   (other widths above 32)
//   k_conv2d_t<128x32x32>   4 x 1 waves, wave tile 32 x 32:   69 + 16 registers, 66 560 B LDS   (cout_pad 16 / 32: the head's output layer)
// Each allows 2 workgroups per CU: the registers would allow 2 / 4 / 5 waves per SIMD, LDS (160 KB) allows 2 workgroups.  0 bytes of
// scratch, no spilled VGPR (tests/test_conv2d_limb3_build.py reads the report).  BC = 128 re-splits a 256-channel layer's input rows
// twice; a 256-wide tile would be 86 KB at KC = 16 - one workgroup, one wave per SIMD - and was not built.
#include "hgemm.h"
#include "limb3.h"

namespace dz {

// The tile (limb3.h): BP pixels x BC output channels, KC channels of one tap per chunk, WP x WC waves
template <int BP, int BC, int KC, int WP, int WC>
struct C2TTile : Limb3Tile<BP, BC, KC, WP, WC> {};

constexpr int C2T_ROW_MULT = 32;        // output-channel rows per (group, tap) of the packed weights: cout_pad rounded up to this

template <class T>
__global__ __launch_bounds__(T::THREADS) void k_conv2d_t(dz_conv2d_desc p, unsigned int m_total, unsigned int in_bytes, unsigned int w_bytes, int wrows) {
    constexpr int P = T::P_PER_THREAD, C = T::C_PER_THREAD, PT = T::PT, CT = T::CT, G = T::G, ROWB = T::ROWB;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *const Ps0 = smem, *const Cs0 = smem + 2 * T::PS_BYTES;      // [2][PS], [2][CS]

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wp = wid / T::WC, wc = wid % T::WC, l31 = lane & 31, kh = lane >> 5;
    const int ntn = (wrows + T::BC - 1) / T::BC;            // channel tiles per group
    const int grp = blockIdx.y / ntn;
    const int n0 = (blockIdx.y % ntn) * T::BC;
    const unsigned int row0 = blockIdx.x * (unsigned int)T::BP;
    const int taps = p.kh * p.kw;
    const int kchunks = p.cin / T::KC;
    const int nchunks = taps * kchunks;
    const __amdgpu_buffer_rsrc_t prsrc = make_rsrc(p.in, in_bytes), crsrc = make_rsrc(p.w, w_bytes);
    const unsigned int wrow_bytes = (unsigned int)p.cin * 6u;                  // cin / 8 groups of 48 bytes
    const unsigned int tap_bytes = (unsigned int)wrows * wrow_bytes;

    // row m -> (b, y, x): k_conv2d's mapping
    auto in_pixel = [&](unsigned int mrow) {
        const unsigned int x = mrow % (unsigned int)p.wo, t = mrow / (unsigned int)p.wo;
        const unsigned int y = t % (unsigned int)p.ho, b = t / (unsigned int)p.ho;
        return (long)((int)b * p.in_hp + (int)y * p.stride + p.in_off) * p.in_wp + (int)x * p.stride + p.in_off;
    };

    unsigned int cvoff[C], clds[C];         // my pieces of a chunk's weight slice: rows n0 .. n0 + BC - 1 of the group's packed rows
    limb3_weight_pieces<T>(tid, n0, wrows, wrow_bytes, cvoff, clds);
    // my 8-channel groups of the input chunk: byte offset of tap (0, 0), channel slice 0 (fixed for the whole tile), and where the
    // group goes in an LDS buffer
    const long cbase = p.in_coff + (long)grp * p.cin;
    unsigned int pvoff[P], plds[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int idx = tid + i * T::THREADS;
        const int r = idx / G, g = idx % G;
        pvoff[i] = row0 + r < m_total ? (unsigned int)((in_pixel(row0 + r) * p.in_cstride + cbase + g * 8) * 4) : OOB_OFFSET;
        plds[i] = (unsigned int)(r * ROWB + g * 48);
    }
    const int poff = limb3_frag_base<T>(wp, PT, lane), coff = limb3_frag_base<T>(wc, CT, lane);

    f32x16 acc[CT][PT];
    limb3_zero<T>(acc);

    // chunk iterator of the loads, without divisions: taps outermost (ky, kx), channel slices inside a tap
    int ky = 0, kx = 0, kc = 0;
    unsigned int padd = 0u;                                               // input byte offset of the chunk relative to pvoff
    unsigned int cadd = (unsigned int)(grp * taps) * tap_bytes;           // weight byte offset of the chunk relative to cvoff
    auto advance = [&]() {
        cadd += (unsigned int)(G * 48);
        if (++kc == kchunks) {
            kc = 0;
            cadd += tap_bytes - (unsigned int)kchunks * (unsigned int)(G * 48);
            if (++kx == p.kw) { kx = 0; ++ky; }
        }
        padd = (unsigned int)(((ky * p.in_wp + kx) * p.in_cstride + kc * T::KC) * 4);
    };
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
    };
    auto store = [&](int buf) { limb3_store<T>(Ps0 + buf * T::PS_BYTES, Cs0 + buf * T::CS_BYTES, sp, sw, plds, clds); };

    issue();                // chunk 0
    advance();
    store(0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int cur = c & 1;
        const bool has1 = c + 1 < nchunks;
        if (has1) {
            issue();        // chunk c + 1: lands in registers behind this chunk's MFMAs
            advance();
        }
        limb3_mma<T>(Ps0 + cur * T::PS_BYTES + poff, Cs0 + cur * T::CS_BYTES + coff, acc);
        if (has1) store(cur ^ 1);
        __syncthreads();
    }

    // ---- epilogue: register quad j of fragment (ct, pt) = channels ct*32 + 8 j + 4 kh .. + 3 of my pixel
    const int gcout = p.g_cout[grp];
    const int ooff = p.out_coff + p.g_ooff[grp];
    const bool vec = ((p.out_cstride | ooff) & 3) == 0 && (reinterpret_cast<size_t>(p.out) & 15) == 0;       // 16-byte aligned quads
    const bool has_sc = p.scale != nullptr, has_sh = p.shift != nullptr;
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
        const unsigned int mrow = row0 + wp * PT * 32 + pt * 32 + l31;
        if (mrow >= m_total) continue;
        const unsigned int x = mrow % (unsigned int)p.wo, t = mrow / (unsigned int)p.wo;
        const unsigned int y = t % (unsigned int)p.ho, b = t / (unsigned int)p.ho;
        const size_t op = ((size_t)b * p.out_hp + (size_t)y * p.out_sy + p.out_dy) * p.out_wp + (size_t)x * p.out_sx + p.out_dx;
        float *const orow = p.out + op * p.out_cstride + ooff;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            // (scale / shift of the fragment are requested before the first is used: one memory round trip)
            float4 sc[4], sh[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = n0 + wc * CT * 32 + ct * 32 + j * 8 + kh * 4;
                const bool live = col < gcout;                // (col % 4 == 0 and cout_pad % 16 == 0: the quad lies inside the vectors)
                const float *const s = p.scale + grp * p.cout_pad + col, *const b = p.shift + grp * p.cout_pad + col;
                sc[j] = has_sc && live ? make_float4(s[0], s[1], s[2], s[3]) : make_float4(1.f, 1.f, 1.f, 1.f);      // (word loads: the vectors
                sh[j] = has_sh && live ? make_float4(b[0], b[1], b[2], b[3]) : make_float4(0.f, 0.f, 0.f, 0.f);      // need no 16-byte alignment)
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = n0 + wc * CT * 32 + ct * 32 + j * 8 + kh * 4;
                if (col >= gcout) continue;
                float v[4] = {fmaf(acc[ct][pt][4 * j], sc[j].x, sh[j].x), fmaf(acc[ct][pt][4 * j + 1], sc[j].y, sh[j].y),
                              fmaf(acc[ct][pt][4 * j + 2], sc[j].z, sh[j].z), fmaf(acc[ct][pt][4 * j + 3], sc[j].w, sh[j].w)};
                if (p.relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                float *const o = orow + col;
                if (vec && col + 4 <= gcout) {
                    *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (col + e < gcout) o[e] = v[e];
                }
            }
        }
    }
}

// The instances: BP x BC x KC.  LDS is 1.5 x an fp16-pair tile's (limb rows), so the tiles are the ones at which two workgroups still
// share a CU (k_spconv_gt's choice; the register and LDS figures are in the header of this file).  Tried on an MI355X and not kept
// (DESIGN.md 2a-quater): KC = 16 for the 32-channel tile (four workgroups per CU) and an XCD-aware tile order that runs the channel
// tiles of a row tile back to back on one XCD - neither moved a layer by more than 3 % - and a second register set that keeps the loads
// of chunk c + 2 in flight (144 + 64 registers): 4 - 9 % slower on every layer, so the kernel is not waiting for its loads.
using C2T_128_16 = C2TTile<128, 128, 16, 2, 2>;
using C2T_64_32 = C2TTile<128, 64, 32, 4, 1>;
using C2T_32_32 = C2TTile<128, 32, 32, 4, 1>;
static_assert(2 * C2T_128_16::LDS_BYTES <= 160 * 1024 && 2 * C2T_64_32::LDS_BYTES <= 160 * 1024 && 2 * C2T_32_32::LDS_BYTES <= 160 * 1024,
              "two workgroups per CU");

static inline int c2t_wrows(const dz_conv2d_desc &p) { return (p.cout_pad + C2T_ROW_MULT - 1) / C2T_ROW_MULT * C2T_ROW_MULT; }
static inline size_t c2t_in_bytes(const dz_conv2d_desc &p) { return (size_t)p.batch * p.in_hp * p.in_wp * p.in_cstride * sizeof(float); }
static inline size_t c2t_w_bytes(const dz_conv2d_desc &p) { return (size_t)p.groups * p.kh * p.kw * c2t_wrows(p) * p.cin * 6; }

template <class T>
static int launch_c2t(const dz_conv2d_desc &p, hipStream_t stream) {
    static PerDeviceFlags done;
    if (int rc = reserve_lds(reinterpret_cast<const void *>(&k_conv2d_t<T>), T::LDS_BYTES, done, "dz_conv2d_limb3_forward")) return rc;
    const long m_total = (long)p.batch * p.ho * p.wo;
    const int wrows = c2t_wrows(p);
    dim3 grid((unsigned int)ceil_div(m_total, T::BP), (unsigned int)(ceil_div(wrows, T::BC) * p.groups));
    hipLaunchKernelGGL((k_conv2d_t<T>), grid, dim3(T::THREADS), T::LDS_BYTES, stream, p, (unsigned int)m_total, (unsigned int)c2t_in_bytes(p),
                       (unsigned int)c2t_w_bytes(p), wrows);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

enum C2TVariant { C2T_NONE = 0, C2T_V_128_16, C2T_V_64_32, C2T_V_32_32 };
using C2TLaunch = int (*)(const dz_conv2d_desc &, hipStream_t);
struct C2TEntry { const char *name; C2TLaunch launch; };
static const C2TEntry kC2T[] = {
    {"none", nullptr},
    {"k_conv2d_t<128x128x16>", launch_c2t<C2T_128_16>},
    {"k_conv2d_t<128x64x32>", launch_c2t<C2T_64_32>},
    {"k_conv2d_t<128x32x32>", launch_c2t<C2T_32_32>},
};

// The field that keeps a layer off this engine, or nullptr: what dz_conv2d_limb3_supported answers and _forward reports
static const char *c2t_refusal(const dz_conv2d_desc &p) {
    if (p.group_shift) return "group_shift";
    if (p.group_max) return "group_max";
    if (p.phase_groups) return "phase_groups";
    if (p.in_rowidx) return "in_rowidx";
    if (p.in_tiles) return "in_tiles";
    if (p.kh != p.kw || (p.kh != 1 && p.kh != 3)) return "kh / kw (1 x 1 or 3 x 3)";
    if (p.stride != 1 && p.stride != 2) return "stride (1 or 2)";
    if (p.groups < 1 || p.groups > 8) return "groups (1..8)";
    if (p.cin <= 0 || p.cin % 32 != 0) return "cin (a multiple of 32)";
    if (p.cout_pad <= 0 || p.cout_pad % 16 != 0) return "cout_pad (a multiple of 16)";
    if (p.batch < 0 || p.ho < 0 || p.wo < 0 || p.in_hp <= 0 || p.in_wp <= 0 || p.in_cstride <= 0) return "batch / ho / wo / in_hp / in_wp / in_cstride (extent)";
    if (c2t_in_bytes(p) >= 0x80000000ull) return "in (image at or beyond the 2 GiB buffer-addressing limit)";
    if (c2t_w_bytes(p) >= 0x80000000ull) return "w (weights at or beyond the 2 GiB buffer-addressing limit)";
    return nullptr;
}

// The one decision of this engine: a pure function of the descriptor (the channel width alone picks the tile)
static C2TVariant conv2d_t_select(const dz_conv2d_desc &p) {
    if (c2t_refusal(p)) return C2T_NONE;
    if (p.cout_pad % 128 == 0) return C2T_V_128_16;
    if (p.cout_pad > 32) return C2T_V_64_32;
    return C2T_V_32_32;
}

}  // namespace dz

using namespace dz;

extern "C" {

int dz_conv2d_limb3_supported(const dz_conv2d_desc *d) { return d && conv2d_t_select(*d) != C2T_NONE ? 1 : 0; }

const char *dz_conv2d_limb3_variant(const dz_conv2d_desc *d) { return kC2T[d ? conv2d_t_select(*d) : C2T_NONE].name; }

int dz_conv2d_limb3_forward(const dz_conv2d_desc *d, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(d, "dz_conv2d_limb3_forward: null descriptor");
    if (const char *why = c2t_refusal(*d)) {
        set_error("dz_conv2d_limb3_forward: %s is not covered by the bf16x3 engine (k %dx%d stride %d groups %d cin %d cout_pad %d)", why, d->kh,
                  d->kw, d->stride, d->groups, d->cin, d->cout_pad);
        return DZ_ERR_UNSUPPORTED;
    }
    DZ_CHECK_ARG(d->in && d->out && d->w, "dz_conv2d_limb3_forward: null pointer");
    DZ_CHECK_ARG(d->in_cstride % 4 == 0 && d->in_coff % 4 == 0 && d->in_coff >= 0 && d->in_coff + d->groups * d->cin <= d->in_cstride,
                 "dz_conv2d_limb3_forward: input channels [%d, %d) must lie inside the row of %d at 16-byte alignment", d->in_coff,
                 d->in_coff + d->groups * d->cin, d->in_cstride);
    for (int g = 0; g < d->groups; ++g) {
        DZ_CHECK_ARG(d->g_cout[g] >= 1 && d->g_cout[g] <= d->cout_pad, "dz_conv2d_limb3_forward: bad g_cout[%d]", g);
        DZ_CHECK_ARG(d->out_coff + d->g_ooff[g] >= 0 && d->out_coff + d->g_ooff[g] + d->g_cout[g] <= d->out_cstride,
                     "dz_conv2d_limb3_forward: output channels of group %d leave the row of %d", g, d->out_cstride);
    }
    if ((long)d->batch * d->ho * d->wo == 0) return DZ_OK;
    // the last tap of the last enumerated pixel must stay inside the input image
    DZ_CHECK_ARG((d->ho - 1) * d->stride + d->in_off + d->kh - 1 < d->in_hp && (d->wo - 1) * d->stride + d->in_off + d->kw - 1 < d->in_wp &&
                 d->in_off >= 0, "dz_conv2d_limb3_forward: taps leave the input image");
    DZ_CHECK_ARG(d->out_sy >= 0 && d->out_sx >= 0 && d->out_dy >= 0 && d->out_dx >= 0 && (d->ho - 1) * d->out_sy + d->out_dy < d->out_hp &&
                 (d->wo - 1) * d->out_sx + d->out_dx < d->out_wp,
                 "dz_conv2d_limb3_forward: output leaves the output image");
    return kC2T[conv2d_t_select(*d)].launch(*d, stream);
}

}  // extern "C"
