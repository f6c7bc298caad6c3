// 3x3 stride-1 dense BEV convolution of the exact-fp32 mode on the bf16 matrix pipe: every fp32 operand as THREE bf16 limbs.
//
// Any finite fp32 value x is exactly the sum of three bf16 values
//        h = rn(x),   m = rn(x - h),   l = x - h - m                      (8 + 8 + 8 = 24 significant bits)
// because each remainder is exact in fp32 and is at most half an ulp of the limb before it.  Every bf16 x bf16 product is exact
// in fp32, so a product x.w evaluated as
//        h.h + h.m + m.h + h.l + l.h + m.m                                 (six v_mfma_f32_32x32x16_bf16, fp32 accumulation)
// misses only m.l + l.m + l.l, at most 2^-26 of |x.w|: fp32-class arithmetic, in another accumulation order than k_conv2d.
// Saturation: x is clamped to +-bf16-max (0x7F7F) before the FIRST rounding only (the rule of MathF16::split), so a finite fp32
// near the top of the range gets no inf limb: the rest goes to m and l, and the sum stays exact.
// Tiny values: for |x| < 2^-100 the l limb (below 2^-109 the m limb too) is a bf16 subnormal.  Measured on an MI355X: the bf16 MFMA
// KEEPS subnormal inputs - with inputs of exponent [-120, -104] against one-hot weights every output equals (h + m + l) . w bit for
// bit, none the value with those limbs flushed (test_subnormal_limbs_are_measured).  Below 2^-110 the split itself
// stops being exact (bf16's quantum there is 2^-133): the result is then within 2^-133 |w| of x . w.
//
// No tensor format: activations stay the fp32 zero-bordered channel-last images of the f32 engine (same HBM bytes).  The scheme
// is conv3x3_h.hip's: a 512-thread workgroup owns 8 rows x 32 columns of output pixels x BC output channels and keeps the tile's
// 10 x 34 input pixels of the current 32-channel chunk resident in LDS - loaded as fp32 and split by VALU into three bf16 planes on
// their way in (once per staged value; nine taps x BC channels reuse it).  All nine taps take their operand fragments from those
// planes at a row / column offset.  The weights are split at plan time (ops.pack_weight_limb3: per 8 input channels 16 B of h,
// 16 B of m, 16 B of l) and stream, one tap slice ahead, through registers into double-buffered LDS.
//   LDS row (pixel or output channel) = 4 groups x 48 B + 16 B of padding = 13 x 16 B (odd: conflict-free ds_read_b128)
//   waves: 4 (pairs of image rows) x 2 (halves of BC); wave tile = 2 x 32 pixels x BC/2 channels; 48 (BC = 128) MFMAs per tap
//   persistent workgroups, XCD-banded like k_conv3x3_h; a workgroup keeps one channel tile, its weight stream wraps from tile to tile
#include "hgemm.h"
#include "limb3.h"

namespace dz {

constexpr int T3_TW = 32, T3_KC = 32, T3_NT = 512;
constexpr int T3_GRP_U4 = 3;                                      // one 8-channel group: h, m, l
constexpr int T3_ROW_U4 = (T3_KC / 8) * T3_GRP_U4 + 1;            // 208-byte LDS rows
constexpr int T3_PXW = T3_TW + 2;

template <int BC>
struct T3Cfg {
    static constexpr int PT = 2, WC = 2;
    static constexpr int WP = T3_NT / 64 / WC;                    // row pairs
    static constexpr int TH = WP * PT;                            // tile height (8)
    static constexpr int CT = BC / (32 * WC);                     // 32-channel fragments per wave
    static constexpr int PXH = TH + 2, PX_ROWS = T3_PXW * PXH, PX_PIECES = PX_ROWS * (T3_KC / 4);   // 16-byte fp32 pieces of the input tile
    static constexpr int PXPT = (PX_PIECES + T3_NT - 1) / T3_NT;
    static constexpr int W_ROW_PIECES = (T3_KC / 8) * T3_GRP_U4;  // 16-byte pieces of a weight row's chunk (12)
    static constexpr int W_PIECES = BC * W_ROW_PIECES;
    static constexpr int WPT = (W_PIECES + T3_NT - 1) / T3_NT;
    static constexpr int W_U4 = BC * T3_ROW_U4;                   // one weight buffer
    static constexpr int LDS_MAIN_BYTES = (PX_ROWS * T3_ROW_U4 + 2 * W_U4) * 16;
    static constexpr int LDS_BYTES = LDS_MAIN_BYTES + 2 * BC * 4; // + scale / shift of the channel tile
    static_assert(BC == 64 || BC == 128, "BC is 64 or 128");
    static_assert(LDS_BYTES <= 160 * 1024, "tile does not fit the LDS of a CU");
};

template <int BC>
__global__ __launch_bounds__(T3_NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_conv3x3_t(dz_conv2d_desc p, int tiles_x, int tiles_y, unsigned int in_bytes,
                                                                                                unsigned int w_bytes, int pair0, int ny) {
    using C = T3Cfg<BC>;
    constexpr int CT = C::CT, PT = C::PT, WPT = C::WPT, PXPT = C::PXPT, WC = C::WC;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    v4u *const px_s = reinterpret_cast<v4u *>(smem_raw);                     // [340][ROW_U4]
    v4u *const w_s = px_s + C::PX_ROWS * T3_ROW_U4;                          // [2][BC][ROW_U4]
    float *const sc_s = reinterpret_cast<float *>(smem_raw + C::LDS_MAIN_BYTES), *const sh_s = sc_s + BC;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wp = wid / WC, wc = wid % WC;                                  // image-row pair, channel half
    // persistent, XCD-banded (k_conv3x3_h): workgroup b runs on XCD b % 8; XCD k walks the k-th eighth of the pixel tiles, its
    // workgroups side by side; this launch covers the channel tiles pair0 .. pair0 + ny - 1
    const int ntn = p.cout_pad / BC;
    const int npx = p.batch * tiles_x * tiles_y;
    const int xcd = blockIdx.x & 7, jloc = blockIdx.x >> 3, nj = gridDim.x >> 3;
    const int n0 = ((pair0 + jloc % ny) % ntn) * BC;
    const int per_xcd = (npx + 7) >> 3;
    const int band_lo = xcd * per_xcd, band_hi = min(npx, band_lo + per_xcd);
    const int tstep = nj / ny;                                    // workgroups of this XCD that share my channel tile
    int tile = band_lo + jloc / ny;
    if (tstep == 0 || tile >= band_hi) return;

    const __amdgpu_buffer_rsrc_t prsrc = make_rsrc(p.in, in_bytes);
    const __amdgpu_buffer_rsrc_t crsrc = make_rsrc(p.w, w_bytes);
    auto tile_origin = [&](int t, int &ox, int &oy, int &ob) {
        ox = (t % tiles_x) * T3_TW;
        oy = ((t / tiles_x) % tiles_y) * C::TH;
        ob = t / (tiles_x * tiles_y);
    };
    // input pieces of a tile: pixel (y0 + in_off + ry, x0 + in_off + rx) of the padded image, rx < 34, ry < 10.  The tile's origin
    // rides in the scalar offset of the load (which the range check does not see: a piece is fetched only where its pixel lies
    // inside the padded image); pieces past the image edge get an out-of-range voffset and read as zeros.
    struct TileGeo { unsigned int base; int rows, cols; };
    auto tile_geo = [&](int t) {
        int ox, oy, ob;
        tile_origin(t, ox, oy, ob);
        TileGeo g;
        g.base = (unsigned int)((((long)(ob * p.in_hp + oy + p.in_off) * p.in_wp + ox + p.in_off) * p.in_cstride + p.in_coff) * 4);
        g.rows = p.in_hp - (oy + p.in_off);
        g.cols = p.in_wp - (ox + p.in_off);
        return g;
    };
    TileGeo geo = tile_geo(tile), geo_next = geo;
    bool has_next = tile + tstep < band_hi;
    const int prow = tid / (T3_KC / 4), pq = tid % (T3_KC / 4);
    const unsigned int w_row_bytes = (unsigned int)p.cin * 6u;                   // cin / 8 groups of 48 bytes
    const unsigned int tap_bytes = (unsigned int)p.cout_pad * w_row_bytes;
    unsigned int cvoff[WPT];
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
        const int idx = tid + i * T3_NT;
        cvoff[i] = idx < C::W_PIECES ? (unsigned int)(n0 + idx / C::W_ROW_PIECES) * w_row_bytes + (unsigned int)(idx % C::W_ROW_PIECES) * 16u : OOB_OFFSET;
    }
    const int nk = p.cin / T3_KC;

    v4u wreg[WPT];          // weight slice of the next tap
    v4u pst[PXPT];          // input tile (fp32) of the next channel chunk
    // the weight stream: slice (kc, tap) of the current tile lies at byte w_add of a row's tap-0 chunk-0 piece; past the tile's last
    // slice the stream wraps to the next tile's first one (same weights), or - after the last tile - to out-of-range offsets (zeros
    // come back, nothing is fetched)
    unsigned int w_add = 0u;
    bool w_live = true;
    auto issue_w = [&]() {
#pragma unroll
        for (int i = 0; i < WPT; ++i)
            wreg[i] = __builtin_amdgcn_raw_buffer_load_b128(crsrc, (!w_live || cvoff[i] == OOB_OFFSET) ? OOB_OFFSET : cvoff[i] + w_add, 0, 0);
    };
    auto next_w = [&](int kc, int t) {                            // (kc, t): the tap being computed; the stream moves to the one after it
        if (t < 8) { w_add += tap_bytes; return; }
        w_add -= 8u * tap_bytes;
        if (kc + 1 < nk) { w_add += (unsigned int)((T3_KC / 8) * T3_GRP_U4 * 16); return; }
        w_add = 0u;
        w_live = has_next;
    };
    auto store_w = [&](int buf) {
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int idx = tid + i * T3_NT;
            if (C::W_PIECES % T3_NT == 0 || idx < C::W_PIECES) w_s[buf * C::W_U4 + (idx / C::W_ROW_PIECES) * T3_ROW_U4 + idx % C::W_ROW_PIECES] = wreg[i];
        }
    };
    auto issue_px = [&](int kc) {
        // input tile of channel chunk kc; kc == nk: chunk 0 of the next tile
        const bool cur = kc < nk;
        const TileGeo g = cur ? geo : geo_next;
        const unsigned int sbase = g.base + (cur ? (unsigned int)(kc * T3_KC * 4) : 0u);
        const bool any = cur || has_next;
#pragma unroll
        for (int i = 0; i < PXPT; ++i) {
            const int r = prow + i * (T3_NT / (T3_KC / 4));
            const int ry = r / T3_PXW, rx = r - ry * T3_PXW;
            const bool ok = any && r < C::PX_ROWS && ry < g.rows && rx < g.cols;
            const unsigned int off = ok ? (unsigned int)(((ry * p.in_wp + rx) * p.in_cstride + pq * 4) * 4) : OOB_OFFSET;
            pst[i] = __builtin_amdgcn_raw_buffer_load_b128(prsrc, off, sbase, 0);
        }
    };
    auto store_px = [&]() {
        // 4 fp32 channels of a pixel -> 8 bytes in each of the three planes of their 8-channel group
#pragma unroll
        for (int i = 0; i < PXPT; ++i) {
            const int r = prow + i * (T3_NT / (T3_KC / 4));
            if (r < C::PX_ROWS) {
                uint2 h, m, l;
                split3x2(__uint_as_float(pst[i].x), __uint_as_float(pst[i].y), h.x, m.x, l.x);
                split3x2(__uint_as_float(pst[i].z), __uint_as_float(pst[i].w), h.y, m.y, l.y);
                unsigned char *d = reinterpret_cast<unsigned char *>(px_s + r * T3_ROW_U4 + (pq >> 1) * T3_GRP_U4) + (pq & 1) * 8;
                *reinterpret_cast<uint2 *>(d) = h;
                *reinterpret_cast<uint2 *>(d + 16) = m;
                *reinterpret_cast<uint2 *>(d + 32) = l;
            }
        }
    };

    f32x16 acc[CT][PT];
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < CT; ++i)
#pragma unroll
            for (int j = 0; j < PT; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    };
    zero_acc();

    // fragment base addresses (16-byte units): pixel fragment pt = image row 2*wp + pt, column lane & 31; k group = lane >> 5
    const int kg = (lane >> 5) * T3_GRP_U4;
    const int pbase = ((PT * wp) * T3_PXW + (lane & 31)) * T3_ROW_U4 + kg;
    const int wbase = (wc * CT * 32 + (lane & 31)) * T3_ROW_U4 + kg;
    struct Frag { v4u pf[PT][3], cf[CT][3]; };
    auto load_frag = [&](Frag &f, int tap, int buf, int q) {
        const int ky = tap / 3, kx = tap - ky * 3;
        const v4u *pp = px_s + pbase + (ky * T3_PXW + kx) * T3_ROW_U4 + q * 2 * T3_GRP_U4;
#pragma unroll
        for (int pt = 0; pt < PT; ++pt)
#pragma unroll
            for (int s = 0; s < 3; ++s) f.pf[pt][s] = pp[pt * T3_PXW * T3_ROW_U4 + s];
        const v4u *cp = w_s + buf * C::W_U4 + wbase + q * 2 * T3_GRP_U4;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int s = 0; s < 3; ++s) f.cf[ct][s] = cp[ct * 32 * T3_ROW_U4 + s];
    };
    auto mma = [&](const Frag &f) {
        // term-major, so consecutive MFMAs go to different accumulators
        limb3_terms([&](auto wl, auto xl) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = MathBF16::mma(f.cf[ct][wl], f.pf[pt][xl], acc[ct][pt]);
        });
    };
    auto tap_mma = [&](int tap, int buf) {
        // both k-steps' fragments are requested up front: the second set lands under the first set's MFMAs
        Frag f0, f1;
        load_frag(f0, tap, buf, 0);
        load_frag(f1, tap, buf, 1);
        mma(f0);
        mma(f1);
    };

    if (tid < BC) {
        const bool in = n0 + tid < p.g_cout[0];
        sc_s[tid] = (in && p.scale) ? p.scale[n0 + tid] : 1.f;
        sh_s[tid] = (in && p.shift) ? p.shift[n0 + tid] : 0.f;
    }
    // ---- prologue: input tile of chunk 0 and the weight slice of (chunk 0, tap 0) into LDS
    issue_px(0);
    issue_w();
    store_px();
    store_w(0);
    __syncthreads();

    int par = 0;                                                  // LDS weight buffer of the current tap
    for (;;) {
        if (has_next) geo_next = tile_geo(tile + tstep);
        for (int kc = 0; kc < nk; ++kc) {
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                next_w(kc, t);
                issue_w();                                        // next tap's slice: lands during this tap's MFMAs
                if (t == 0) issue_px(kc + 1);                     // next chunk's input tile: lands during this chunk's nine taps
                tap_mma(t, par);
                store_w(par ^ 1);
                __syncthreads();
                if (t == 8) {
                    // channel-chunk boundary: every wave is past its last read of the old planes; split the prefetched tile in
                    store_px();
                    __syncthreads();
                }
                par ^= 1;
            }
        }
        // ---- epilogue: 32x32 accumulator: pixel column = lane & 31, channel = 8*(reg>>2) + 4*(lane>>5) + (reg&3)
        {
            int x0, y0, b;
            tile_origin(tile, x0, y0, b);
            int h = lane >> 5;
            asm volatile("" : "+v"(h));                           // (likewise: keeps the epilogue's addresses out of the main loop's registers)
            int gcout = p.g_cout[0];
            // (opaque per tile: the channel predicates below are loop-invariant lane masks, and hoisted out of the tile loop they
            // occupy some 80 scalar registers for the whole kernel)
            asm volatile("" : "+s"(gcout));
            const int ooff = p.out_coff + p.g_ooff[0];
            const bool vec = ((p.out_cstride | ooff) & 3) == 0;   // 16-byte aligned quads
#pragma unroll
            for (int pt = 0; pt < PT; ++pt) {
                const int y = y0 + PT * wp + pt, x = x0 + (lane & 31);
                if (y >= p.ho || x >= p.wo) continue;
                const size_t op = ((size_t)b * p.out_hp + (size_t)y * p.out_sy + p.out_dy) * p.out_wp + (size_t)x * p.out_sx + p.out_dx;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int col = n0 + wc * CT * 32 + ct * 32 + 8 * j + 4 * h;
                        if (col >= gcout) continue;
                        float *o = p.out + op * p.out_cstride + ooff + col;
                        float v[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int lc = col - n0 + e;
                            v[e] = fmaf(acc[ct][pt][4 * j + e], sc_s[lc], sh_s[lc]);
                            if (p.relu) v[e] = fmaxf(v[e], 0.f);
                        }
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
        // ---- next tile: its first input chunk is already in LDS, its first weight slice too
        if (!has_next) break;
        tile += tstep;
        geo = geo_next;
        has_next = tile + tstep < band_hi;
        zero_acc();
    }
}

static bool limb3_ok(const dz_conv2d_desc &p) {
    if (p.kh != 3 || p.kw != 3 || p.stride != 1 || p.groups != 1) return false;
    if (p.cin <= 0 || p.cin % T3_KC != 0 || p.cout_pad <= 0 || p.cout_pad % 64 != 0) return false;
    if (p.phase_groups || p.in_rowidx || p.in_tiles || p.group_shift || p.group_max) return false;
    if (p.batch < 0 || p.in_hp <= 0 || p.in_wp <= 0 || p.in_cstride <= 0) return false;
    const size_t in_bytes = (size_t)p.batch * p.in_hp * p.in_wp * p.in_cstride * sizeof(float);
    const size_t w_bytes = (size_t)9 * p.cout_pad * p.cin * 6;
    return in_bytes < 0x80000000ull && w_bytes < 0x80000000ull;
}

// the fill rule of conv3x3_h_variant: the 128-channel tile wherever the padded channel count allows it
static int limb3_bc(const dz_conv2d_desc &p) { return !limb3_ok(p) ? 0 : (p.cout_pad % 128 == 0 ? 128 : 64); }

template <int BC>
static int launch_t3(const dz_conv2d_desc &p, hipStream_t stream) {
    using C = T3Cfg<BC>;
    const int tiles_x = ceil_div(p.wo, T3_TW), tiles_y = ceil_div(p.ho, C::TH);
    const size_t in_bytes = (size_t)p.batch * p.in_hp * p.in_wp * p.in_cstride * sizeof(float);
    const size_t w_bytes = (size_t)9 * p.cout_pad * p.cin * 6;
    static PerDeviceFlags lds_done;
    if (int rc_ = reserve_lds(reinterpret_cast<const void *>(&k_conv3x3_t<BC>), C::LDS_BYTES, lds_done, "dz_conv3x3_limb3_forward")) return rc_;
    // persistent: one workgroup per CU; every XCD runs a multiple of the channel-tile count.  With 3 tiles (the head's 64 -> 384
    // layer) that is 30 of 32 workgroups: such a layer runs as two launches over 2 + 1 tiles, each on all 256 CUs (launch_c3's rule)
    const int nty = p.cout_pad / BC;
    const int slots = 32;
    int parts[2][2] = {{0, nty}, {0, 0}};
    const long pair_tiles = (long)p.batch * tiles_x * tiles_y * nty;
    if (slots % nty != 0 && nty < slots && pair_tiles >= 5000) {
        int a = 1;
        while (a * 2 <= nty) a *= 2;
        if (slots % a == 0 && slots % (nty - a) == 0) { parts[0][1] = a; parts[1][0] = a; parts[1][1] = nty - a; }
    }
    for (int k = 0; k < 2 && parts[k][1] > 0; ++k) {
        const int ny = parts[k][1];
        int per_xcd = slots / ny * ny;
        if (per_xcd < ny) per_xcd = ny;
        hipLaunchKernelGGL((k_conv3x3_t<BC>), dim3((unsigned int)(8 * per_xcd)), dim3(T3_NT), C::LDS_BYTES, stream, p, tiles_x, tiles_y,
                           (unsigned int)in_bytes, (unsigned int)w_bytes, parts[k][0], ny);
        DZ_LAUNCH_CHECK();
    }
    return DZ_OK;
}

}  // namespace dz

using namespace dz;

extern "C" {

int dz_conv3x3_limb3_supported(const dz_conv2d_desc *d) { return d && limb3_ok(*d) ? 1 : 0; }

const char *dz_conv3x3_limb3_variant(const dz_conv2d_desc *d) {
    const int bc = d ? limb3_bc(*d) : 0;
    return bc == 128 ? "k_conv3x3_t<8x32x128>" : bc == 64 ? "k_conv3x3_t<8x32x64>" : "none";
}

int dz_conv3x3_limb3_forward(const dz_conv2d_desc *d, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(d, "dz_conv3x3_limb3_forward: null descriptor");
    const int bc = limb3_bc(*d);
    if (!bc) {
        set_error("dz_conv3x3_limb3_forward: not a plain 3x3 stride-1 layer with cin %% 32 == 0, cout_pad %% 64 == 0 inside the 2 GiB window "
                  "(k %dx%d stride %d groups %d cin %d cout_pad %d)", d->kh, d->kw, d->stride, d->groups, d->cin, d->cout_pad);
        return DZ_ERR_UNSUPPORTED;
    }
    DZ_CHECK_ARG(d->in && d->out && d->w, "dz_conv3x3_limb3_forward: null pointer");
    DZ_CHECK_ARG(d->batch >= 0 && d->ho >= 0 && d->wo >= 0, "dz_conv3x3_limb3_forward: negative extent");
    DZ_CHECK_ARG(d->in_cstride % 4 == 0 && d->in_coff % 4 == 0 && d->in_coff >= 0 && d->in_coff + d->cin <= d->in_cstride,
                 "dz_conv3x3_limb3_forward: input channels [%d, %d) must lie inside the row of %d at 16-byte alignment", d->in_coff,
                 d->in_coff + d->cin, d->in_cstride);
    DZ_CHECK_ARG(d->g_cout[0] >= 1 && d->g_cout[0] <= d->cout_pad, "dz_conv3x3_limb3_forward: bad g_cout[0]");
    DZ_CHECK_ARG(d->out_coff + d->g_ooff[0] >= 0 && d->out_coff + d->g_ooff[0] + d->g_cout[0] <= d->out_cstride,
                 "dz_conv3x3_limb3_forward: output channels leave the row of %d", d->out_cstride);
    if ((long)d->batch * d->ho * d->wo == 0) return DZ_OK;
    // the last tap of the last enumerated pixel must stay inside the input image
    DZ_CHECK_ARG(d->ho - 1 + d->in_off + 2 < d->in_hp && d->wo - 1 + d->in_off + 2 < d->in_wp && d->in_off >= 0,
                 "dz_conv3x3_limb3_forward: taps leave the input image");
    DZ_CHECK_ARG(d->out_sy >= 0 && d->out_sx >= 0 && d->out_dy >= 0 && d->out_dx >= 0 && (d->ho - 1) * d->out_sy + d->out_dy < d->out_hp &&
                 (d->wo - 1) * d->out_sx + d->out_dx < d->out_wp,
                 "dz_conv3x3_limb3_forward: output leaves the output image");
    return bc == 128 ? launch_t3<128>(*d, stream) : launch_t3<64>(*d, stream);
}

}  // extern "C"
