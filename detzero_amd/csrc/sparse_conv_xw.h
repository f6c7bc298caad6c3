// The frame shared by the two x-run kernels of the exact-fp32 mode, k_spconv_xf (sparse_conv_xf.hip: fp32 MFMA) and k_spconv_xt
// (sparse_conv_xt.hip: three bf16 limbs per operand): everything the INDEX decides - the unit, its windows and the zero rows behind
// them, the packed table words, the direct load of a window run - and everything behind the step loop - the epilogue with its write
// contract, the launch, the checks of the C entry points.  What a step's weights are and what a tap does with its operand is each
// kernel's own; the step loop, with the operand fetch of a tap, stays written out in each file (moved here, the compiler's code for
// the loop changes).  A configuration C is an XFCfg / XTCfg: UR, RCAP, SPS, WC, CT, COUT, THREADS, OFF_WIN, WIN_BYTES, LDS_BYTES.
#pragma once
#include "hgemm.h"

namespace dz {

struct SpConvXWArgs {
    const float *in;            // fp32 rows (in_rows, cin)
    const int *nbr;             // packed table (9, cap), in tap-set order when perm is given
    const int *win;             // (units, 3, 2): first input row, row count of the window of (unit, tz)
    const int *d_m_out;
    const float *w;             // k_spconv_xf: (27, cin, cout) fp32; k_spconv_xt: (27, cout, cin / 8, 3 x 16 B) limb words
    const float *scale, *shift, *residual;
    float *out;
    const int *perm;            // output row of each position when the table is in tap-set order, or null
    int cin, cout, cap, relu;
    unsigned int in_bytes, w_bytes;
};

__device__ __forceinline__ int xw_pick(const int (&v)[3], int z) { return z == 0 ? v[0] : (z == 1 ? v[1] : v[2]); }

// What a workgroup knows of its unit before the first step.  Constructed by all threads of a unit that has a row below m.
template <class C>
struct XWUnit {
    int nk;                         // 16-channel chunks of a row
    unsigned int row_bytes;
    srsrc_t prsrc;
    int wlo[3], wn[3];              // windows of the unit: (first row, rows) per z slab
    int zlist, nz;                  // the slabs that have any neighbour, in order, two bits each (the centre slab always has)
    int pos;                        // my row (position) of the level
    unsigned int pw[9];             // packed table words of my row, all nine (tz, ty) lines
    int lrow;                       // direct loads: my row and source piece of a window run (below)
    unsigned int lpiece;

    __device__ __forceinline__ XWUnit(const SpConvXWArgs &a, unsigned char *smem, int m, int wid, int lane)
        : nk(a.cin / 16), row_bytes((unsigned int)a.cin * 4u), prsrc(make_srsrc(a.in, a.in_bytes)) {
        const int tid = threadIdx.x, unit = blockIdx.x;
        // the zero rows of the two window buffers
        if (tid < 32) reinterpret_cast<unsigned int *>(smem + C::OFF_WIN + (tid >> 4) * C::WIN_BYTES + C::RCAP * 64)[tid & 15] = 0u;
#pragma unroll
        for (int z = 0; z < 3; ++z) {
            wlo[z] = __builtin_amdgcn_readfirstlane(a.win[(size_t)unit * 6 + 2 * z]);
            wn[z] = __builtin_amdgcn_readfirstlane(a.win[(size_t)unit * 6 + 2 * z + 1]);
        }
        zlist = 0, nz = 0;
#pragma unroll
        for (int z = 0; z < 3; ++z)
            if (wn[z] > 0) { zlist |= z << (2 * nz); ++nz; }
        // zero = no neighbour for positions past the level's end
        pos = unit * C::UR + (wid / C::WC) * 32 + (lane & 31);
#pragma unroll
        for (int g = 0; g < 9; ++g) pw[g] = pos < m ? (unsigned int)a.nbr[(size_t)g * a.cap + pos] : 0u;
        // lane L of a 1 KB direct load writes LDS bytes [16 L, 16 L + 16) of its run.  Window runs = 16 rows x 64 bytes: row L >> 2,
        // slot L & 3, which holds source piece slot ^ ((row >> 2) & 3), and (row >> 2) & 3 == (L >> 4) & 3 because runs start at
        // multiples of 16 rows.
        lrow = lane >> 2;
        lpiece = (unsigned int)((lane & 3) ^ ((lane >> 4) & 3)) << 4;
    }

    // step i: stage st = i / SPS = (slab tz, chunk kc), r = i % SPS
    __device__ __forceinline__ void stage_of(int i, int &tz, int &kc, int &r) const {
        const int st = i / C::SPS;
        r = i - st * C::SPS;
        const int zi = st / nk;
        kc = st - zi * nk;
        tz = (zlist >> (2 * zi)) & 3;
    }

    // run j (16 rows) of the window of stage st (n rows from input row lo), chunk kc -> LDS.  A wave stages runs j < (n + 15) >> 4 of a
    // window of n <= RCAP rows, so the zero row is never overwritten.
    __device__ __forceinline__ void load_window_run(int st, int j, int lo, int n, int kc) const {
        // (rows past the window's end re-read its last row: inside the input, never referenced)
        const int left = n - 1 - j * 16;
        const unsigned int voff = (unsigned int)min(lrow, left) * row_bytes + lpiece;
        load16_lds((unsigned int)(C::OFF_WIN + (st & 1) * C::WIN_BYTES) + (unsigned int)j * 1024u, voff, prsrc,
                   (unsigned int)(lo + j * 16) * row_bytes + (unsigned int)(kc * 64));
    }
};

// Epilogue: out = relu?(acc * scale + shift (+ residual)), as dz_spconv_forward.  Register quad j of fragment ct = channels
// ct*32 + 8 j + 4 kh .. + 3 of my row, 16 bytes per store; rows at or beyond m are never written.
template <class C>
__device__ __forceinline__ void xw_epilogue(const SpConvXWArgs &a, const f32x16 (&acc)[C::CT], int pos, int m, int wc, int kh) {
    constexpr int CT = C::CT, COUT = C::COUT;
    if (pos >= m) return;
    const int orow = a.perm ? a.perm[pos] : pos;
    const size_t rbase = (size_t)orow * COUT;
    // (per 32-channel fragment all of scale / shift / residual are requested before the first is used: one memory round trip, not twelve)
    const bool has_sc = a.scale != nullptr, has_sh = a.shift != nullptr, has_res = a.residual != nullptr;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        float4 sc[4], sh[4], rs[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ch = wc * CT * 32 + ct * 32 + j * 8 + kh * 4;
            sc[j] = has_sc ? *reinterpret_cast<const float4 *>(a.scale + ch) : make_float4(1.f, 1.f, 1.f, 1.f);
            sh[j] = has_sh ? *reinterpret_cast<const float4 *>(a.shift + ch) : make_float4(0.f, 0.f, 0.f, 0.f);
            rs[j] = has_res ? *reinterpret_cast<const float4 *>(a.residual + rbase + ch) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ch = wc * CT * 32 + ct * 32 + j * 8 + kh * 4;
            float4 v = make_float4(fmaf(acc[ct][4 * j], sc[j].x, sh[j].x), fmaf(acc[ct][4 * j + 1], sc[j].y, sh[j].y),
                                   fmaf(acc[ct][4 * j + 2], sc[j].z, sh[j].z), fmaf(acc[ct][4 * j + 3], sc[j].w, sh[j].w));
            if (has_res) { v.x += rs[j].x; v.y += rs[j].y; v.z += rs[j].z; v.w += rs[j].w; }
            if (a.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            *reinterpret_cast<float4 *>(a.out + rbase + ch) = v;
        }
    }
}

// ---- host side.  `who` is the C entry point, for its messages.
template <void (*K)(SpConvXWArgs), class C>
static int launch_xw(const SpConvXWArgs &a, hipStream_t stream, const char *who) {
    static PerDeviceFlags done;
    if (int rc = reserve_lds(reinterpret_cast<const void *>(K), C::LDS_BYTES, done, who)) return rc;
    hipLaunchKernelGGL(K, dim3(ceil_div(a.cap, C::UR)), dim3(C::THREADS), C::LDS_BYTES, stream, a);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

// The configurations of an engine, by channel count (cin == cout).  unit_rows = dz_spconv_x_tile_rows of the pair16 engine's shipped
// configurations: one index serves every arithmetic.
struct XWVariant {
    int channels, unit_rows, window_rows;
    const char *name;
    int (*launch)(const SpConvXWArgs &, hipStream_t, const char *who);
};

template <size_t N>
static const XWVariant *xw_select(const XWVariant (&table)[N], int cin, int cout) {
    for (const XWVariant &v : table)
        if (cin == cout && cout == v.channels) return &v;
    return nullptr;
}

// The checked front of both entry points: v = the engine's row for (cin, cout) or null, w_bytes = the size of its weights.
static int xw_forward(const char *who, const XWVariant *v, size_t w_bytes, const float *in, int in_rows, int cin, const int *nbr_packed,
                      const int *perm, int *windows, int tile_rows, int cap_out, const int *d_m_out, const float *w, const float *scale,
                      const float *shift, const float *residual, int relu, float *out, int cout, void *stream) {
    DZ_CHECK_ARG(in && nbr_packed && windows && d_m_out && w && out, "%s: null pointer", who);
    if (!v) {
        set_error("%s: %d -> %d channels (submanifold 32 -> 32, 64 -> 64, 128 -> 128 only)", who, cin, cout);
        return DZ_ERR_UNSUPPORTED;
    }
    DZ_CHECK_ARG(tile_rows == v->unit_rows, "%s: windows built for %d-row tiles, the %d-channel kernel uses %d", who, tile_rows, cout, v->unit_rows);
    DZ_CHECK_ARG(cap_out >= 0 && cap_out < (1 << 29), "%s: capacity %d outside the packed table's 29-bit ranks", who, cap_out);
    const size_t in_bytes = (size_t)(in_rows < 0 ? 0 : in_rows) * cin * sizeof(float), out_bytes = (size_t)cap_out * cout * sizeof(float);
    if (in_rows < 0 || in_bytes >= 0x80000000ull || out_bytes >= 0x80000000ull) {
        set_error("%s: input of %zu / output of %zu bytes exceeds the 2 GiB buffer-addressing limit", who, in_bytes, out_bytes);
        return DZ_ERR_UNSUPPORTED;
    }
    if (cap_out == 0) return DZ_OK;
    const SpConvXWArgs a{in, nbr_packed, windows, d_m_out, w, scale, shift, residual, out, perm, cin, cout, cap_out, relu,
                         (unsigned int)in_bytes, (unsigned int)w_bytes};
    return v->launch(a, (hipStream_t)stream, who);
}

}  // namespace dz
