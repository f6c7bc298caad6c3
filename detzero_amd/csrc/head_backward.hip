// CenterHead: backward through the head's 3 x 3 convolutions (gfx950).  include/detzero_hip.h and DESIGN.md 7q state the contracts.
//
//   k_c3_wgrad       Graw[tap][ci][c] = sum over pixels of x_img[pixel + tap][ci] * g[pixel][c] on the fp32 MFMA (32x32x2): the reduction
//                    index of the GEMM is the pixel, so both operands are read channel-contiguous from the channel-last images - lane l
//                    holds A[i = l & 31][k = l >> 5] (an input channel of one tap at one of two pixels) and B[k][j = l & 31] (an output
//                    channel at that pixel).  A workgroup owns 64 input channels x 9 taps x 64 (32) output channels and a chunk of
//                    16 rows of a band of 32 pixel columns; it keeps a rolling window of three x rows (with the one-pixel halo) and the
//                    g row in LDS, so every x value staged serves all nine taps, and writes its partial to the workspace;
//   k_wgrad_reduce   the chunks' partials in chunk order -> the result.
//   k_relu_grad      g = g_y where y > 0 into the interior of a zero-bordered image, float64 channel sums per workgroup;
//   k_hfb_dgrad      the grouped output layer's data gradient (27 multiply-adds per value) with the hidden layer's mask and sums fused;
//   k_col_sums       float64 column sums of the head map's gradient (the output layer's bias gradient), per workgroup;
//   k_sum_partials   per-workgroup float64 partials in index order -> the sums.
// No floating-point atomics: every sum has a fixed order.  Plain C++ and MFMA builtins only; every store is a vector store.
#include "common.h"

namespace dz {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int WG_TW = DZ_WGRAD_TILE_W;              // pixel columns of a band
constexpr int WG_ROWS = DZ_WGRAD_CHUNK_ROWS;        // rows of a chunk
constexpr int WG_CI = 64;                           // input channels of a workgroup (two row fragments per tap)
constexpr int WG_THREADS = 384;                     // six waves: (ky, half of the 64 input channels); a wave runs the three kx taps
constexpr int WG_XW = WG_TW + 2;                    // staged x pixels of a row
constexpr int WG_XV = WG_XW * WG_CI / 4;            // float4 of a staged x row
constexpr int WG_XLD = (WG_XV + WG_THREADS - 1) / WG_THREADS;
constexpr int WG_MAX_GROUPS = 8;
constexpr int WG_GROUP_PAD = 16;                    // columns of a group in the grouped layout
constexpr int BW_THREADS = 256;
constexpr int BW_MAX_BLOCKS = 1024;                 // workgroups (and partial rows) of the streaming passes
constexpr int HFB_MAX_C = 128;
constexpr int HFB_COLS = 12;                        // columns of a head map
constexpr int HFB_MAX_GCOUT = 3;

template <int NCF>
struct WgradLds {
    float x[3][WG_XW][WG_CI];                       // padded rows py % 3
    float g[WG_TW][NCF * 32];
};
static_assert(sizeof(WgradLds<2>) <= 40 * 1024, "k_c3_wgrad: LDS budget (four workgroups per CU)");
static_assert(WG_XLD == 2 && WG_TW * 64 / 4 <= 2 * WG_THREADS && WG_TW * 32 <= 3 * WG_THREADS, "k_c3_wgrad: staging registers");

struct WgradArgs {
    const float *x, *g;
    float *part;                                    // (chunks, groups, 9, cin, cout_pad)
    int B, H, W, cin, x_cs, g_cs, g_border, cout_pad, groups, bands, row_chunks, ci_slices, co_slices;
    int g_cout[WG_MAX_GROUPS], g_ooff[WG_MAX_GROUPS];
};

// NCF: 32-column fragments of the workgroup's output-channel slice.  GROUPED: the slice is one group's (at most 16) columns, read
// with scalar loads from a map whose rows are not 16-byte multiples; otherwise whole float4.
template <int NCF, bool GROUPED>
__global__ __launch_bounds__(WG_THREADS) void k_c3_wgrad(WgradArgs a) {
    __shared__ WgradLds<NCF> s;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ky = wid >> 1, half = wid & 1, l31 = lane & 31, kp = lane >> 5;
    int chunk = blockIdx.x;
    const int band = chunk % a.bands; chunk /= a.bands;
    const int rc = chunk % a.row_chunks;
    const int b = chunk / a.row_chunks;
    int slice = blockIdx.y;
    const int cis = slice % a.ci_slices; slice /= a.ci_slices;
    const int cos = slice % a.co_slices;
    const int grp = slice / a.co_slices;
    const int x0 = band * WG_TW, y0 = rc * WG_ROWS;
    const int y1 = y0 + WG_ROWS < a.H ? y0 + WG_ROWS : a.H;
    const int ci0 = cis * WG_CI, co0 = cos * (NCF * 32);
    const int Hp = a.H + 2, Wp = a.W + 2;
    const float *xb = a.x + (size_t)b * Hp * Wp * a.x_cs + (size_t)grp * a.cin + ci0;
    const int gW = a.g_border ? Wp : a.W, gH = a.g_border ? Hp : a.H, gd = a.g_border ? 1 : 0;
    const float *gb = a.g + (size_t)b * gH * gW * a.g_cs;
    const int ncol = GROUPED ? a.g_cout[grp] : (a.cout_pad - co0 < NCF * 32 ? a.cout_pad - co0 : NCF * 32);     // columns of the slice
    const int gcol0 = GROUPED ? a.g_ooff[grp] : co0;

    float4 xr[WG_XLD];
    float4 gr4[2];
    float gr1[3];
    // padded row py of the band into registers: pixels x0 .. x0 + 33 (padded), zero beyond the image and beyond cin
    auto load_x = [&](int py) {
#pragma unroll
        for (int j = 0; j < WG_XLD; ++j) {
            const int i = tid + j * WG_THREADS;
            const int px = i >> 4, q = i & 15;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < WG_XV && x0 + px < Wp && ci0 + q * 4 < a.cin)
                v = *reinterpret_cast<const float4 *>(xb + ((size_t)py * Wp + x0 + px) * a.x_cs + q * 4);
            xr[j] = v;
        }
    };
    auto store_x = [&](int slot) {
#pragma unroll
        for (int j = 0; j < WG_XLD; ++j) {
            const int i = tid + j * WG_THREADS;
            if (i < WG_XV) *reinterpret_cast<float4 *>(&s.x[slot][i >> 4][(i & 15) * 4]) = xr[j];
        }
    };
    auto load_g = [&](int y) {
        if (GROUPED) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int i = tid + j * WG_THREADS;
                const int px = i >> 5, c = i & 31;
                float v = 0.f;
                if (i < WG_TW * 32 && x0 + px < a.W && c < ncol) v = gb[((size_t)(y + gd) * gW + x0 + px + gd) * a.g_cs + gcol0 + c];
                gr1[j] = v;
            }
        } else {
            constexpr int QP = NCF * 8;             // float4 per pixel
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int i = tid + j * WG_THREADS;
                const int px = i / QP, q = i % QP;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (i < WG_TW * QP && x0 + px < a.W && q * 4 < ncol)
                    v = *reinterpret_cast<const float4 *>(gb + ((size_t)(y + gd) * gW + x0 + px + gd) * a.g_cs + gcol0 + q * 4);
                gr4[j] = v;
            }
        }
    };
    auto store_g = [&]() {
        if (GROUPED) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int i = tid + j * WG_THREADS;
                if (i < WG_TW * 32) s.g[i >> 5][i & 31] = gr1[j];
            }
        } else {
            constexpr int QP = NCF * 8;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int i = tid + j * WG_THREADS;
                if (i < WG_TW * QP) *reinterpret_cast<float4 *>(&s.g[i / QP][(i % QP) * 4]) = gr4[j];
            }
        }
    };

    f32x16 acc[3][NCF];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int cf = 0; cf < NCF; ++cf)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[kx][cf][r] = 0.f;

    // padded rows y0 and y0 + 1 first; step y then adds padded row y + 2 and the g row y
    load_x(y0);
    store_x(y0 % 3);
    load_x(y0 + 1);
    store_x((y0 + 1) % 3);
    load_x(y0 + 2);
    load_g(y0);
    for (int y = y0; y < y1; ++y) {
        __syncthreads();                            // the previous step has left the slot and the g row
        store_x((y + 2) % 3);
        store_g();
        __syncthreads();
        if (y + 1 < y1) {                           // the next step's loads fly over this step's MFMAs
            load_x(y + 3);
            load_g(y + 1);
        }
        const float *xs = &s.x[(y + ky) % 3][kp][half * 32 + l31];
        const float *gs = &s.g[kp][l31];
#pragma unroll 4
        for (int kk = 0; kk < WG_TW / 2; ++kk) {
            float bv[NCF];
#pragma unroll
            for (int cf = 0; cf < NCF; ++cf) bv[cf] = gs[kk * 2 * (NCF * 32) + cf * 32];
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float av = xs[(kk * 2 + kx) * WG_CI];
#pragma unroll
                for (int cf = 0; cf < NCF; ++cf) acc[kx][cf] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[cf], acc[kx][cf], 0, 0, 0);
            }
        }
    }

    // C/D of the 32x32 forms: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    float *part = a.part + ((size_t)blockIdx.x * a.groups + grp) * 9 * a.cin * a.cout_pad;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int cf = 0; cf < NCF; ++cf) {
            const int co = co0 + cf * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = ci0 + half * 32 + (r & 3) + 8 * (r >> 2) + 4 * kp;
                if (ci < a.cin && co < a.cout_pad) part[((size_t)(ky * 3 + kx) * a.cin + ci) * a.cout_pad + co] = acc[kx][cf][r];
            }
        }
}

__global__ __launch_bounds__(BW_THREADS) void k_wgrad_reduce(const float4 *__restrict__ part, long long nvec, int chunks, float4 *__restrict__ out) {
    const long long step = (long long)gridDim.x * BW_THREADS;
    for (long long i = (long long)blockIdx.x * BW_THREADS + threadIdx.x; i < nvec; i += step) {
        float4 sum = part[i];
        for (int k = 1; k < chunks; ++k) {
            const float4 v = part[(size_t)k * nvec + i];
            sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
        }
        out[i] = sum;
    }
}

// ------------------------------------------------------------------------------------------
// streaming passes: a workgroup walks pixels, a thread owns (pixel slot, four channels); float64 sums
// ------------------------------------------------------------------------------------------
// the threads' four sums -> part[blockIdx][c]: the pixel slots of a channel in slot order
__device__ __forceinline__ void bw_block_sums(const double (&sum)[4], bool active, int ps, int q, int pslots, int c, double *red, double *part) {
    if (active) {
#pragma unroll
        for (int e = 0; e < 4; ++e) red[(size_t)ps * c + q * 4 + e] = sum[e];
    }
    __syncthreads();
    for (int ch = threadIdx.x; ch < c; ch += BW_THREADS) {
        double t = 0.0;
        for (int p = 0; p < pslots; ++p) t += red[(size_t)p * c + ch];
        part[(size_t)blockIdx.x * c + ch] = t;
    }
}

__global__ __launch_bounds__(BW_THREADS) void k_relu_grad(const float *gy, int gy_border, const float *__restrict__ yimg, int B, int H,
                                                           int W, int c, float *gimg, double *__restrict__ part) {      // (gimg may be gy)
    __shared__ double red_s[BW_THREADS * 4];
    const int Q = c >> 2, pslots = BW_THREADS / Q;
    const int tid = threadIdx.x, ps = tid / Q, q = tid - ps * Q;
    const bool active = ps < pslots;
    const long long pixels = (long long)B * H * W;
    const int Wp = W + 2, Hp = H + 2;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    if (active) {
        for (long long p = (long long)blockIdx.x * pslots + ps; p < pixels; p += (long long)gridDim.x * pslots) {
            const int b = (int)(p / ((long long)H * W));
            const int r = (int)(p - (long long)b * H * W);
            const int y = r / W, x = r - y * W;
            const size_t pp = (((size_t)b * Hp + y + 1) * Wp + x + 1) * c + q * 4;
            const float4 yv = *reinterpret_cast<const float4 *>(yimg + pp);
            const float4 gv = *reinterpret_cast<const float4 *>(gy_border ? gy + pp : gy + (size_t)p * c + q * 4);
            float4 o;
            o.x = yv.x > 0.f ? gv.x : 0.f; o.y = yv.y > 0.f ? gv.y : 0.f; o.z = yv.z > 0.f ? gv.z : 0.f; o.w = yv.w > 0.f ? gv.w : 0.f;
            *reinterpret_cast<float4 *>(gimg + pp) = o;
            sum[0] += (double)o.x; sum[1] += (double)o.y; sum[2] += (double)o.z; sum[3] += (double)o.w;
        }
    }
    bw_block_sums(sum, active, ps, q, pslots, c, red_s, part);
}

struct HfbArgs {
    const float *grad_head, *w2, *hidden;
    float *g_hidden;
    double *part;                                   // (blocks, groups * c)
    int B, H, W, c, groups;
    int g_cout[WG_MAX_GROUPS], g_ooff[WG_MAX_GROUPS];
};

__global__ __launch_bounds__(BW_THREADS) void k_hfb_dgrad(HfbArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hfb_lds[];
    // the weights the pass reads, channel-contiguous: w_s[group][tap][column < 3][channel]; then the sums' staging
    const int C = a.groups * a.c, Q = C >> 2, pslots = BW_THREADS / Q, qg = a.c >> 2;
    float *w_s = reinterpret_cast<float *>(hfb_lds);
    double *red_s = reinterpret_cast<double *>(hfb_lds + (size_t)a.groups * 9 * HFB_MAX_GCOUT * a.c * sizeof(float));
    const int tid = threadIdx.x;
    for (int i = tid; i < a.groups * 9 * HFB_MAX_GCOUT * a.c; i += BW_THREADS) {
        const int ch = i % a.c, o = (i / a.c) % HFB_MAX_GCOUT, gt = i / (a.c * HFB_MAX_GCOUT);      // gt = group * 9 + tap
        w_s[i] = o < a.g_cout[gt / 9] ? a.w2[((size_t)gt * a.c + ch) * WG_GROUP_PAD + o] : 0.f;
    }
    __syncthreads();
    const int ps = tid / Q, q = tid - ps * Q;
    const bool active = ps < pslots;
    const int grp = active ? q / qg : 0, ch0 = (q - grp * qg) * 4;
    const int ncol = a.g_cout[grp], off = a.g_ooff[grp];
    const long long pixels = (long long)a.B * a.H * a.W;
    const int Wp = a.W + 2, Hp = a.H + 2;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    if (active) {
        for (long long p = (long long)blockIdx.x * pslots + ps; p < pixels; p += (long long)gridDim.x * pslots) {
            const int b = (int)(p / ((long long)a.H * a.W));
            const int r = (int)(p - (long long)b * a.H * a.W);
            const int y = r / a.W, x = r - y * a.W;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int yo = y - ky + 1;
                if (yo < 0 || yo >= a.H) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int xo = x - kx + 1;
                    if (xo < 0 || xo >= a.W) continue;
                    const float *gh = a.grad_head + (((size_t)b * a.H + yo) * a.W + xo) * HFB_COLS + off;
                    const float *wt = w_s + (size_t)((grp * 9 + ky * 3 + kx) * HFB_MAX_GCOUT) * a.c + ch0;
#pragma unroll
                    for (int o = 0; o < HFB_MAX_GCOUT; ++o) {
                        if (o >= ncol) continue;
                        const float gv = gh[o];
                        const float4 wv = *reinterpret_cast<const float4 *>(wt + o * a.c);
                        acc.x += gv * wv.x; acc.y += gv * wv.y; acc.z += gv * wv.z; acc.w += gv * wv.w;
                    }
                }
            }
            const size_t pp = (((size_t)b * Hp + y + 1) * Wp + x + 1) * C + q * 4;
            const float4 hv = *reinterpret_cast<const float4 *>(a.hidden + pp);
            float4 o;
            o.x = hv.x > 0.f ? acc.x : 0.f; o.y = hv.y > 0.f ? acc.y : 0.f; o.z = hv.z > 0.f ? acc.z : 0.f; o.w = hv.w > 0.f ? acc.w : 0.f;
            *reinterpret_cast<float4 *>(a.g_hidden + pp) = o;
            sum[0] += (double)o.x; sum[1] += (double)o.y; sum[2] += (double)o.z; sum[3] += (double)o.w;
        }
    }
    bw_block_sums(sum, active, ps, q, pslots, C, red_s, a.part);
}

// part[blockIdx][groups * 16]: the float64 sums of the groups' columns of grad_head over the workgroup's cells, 0 in the pad columns
__global__ __launch_bounds__(BW_THREADS) void k_col_sums(HfbArgs a, double *__restrict__ part) {
    __shared__ double red_s[BW_THREADS];
    const int tid = threadIdx.x, slot = tid >> 4, col = tid & 15;      // 16 cell slots x 16 columns (12 used)
    const long long cells = (long long)a.B * a.H * a.W;
    double sum = 0.0;
    bool owned = false;                             // a column no group owns is not loaded
    for (int q = 0; q < a.groups; ++q) owned = owned || (col >= a.g_ooff[q] && col < a.g_ooff[q] + a.g_cout[q]);
    if (owned)
        for (long long p = (long long)blockIdx.x * 16 + slot; p < cells; p += (long long)gridDim.x * 16) sum += (double)a.grad_head[p * HFB_COLS + col];
    red_s[tid] = sum;
    __syncthreads();
    if (tid < a.groups * WG_GROUP_PAD) {
        const int grp = tid >> 4, o = tid & 15;
        double t = 0.0;
        if (o < a.g_cout[grp])
            for (int sl = 0; sl < 16; ++sl) t += red_s[sl * 16 + a.g_ooff[grp] + o];
        part[(size_t)blockIdx.x * a.groups * WG_GROUP_PAD + tid] = t;
    }
}

__global__ __launch_bounds__(BW_THREADS) void k_sum_partials(const double *__restrict__ part, int blocks, int n, double *__restrict__ out) {
    const int i = blockIdx.x * BW_THREADS + threadIdx.x;
    if (i >= n) return;
    double t = 0.0;
    for (int k = 0; k < blocks; ++k) t += part[(size_t)k * n + i];
    out[i] = t;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static const long long BW_2GIB = 1LL << 31;

static int bw_blocks(int batch, int h, int w, int pslots) {
    const long long t = ((long long)batch * h * w + pslots - 1) / pslots;
    return (int)(t < 1 ? 1 : (t > BW_MAX_BLOCKS ? BW_MAX_BLOCKS : t));
}

static long long bw_image_bytes(int batch, int h, int w, int c, bool border) {
    return (long long)batch * (h + (border ? 2 : 0)) * (w + (border ? 2 : 0)) * c * 4;
}

struct WgradPlan { int bands, row_chunks, chunks, cout_pad, ncf, ci_slices, co_slices; size_t elems; };

// 0 = a shape the kernel takes
static int wgrad_plan(int batch, int h, int w, int cin, int cout, int groups, WgradPlan &p, bool report) {
    const bool grouped = groups > 1;
    if (cin % 16 || cin < 16 || cin > 512 || cout > 512 || (!grouped && cout % 16) || groups > WG_MAX_GROUPS) {
        if (report) set_error("dz_conv3x3_wgrad: %d -> %d channels in %d groups (cin %% 16 == 0, cout %% 16 == 0, both at most 512; up to %d groups)",
                              cin, cout, groups, WG_MAX_GROUPS);
        return DZ_ERR_UNSUPPORTED;
    }
    if (bw_image_bytes(batch, h, w, groups * cin, true) >= BW_2GIB || bw_image_bytes(batch, h, w, cout, true) >= BW_2GIB) {
        if (report) set_error("dz_conv3x3_wgrad: an image of %d x %d x %d of 2 GiB or more", batch, h, w);
        return DZ_ERR_UNSUPPORTED;
    }
    p.bands = (w + WG_TW - 1) / WG_TW;
    p.row_chunks = (h + WG_ROWS - 1) / WG_ROWS;
    p.chunks = batch * p.bands * p.row_chunks;
    p.cout_pad = grouped ? WG_GROUP_PAD : cout;
    p.ncf = p.cout_pad <= 32 ? 1 : 2;
    p.ci_slices = (cin + WG_CI - 1) / WG_CI;
    p.co_slices = (p.cout_pad + p.ncf * 32 - 1) / (p.ncf * 32);
    p.elems = (size_t)groups * 9 * cin * p.cout_pad;
    return DZ_OK;
}

static int wgrad_launch(const float *x_img, const float *g_img, int g_border, int batch, int h, int w, int cin, int cout, int groups,
                        const int *g_cout, const int *g_ooff, float *out, void *ws, const WgradPlan &p, hipStream_t stream) {
    WgradArgs a;
    a.x = x_img; a.g = g_img; a.part = (float *)ws;
    a.B = batch; a.H = h; a.W = w; a.cin = cin; a.x_cs = groups * cin; a.g_cs = cout; a.g_border = g_border ? 1 : 0; a.cout_pad = p.cout_pad;
    a.groups = groups; a.bands = p.bands; a.row_chunks = p.row_chunks; a.ci_slices = p.ci_slices; a.co_slices = p.co_slices;
    for (int i = 0; i < WG_MAX_GROUPS; ++i) { a.g_cout[i] = groups > 1 && i < groups ? g_cout[i] : 0; a.g_ooff[i] = groups > 1 && i < groups ? g_ooff[i] : 0; }
    const dim3 grid(p.chunks, p.ci_slices * p.co_slices * groups);
    if (groups > 1) hipLaunchKernelGGL((k_c3_wgrad<1, true>), grid, dim3(WG_THREADS), 0, stream, a);
    else if (p.ncf == 1) hipLaunchKernelGGL((k_c3_wgrad<1, false>), grid, dim3(WG_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((k_c3_wgrad<2, false>), grid, dim3(WG_THREADS), 0, stream, a);
    DZ_LAUNCH_CHECK();
    const long long nvec = (long long)(p.elems / 4);
    hipLaunchKernelGGL(k_wgrad_reduce, dim3(stream_grid(nvec, BW_THREADS)), dim3(BW_THREADS), 0, stream, (const float4 *)ws, nvec, p.chunks, (float4 *)out);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

static int groups_ok(const char *who, int groups, const int *g_cout, const int *g_ooff, int n_g, int cols, int max_cout) {
    DZ_CHECK_ARG(g_cout && g_ooff, "%s: null g_cout / g_ooff", who);
    DZ_CHECK_ARG(n_g == groups, "%s: %d g_cout / g_ooff entries for %d groups", who, n_g, groups);
    for (int i = 0; i < groups; ++i)
        DZ_CHECK_ARG(g_cout[i] >= 1 && g_cout[i] <= max_cout && g_ooff[i] >= 0 && g_ooff[i] + g_cout[i] <= cols,
                     "%s: group %d reads columns [%d, %d) of %d (1..%d columns per group)", who, i, g_ooff[i], g_ooff[i] + g_cout[i], cols, max_cout);
    return DZ_OK;
}

// k_hfb_dgrad's LDS: the compact weights, then the sums' staging (one row per pixel slot)
constexpr size_t HFB_MAX_LDS = 64 * 1024;
static size_t hfb_lds_bytes(int c, int groups) {
    const int C = groups * c;
    return (size_t)groups * 9 * HFB_MAX_GCOUT * c * sizeof(float) + (size_t)(BW_THREADS / (C / 4)) * C * sizeof(double);
}

static size_t hfb_part_bytes(int c, int groups) {       // the two partial tables of dz_head_final_backward
    return align_up((size_t)BW_MAX_BLOCKS * groups * (c + WG_GROUP_PAD) * sizeof(double), 256);
}

}  // namespace dz

using namespace dz;

extern "C" {

size_t dz_conv3x3_wgrad_ws_bytes(int batch, int h, int w, int cin, int cout, int groups) {
    WgradPlan p;
    if (batch <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || groups <= 0 || wgrad_plan(batch, h, w, cin, cout, groups, p, false)) return 0;
    return align_up((size_t)p.chunks * p.elems * sizeof(float), 256);
}

int dz_conv3x3_wgrad(const float *x_img, const float *g_img, int g_border, int batch, int h, int w, int cin, int cout, int groups,
                     const int *g_cout, const int *g_ooff, int n_g, float *out, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(x_img && g_img && out && ws, "dz_conv3x3_wgrad: null pointer");
    DZ_CHECK_ARG(batch > 0 && h > 0 && w > 0 && cin > 0 && cout > 0 && groups > 0, "dz_conv3x3_wgrad: sizes %d x %d x %d, %d -> %d, %d groups",
                 batch, h, w, cin, cout, groups);
    WgradPlan p;
    const int rc = wgrad_plan(batch, h, w, cin, cout, groups, p, true);
    if (rc) return rc;
    if (groups > 1) {
        const int ok = groups_ok("dz_conv3x3_wgrad", groups, g_cout, g_ooff, n_g, cout, WG_GROUP_PAD);
        if (ok) return ok;
    } else {
        DZ_CHECK_ARG((((uintptr_t)x_img | (uintptr_t)g_img) & 15) == 0, "dz_conv3x3_wgrad: images must be 16-byte aligned");
    }
    DZ_CHECK_ARG(((uintptr_t)x_img & 15) == 0 && (((uintptr_t)out | (uintptr_t)ws) & 15) == 0, "dz_conv3x3_wgrad: buffers must be 16-byte aligned");
    if (ws_bytes < dz_conv3x3_wgrad_ws_bytes(batch, h, w, cin, cout, groups)) {
        set_error("dz_conv3x3_wgrad: workspace of %zu bytes, %zu needed", ws_bytes, dz_conv3x3_wgrad_ws_bytes(batch, h, w, cin, cout, groups));
        return DZ_ERR_WORKSPACE;
    }
    return wgrad_launch(x_img, g_img, g_border, batch, h, w, cin, cout, groups, g_cout, g_ooff, out, ws, p, stream);
}

size_t dz_relu_grad_ws_bytes(int batch, int h, int w, int c) {
    if (batch <= 0 || h <= 0 || w <= 0 || c < 4 || c > 512 || c % 4) return 0;
    return align_up((size_t)BW_MAX_BLOCKS * c * sizeof(double), 256);
}

int dz_relu_grad(const float *g_y, int gy_border, const float *y_img, int batch, int h, int w, int c, float *g_img, double *sums, void *ws,
                 size_t ws_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(g_y && y_img && g_img && sums && ws, "dz_relu_grad: null pointer");
    DZ_CHECK_ARG(batch > 0 && h > 0 && w > 0 && c > 0, "dz_relu_grad: sizes %d x %d x %d x %d", batch, h, w, c);
    if (c % 4 || c > 512) {
        set_error("dz_relu_grad: %d channels (a multiple of 4, at most 512)", c);
        return DZ_ERR_UNSUPPORTED;
    }
    if (bw_image_bytes(batch, h, w, c, true) >= BW_2GIB) {
        set_error("dz_relu_grad: an image of %d x %d x %d x %d of 2 GiB or more", batch, h, w, c);
        return DZ_ERR_UNSUPPORTED;
    }
    DZ_CHECK_ARG((((uintptr_t)g_y | (uintptr_t)y_img | (uintptr_t)g_img) & 15) == 0, "dz_relu_grad: images must be 16-byte aligned");
    if (ws_bytes < dz_relu_grad_ws_bytes(batch, h, w, c)) {
        set_error("dz_relu_grad: workspace of %zu bytes, %zu needed", ws_bytes, dz_relu_grad_ws_bytes(batch, h, w, c));
        return DZ_ERR_WORKSPACE;
    }
    const int blocks = bw_blocks(batch, h, w, BW_THREADS / (c / 4));
    hipLaunchKernelGGL(k_relu_grad, dim3(blocks), dim3(BW_THREADS), 0, stream, g_y, gy_border ? 1 : 0, y_img, batch, h, w, c, g_img, (double *)ws);
    DZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sum_partials, dim3(ceil_div(c, BW_THREADS)), dim3(BW_THREADS), 0, stream, (const double *)ws, blocks, c, sums);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

size_t dz_head_final_backward_ws_bytes(int batch, int h, int w, int c, int groups) {
    if (c <= 0 || groups < 2 || c > HFB_MAX_C || c % 16 || hfb_lds_bytes(c, groups) > HFB_MAX_LDS) return 0;
    const size_t wg = dz_conv3x3_wgrad_ws_bytes(batch, h, w, c, HFB_COLS, groups);
    return wg ? wg + hfb_part_bytes(c, groups) : 0;
}

int dz_head_final_backward(const float *grad_head, const float *w2, const float *hidden, int batch, int h, int w, int c, int groups,
                           const int *g_cout, const int *g_ooff, int n_g, float *g_hidden, double *sums_hidden, float *d_w2,
                           double *d_bias, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(grad_head && w2 && hidden && g_hidden && sums_hidden && d_w2 && d_bias && ws, "dz_head_final_backward: null pointer");
    DZ_CHECK_ARG(batch > 0 && h > 0 && w > 0 && c > 0 && groups > 0, "dz_head_final_backward: sizes %d x %d x %d, %d channels, %d groups",
                 batch, h, w, c, groups);
    if (c % 16 || c > HFB_MAX_C || groups < 2 || groups > WG_MAX_GROUPS || hfb_lds_bytes(c, groups) > HFB_MAX_LDS) {
        set_error("dz_head_final_backward: %d groups of %d channels (2..%d groups; channels a multiple of 16, at most %d; %zu bytes of LDS at most)",
                  groups, c, WG_MAX_GROUPS, HFB_MAX_C, HFB_MAX_LDS);
        return DZ_ERR_UNSUPPORTED;
    }
    WgradPlan p;
    const int rc = wgrad_plan(batch, h, w, c, HFB_COLS, groups, p, true);
    if (rc) return rc;
    const int ok = groups_ok("dz_head_final_backward", groups, g_cout, g_ooff, n_g, HFB_COLS, HFB_MAX_GCOUT);
    if (ok) return ok;
    DZ_CHECK_ARG((((uintptr_t)hidden | (uintptr_t)g_hidden | (uintptr_t)d_w2 | (uintptr_t)ws) & 15) == 0,
                 "dz_head_final_backward: buffers must be 16-byte aligned");
    if (ws_bytes < dz_head_final_backward_ws_bytes(batch, h, w, c, groups)) {
        set_error("dz_head_final_backward: workspace of %zu bytes, %zu needed", ws_bytes, dz_head_final_backward_ws_bytes(batch, h, w, c, groups));
        return DZ_ERR_WORKSPACE;
    }
    const int C = groups * c;
    HfbArgs a;
    a.grad_head = grad_head; a.w2 = w2; a.hidden = hidden; a.g_hidden = g_hidden; a.part = (double *)ws;
    a.B = batch; a.H = h; a.W = w; a.c = c; a.groups = groups;
    for (int i = 0; i < WG_MAX_GROUPS; ++i) { a.g_cout[i] = i < groups ? g_cout[i] : 0; a.g_ooff[i] = i < groups ? g_ooff[i] : 0; }
    double *part_cols = a.part + (size_t)BW_MAX_BLOCKS * C;
    void *ws_wgrad = (char *)ws + hfb_part_bytes(c, groups);
    const int pslots = BW_THREADS / (C / 4);
    const int blocks = bw_blocks(batch, h, w, pslots);
    const size_t lds = hfb_lds_bytes(c, groups);
    static PerDeviceFlags lds_done;
    const int lr = reserve_lds((const void *)k_hfb_dgrad, (int)HFB_MAX_LDS, lds_done, "dz_head_final_backward");
    if (lr) return lr;
    hipLaunchKernelGGL(k_hfb_dgrad, dim3(blocks), dim3(BW_THREADS), lds, stream, a);
    DZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sum_partials, dim3(ceil_div(C, BW_THREADS)), dim3(BW_THREADS), 0, stream, (const double *)a.part, blocks, C, sums_hidden);
    DZ_LAUNCH_CHECK();
    const int cblocks = bw_blocks(batch, h, w, 16);
    hipLaunchKernelGGL(k_col_sums, dim3(cblocks), dim3(BW_THREADS), 0, stream, a, part_cols);
    DZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(BW_THREADS), 0, stream, (const double *)part_cols, cblocks, groups * WG_GROUP_PAD, d_bias);
    DZ_LAUNCH_CHECK();
    return wgrad_launch(hidden, grad_head, 0, batch, h, w, c, HFB_COLS, groups, g_cout, g_ooff, d_w2, ws_wgrad, p, stream);
}

}  // extern "C"
