// pair16 <-> fp32 conversion and the memory-bound row movers of the split-precision path (gfx950).
// Layout and arithmetic: hgemm.h.  These kernels only stand at the ends of the pipeline (input voxel features,
// tensors handed back to PyTorch callers) and at the sparse -> BEV hand-over (height_compression.py:20-24).
#include "hgemm.h"

namespace dz {

template <class M>
__global__ void k_pair16_from_f32(const float *__restrict__ src, long rows, int c_src, int c_dst, uint4 *__restrict__ dst) {
    const int groups = c_dst / 8;
    const long total = rows * groups;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long r = idx / groups;
        const int g = (int)(idx % groups);
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (g * 8 + e < c_src) ? src[r * c_src + g * 8 + e] : 0.f;
        const float a[4] = {v[0], v[1], v[2], v[3]}, b[4] = {v[4], v[5], v[6], v[7]};
        uint2 h0, l0, h1, l1;
        split4<M>(a, h0, l0);
        split4<M>(b, h1, l1);
        dst[idx * 2] = make_uint4(h0.x, h0.y, h1.x, h1.y);
        dst[idx * 2 + 1] = make_uint4(l0.x, l0.y, l1.x, l1.y);
    }
}

template <class M>
__global__ void k_pair16_to_f32(const uint4 *__restrict__ src, long rows, int c, float *__restrict__ dst) {
    const int groups = c / 8;
    const long total = rows * groups;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const uint4 h = src[idx * 2], l = src[idx * 2 + 1];
        const unsigned int hw[4] = {h.x, h.y, h.z, h.w}, lw[4] = {l.x, l.y, l.z, l.w};
        float4 o0, o1;
        float o[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[2 * e] = M::join(hw[e] & 0xFFFFu, lw[e] & 0xFFFFu);
            o[2 * e + 1] = M::join(hw[e] >> 16, lw[e] >> 16);
        }
        o0 = make_float4(o[0], o[1], o[2], o[3]);
        o1 = make_float4(o[4], o[5], o[6], o[7]);
        reinterpret_cast<float4 *>(dst)[idx * 2] = o0;
        reinterpret_cast<float4 *>(dst)[idx * 2 + 1] = o1;
    }
}

template <class M>
__global__ void k_scatter_rows_split(const float *__restrict__ src, const int *__restrict__ rank, const int *__restrict__ d_n,
                                     int n_cap, int c_src, uint4 *__restrict__ dst, int c_dst) {
    const int n = d_n ? min(*d_n, n_cap) : n_cap;
    const int groups = c_dst / 8;
    const long total = (long)n * groups;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int i = (int)(idx / groups), g = (int)(idx % groups);
        const int r = rank[i];
        if (r < 0) continue;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (g * 8 + e < c_src) ? src[(size_t)i * c_src + g * 8 + e] : 0.f;
        const float a[4] = {v[0], v[1], v[2], v[3]}, b[4] = {v[4], v[5], v[6], v[7]};
        uint2 h0, l0, h1, l1;
        split4<M>(a, h0, l0);
        split4<M>(b, h1, l1);
        const size_t o = ((size_t)r * groups + g) * 2;
        dst[o] = make_uint4(h0.x, h0.y, h1.x, h1.y);
        dst[o + 1] = make_uint4(l0.x, l0.y, l1.x, l1.y);
    }
}

// bev[b][y+pad][x+pad][ch*D + z] <- feats[o][ch]: one thread moves the hi and lo halves of one channel
__global__ void k_sparse_to_bev_split(const unsigned short *__restrict__ feats, const int *__restrict__ coords,
                                      const int *__restrict__ d_m, int cap, int c, int d, int h, int w, int pad,
                                      unsigned short *__restrict__ bev) {
    const int m = min(*d_m, cap);
    const long total = (long)m * c;
    const int hp = h + 2 * pad, wp = w + 2 * pad;
    const int cd = c * d;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int o = (int)(idx / c), ch = (int)(idx % c);
        const int4 cc = reinterpret_cast<const int4 *>(coords)[o];  // [b,z,y,x]
        const size_t pix = ((size_t)cc.x * hp + (cc.z + pad)) * wp + (cc.w + pad);
        const unsigned short *s = feats + ((size_t)o * c + (ch & ~7)) * 2 + (ch & 7);   // 16-bit units: group start * 2
        const int oc = ch * d + cc.y;
        unsigned short *t = bev + (pix * cd + (oc & ~7)) * 2 + (oc & 7);
        t[0] = s[0];
        t[8] = s[8];
    }
}

// The same hand-over written DENSE for two z slabs (the encoded tensor of VoxelResBackBone8x): one thread per (pixel, group of 8
// output channels) looks the pixel's two cells up in the level's bitmap and writes the group - 4 channels of the z = 0 row
// interleaved with 4 of the z = 1 row (channel ch * 2 + z), zeros where a cell is empty or the pixel is border.  Every byte of
// the image is written once with 16-byte stores: no zero-fill pass over the 591 MB canvas and no 2-byte scatter stores.
__global__ __launch_bounds__(256) void k_sparse_to_bev_split_dense2(const uint2 *__restrict__ feats, const uint32_t *__restrict__ bitmap,
                                                                     const uint32_t *__restrict__ prefix, LevelGeom lg, int c, int pad,
                                                                     uint4 *__restrict__ bev, int feat_rows) {
    const int hp = lg.h + 2 * pad, wp = lg.w + 2 * pad;
    const int groups = c * 2 / 8, in_groups = c / 8;
    const long total = (long)lg.b * hp * wp * groups;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int og = (int)(idx % groups);
        const long pix = idx / groups;
        const int xp = (int)(pix % wp), yp = (int)((pix / wp) % hp), b = (int)(pix / ((long)wp * hp));
        const int x = xp - pad, y = yp - pad;
        uint2 h0 = make_uint2(0u, 0u), l0 = h0, h1 = h0, l1 = h0;
        if ((unsigned)x < (unsigned)lg.w && (unsigned)y < (unsigned)lg.h) {
            int r0 = bitmap_find(bitmap, prefix, lg.key(b, 0, y, x)), r1 = bitmap_find(bitmap, prefix, lg.key(b, 1, y, x));
            // a level that overflowed its row capacity still has every site in its bitmap: ranks past the feature rows read as empty
            // cells (the pipeline's overflow flag reports the frame; nothing is read past the buffer)
            if (r0 >= feat_rows) r0 = -1;
            if (r1 >= feat_rows) r1 = -1;
            // input group og / 2 (16 B hi | 16 B lo = four uint2), its channels (og & 1) * 4 .. + 3
            if (r0 >= 0) { const uint2 *s = feats + ((size_t)r0 * in_groups + (og >> 1)) * 4 + (og & 1); h0 = s[0]; l0 = s[2]; }
            if (r1 >= 0) { const uint2 *s = feats + ((size_t)r1 * in_groups + (og >> 1)) * 4 + (og & 1); h1 = s[0]; l1 = s[2]; }
        }
        auto zip = [](uint2 a, uint2 z) {       // 16-bit interleave: a0 z0 a1 z1 a2 z2 a3 z3
            return make_uint4((a.x & 0xFFFFu) | (z.x << 16), (a.x >> 16) | (z.x & 0xFFFF0000u), (a.y & 0xFFFFu) | (z.y << 16),
                              (a.y >> 16) | (z.y & 0xFFFF0000u));
        };
        bev[idx * 2] = zip(h0, h1);
        bev[idx * 2 + 1] = zip(l0, l1);
    }
}

// Row-index image of a level with two z slabs: idx[b][y + pad][x + pad][z] = feature row of cell (b, z, y, x), -1 where the cell is
// empty, the pixel is border, or the rank lies past the feature rows (a level that overflowed its calibrated capacity).  8 bytes
// per pixel instead of the pixel's 2 x C channels: what the sparse-input convolution (conv3x3_h.hip, dz_conv2d_desc.in_rowidx)
// reads in place of the dense BEV image.
__global__ __launch_bounds__(256) void k_bev_row_index(const uint32_t *__restrict__ bitmap, const uint32_t *__restrict__ prefix, LevelGeom lg, int pad,
                                                       int feat_rows, int2 *__restrict__ idx) {
    const int hp = lg.h + 2 * pad, wp = lg.w + 2 * pad;
    const long total = (long)lg.b * hp * wp;
    for (long pix = (long)blockIdx.x * blockDim.x + threadIdx.x; pix < total; pix += (long)gridDim.x * blockDim.x) {
        const int xp = (int)(pix % wp), yp = (int)((pix / wp) % hp), b = (int)(pix / ((long)wp * hp));
        const int x = xp - pad, y = yp - pad;
        int r0 = -1, r1 = -1;
        if ((unsigned)x < (unsigned)lg.w && (unsigned)y < (unsigned)lg.h) {
            r0 = bitmap_find(bitmap, prefix, lg.key(b, 0, y, x));
            r1 = bitmap_find(bitmap, prefix, lg.key(b, 1, y, x));
            if (r0 >= feat_rows) r0 = -1;
            if (r1 >= feat_rows) r1 = -1;
        }
        idx[pix] = make_int2(r0, r1);
    }
}

// ---- pixel tiles (8 x 32 output pixels, conv3x3_h.hip) of the first BEV block whose result is the network's ZERO-INPUT RESPONSE.
// With D = the Chebyshev distance of a pixel to the nearest pixel that holds a row (outside the image there are none), the block's 3 x 3
// stride-1 layer number l (1 = the sparse-input layer) sees around a pixel with D >= l + 1 exactly what it sees on an all-zero input, and
// produces what it produces there: ReLU(shift) at layer 1 (acc = 0 -> fmaf(0, scale, shift) -> ReLU -> the (hi, lo) split), the layer's
// zero-response image behind it.  Per 8-row band [y0, y0 + 8) and layer l, column x is BUSY if some occupied pixel lies in rows
// [y0 - l, y0 + 7 + l] and columns [x - l, x + l] - one of the column's pixels has D <= l.  The launch of layer l has to cover the busy
// columns; every other pixel is a copy (k_bev_fill_spans).
//   cover list: sweep x from 0, put a tile [x, x + 32) at the first busy column not yet covered, go on at x + 32 - for one band the fewest
//               tiles that cover its busy columns; entries carry their own origin (tile_xy_pack), spans = the complement per band;
//   grid list:  the tiles of the fixed 32-column grid that hold a busy column (tile id = (b * tiles_y + ty) * tiles_x + tx).
constexpr int BEV_DCAP = 8;             // layers 1 .. BEV_DCAP - 2 (a column's distance to the band is capped at BEV_DCAP - 1)
constexpr int BEV_MAX_W = 1024;         // columns of a band the planner takes (its grid mask is one 32-bit word)
// words of one (band, layer) slot of the planner's workspace: n tiles, n spans, grid mask, tile columns, spans (xs | xe << 16)
static inline __host__ __device__ int bev_slot_words(int tiles_x) { return 3 + tiles_x + tiles_x + 1; }

// one workgroup per (frame, band): vertical distance of every column to the band in ONE pass over the band's window, then per layer the
// busy mask (ballots) and a sweep of at most tiles_x steps by one thread
__global__ __launch_bounds__(256) void k_bev_cover_plan(const int2 *__restrict__ idx, int hp, int wp, int ho, int wo, int tiles_y, int tiles_x, int nl,
                                                        int *__restrict__ slots) {
    __shared__ unsigned char vd[BEV_MAX_W];
    __shared__ unsigned long long busy[BEV_DCAP - 2][BEV_MAX_W / 64];
    const int tid = threadIdx.x, ty = blockIdx.x % tiles_y, b = blockIdx.x / tiles_y, y0 = ty * 8;
    for (int k = tid; k < (BEV_DCAP - 2) * (BEV_MAX_W / 64); k += 256) (&busy[0][0])[k] = 0ull;
    for (int x = tid; x < wo; x += 256) {
        int v = BEV_DCAP - 1;
        for (int r = -nl; r < 8 + nl; ++r) {
            const int y = y0 + r;
            if ((unsigned)y >= (unsigned)ho) continue;
            const int2 e = idx[((size_t)b * hp + y + 1) * wp + x + 1];
            if (e.x >= 0 || e.y >= 0) v = min(v, r < 0 ? -r : r > 7 ? r - 7 : 0);
        }
        vd[x] = (unsigned char)v;
    }
    __syncthreads();
    const int wo64 = (wo + 63) & ~63;
    for (int l = 1; l <= nl; ++l)
        for (int x = tid; x < wo64; x += 256) {             // (whole wavefronts: wo64 is a multiple of 64)
            bool bz = false;
            if (x < wo)
                for (int k = max(0, x - l); k <= min(wo - 1, x + l); ++k) bz |= vd[k] <= l;
            const unsigned long long m = __ballot(bz);
            if ((tid & 63) == 0) busy[l - 1][x >> 6] = m;
        }
    __syncthreads();
    if (tid >= nl) return;
    const unsigned long long *const bm = busy[tid];
    int *const s = slots + ((size_t)blockIdx.x * nl + tid) * bev_slot_words(tiles_x);
    const int nw = wo64 >> 6;
    int n = 0, ns = 0, pos = 0;
    for (;;) {                                              // pos < wo
        int w = pos >> 6, x = wo;
        unsigned long long m = bm[w] & (~0ull << (pos & 63));
        while (!m && ++w < nw) m = bm[w];
        if (m) x = w * 64 + __ffsll(m) - 1;                 // first busy column at or behind pos
        if (x > pos) s[3 + tiles_x + ns++] = pos | (x << 16);
        if (x >= wo) break;
        s[3 + n++] = x;
        pos = x + 32;
        if (pos >= wo) break;
    }
    unsigned int gm = 0u;
    for (int tx = 0; tx < tiles_x; ++tx) gm |= (unsigned int)(bm[tx >> 1] >> (32 * (tx & 1))) ? 1u << tx : 0u;
    s[0] = n;
    s[1] = ns;
    s[2] = (int)gm;
}

// slots -> lists: one wavefront per (64 bands, layer).  It sums the counts of the bands before its own (a few hundred words), scans its own
// 64 and writes their entries: order ascending in (b, ty, x), as the slots are.  List l at lists + (l - 1) * stride:
// [grid: n run, n skippable, ids to run, skippable ids][cover at + 2 + n_bands * tiles_x: n run, n spans, tile entries, spans (2 words each)]
__global__ __launch_bounds__(64) void k_bev_cover_compact(const int *__restrict__ slots, int n_bands, int tiles_y, int tiles_x, int nl, int *__restrict__ lists,
                                                          int stride) {
    const int lane = threadIdx.x, l = blockIdx.y, first = blockIdx.x * 64, sw = bev_slot_words(tiles_x);
    auto slot = [&](int i) { return slots + ((size_t)i * nl + l) * sw; };
    int before[3] = {0, 0, 0}, total[3] = {0, 0, 0};        // tiles, spans, grid tiles to run
    for (int i = lane; i < n_bands; i += 64) {
        const int *s = slot(i);
        const int c[3] = {s[0], s[1], (int)__popc((unsigned int)s[2])};
        for (int k = 0; k < 3; ++k) { total[k] += c[k]; if (i < first) before[k] += c[k]; }
    }
    for (int k = 0; k < 3; ++k)
        for (int d = 32; d >= 1; d >>= 1) { total[k] += __shfl_xor(total[k], d); before[k] += __shfl_xor(before[k], d); }
    const int me = first + lane;
    const bool live = me < n_bands;
    const int *const s = slot(live ? me : 0);
    const int n = live ? s[0] : 0, ns = live ? s[1] : 0;
    const unsigned int gm = live ? (unsigned int)s[2] : 0u;
    int pre[3] = {n, ns, (int)__popc(gm)};
    for (int k = 0; k < 3; ++k) {
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(pre[k], d); if (lane >= d) pre[k] += t; }
        pre[k] += before[k];                                 // inclusive over all bands up to mine
    }
    int *const grid = lists + (size_t)l * stride, *const cover = grid + 2 + n_bands * tiles_x;
    if (blockIdx.x == 0 && lane == 0) {
        grid[0] = total[2];
        grid[1] = n_bands * tiles_x - total[2];
        cover[0] = total[0];
        cover[1] = total[1];
    }
    if (!live) return;
    const int b = me / tiles_y, ty = me % tiles_y;
    int *o = cover + 2 + pre[0] - n;
    for (int k = 0; k < n; ++k) o[k] = tile_xy_pack(b, ty, s[3 + k]);
    o = cover + 2 + total[0] + 2 * (pre[1] - ns);
    for (int k = 0; k < ns; ++k) {
        const int sp = s[3 + tiles_x + k];
        o[2 * k] = tile_xy_pack(b, ty, sp & 0xFFFF);
        o[2 * k + 1] = sp >> 16;
    }
    int run = pre[2] - (int)__popc(gm);                          // grid tiles to run before tile (me, tx)
    for (int tx = 0; tx < tiles_x; ++tx) {
        const int id = me * tiles_x + tx;
        if ((gm >> tx) & 1u) grid[2 + run++] = id;
        else grid[2 + total[2] + id - run] = id;
    }
}

// The pixels a list's launch leaves out get the layer's zero-input response.  The entries behind the list's tiles to run: spans of a
// cover list ([xs, xe) of a band, two words) or skippable tiles of a grid list (ids).  A fixed grid of wavefronts (a multiple of 8
// workgroups) walks (entry, row): one row of a span is one contiguous run of 16-byte pieces in the image and in the response; every lane
// has FILL_DEPTH loads in flight before its first store.
constexpr int FILL_DEPTH = 8;
template <class M>
__global__ __launch_bounds__(256) void k_bev_fill_spans(const int *__restrict__ list, int batch, int tiles_y, int tiles_x, int ho, int wo,
                                                        const float *__restrict__ shift, int relu, int cout, float *__restrict__ out, int out_hp, int out_wp,
                                                        int out_cstride, int out_coff, const float *__restrict__ zero_resp) {
    const int n_run = list[0], n_fill = min(list[1], batch * tiles_y * (tiles_x + 1));
    if (n_fill <= 0) return;
    const int *const ent = list + 2 + n_run;
    const bool xy = ent[0] < 0;
    const int lane = threadIdx.x & 63;
    // workgroup j runs on XCD j % 8 (own L2 each): XCD k copies row k of every band, so it reads one eighth of the response image
    // (2.3 MB at 188 x 188 x 128) - after the first frame from its L2 - instead of all of it once per frame
    const int y8 = blockIdx.x & 7;
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x >> 3) * 4 + (threadIdx.x >> 6))), nwaves = (gridDim.x >> 3) * 4;
    const int ppp = cout / 4;                                // 16-byte pieces of a pixel: (hi, lo) of each group of 8 channels
    // a unit = 64 columns of a span's row (16 wavefront rounds at 128 channels): full-width spans of the empty bands would otherwise
    // keep single wavefronts busy long after the others have finished
    const int nseg = (wo + 63) / 64;
    for (int u = wave; u < n_fill * nseg; u += nwaves) {
        const int i = u / nseg, seg = u - i * nseg;
        int b, ty, xs, xe;
        if (xy) {
            tile_xy_unpack(ent[2 * i], b, ty, xs);
            xe = ent[2 * i + 1];
        } else {
            const int t = ent[i];
            xs = (t % tiles_x) * 32, xe = min(xs + 32, wo), ty = (t / tiles_x) % tiles_y, b = t / (tiles_x * tiles_y);
        }
        const int y = ty * 8 + y8;
        if ((unsigned)b >= (unsigned)batch || y >= ho || xs < 0 || xe > wo) continue;
        xs += seg * 64;
        if (xs >= xe) continue;
        xe = min(xe, xs + 64);
        const int np = (xe - xs) * ppp;
        float *const drow = out + (((size_t)b * out_hp + y + 1) * out_wp + xs + 1) * out_cstride + out_coff;
        const uint4 *const srow = zero_resp ? reinterpret_cast<const uint4 *>(zero_resp + ((size_t)(y + 1) * out_wp + xs + 1) * cout) : nullptr;
        for (int p0 = lane; p0 < np; p0 += 64 * FILL_DEPTH) {
            uint4 v[FILL_DEPTH];
#pragma unroll
            for (int k = 0; k < FILL_DEPTH; ++k) {
                const int p = p0 + 64 * k;
                if (p >= np) continue;
                if (srow) { v[k] = srow[p]; continue; }
                const int g = (p % ppp) >> 1;                // the constant ReLU(shift): hi or lo words of channel group g
                float v0[4], v1[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float a = shift ? shift[g * 8 + e] : 0.f, bb = shift ? shift[g * 8 + 4 + e] : 0.f;
                    v0[e] = relu ? fmaxf(a, 0.f) : a;
                    v1[e] = relu ? fmaxf(bb, 0.f) : bb;
                }
                uint2 h0, l0, h1, l1;
                split4<M>(v0, h0, l0);
                split4<M>(v1, h1, l1);
                v[k] = (p & 1) ? make_uint4(l0.x, l0.y, l1.x, l1.y) : make_uint4(h0.x, h0.y, h1.x, h1.y);
            }
#pragma unroll
            for (int k = 0; k < FILL_DEPTH; ++k) {
                const int p = p0 + 64 * k;
                if (p < np) *reinterpret_cast<uint4 *>(drow + (size_t)(p / ppp) * out_cstride + (p % ppp) * 4) = v[k];
            }
        }
    }
}

}  // namespace dz

using namespace dz;

extern "C" {

static inline int bev_bands(int batch, int ho) { return batch * ceil_div(ho, 8); }
size_t dz_bev_tile_cover_offset(int batch, int ho, int wo) { return (size_t)bev_bands(batch, ho) * ceil_div(wo, 32) + 2; }
size_t dz_bev_tile_cover_words(int batch, int ho, int wo) {
    const size_t n = bev_bands(batch, ho), tx = ceil_div(wo, 32);
    return dz_bev_tile_cover_offset(batch, ho, wo) + 2 + n * tx + 2 * n * (tx + 1);
}
size_t dz_bev_tile_cover_ws_words(int batch, int ho, int wo, int nlists) { return (size_t)bev_bands(batch, ho) * nlists * bev_slot_words(ceil_div(wo, 32)); }

int dz_bev_tile_cover(const int *idx, int batch, int hp, int wp, int ho, int wo, int nlists, int *lists, int *ws, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(idx && lists && ws && batch > 0 && ho > 0 && wo > 0 && hp >= ho + 2 && wp >= wo + 2 && nlists >= 1 && nlists <= BEV_DCAP - 2,
                 "dz_bev_tile_cover: bad argument (1 <= nlists <= %d)", BEV_DCAP - 2);
    const int ty = ceil_div(ho, 8), tx = ceil_div(wo, 32), n = batch * ty;
    DZ_CHECK_ARG(wo <= BEV_MAX_W && wo <= TILE_XY_MAX_X && ty <= TILE_XY_MAX_TY && batch <= TILE_XY_MAX_B,
                 "dz_bev_tile_cover: %d frames of %d x %d pixels exceed the list entry (%d frames, %d rows, %d columns)", batch, ho, wo, TILE_XY_MAX_B,
                 TILE_XY_MAX_TY * 8, BEV_MAX_W);
    hipLaunchKernelGGL(k_bev_cover_plan, dim3(n), dim3(256), 0, stream, reinterpret_cast<const int2 *>(idx), hp, wp, ho, wo, ty, tx, nlists, ws);
    hipLaunchKernelGGL(k_bev_cover_compact, dim3(ceil_div(n, 64), nlists), dim3(64), 0, stream, ws, n, ty, tx, nlists, lists,
                       (int)dz_bev_tile_cover_words(batch, ho, wo));
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_bev_fill_spans(const int *list, int batch, int ho, int wo, const float *shift, int relu, int cout, float *out, int out_hp, int out_wp,
                      int out_cstride, int out_coff, const float *zero_resp, int math, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(list && out && batch > 0 && ho > 0 && wo > 0 && cout > 0 && cout % 8 == 0 && out_cstride % 8 == 0 && out_coff % 8 == 0 &&
                 out_hp >= ho + 2 && out_wp >= wo + 2, "dz_bev_fill_spans: bad argument");
    DZ_CHECK_ARG(math == DZ_MATH_F16X2 || math == DZ_MATH_BF16X2 || math == DZ_MATH_F16, "dz_bev_fill_spans: math %d is not a split mode", math);
    const int ty = ceil_div(ho, 8), tx = ceil_div(wo, 32);
    const dim3 grid((4 * device_cus() + 7) / 8 * 8);        // the fill is a copy: four workgroups per CU, whatever the list holds
    if (math == DZ_MATH_BF16X2)
        hipLaunchKernelGGL(k_bev_fill_spans<MathBF16>, grid, dim3(256), 0, stream, list, batch, ty, tx, ho, wo, shift, relu, cout, out, out_hp, out_wp,
                           out_cstride, out_coff, zero_resp);
    else
        hipLaunchKernelGGL(k_bev_fill_spans<MathF16>, grid, dim3(256), 0, stream, list, batch, ty, tx, ho, wo, shift, relu, cout, out, out_hp, out_wp,
                           out_cstride, out_coff, zero_resp);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_bev_row_index(const uint32_t *bitmap, const uint32_t *prefix, int batch, int d, int h, int w, int layout, int pad, int feat_rows, int *idx,
                     void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(bitmap && prefix && idx && batch > 0 && h > 0 && w > 0 && pad >= 0 && feat_rows >= 0, "dz_bev_row_index: bad argument");
    if (d != 2) { set_error("dz_bev_row_index: %d z slabs (the sparse-input convolution reads exactly 2)", d); return DZ_ERR_UNSUPPORTED; }
    DZ_CHECK_ARG(layout == DZ_LAYOUT_LINEAR || layout == DZ_LAYOUT_BRICK, "dz_bev_row_index: bad layout %d", layout);
    const LevelGeom lg = make_level(batch, d, h, w, layout);
    const long total = (long)batch * (h + 2 * pad) * (w + 2 * pad);
    hipLaunchKernelGGL(k_bev_row_index, dim3(stream_grid(total, 256)), dim3(256), 0, stream, bitmap, prefix, lg, pad, feat_rows, reinterpret_cast<int2 *>(idx));
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_pair16_from_f32(const float *src, long rows, int c_src, int c_dst, int math, float *dst, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(rows >= 0 && c_src >= 1 && c_dst >= c_src && c_dst % 8 == 0, "dz_pair16_from_f32: bad sizes");
    DZ_CHECK_ARG(math == DZ_MATH_F16X2 || math == DZ_MATH_BF16X2, "dz_pair16_from_f32: math %d is not a split mode", math);
    if (rows == 0) return DZ_OK;
    DZ_CHECK_ARG(src && dst, "dz_pair16_from_f32: null pointer");
    const dim3 grid(stream_grid(rows * (c_dst / 8), 256));
    if (math == DZ_MATH_F16X2)
        hipLaunchKernelGGL(k_pair16_from_f32<MathF16>, grid, dim3(256), 0, stream, src, rows, c_src, c_dst, reinterpret_cast<uint4 *>(dst));
    else
        hipLaunchKernelGGL(k_pair16_from_f32<MathBF16>, grid, dim3(256), 0, stream, src, rows, c_src, c_dst, reinterpret_cast<uint4 *>(dst));
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_pair16_to_f32(const float *src, long rows, int c, int math, float *dst, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(rows >= 0 && c >= 8 && c % 8 == 0, "dz_pair16_to_f32: bad sizes");
    DZ_CHECK_ARG(math == DZ_MATH_F16X2 || math == DZ_MATH_BF16X2, "dz_pair16_to_f32: math %d is not a split mode", math);
    if (rows == 0) return DZ_OK;
    DZ_CHECK_ARG(src && dst, "dz_pair16_to_f32: null pointer");
    const dim3 grid(stream_grid(rows * (c / 8), 256));
    if (math == DZ_MATH_F16X2)
        hipLaunchKernelGGL(k_pair16_to_f32<MathF16>, grid, dim3(256), 0, stream, reinterpret_cast<const uint4 *>(src), rows, c, dst);
    else
        hipLaunchKernelGGL(k_pair16_to_f32<MathBF16>, grid, dim3(256), 0, stream, reinterpret_cast<const uint4 *>(src), rows, c, dst);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_scatter_rows_split(const float *src, const int *rank, const int *d_n, int n_cap, int c_src, float *dst, int c_dst,
                          int math, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(n_cap >= 0 && c_src >= 1 && c_dst >= c_src && c_dst % 8 == 0, "dz_scatter_rows_split: bad sizes");
    DZ_CHECK_ARG(math == DZ_MATH_F16X2 || math == DZ_MATH_BF16X2, "dz_scatter_rows_split: math %d is not a split mode", math);
    if (n_cap == 0) return DZ_OK;
    DZ_CHECK_ARG(src && rank && dst, "dz_scatter_rows_split: null pointer");
    const dim3 grid(stream_grid((long)n_cap * (c_dst / 8), 256));
    if (math == DZ_MATH_F16X2)
        hipLaunchKernelGGL(k_scatter_rows_split<MathF16>, grid, dim3(256), 0, stream, src, rank, d_n, n_cap, c_src,
                           reinterpret_cast<uint4 *>(dst), c_dst);
    else
        hipLaunchKernelGGL(k_scatter_rows_split<MathBF16>, grid, dim3(256), 0, stream, src, rank, d_n, n_cap, c_src,
                           reinterpret_cast<uint4 *>(dst), c_dst);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_sparse_to_bev_split(const float *feats, const int *coords, const int *d_m, int cap, int c, int d, int h, int w,
                           int pad, float *bev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(feats && coords && d_m && bev && c > 0 && c % 8 == 0 && d > 0 && (c * d) % 8 == 0 && pad >= 0,
                 "dz_sparse_to_bev_split: bad argument");
    if (cap == 0) return DZ_OK;
    hipLaunchKernelGGL(k_sparse_to_bev_split, dim3(stream_grid((long)cap * c, 256)), dim3(256), 0, stream,
                       reinterpret_cast<const unsigned short *>(feats), coords, d_m, cap, c, d, h, w, pad,
                       reinterpret_cast<unsigned short *>(bev));
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

int dz_sparse_to_bev_split_dense(const float *feats, int feat_rows, const uint32_t *bitmap, const uint32_t *prefix, int batch, int c, int d,
                                 int h, int w, int layout, int pad, float *bev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DZ_CHECK_ARG(feats && bitmap && prefix && bev && batch > 0 && c > 0 && c % 8 == 0 && h > 0 && w > 0 && pad >= 0 && feat_rows >= 0,
                 "dz_sparse_to_bev_split_dense: bad argument");
    if (d != 2) { set_error("dz_sparse_to_bev_split_dense: %d z slabs (the dense form interleaves exactly 2)", d); return DZ_ERR_UNSUPPORTED; }
    DZ_CHECK_ARG(layout == DZ_LAYOUT_LINEAR || layout == DZ_LAYOUT_BRICK, "dz_sparse_to_bev_split_dense: bad layout %d", layout);
    const LevelGeom lg = make_level(batch, d, h, w, layout);
    const long total = (long)batch * (h + 2 * pad) * (w + 2 * pad) * (c * 2 / 8);
    hipLaunchKernelGGL(k_sparse_to_bev_split_dense2, dim3(stream_grid(total, 256)), dim3(256), 0, stream,
                       reinterpret_cast<const uint2 *>(feats), bitmap, prefix, lg, c, pad, reinterpret_cast<uint4 *>(bev), feat_rows);
    DZ_LAUNCH_CHECK();
    return DZ_OK;
}

}  // extern "C"
