/*
 * libdetzero_hip — C ABI of the MI355X (gfx950) implementation of DetZero's per-frame detection
 * hot path.  Plain pointers and sizes only (no torch types); every pointer is a caller-owned
 * DEVICE pointer unless the name starts with `h_`; every call is asynchronous on `stream`
 * (a hipStream_t passed as void*), allocates nothing, never exits the process and returns
 * DZ_OK (0) or a negative error code (message via dz_last_error()).
 *
 * Counts that are only known on the device (number of voxels, of active sites, of kept boxes)
 * live in device int32 words (`d_*`); kernels read them, so a whole frame can be enqueued — or
 * captured in a hipGraph — without a host round trip.  `cap` arguments are the row capacities
 * of the caller's buffers (upper bounds).
 *
 * Each entry point names the reference interface it stands in for (paths relative to the
 * reference repository root).  spconv / cumm / torch_scatter are un-vendored pip dependencies
 * of the reference; their Python call sites are cited instead.
 */
#ifndef DETZERO_HIP_H
#define DETZERO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DZ_OK 0
#define DZ_ERR_INVALID (-1)     /* bad argument */
#define DZ_ERR_WORKSPACE (-2)   /* workspace too small */
#define DZ_ERR_HIP (-3)         /* HIP runtime error */
#define DZ_ERR_UNSUPPORTED (-4) /* shape not supported by this build */

const char *dz_version(void);
const char *dz_last_error(void);
/* number of compute units of the current device (used by callers to size persistent grids) */
int dz_device_cu_count(void);

/* ---------------------------------------------------------------------------------------------
 * Points -> voxels
 * ------------------------------------------------------------------------------------------- */

/* Hard voxelization == spconv.utils.Point2VoxelCPU3d(...).point_to_voxel(points)
 * as called from detection/detzero_det/datasets/processor/data_processor.py:69-83.
 *   points (n,c) f32; h_range6 = [x0,y0,z0,x1,y1,z1]; h_vsize3; h_grid3 = (gx,gy,gz)
 *   voxels (max_voxels,max_points,c) f32 zero padded; coords_zyx (max_voxels,3) i32;
 *   num_points (max_voxels) i32; d_num_voxels: device i32, number of voxels produced.
 * Voxel order = first appearance in the input, points per voxel = first max_points in input order.
 * xy_range_mask != 0 additionally applies DataProcessor.mask_points_and_boxes_outside_range
 * (data_processor.py:24-37: keep lo <= x,y <= hi, inclusive) so device-resident frames need no
 * separate compaction pass. */
size_t dz_voxelize_hard_workspace_bytes(int n, int gx, int gy, int gz, int max_points);
int dz_voxelize_hard(const float *points, int n, int c, const float *h_range6, const float *h_vsize3,
                     const int *h_grid3, int xy_range_mask, int max_points, int max_voxels, float *voxels,
                     int *coords_zyx, int *num_points, int *d_num_voxels, void *ws, size_t ws_bytes,
                     void *stream);
/* dz_voxelize_hard + MeanVFE (vfe.py:58-83) fused for batched pipelines: row r < *d_num_voxels of `feats`
 * (row stride c_stride >= c, extra channels zero) receives the mean of voxel r's first <= max_points points, and
 * coords_bzyx row r = [batch_index, z, y, x]; rows beyond the count are left untouched (callers pre-fill the
 * coordinate rows with -1 so that dz_index_from_coords ignores them).  Same workspace as dz_voxelize_hard. */
int dz_voxelize_hard_mean(const float *points, int n, int c, const float *h_range6, const float *h_vsize3,
                          const int *h_grid3, int xy_range_mask, int max_points, int max_voxels, int batch_index,
                          float *feats, int c_stride, int *coords_bzyx, int *d_num_voxels, void *ws, size_t ws_bytes,
                          void *stream);
/* the same for `batch` equally long frames stored back to back (points (batch*n_per_frame, c)) in ONE launch chain:
 * frame f's voxels (first-appearance order within the frame, cut at max_voxels) go to rows f*cap_per_frame + r of
 * feats / coords_bzyx with batch index f; d_num_voxels (batch) receives the per-frame counts. */
size_t dz_voxelize_hard_batched_workspace_bytes(int n_per_frame, int batch, int gx, int gy, int gz, int max_points);
int dz_voxelize_hard_mean_batched(const float *points, int n_per_frame, int batch, int c, const float *h_range6,
                                  const float *h_vsize3, const int *h_grid3, int xy_range_mask, int max_points,
                                  int max_voxels, float *feats, int c_stride, int *coords_bzyx, int cap_per_frame,
                                  int *d_num_voxels, void *ws, size_t ws_bytes, void *stream);
/* Voxelize a batch straight into the level-1 sparse index of the backbone (data_processor.py:61-91 + vfe.py:66-83 +
 * the SparseConvTensor construction of backbone3d.py:302-307 in one chain): fills the level's bitmap / prefix /
 * canonical coordinates / count (the arrays dz_index_from_coords would produce for the frames' voxels, level shape
 * (level_d, gy, gx)) and writes every voxel's mean to its canonical row of `feats` (cap, c_dst), channels >= c zero,
 * fp32 (math 0) or pair16.  Valid only when a frame cannot exceed max_voxels (n_per_frame <= max_voxels; otherwise
 * DZ_ERR_UNSUPPORTED: the first-appearance cut of the reference needs dz_voxelize_hard_mean_batched). */
size_t dz_voxelize_to_level_workspace_bytes(int n_per_frame, int batch, int max_points, int cap, int d, int h, int w, int layout);
int dz_voxelize_to_level(const float *points, int n_per_frame, int batch, int c, const float *h_range6,
                         const float *h_vsize3, const int *h_grid3, int xy_range_mask, int max_points, int max_voxels,
                         int level_d, int layout, uint32_t *bitmap, uint32_t *prefix, int *coords_out, int *d_m, int cap,
                         float *feats, int c_dst, int math, void *ws, size_t ws_bytes, void *stream);

/* MeanVFE.forward — detection/detzero_det/models/centerpoint_modules/vfe.py:66-83.
 * out (m, c_out_stride) f32: columns [0,c) = sum over slots / max(num_points,1); columns
 * [c, c_out_stride) are written as 0 (channel padding used by the sparse backbone). */
int dz_mean_vfe(const float *voxels, const int *num_points, const int *d_m, int cap, int max_points,
                int c, float *out, int c_out_stride, void *stream);

/* DynamicMeanVFE.forward — vfe.py:109-147 (torch.unique + torch_scatter.scatter_mean).
 *   points_b (n,1+c) f32 rows [b,x,y,z,...]; feats (cap,c) f32; coords_bzyx (cap,4) i32 in
 *   ascending merge-key order (key = b*gx*gy*gz + cx*gy*gz + cy*gz + cz). */
size_t dz_voxelize_dynamic_workspace_bytes(int n, int batch, int gx, int gy, int gz, int c, int cap);
int dz_voxelize_dynamic_mean(const float *points_b, int n, int c, const float *h_range6,
                             const float *h_vsize3, const int *h_grid3, int xy_range_mask, int batch, float *feats,
                             int *coords_bzyx, int *d_num_voxels, int cap, void *ws, size_t ws_bytes,
                             void *stream);

/* ---------------------------------------------------------------------------------------------
 * Sparse tensor index ("indice" machinery of spconv.pytorch.SparseConvTensor / SubMConv3d /
 * SparseConv3d — call sites detection/detzero_det/models/centerpoint_modules/backbone3d.py:
 * 243-280, 302-307).  A level is a bit per cell of the (B,D,H,W) grid plus an exclusive
 * popcount prefix per 32-bit word (dz_voxelize_to_level writes it only at words that hold at least one bit - the only ones
 * the rank query of an ACTIVE cell reads; its level-1 bitmap is > 97 % empty words); active sites are numbered in ascending cell
 * key, which is also their row in the feature matrix.  `layout` selects the key of cell (b, z, y, x):
 *   DZ_LAYOUT_LINEAR  ((b*D+z)*H+y)*W+x: rows in ascending (b, z, y, x) order - the canonical order of SURVEY App. C;
 *   DZ_LAYOUT_BRICK   the (y, x) plane cut into 8 x 8 columns through all of z, column-major:
 *                     ((((b*ceil(H/8) + y/8)*ceil(W/8) + x/8)*D + z) << 6) | (y%8 << 3) | x%8.  Rows of a spatial neighbourhood are
 *                     then neighbours in memory (the order the backbone keeps its levels in: dz_spconv_tiles_forward stages the
 *                     1.3-1.8x halo of a 128..512-row tile in LDS instead of gathering every (row, tap) pair from L2).  spconv's own
 *                     row order is a hash-table detail: parity is stated on rows sorted by the linear key.
 * Every function below that takes (b, d, h, w) takes the layout next to it; bitmap / prefix sizes depend on it.
 * ------------------------------------------------------------------------------------------- */
#define DZ_LAYOUT_LINEAR 0
#define DZ_LAYOUT_BRICK 1
size_t dz_index_words(int b, int d, int h, int w, int layout);            /* uint32 words in bitmap / prefix */
size_t dz_index_workspace_bytes(int b, int d, int h, int w, int layout);

/* Build a level from (n,4) i32 [b,z,y,x] coordinates in any order (duplicates allowed).
 * d_n may be NULL (then n_cap rows are all valid).  Writes bitmap, prefix, canonical coords and
 * *d_m; rank_of_input (n_cap) receives the canonical row of each input row (may be NULL). */
int dz_index_from_coords(const int *coords, const int *d_n, int n_cap, int b, int d, int h, int w, int layout,
                         uint32_t *bitmap, uint32_t *prefix, int *coords_out, int *d_m, int cap_out,
                         int *rank_of_input, void *ws, size_t ws_bytes, void *stream);

/* Output level of a regular sparse convolution (SparseConv3d, backbone3d.py:256-277):
 * out dims = floor((in + 2p - k)/s) + 1; a site is active iff >=1 active input in its window. */
int dz_index_downsample(const int *coords_in, const int *d_m_in, int cap_in, int b, int d, int h,
                        int w, int layout, const int *h_k3, const int *h_s3, const int *h_p3, uint32_t *bitmap_out,
                        uint32_t *prefix_out, int *coords_out, int *d_m_out, int cap_out, void *ws,
                        size_t ws_bytes, void *stream);

/* Rulebook in output-stationary form: nbr[t*cap_out + o] = input row feeding output row o
 * through kernel tap t = (tz*kH+ty)*kW+tx (input coordinate = o*s - p + t), or -1.
 * SubMConv3d = (k=3,s=1,p=1) with the output level equal to the input level. */
int dz_build_neighbors(const int *coords_out, const int *d_m_out, int cap_out, const uint32_t *bitmap_in,
                       const uint32_t *prefix_in, int b, int d, int h, int w, int layout, const int *h_k3,
                       const int *h_s3, const int *h_p3, int *nbr, uint32_t *tile_masks, void *stream);
/* tile_masks (dz_tile_masks_words(cap_out) words, 16-byte aligned, or NULL): bit t of word o/32 = some row of the 32-row
 * group o/32 has a neighbour at tap t (what the conv kernels need to skip empty taps without scanning the table). */
int dz_tile_masks_words(int cap_out);
/* The same rulebook PACKED (DZ_NBR_PACKED) for 3 x 3 x 3 windows with x padding 1 on linear keys (every 27-tap table of
 * VoxelResBackBone8x, backbone3d.py:243-280): rows are in key order, so the three x taps of a (tz, ty) row are consecutive input
 * rows - one word per (tz, ty) and output row holds them: nbr[(tz*3+ty)*cap_out + o] = r | left << 29 | centre << 30 | right << 31
 * with r = active input cells below the centre cell of the window; left neighbour = r - 1, centre = r, right = r + centre (each
 * only when its bit is set).  9 words per output row instead of 27: a third of the table bytes written here and read by every
 * convolution of the level.  tile_masks as dz_build_neighbors (required).  DZ_ERR_UNSUPPORTED for other windows / layouts. */
int dz_build_neighbors_packed(const int *coords_out, const int *d_m_out, int cap_out, const uint32_t *bitmap_in,
                              const uint32_t *prefix_in, int b, int d, int h, int w, int layout, const int *h_k3,
                              const int *h_s3, const int *h_p3, int *nbr, uint32_t *tile_masks, void *stream);

/* dst[rank[i]][0:c_src] = src[i][0:c_src]; dst[rank[i]][c_src:c_dst] = 0 (rows with rank<0 skipped) */
int dz_scatter_rows(const float *src, const int *rank, const int *d_n, int n_cap, int c_src, float *dst,
                    int c_dst, void *stream);

/* Sparse convolution forward with fused epilogue
 *   out[o] = relu?( (sum_t in[nbr[t][o]] . W[t]) * scale + shift (+ residual[o]) )
 * == SubMConv3d/SparseConv3d + BatchNorm1d(eval, folded into scale/shift together with the conv
 * bias) + residual add + ReLU of backbone3d.py:77-81,105-121.  fp32 in, fp32 MFMA accumulate.
 *   in (in_rows, cin) f32 (in_rows = row capacity of the buffer, < 2 GiB), cin in {16,32,64,128};
 *   w (kvol,cin,cout) f32; cout in {16,32,64,128}. */
int dz_spconv_forward(const float *in, int in_rows, int cin, const int *nbr, int kvol, int cap_out, const int *d_m_out,
                      const float *w, const float *scale, const float *shift, const float *residual,
                      int relu, float *out, int cout, void *stream);

/* spconv SparseConvTensor.dense() + HeightCompression reshape (height_compression.py:20-24),
 * written channel-last into a zero-bordered BEV image: bev[b][y+pad][x+pad][c*D + z] = feats[o][c].
 * The caller zero-fills `bev` (hipMemsetAsync) before the call. */
int dz_sparse_to_bev(const float *feats, const int *coords, const int *d_m, int cap, int c, int d, int h,
                     int w, int pad, float *bev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Dense BEV network (torch.nn.Conv2d / ConvTranspose2d / BatchNorm2d / ReLU of
 * backbone2d.py:33-120 and center_head.py:14-48,81-102), channel-last implicit GEMM on fp32 MFMA.
 * ------------------------------------------------------------------------------------------- */
typedef struct dz_conv2d_desc {
    const float *in;      /* (B, in_hp, in_wp, in_cstride) channel-last, zero border included   */
    float *out;           /* (B, out_hp, out_wp, out_cstride)                                  */
    const float *w;       /* (groups, kh*kw, cin, cout_pad)                                    */
    const float *scale;   /* (groups*cout_pad) or NULL (=1)                                    */
    const float *shift;   /* (groups*cout_pad) or NULL (=0)                                    */
    int batch, ho, wo;    /* logical output extent enumerated by the kernel                    */
    int in_hp, in_wp, in_cstride, in_coff, cin;
    int kh, kw, stride, in_off; /* input pixel = (y*stride + ky + in_off, x*stride + kx + in_off) */
    int out_hp, out_wp, out_cstride, out_coff;
    int out_sy, out_sx, out_dy, out_dx; /* output pixel = (y*out_sy + out_dy, x*out_sx + out_dx) (pad included) */
    int groups, cout_pad;
    int g_cout[8];        /* valid output channels of each group                               */
    int g_ooff[8];        /* output channel offset of each group (added to out_coff)           */
    /* A launch writes exactly channels [out_coff + g_ooff[g], + g_cout[g]) of the output pixels it enumerates, in every engine
     * and output format: never the zero border, other channels of the pixel, the pad channels g_cout .. cout_pad - 1 of a group
     * (pair16 included: pair16 output has g_cout % 8 == 0, so a written 8-channel group is always a whole one), the pixels of
     * other phases, or - with in_tiles on the resident-tile kernel - the pixels of tiles not listed (tests/test_gpu_dense_conv.py) */
    int relu;
    const float *group_shift; /* optional (n_row_groups, cout_pad): added to the accumulator BEFORE scale/shift, */
    int group_rows;           /* row group = output row / group_rows (per-object bias of the PointNet concat)   */
    int group_max;            /* dz_linear_forward_split only: out = (row groups, out_cstride) fp32 pre-filled with -inf, the max over each
                                 group's rows is taken in the epilogue (no (rows, cout) result is written)          */
    int phase_groups;         /* dz_conv2d_forward_split only, != 0: the `groups` are the out_sy x out_sx PHASES of a ConvTranspose2d with
                                 kernel == stride (backbone2d.py:89-99) in ONE launch: every group reads the SAME cin input channels
                                 (no per-group input offset), has its own weights w[g], shares scale / shift (cout_pad entries), and
                                 writes output pixel (y*out_sy + out_dy + g / out_sx, x*out_sx + out_dx + g % out_sx); the phases of a
                                 pixel tile are scheduled next to each other on one XCD, so the input image is fetched from HBM once */
    const int *in_rowidx;     /* dz_conv2d_forward_split only, != NULL: SPARSE INPUT of a 3 x 3 stride-1 layer - the image is never built.
                                 `in` = the rows of a sparse level with two z slabs (in_rows x in_row_channels pair16), in_rowidx =
                                 (batch, in_hp, in_wp, 2) int32: the row of every (pixel, z slab) of the zero-bordered image, -1 = empty
                                 (dz_bev_row_index).  Logical input channel j = z * in_row_channels + c (z-MAJOR: the layer's weights
                                 are permuted accordingly - HeightCompression's own order is c * 2 + z); cin = 2 * in_row_channels;
                                 in_cstride is ignored.  HeightCompression (height_compression.py:20-24) + the first block's ZeroPad2d
                                 (backbone2d.py:41-46) fused into that block's convolution */
    int in_row_channels, in_rows;
    const int *in_tiles;      /* 3 x 3 stride-1 resident-tile layers, optional: a list of dz_bev_tile_cover (8 x 32 pixel tiles; grid ids, or entries with their own origin -
                                 an entry says which by its bit 31) - the launch covers its tiles to run only.
                                 Walked by the 64- / 128-channel tile kernels (pair16 output); IGNORED by the generic kernel (every pixel computed); refused
                                 (DZ_ERR_UNSUPPORTED) on the 32-channel tile kernel, whose tiles are 16 x 32 */
} dz_conv2d_desc;
int dz_conv2d_forward(const dz_conv2d_desc *h_desc, void *stream);
/* name of the kernel instance dz_conv2d_forward / dz_spconv_forward dispatch to (for profiling reports) */
const char *dz_conv2d_variant(const dz_conv2d_desc *h_desc);
const char *dz_spconv_variant(int cin, int cout);

/* ---------------------------------------------------------------------------------------------
 * Split-precision engine: the same sparse / dense convolutions on the 16-bit matrix cores.
 * Every fp32 value x travels as a pair of 16-bit floats (hi = rn16(x), lo = rn16(x - hi)); a product is
 * hi.hi + lo.hi + hi.lo in three v_mfma_f32_32x32x16_{f16,bf16} with fp32 accumulation (csrc/hgemm.h).
 * fp16 pairs carry 22 significant bits (results indistinguishable from fp32 summation-order noise, values
 * saturate at +-131008), bf16 pairs 16 bits with the full fp32 exponent range.
 * "pair16" layout of a row of C channels (C % 8 == 0): C 32-bit words, i.e. the byte size of the fp32 row;
 * each group of 8 channels = 16 bytes of hi values then 16 bytes of lo values.  Tensors keep the shapes,
 * strides and capacities of their fp32 counterparts (pointers are typed float* for that reason).
 * There is no fp32 conv in the reference to replace here beyond the ones named above: these entry points
 * are the throughput path of the same layers ("fp16/bf16-in / fp32-acc MFMA").
 * ------------------------------------------------------------------------------------------- */
#define DZ_MATH_F32 0
#define DZ_MATH_F16X2 1
#define DZ_MATH_BF16X2 2
#define DZ_MATH_F16 3      /* convolution entry points only: fp16-pair tensors (DZ_MATH_F16X2 storage), ONE fp16 MFMA per product (hi halves): plain-fp16 inputs, fp32 accumulation - a third of the matrix work, NOT fp32-class (opt-in fast mode) */
/* dst (rows, c_dst) pair16 <- src (rows, c_src) f32, channels c_src..c_dst-1 zero; c_dst % 8 == 0 */
int dz_pair16_from_f32(const float *src, long rows, int c_src, int c_dst, int math, float *dst, void *stream);
/* dst (rows, c) f32 <- src (rows, c) pair16 (hi + lo) */
int dz_pair16_to_f32(const float *src, long rows, int c, int math, float *dst, void *stream);
/* Range probe of a stored tensor: one streaming read that ADDS to a device record `slot` of four 64-bit words
 *   slot[0] peak       max |v| over the finite elements, kept as the bits of a non-negative fp32 (zero-extended); v = the element (fp32 storage)
 *                      or float(hi) + float(lo) in fp32 (pair16 storage)
 *   slot[1] saturated  DZ_MATH_F16X2 / DZ_MATH_F16 storage only: elements whose hi half is +-65504 (bits 0x7BFF without the sign) - what the
 *                      clamp of the fp16-pair split leaves behind; always 0 for the other storages
 *   slot[2] nonfinite  elements that are inf / NaN (pairs: either half has an all-ones exponent); such an element does not enter the peak
 *   slot[3] elements   elements looked at = rows read x c
 * Records accumulate over calls (max for the peak, sums for the counters) with device-scope atomics: several launches, frame groups and
 * streams may share a slot.  No host synchronisation, no allocation.  x: rows of row_stride_words 32-bit words (a multiple of 4, x 16-byte
 * aligned), of which channels [c_off, c_off + c) are read (both multiples of 8); rows = the row capacity, d_rows = optional device count:
 * min(*d_rows, rows) rows are read.  math = the STORAGE of x: DZ_MATH_F32, or pair16 of DZ_MATH_F16X2 (= DZ_MATH_F16) / DZ_MATH_BF16X2.
 * rows == 0: DZ_OK without a launch (x may then be NULL).  dz_range_reset zeroes n_slots consecutive records. */
int dz_range_probe(const float *x, long rows, const int *d_rows, int row_stride_words, int c_off, int c, int math, unsigned long long *slot,
                   void *stream);
int dz_range_reset(unsigned long long *table, int n_slots, void *stream);
/* dz_scatter_rows writing pair16 rows */
int dz_scatter_rows_split(const float *src, const int *rank, const int *d_n, int n_cap, int c_src, float *dst,
                          int c_dst, int math, void *stream);
/* dz_spconv_forward on pair16 operands: in / residual / out pair16 rows, w (kvol, cout_pad, cin) pair16 with
 * cout_pad = max(cout, 32) (rows cout..cout_pad-1 zero), scale / shift (cout) f32. */
int dz_spconv_forward_split(const float *in, int in_rows, int cin, const int *nbr, const uint32_t *tile_masks, int kvol,
                            int cap_out, const int *d_m_out, const float *w, const float *scale, const float *shift,
                            const float *residual, int relu, float *out, int cout, int math, void *stream);
/* tile_masks: the buffer dz_build_neighbors filled for this table (NULL: the kernel scans the table itself, slower). */
/* Tile-resident sparse convolution (csrc/sparse_conv_t.hip; the same SubMConv3d / SparseConv3d call sites as dz_spconv_forward:
 * backbone3d.py:64-121, :243-280).  dz_build_tiles turns a neighbour table of dz_build_neighbors (kvol x cap_out, once per
 * indice_key) into, per tile of dz_spconv_tile_rows() = 512 consecutive output rows:
 *   halo   (ntiles x dz_build_tiles_halo_stride(kvol) int32)  the DISTINCT input rows the tile reads;
 *   tinfo  (ntiles x dz_spconv_tile_info_words() = 64 int32)  [0] slots = non-empty kernel taps of the tile, [1] halo rows,
 *          [4..35] tap of slot s (ascending; -1 beyond), [36..51] bit s of word f: sorted fragment f (32 rows) has a row with slot s;
 *   rowmap (ntiles x 512 uint16)  the tile's rows sorted by their tap set: row (relative to the tile) at sorted position q;
 *   ltab   (ntiles x dz_spconv_tile_table_entries() = 16384 uint16)  position in the halo list of the neighbour of (slot s, sorted
 *          position q), 0xFFFF = none, at [s / 4][q / 64][q % 32][s % 4][q / 32 % 2].
 * dz_spconv_tiles_forward stages a tile's halo rows in LDS once per 16-channel chunk and runs every kernel tap from there -
 * same operands, same result convention (pair16 in / out, BatchNorm scale / shift, residual, ReLU) as dz_spconv_forward_split.
 * kvol 27 with cout in {16, 32, 64, 128}, kvol in [3, 10] with cout 128; cin % 16 == 0.  Any row order of the level is correct;
 * the brick layout (DZ_LAYOUT_BRICK) is what keeps a tile's halo small. */
int dz_spconv_tile_rows(void);
int dz_spconv_tile_info_words(void);
int dz_spconv_tile_table_entries(void);
size_t dz_build_tiles_halo_stride(int kvol);
int dz_build_tiles(const int *nbr, int kvol, int cap_out, const int *d_m_out, int *halo, int *tinfo, unsigned short *ltab,
                   unsigned short *rowmap, void *stream);
int dz_spconv_tiles_forward(const float *in, int in_rows, int cin, const int *halo, const int *tinfo, const unsigned short *ltab,
                            const unsigned short *rowmap, int kvol, int cap_out, const int *d_m_out, const float *w,
                            const float *scale, const float *shift, const float *residual, int relu, float *out, int cout,
                            int math, void *stream);
const char *dz_spconv_tiles_variant(int cin, int cout);
/* dz_spconv_forward_split over a PACKED 27-tap table (dz_build_neighbors_packed): the small-channel levels (16 -> 16, 16 -> 32,
 * 32 -> 32), whose HBM bytes are one third table in the unpacked form.  Same arithmetic, bit-identical results. */
int dz_spconv_forward_split_packed(const float *in, int in_rows, int cin, const int *nbr_packed, const uint32_t *tile_masks,
                                   int cap_out, const int *d_m_out, const float *w, const float *scale, const float *shift,
                                   const float *residual, int relu, float *out, int cout, int math, void *stream);
/* Submanifold 3 x 3 x 3 convolutions with the inputs of a z slab staged once per tile (csrc/sparse_conv_x.hip, the "x-run" engine;
 * the SubMConv3d pairs of SparseBasicBlock, backbone3d.py:93-121, at 32 / 64 / 128 channels: conv2, conv3, conv4 of
 * VoxelResBackBone8x, backbone3d.py:261-280).  Rows of a level are in ascending linear key, so the nine taps of one z offset of a tile
 * of T consecutive output rows read ONE contiguous range of input rows (a "window").
 *   dz_spconv_x_tile_rows(cin, cout): rows per UNIT of the kernel for this layer (a tile is two consecutive units; the last tiles of
 *     a launch are single units, for load balance), 0 = layer not covered (cin != cout, other widths).
 *   dz_spconv_x_windows: from the PACKED table of the level (dz_build_neighbors_packed, input level == output level) the windows of
 *     every unit: windows[(unit*3 + tz)*2 + {0, 1}] = first input row, number of rows (0 = slab has no neighbour; the centre slab of a
 *     live unit always has one), followed by 16 words of tile-queue state the convolution kernels use (zeroed here, left zero by
 *     every launch).  dz_spconv_x_windows_words(cap_out, tile_rows) int32 in all.  Once per indice_key, shared by the level's
 *     convolutions (which therefore must not run concurrently on the same windows buffer).
 *   dz_spconv_forward_split_x: operands, result convention and arithmetic of dz_spconv_forward_split (pair16 in / residual / out,
 *     w (27, cout, cin) pair16, BatchNorm scale / shift, ReLU); per output element the products are accumulated in the order
 *     (tz, 16-channel chunk, tap), so results agree with dz_spconv_forward_split to fp32 summation-order noise, not bit for bit. */
int dz_spconv_x_tile_rows(int cin, int cout);
/* rows of a z-slab window the kernel can stage in LDS for this layer (0 = layer not covered); a (tile, slab) whose window is longer
 * runs in gather mode - same taps, same accumulation order, operands fetched per lane instead of from the staged window */
int dz_spconv_x_window_rows(int cin, int cout);
size_t dz_spconv_x_windows_words(int cap_out, int tile_rows);
int dz_spconv_x_windows(const int *nbr_packed, int cap_out, const int *d_m_out, int tile_rows, int *windows, int *nbr_sorted, int *perm,
                        void *stream);
/* dz_build_neighbors_packed (3 x 3 x 3 submanifold table of a level onto itself, linear keys) and dz_spconv_x_windows in ONE launch:
 * the packed table, its per-32-row tap masks, the windows of every unit of tile_rows (128 | 256 = dz_spconv_x_tile_rows) rows and -
 * optionally, both or neither - the table / row map in tap-set order.  Same outputs, bit for bit, as the two calls; a workgroup
 * owns a 256-row block and keeps the nine words of a row in registers instead of reading the table back (round 5: the second
 * launch cost 105 us per level and step at 32 frames).  (b, d, h, w) = the level's grid; coords / d_m / bitmap / prefix its index. */
int dz_build_neighbors_packed_x(const int *coords, const int *d_m, int cap, const uint32_t *bitmap, const uint32_t *prefix, int b, int d,
                                int h, int w, int *nbr_packed, uint32_t *tile_masks, int tile_rows, int *windows, int *nbr_sorted,
                                int *perm, void *stream);
/* nbr_sorted (9 x cap_out) / perm (cap_out), both or neither: the rows of every unit re-ordered by their tap set (ascending in even
 * units, descending in odd ones): perm[position] = output row, nbr_sorted = the packed table in that order.  Fragments of 32 rows
 * with similar tap sets let the kernel skip 11-13 % more (fragment, tap) pairs; pass both to dz_spconv_forward_split_x. */
int dz_spconv_forward_split_x(const float *in, int in_rows, int cin, const int *nbr_packed, const int *perm, int *windows, int tile_rows,
                              int cap_out, const int *d_m_out, const float *w, const float *scale, const float *shift,
                              const float *residual, int relu, float *out, int cout, int math, void *stream);
/* (nbr_packed = the level's packed table and perm = NULL, or nbr_sorted and its perm) */
const char *dz_spconv_x_variant(int cin, int cout);
/* The x-run engine in EXACT fp32 (csrc/sparse_conv_xf.hip): the same layers, the same index (packed table or nbr_sorted + perm, the
 * windows of units of dz_spconv_x_tile_rows(cin, cout) rows - one index serves both arithmetics), fp32 rows and fp32 MFMA.
 *   in (in_rows, cin), residual / out (cap_out, cout) fp32 rows; w (27, cin, cout) fp32, the layout dz_spconv_forward takes;
 *   out = relu?((sum) * scale + shift (+ residual)), scale / shift / residual each optional (NULL); rows at or beyond *d_m_out are
 *   not written.  The 16 queue words behind the windows are not used and stay zero.
 *   Per output element the products are accumulated in the order (tz, 16-channel chunk kc, ty, tx, then channels kc*16 + s and
 *   kc*16 + 8 + s for s = 0..7), one fmaf each, whatever unit the row falls into and whether the slab's window was staged or
 *   gathered: launches agree bit for bit with each other, and with dz_spconv_forward to fp32 summation-order noise, not bit for bit.
 *   DZ_ERR_UNSUPPORTED for layers it does not cover (cin != cout, widths other than 32 / 64 / 128) and for in_rows * cin * 4 or
 *   cap_out * cout * 4 at or beyond 2 GiB; DZ_ERR_INVALID for windows built for another tile_rows or null pointers.
 *   dz_spconv_x_f32_window_rows: rows of a z-slab window the kernel stages in LDS (longer windows run in gather mode), 0 = layer not
 *   covered.  dz_spconv_x_f32_variant: kernel instance name, "none" if not covered. */
int dz_spconv_forward_x_f32(const float *in, int in_rows, int cin, const int *nbr_packed, const int *perm, int *windows, int tile_rows,
                            int cap_out, const int *d_m_out, const float *w, const float *scale, const float *shift,
                            const float *residual, int relu, float *out, int cout, void *stream);
int dz_spconv_x_f32_window_rows(int cin, int cout);
const char *dz_spconv_x_f32_variant(int cin, int cout);
/* The x-run engine of the exact-fp32 mode on the bf16 matrix pipe (csrc/sparse_conv_xt.hip, opt-in): the same layers, the same
 * index and the same fp32 rows as dz_spconv_forward_x_f32, every operand as three exact bf16 limbs (csrc/limb3.h) - the rows are
 * split on chip, no tensor format changes.  w (27, cout, cin * 3 / 2) words: per tap, output channel and group of 8 input
 * channels 16 bytes of h limbs, 16 of m, 16 of l (ops.pack_weight_limb3(w, cout_mult=32)).
 *   Per product six v_mfma_f32_32x32x16_bf16 terms, smallest first (l.h, h.l, m.m, m.h, h.m, h.h), fp32 accumulation; the terms
 *   m.l + l.m + l.l are dropped: at most 2^-26 of |x.w|.  Per output element the k-steps are accumulated in the order (tz,
 *   16-channel chunk kc, ty, tx), the six terms of a k-step in the order above, whatever unit the row falls into and whether
 *   the slab's window was staged or gathered: no atomics, launches agree bit for bit.
 *   out = relu?((sum) * scale + shift (+ residual)); rows at or beyond *d_m_out are not written; the 16 queue words behind the
 *   windows stay zero.  Refusals as dz_spconv_forward_x_f32.
 *   dz_spconv_x_limb3_window_rows: rows of a z-slab window the kernel stages in LDS (longer windows run in gather mode), 0 = layer
 *   not covered (the caller falls back to dz_spconv_forward_x_f32).  dz_spconv_x_limb3_variant: kernel instance name or "none". */
int dz_spconv_forward_x_limb3(const float *in, int in_rows, int cin, const int *nbr_packed, const int *perm, int *windows, int tile_rows,
                              int cap_out, const int *d_m_out, const float *w, const float *scale, const float *shift,
                              const float *residual, int relu, float *out, int cout, void *stream);
int dz_spconv_x_limb3_window_rows(int cin, int cout);
const char *dz_spconv_x_limb3_variant(int cin, int cout);
/* The gather-path sparse convolution of the exact-fp32 mode on the bf16 matrix pipe (csrc/sparse_conv_gt.hip, opt-in): the layers,
 * the plain (kvol, cap_out) table with its 32-row tile masks (dz_build_neighbors) and the fp32 rows of dz_spconv_forward, every
 * operand as three exact bf16 limbs (csrc/limb3.h) - the gathered rows are split on chip on their way into LDS, no tensor format
 * changes.  Channels 16 -> 16, 16 -> 32, 32 -> 32, 32 -> 64, 64 -> 64, 64 -> 128, 128 -> 128; kvol 1..27.
 *   w_limb (kvol, cout_pad, cin * 3 / 2) words, cout_pad = max(cout, 32) (a 16-channel output is padded with zero rows, stores
 *   are masked to cout): per tap, output channel and group of 8 input channels 16 bytes of h limbs, 16 of m, 16 of l
 *   (ops.pack_weight_limb3(w, cout_mult=32)).
 *   Per product six v_mfma_f32_32x32x16_bf16 terms, smallest first (l.h, h.l, m.m, m.h, h.m, h.h), fp32 accumulation; the terms
 *   m.l + l.m + l.l are dropped: at most 2^-26 of |x.w|.  Per output element: channel slice ascending, live taps ascending,
 *   16-channel k-step ascending, whatever tile the row falls into: no atomics, launches agree bit for bit.
 *   out = relu?((sum) * scale + shift (+ residual)); scale, shift, residual may be NULL.  Rows below m = min(*d_m_out, cap_out)
 *   are fully written, rows at or beyond m and anything behind cap_out are not touched; missing neighbours and rows beyond m
 *   fetch nothing.
 *   Refused before any launch: null pointers (tile_masks included) and kvol outside 1..27 (DZ_ERR_INVALID), channels the selector
 *   does not cover, and an input, output or table of 2 GiB or more (DZ_ERR_UNSUPPORTED).
 *   dz_spconv_limb3_tile_rows: the row tile of the layer's instance, 0 = not covered (the caller keeps dz_spconv_forward).
 *   dz_spconv_limb3_variant: kernel instance name or "none". */
int dz_spconv_forward_limb3(const float *in, int in_rows, int cin, const int *nbr, const uint32_t *tile_masks, int kvol, int cap_out,
                            const int *d_m_out, const float *w_limb, const float *scale, const float *shift, const float *residual,
                            int relu, float *out, int cout, void *stream);
int dz_spconv_limb3_tile_rows(int cin, int cout);
const char *dz_spconv_limb3_variant(int cin, int cout);
/* The wave-private form of dz_spconv_forward_limb3 for the 16-channel layers (csrc/sparse_conv_wt.hip, opt-in): channels 16 -> 16
 * and 16 -> 32, the same table, tile masks, fp32 rows, w_limb words (rows at or beyond cout are not read), epilogue and write
 * contract.  A wave owns 32 output rows, the limbs of all kvol taps of the weights stay in LDS, gathered rows go straight into
 * registers and are split there; per (tap, 16-row half, 16-channel output block) three v_mfma_f32_16x16x32_bf16 carry the same six
 * limb terms, smallest first: [w_h | w_l].[x_l | x_h], [w_m | w_m].[x_h | x_m], [w_h | w_h].[x_h | x_m].  Per output element: taps
 * ascending, then those three, whatever the grid: launches agree bit for bit.
 *   max_workgroups: 0 = as many persistent workgroups as fit; n > 0 is rounded up to a multiple of 8 and caps the grid (tests and
 *   tools: a small input then reaches a wave's second batch of 64 tile masks and several deal rounds).
 *   Refused before any launch, as dz_spconv_forward_limb3: null pointers (tile_masks included), kvol outside 1..27 and a negative
 *   max_workgroups (DZ_ERR_INVALID), channels the selector does not cover, and an input, output or table of 2 GiB or more
 *   (DZ_ERR_UNSUPPORTED).
 *   dz_spconv_limb3_w_tile_rows: rows one workgroup takes per deal step (32 x its waves), 0 = not covered (the layer keeps the
 *   kernel it has).  dz_spconv_limb3_w_variant: "k_spconv_wt<16x16>", "k_spconv_wt<16x32>" or "none". */
int dz_spconv_forward_limb3_w(const float *in, int in_rows, int cin, const int *nbr, const uint32_t *tile_masks, int kvol, int cap_out,
                              const int *d_m_out, const float *w_limb, const float *scale, const float *shift, const float *residual,
                              int relu, float *out, int cout, int max_workgroups, void *stream);
int dz_spconv_limb3_w_tile_rows(int cin, int cout);
const char *dz_spconv_limb3_w_variant(int cin, int cout);
/* HeightCompression WITHOUT the dense image (round 5): idx (batch, h + 2 pad, w + 2 pad, 2) int32 = the feature row of every
 * (pixel, z slab) of a two-slab level, -1 = empty cell / border / rank >= feat_rows (overflowed capacity).  The first block of
 * BaseBEVBackbone reads the level's rows through it (dz_conv2d_desc.in_rowidx): height_compression.py:20-24 and the ZeroPad2d of
 * backbone2d.py:41-46 never touch HBM.  DZ_ERR_UNSUPPORTED for d != 2. */
int dz_bev_row_index(const uint32_t *bitmap, const uint32_t *prefix, int batch, int d, int h, int w, int layout, int pad, int feat_rows,
                     int *idx, void *stream);
/* Pixel tiles (8 x 32 output pixels) of the first BEV block whose result is the network's ZERO-INPUT RESPONSE.  With D = the Chebyshev
 * distance of a pixel to the nearest pixel holding a row (nothing outside the image), the 3 x 3 stride-1 layer number l of the block
 * (l = 1: the sparse-input layer) sees around a pixel with D >= l + 1 exactly what it sees on an all-zero input - and produces what it
 * produces there.  Per 8-row band [y0, y0 + 8) column x is BUSY at layer l if an occupied pixel lies in rows [y0 - l, y0 + 7 + l] and
 * columns [x - l, x + l]; the launch of layer l has to cover the busy columns only.
 * dz_bev_tile_cover (idx = the row-index image of dz_bev_row_index, pad 1) writes, for l = 1 .. nlists (<= 6), at
 * lists + (l - 1) * dz_bev_tile_cover_words two lists of the same [n to run, n to fill, entries to run ..., entries to fill ...] shape:
 *   + 0                         the GRID list: tiles of the fixed 32-column grid holding a busy column, ids ascending
 *                               (id = (b * tiles_y + ty) * tiles_x + tx), then the ids of the skippable ones;
 *   + dz_bev_tile_cover_offset  the COVER list: per band, sweeping x from 0, a tile [x, x + 32) at the first busy column not yet covered -
 *                               the fewest tiles that cover the band's busy columns, never more than the grid's.  A tile entry carries
 *                               its origin: bit 31 | b << 21 | ty << 12 | x (ascending in (b, ty, x)); a tile may reach past wo.  To fill:
 *                               the maximal column intervals [xs, xe) of every band outside its tiles, two words each: the entry of
 *                               (b, ty, xs), then xe.
 * ws = dz_bev_tile_cover_ws_words ints.  Two launches, counts stay on the device.  wo <= 1024, ho <= 4096, batch <= 1024.
 * Pass either list as dz_conv2d_desc.in_tiles of layer l: the launch walks the tiles to run only.  dz_bev_fill_spans gives the other
 * pixels of that list their result: zero_resp = the layer's output on an all-zero input (1, out_hp, out_wp, cout) pair16, computed once
 * per model by the same kernels - or NULL for layer 1, whose response is the constant ReLU(shift).  Bit-identical to running every tile (a
 * pixel's result depends on its 3 x 3 input neighbourhood only, and its accumulation order does not depend on the tile's origin). */
size_t dz_bev_tile_cover_words(int batch, int ho, int wo);
size_t dz_bev_tile_cover_offset(int batch, int ho, int wo);
size_t dz_bev_tile_cover_ws_words(int batch, int ho, int wo, int nlists);
int dz_bev_tile_cover(const int *idx, int batch, int hp, int wp, int ho, int wo, int nlists, int *lists, int *ws, void *stream);
int dz_bev_fill_spans(const int *list, int batch, int ho, int wo, const float *shift, int relu, int cout, float *out, int out_hp, int out_wp,
                      int out_cstride, int out_coff, const float *zero_resp, int math, void *stream);
/* dz_sparse_to_bev on pair16 rows / images (the 16-bit halves are moved, no arithmetic) */
int dz_sparse_to_bev_split(const float *feats, const int *coords, const int *d_m, int cap, int c, int d, int h,
                           int w, int pad, float *bev, void *stream);
/* the same image written whole (zeros included) from the level's own index instead of scattered into a zero-filled canvas:
 * for d == 2 z slabs (VoxelResBackBone8x's encoded tensor; DZ_ERR_UNSUPPORTED otherwise).  bitmap / prefix = the level's index
 * (dz_index_downsample), batch / d / h / w / layout its grid.  Same bytes as fill + dz_sparse_to_bev_split
 * (height_compression.py:20-24: channel = ch * D + z).  feat_rows = rows of the `feats` buffer (the level's row capacity): a cell
 * whose rank is not below it - a level that overflowed a calibrated capacity keeps every site in its bitmap - is written as empty,
 * exactly what the scatter form does with the rows it drops; nothing is read past the buffer. */
int dz_sparse_to_bev_split_dense(const float *feats, int feat_rows, const uint32_t *bitmap, const uint32_t *prefix, int batch, int c,
                                 int d, int h, int w, int layout, int pad, float *bev, void *stream);
/* dz_conv2d_forward on pair16 images: desc->in pair16, desc->w (groups, kh*kw, cout_pad, cin) pair16
 * (cout_pad % 32 == 0, cin % 32 == 0), desc->out pair16 or, with out_f32 != 0, plain fp32 (last head conv). */
int dz_conv2d_forward_split(const dz_conv2d_desc *h_desc, int math, int out_f32, void *stream);
/* the kernel and tile dz_conv2d_forward_split runs for this descriptor and out_f32, "none" where it refuses the layer */
const char *dz_conv2d_variant_split(const dz_conv2d_desc *h_desc, int out_f32);
/* Opt-in engine of the exact-fp32 mode for the 3 x 3 stride-1 layers (csrc/conv3x3_t.hip): fp32 images in and out exactly as
 * dz_conv2d_forward takes and writes them, every operand on the bf16 matrix pipe as THREE bf16 limbs.  Any finite fp32 x is exactly
 * h + m + l with h = rn(x), m = rn(x - h), l = x - h - m (8 + 8 + 8 = 24 bits; x is clamped to +-bf16-max before the first rounding
 * only, so no limb is inf); a product is h.h + h.m + m.h + h.l + l.h + m.m, six bf16 MFMAs whose products are exact in fp32 - the
 * dropped terms are at most 2^-26 of |x.w|.  fp32-class results in another accumulation order than dz_conv2d_forward's.  For
 * |x| < 2^-100 the l limb is a bf16 subnormal; the matrix pipe keeps it (measured).
 *   desc->w = the weights split at plan time: (9, cout_pad, cin / 8, 3, 8) bf16 - per output-channel row and group of 8 input
 *   channels 16 bytes of h, 16 of m, 16 of l (ops.pack_weight_limb3).  Epilogue and write contract as dz_conv2d_forward.
 * dz_conv3x3_limb3_supported (host only, no GPU needed) is 1 exactly for kh == kw == 3, stride 1, groups 1, cin % 32 == 0,
 * cout_pad % 64 == 0, no phase_groups / in_rowidx / in_tiles / group_shift / group_max, and image and weight bytes below 2 GiB;
 * dz_conv3x3_limb3_forward returns DZ_ERR_UNSUPPORTED for anything else without launching.  dz_conv3x3_limb3_variant:
 * "k_conv3x3_t<8x32x128>" (cout_pad % 128 == 0), "k_conv3x3_t<8x32x64>" or "none". */
int dz_conv3x3_limb3_forward(const dz_conv2d_desc *h_desc, void *stream);
int dz_conv3x3_limb3_supported(const dz_conv2d_desc *h_desc);
const char *dz_conv3x3_limb3_variant(const dz_conv2d_desc *h_desc);
/* Opt-in engine of the exact-fp32 mode for the dense layers dz_conv3x3_limb3_forward does not take (csrc/conv2d_t.hip): the generic
 * implicit GEMM of dz_conv2d_forward in the three-limb arithmetic above - same fp32 images in and out, same pixel mapping, epilogue
 * and write contract (never the border, other channels, the pad channels g_cout .. cout_pad - 1, or other phases' pixels).
 *   desc->w = (groups * kh * kw, round_up(cout_pad, 32), cin / 8, 3, 8) bf16: ops.pack_weight_limb3 of the (groups * taps, cin,
 *   cout_pad) weights with cout_mult = 32 (zero rows behind cout_pad).  scale / shift as dz_conv2d_forward (NULL = 1 / 0).
 * dz_conv2d_limb3_supported (host only, no GPU needed) is 1 exactly for kh == kw in {1, 3}, stride in {1, 2}, groups 1..8,
 * cin % 32 == 0, cout_pad % 16 == 0, no group_shift / group_max / phase_groups / in_rowidx / in_tiles, and image and weight bytes
 * below 2 GiB; any in_coff / in_cstride / out_coff / out_cstride / out_s* / out_d* / relu that dz_conv2d_forward takes.
 * dz_conv2d_limb3_forward returns DZ_ERR_UNSUPPORTED, naming the field, for anything else without launching.
 * dz_conv2d_limb3_variant: "k_conv2d_t<128x128x16>" (cout_pad % 128 == 0), "k_conv2d_t<128x64x32>" (other cout_pad above 32),
 * "k_conv2d_t<128x32x32>" (cout_pad 16 or 32) or "none".  Accumulation order: taps, then channels, six limb terms smallest first. */
int dz_conv2d_limb3_forward(const dz_conv2d_desc *h_desc, void *stream);
int dz_conv2d_limb3_supported(const dz_conv2d_desc *h_desc);
const char *dz_conv2d_limb3_variant(const dz_conv2d_desc *h_desc);
/* dz_linear_forward on pair16 rows: x (rows, x_stride words) pair16, w (cout_pad, cin) pair16 (cin, cout_pad % 32 == 0), y pair16
 * rows or, with out_f32 != 0, fp32 rows; group_shift (row groups, cout_pad) fp32 as in dz_linear_forward.
 * group_max != 0 (with out_f32): the torch.max over the points of an object that follows the PointNet encoders
 * (geometry_transformer.py:124,137, position_transformer.py:108,117) fused into the layer: y = (rows / group_rows, y_stride) fp32,
 * the maximum over each group's rows; the (rows, cout) activation is not written.  group_rows % 128 == 0. */
int dz_linear_forward_split(const float *x, long rows, int cin, int x_stride, const float *w, int cout, int cout_pad, const float *scale,
                            const float *shift, const float *group_shift, int group_rows, int relu, float *y, int y_stride, int math,
                            int out_f32, int group_max, void *stream);
const char *dz_spconv_variant_split(int cin, int cout);
/* ... and with the arm of a launch whose table has kvol taps, comes with / without tile masks and is nbr_bytes long: "<instance> ring"
 * (neighbour indices through a register ring) or "<instance> lds" (the table slice staged in LDS: no masks, a table of 2 GiB or
 * more; the 128-row tiles of the layers with up to 32 output channels have this arm only); the k_spconv_w instances have one arm and
 * keep their plain name.  kvol decides nothing. */
const char *dz_spconv_variant_split_arm(int cin, int cout, int kvol, int has_tile_masks, size_t nbr_bytes);
/* ... and of dz_spconv_forward_split_packed ("none": a layer it refuses). */
const char *dz_spconv_variant_split_packed(int cin, int cout);
/* Cross-attention of a few queries over a long memory with the key / value projections folded into the queries (csrc/xattn_fold.hip;
 * multi_head_attention.py:199-288 as called by decoder.py:79-84 for the geometry refiner: 3 queries x 4096 memory points x 8 heads).
 * Equal to  out = softmax(scale * (q_h) . (Wk_h m + bk_h)) (Wv_h m + bv_h)  per head, computed WITHOUT projecting the memory:
 * q (b, lq, e) fp32 = the projected queries (Wq x + bq, NOT yet scaled); mem (b, lk, e) fp32 = the raw memory rows; wk_oi (e, e) = Wk as
 * stored by torch (rows = output channel); wv_io (e, e) = Wv^T (rows = input channel); bv (e); key_padding_mask (b, lk) bytes or NULL
 * (non-zero = ignore); out (b, lq, e) fp32 = the heads' outputs before out_proj.  bk cancels in the softmax.  fp32 throughout.
 * Supported (dz_xattn_folded_supported) when e == 256, e % heads == 0 and heads * lq <= 32; workspace from dz_xattn_folded_workspace_bytes. */
int dz_xattn_folded_supported(int lq, int e, int heads);
size_t dz_xattn_folded_workspace_bytes(int b, int lk);
int dz_xattn_folded(const float *q, const float *mem, const uint8_t *key_padding_mask, const float *wk_oi, const float *wv_io, const float *bv,
                    int b, int lq, int lk, int e, int heads, float scale, float *workspace, size_t workspace_bytes, float *out, void *stream);
/* The refiner's memory branch behind its PointNet encoder in one kernel (csrc/mlp_chain.hip; geometry_transformer.py:56-67,126-133,
 * position_transformer.py:60-72,108-117, multi_head_attention.py:199-236):  h = ReLU(sa * (Wa x + group_shift[row / group_rows]) + ba)
 * (128 -> 512), mem = ReLU(sb * (Wb h) + bb) (512 -> 256), and - when wk is not NULL - K = Wk mem + bk, V = Wv mem + bv (256 -> 256).
 * x (rows, 128) pair16 (the tapped encoder layer); wa (512, 128), wb (256, 512), wk / wv (256, 256) pair16, rows = output channel;
 * group_shift (rows / group_rows, ldg >= 512) fp32 or NULL; mem / k / v (rows, 256) fp32.  Split math only; group_rows % 32 == 0;
 * rows * 1024 < 2 GiB.  Bit-identical to the same layers run one dz_linear_forward_split each. */
int dz_mlp_chain_forward(const float *x, long rows, const float *wa, const float *sa, const float *ba, const float *group_shift, int ldg, int group_rows,
                         const float *wb, const float *sb, const float *bb, const float *wk, const float *bk, const float *wv, const float *bv,
                         float *mem, float *k, float *v, int math, void *stream);
/* Fused PointNet encoder (csrc/pointnet.hip; geometry_transformer.py:34-67,118-140, position_transformer.py:43-124): three
 * point-wise layers 32 -> 128 -> 128 -> c3 (c3 in {128, 256, 512}; BatchNorm scale / shift + ReLU after each) and the max over
 * every group of group_rows consecutive rows (group_rows % 32 == 0, rows % group_rows == 0) in one kernel; the activations never
 * leave the registers.  x (rows, 32) pair16 - or, with x_cols_f32 = 16 / 32, (rows, x_cols_f32) fp32 rows split on the way in (columns
 * beyond x_cols_f32 count as zero); w1 (128, 32), w2 (128, 128), w3 (c3, 128) pair16; out (rows / group_rows, c3) fp32;
 * tap (rows, 128) pair16 or NULL = the second layer's output (the reference reads it through a forward hook).  Split math only. */
int dz_pointnet3_forward(const float *x, long rows, const float *w1, const float *s1, const float *b1, const float *w2, const float *s2,
                         const float *b2, const float *w3, const float *s3, const float *b3, int c3, int group_rows, float *tap, float *out,
                         int x_cols_f32, int math, void *stream);

/* ---------------------------------------------------------------------------------------------
 * CenterHead decode + NMS (center_head.py:315-368, centernet_utils.py:138-230,
 * model_nms_utils.py:6-25, utils/detzero_utils/ops/iou3d_nms/)
 * ------------------------------------------------------------------------------------------- */
/* head (B, HW, 12) channel-last, columns [center 0:2 | center_z 2 | dim 3:6 | rot 6:8 | iou 8 | hm 9:12].
 * Produces, per batch item, the top-K (score = sigmoid(hm)*clamp(iou,0,1)^2) candidates in
 * descending score order that pass the score threshold and the centre range test:
 *   boxes (B,K,7) [x,y,z,dx,dy,dz,heading], scores (B,K), labels (B,K) i32 0-based, d_counts (B). */
size_t dz_centerhead_decode_workspace_bytes(int batch, int hw, int ncls, int k);
int dz_centerhead_decode(const float *head, int batch, int h, int w, int ncls, int k, float score_thresh,
                         const float *h_limit6, const float *h_range6, const float *h_vsize3, int stride,
                         int use_iou, float *boxes, float *scores, int *labels, int *d_counts, void *ws,
                         size_t ws_bytes, void *stream);
/* The two halves of dz_centerhead_decode (which is select followed by decode_selected on one workspace).
 * select reads columns 8:12 of the head map only (iou, hm) and leaves in the workspace, per batch item, the min(K, ncls*HW)
 * selected candidates in descending (score, then ascending flat index) order - 64-bit words  score bits << 32 | ~(cls*HW + pix),
 * DZ_CENTERHEAD_CAND_STRIDE words per item - and that count.  dz_centerhead_candidates_offset gives the byte offset of the list
 * (which = 0) or of the (B) int32 counts (which = 1) inside the workspace.  decode_selected reads the list and columns 0:8 of the
 * head map at the listed cells only - the columns dz_head_at_candidates fills between the two calls. */
#define DZ_CENTERHEAD_CAND_STRIDE 1024
size_t dz_centerhead_candidates_offset(int batch, int hw, int ncls, int k, int which);
int dz_centerhead_select(const float *head, int batch, int h, int w, int ncls, int k, int use_iou, void *ws, size_t ws_bytes, void *stream);
int dz_centerhead_decode_selected(const float *head, int batch, int h, int w, int ncls, int k, float score_thresh,
                                  const float *h_limit6, const float *h_range6, const float *h_vsize3, int stride,
                                  float *boxes, float *scores, int *labels, int *d_counts, void *ws, size_t ws_bytes, void *stream);

/* The regression branches of a CenterHead (center, center_z, dim, rot: center_head.py:14-48) at candidate cells only.
 * shared (B, h+2, w+2, 64) zero-bordered pair16 map of `math` (a split mode); cand / d_ncand: the list dz_centerhead_select writes
 * (cand_stride words per item; slots >= d_ncand[b] do nothing).  w1 / s1 / b1: packed hidden-layer weights (9, w1_cout, 64) with
 * folded BatchNorm scale / shift, of which channels 0 .. 64 * nbranch - 1 are the branches'; w2 (groups, 9, 32, 64), s2 / b2
 * (groups * 32): the grouped output layer, branch g = group g.  For every candidate the 3 x 3 hidden pixels around its cell are
 * evaluated (pixels outside the image are zero, as in the zero-bordered hidden map), rounded to pair16, and the output layer
 * writes columns g_ooff[g] .. + g_cout[g] - 1 of the cell's row of head (B, h*w, 12) fp32.  Accumulation order, MFMA shape and
 * roundings are those of dz_conv2d_forward_split, so the values are the dense route's bit for bit.  dz_head_at_candidates_supported:
 * 1 when (math, shared channels) is served. */
int dz_head_at_candidates_supported(int math, int channels);
int dz_head_at_candidates(const float *shared, int batch, int h, int w, const unsigned long long *cand, const int *d_ncand, int cand_stride,
                          int k, const float *w1, int w1_cout, const float *s1, const float *b1, const float *w2, const float *s2,
                          const float *b2, int nbranch, const int *h_g_cout, const int *h_g_ooff, float *head, int math, void *stream);

/* RoI features of the first-stage boxes (center_head.py:408-432,461-486: get_box_center with num_point 5 + absl_to_relative +
 * centernet_utils.bilinear_interpolate_torch:233-262): boxes (n, 7) of ONE frame; bev = that frame's (h, w, c) map, channel stride 1,
 * pixel / row strides in floats; map cell of a point = (p - lo) / voxel / stride; out (n, 5 * c) = [centre | front | back | left | right]. */
int dz_roi_bev_features(const float *boxes, int n, const float *bev, long row_stride, long pix_stride, int h, int w, int c, float x_lo, float y_lo,
                        float voxel_x, float voxel_y, int stride, float *out, void *stream);

/* iou3d_nms_cuda.nms_gpu (iou3d_nms.cpp:114-160 + nms_kernel iou3d_nms_kernel.cu:386-430), with the
 * suppression sweep done on the device.  boxes (n_cap,7) already in descending score order;
 * *d_n of them valid (d_n may be NULL).  keep (n_cap) i32 receives kept indices in order,
 * *d_num_keep their number (limited to post_max). */
size_t dz_nms_workspace_bytes(int n_cap);
int dz_nms_rotated(const float *boxes, const int *d_n, int n_cap, float thresh, int post_max, int *keep,
                   int *d_num_keep, void *ws, size_t ws_bytes, void *stream);
/* the same for `batch` frames in one launch pair: boxes (batch,n_cap,7), d_n (batch), keep (batch,n_cap),
 * d_num_keep (batch); ws >= batch * dz_nms_workspace_bytes(n_cap) */
int dz_nms_rotated_batched(const float *boxes, const int *d_n, int batch, int n_cap, float thresh, int post_max,
                           int *keep, int *d_num_keep, void *ws, size_t ws_bytes, void *stream);
/* final selection of model_nms_utils.py:22-25 / center_head.py:350-360 as one gather:
 * out (batch, post_max, 9) rows [x,y,z,dx,dy,dz,heading,score,label(1-based)] of the kept candidates, zeros after */
int dz_pack_detections(const float *boxes, const float *scores, const int *labels, const int *keep,
                       const int *d_num_keep, int batch, int k, int post_max, float *out, void *stream);

/* iou3d_nms_cuda.boxes_overlap_bev_gpu / boxes_iou_bev_gpu (iou3d_nms.cpp:60-111) : (na,nb) f32 */
int dz_boxes_overlap_bev(const float *a, int na, const float *b, int nb, float *out, void *stream);
int dz_boxes_iou_bev(const float *a, int na, const float *b, int nb, float *out, void *stream);

/* Pair matrices of the tracker's association metrics (tracking/.../data_association/distance.py), one kernel each, the final
 * value per (i, j): a (na,7), b (nb,7) -> out (na,nb) f32.
 *   DZ_BOXM_UNION_BEV     iou3d_nms_cuda.boxes_union_bev_gpu: area of the convex hull of the two footprints' eight corners (the
 *                         quantity iou3d_nms_kernel.cu:235-326 is meant to compute; its walk reads an unwritten hull[0] and is
 *                         not transcribed)
 *   DZ_BOXM_IOU3D         iou3d_nms_utils.boxes_iou3d_gpu (:74-107), bit-identical to that composition around dz_boxes_overlap_bev
 *   DZ_BOXM_GIOU3D        iou3d_nms_utils.boxes_giou3d_gpu (:110-151) as written: enclosing height = min(tops) - min(bottoms)
 *   DZ_BOXM_GIOU3D_EXACT  the same with enclosing height = max(tops) - min(bottoms), the textbook GIoU
 * Any other `metric`: DZ_ERR_UNSUPPORTED, the value in dz_last_error(). */
#define DZ_BOXM_UNION_BEV 0
#define DZ_BOXM_IOU3D 1
#define DZ_BOXM_GIOU3D 2
#define DZ_BOXM_GIOU3D_EXACT 3
int dz_boxes_pairwise_metric(const float *a, int na, const float *b, int nb, int metric, float *out, void *stream);
/* The same metrics on PAIRED boxes: a, b (n,7) -> out (n,) f32, out[i] = metric(a[i], b[i]) - element (i, i) of
 * dz_boxes_pairwise_metric's matrix bit for bit (one pair body serves both kernels), without the matrix.  n == 0 launches nothing.
 * Any other `metric`, or n * 7 >= 2^31: DZ_ERR_UNSUPPORTED. */
int dz_boxes_paired_metric(const float *a, const float *b, int n, int metric, float *out, void *stream);
/* Recall table of the refining models' generate_recall_record (refining/detzero_refine/models/geometry_refine_model.py:98-141,
 * position_refine_model.py:100-133) for a whole batch of tracks in one launch.
 *   boxes_in / boxes_out / boxes_gt (batch, t_cap, 7) f32, padded; mask (batch, t_cap) uint8, 1 = matched pair, counted;
 *   d_len (batch) int32 on the device: valid rows per track, clamped to 0..t_cap.  Rows with mask 0 or at / beyond d_len[b] are
 *   never read as boxes.
 *   h_thresholds: host array, 1 <= n_thr <= 8, each cast to f32 (as torch compares an fp32 tensor with a Python scalar).
 *   iou_in / iou_out (batch, t_cap) f32, each optional (NULL): the paired DZ_BOXM_IOU3D of (in, gt) resp. (out, gt) on counted
 *   rows, 0 on every other row.
 *   counts (batch, 2, n_thr + 1) int32, zeroed here on `stream`: [b][s][0] = counted rows of track b, [b][s][1 + k] = counted
 *   rows with iou > thresholds[k] (strictly, in fp32); s = 0 input side, s = 1 output side.  Integer adds only: the table is
 *   the same on every run.
 * DZ_ERR_UNSUPPORTED for n_thr outside 1..8 and batch * t_cap * 7 >= 2^31 (checked before any pointer is looked at);
 * DZ_ERR_INVALID for null pointers and negative sizes. */
int dz_track_recall_iou3d(const float *boxes_in, const float *boxes_out, const float *boxes_gt, const unsigned char *mask,
                          const int *d_len, int batch, int t_cap, const double *h_thresholds, int n_thr, float *iou_in,
                          float *iou_out, int *counts, void *stream);

/* iou3d_nms_cuda.nms_normal_gpu (iou3d_nms.cpp + nms_normal_kernel / iou_normal iou3d_nms_kernel.cu:433-491): axis-aligned BEV
 * IoU, the heading ignored, greedy by score.  Arguments, limits (n_cap <= 4096) and workspace (dz_nms_workspace_bytes) of
 * dz_nms_rotated / dz_nms_rotated_batched. */
int dz_nms_normal(const float *boxes, const int *d_n, int n_cap, float thresh, int post_max, int *keep, int *d_num_keep,
                  void *ws, size_t ws_bytes, void *stream);
int dz_nms_normal_batched(const float *boxes, const int *d_n, int batch, int n_cap, float thresh, int post_max, int *keep,
                          int *d_num_keep, void *ws, size_t ws_bytes, void *stream);

/* gather rows: out[i] = src[idx[i]] for i < *d_n (used to apply the NMS keep list on device) */
int dz_gather_rows(const float *src, const int *idx, const int *d_n, int n_cap, int c, float *out,
                   void *stream);

/* ---------------------------------------------------------------------------------------------
 * Refining module, secondary kernel set
 * ------------------------------------------------------------------------------------------- */
/* Points per box: counts[t] = number of points inside box t, the inside test of dz_points_in_boxes_v2, no (T, M) mask
 * (roiaware_pool3d_utils.points_in_boxes_num_gpu -> points_in_boxes_num kernel, used by tracking/detzero_track/datasets/
 * data_processor.py:64-69).  boxes (t,7) f32, pts (m,3) f32, counts (t,) i32 (overwritten). */
int dz_points_in_boxes_count(const float *boxes, const float *pts, int t, int m, int *counts, void *stream);

/* roiaware_pool3d_cuda.points_in_boxes_gpu_v2 (roiaware_pool3d.cpp:135-155,
 * roiaware_pool3d_kernel.cu:352-374): mask (B,T,M) i32, 1 where point m is inside box t. */
int dz_points_in_boxes_v2(const float *boxes, const float *pts, int batch, int t, int m, int *mask,
                          void *stream);
/* Object crop with compaction - the consumer side of points_in_boxes_gpu_v2 in daemon/prepare_object_data.py:250-273,310
 * (`obj_pts = pts[obj_pts_mask[idx, :]]` per object) without the dense (T, M) mask or its D2H copy.
 *   xyz (m,3) f32: point coordinates used for the inside test (same test as dz_points_in_boxes_v2);
 *   boxes (t,7) f32 (already enlarged by the caller); payload (m, payload_words) 32-bit words: the rows to gather
 *   (e.g. 4 float64 = 8 words); out (cap, payload_words): the kept rows of box 0, then box 1, ... each in ascending
 *   point order; out_index (cap) i32 or NULL: source point of every kept row; offsets (t+1) i32: row range of each
 *   box; *d_total: number of kept rows (rows beyond cap are dropped, compare with cap). */
size_t dz_crop_points_workspace_bytes(int m, int t, int cap);
int dz_crop_points_in_boxes(const float *xyz, int m, const float *boxes, int t, const void *payload, int payload_words,
                            void *out, int *out_index, int *offsets, int *d_total, int cap, void *ws, size_t ws_bytes,
                            void *stream);

/* Segmented object crop over the frames of a sequence (csrc/seq_crop.hip): the crop above for F frames at once, in two
 * passes without a (T, M) bitmap and without a capacity.
 *   xyz (m,3) f32: the points of all frames back to back; pt_off (n_frames+1) i32: first point of every frame;
 *   boxes (nb,7) f32 (already enlarged), frame-major; box_off (n_frames+1) i32: first box of every frame;
 *   rank (nb) i32: a permutation of 0..nb-1, the output segment of box b (identity = (frame, box) order);
 *   A chunk is dz_seq_crop_chunk_points() consecutive points of one frame; only frames with boxes and points have chunks.
 *   chunk_frame (n_chunks) i32: frame of every chunk, ascending; chunk_first (n_frames+1) i32: first chunk of every frame;
 *   row_off (nb+1) i32: first entry of every segment's row in the count table - row rank[b] holds one entry per chunk
 *   of box b's frame, row_off[nb] = n_entries.
 * dz_seq_crop_count writes counts (n_entries) i32: points of the chunk inside the box.  The caller forms the exclusive
 * prefix over counts (same shape) and its total: prefix[row_off[r]] is the first output row of segment r.
 * dz_seq_crop_fill writes out (total, payload_words) 32-bit words: payload (m, payload_words) rows of the kept points,
 * segment after segment, ascending point index within a segment; out_index (total) i32 or NULL: the source point.
 * No atomics: the same bytes on every run.  The caller guarantees that rank is a permutation and that the offset arrays
 * ascend and end at m / nb (ops.seq_crop_plan checks it); the kernels clamp what they read from them and write no row
 * at or beyond total.  DZ_ERR_INVALID: a negative size, m / nb / n_chunks / n_entries / total >= 2^31, a null pointer
 * with chunks to work on.  n_chunks == 0 (no frame, no boxes or no points) launches nothing. */
int dz_seq_crop_chunk_points(void);
int dz_seq_crop_count(const float *xyz, long long m, const int *pt_off, const float *boxes, long long nb, const int *box_off,
                      const int *rank, const int *row_off, int n_frames, const int *chunk_frame, const int *chunk_first,
                      long long n_chunks, int *counts, long long n_entries, void *stream);
int dz_seq_crop_fill(const float *xyz, long long m, const int *pt_off, const float *boxes, long long nb, const int *box_off,
                     const int *rank, const int *row_off, int n_frames, const int *chunk_frame, const int *chunk_first,
                     long long n_chunks, const int *counts, const int *prefix, long long n_entries, const void *payload,
                     int payload_words, void *out, int *out_index, long long total, void *stream);

/* multi_head_attention_forward core (refining/detzero_refine/models/transformer/
 * multi_head_attention.py:207-288): q (B,Lq,E), k,v (B,Lk,E) already projected, E = heads*32;
 * key_padding_mask (B,Lk) u8 (1 = ignore) or NULL; out (B,Lq,E).  softmax(q*scale . k^T) . v */
int dz_mha_core(const float *q, const float *k, const float *v, const uint8_t *key_padding_mask, int batch,
                int lq, int lk, int heads, float scale, float *out, void *stream);
/* The same core on the 16-bit matrix cores with q, k, v and the probabilities carried as (hi, lo) 16-bit pairs (csrc/mha_h.hip; three
 * MFMAs per product, fp32 accumulation and softmax): the arithmetic class of dz_linear_forward_split, for long key lists (PRM's
 * cross-attention: 200 queries x 9600 keys).  Same arguments; math = DZ_MATH_F16X2 or DZ_MATH_BF16X2; head dim 32. */
int dz_mha_core_split(const float *q, const float *k, const float *v, const uint8_t *key_padding_mask, int batch, int lq, int lk, int heads,
                      float scale, float *out, int math, void *stream);
/* Opt-in engine of the exact-fp32 mode for the same core (csrc/mha_t.hip, k_mha_block_t): dz_mha_core's arguments and semantics, fp32 in
 * and out, on the bf16 matrix pipe in the three-limb arithmetic of dz_linear_limb3_forward below - q (times scale * log2 e, rounded
 * once), K, V and the probabilities p = exp2(s - max) each as three exact bf16 limbs h + m + l, both products as the six terms
 * l.h  h.l  m.m  m.h  h.m  h.h (K or V limb . q or p limb, smallest first), fp32 accumulation, keys ascending, no atomics: two launches
 * agree bit for bit.  One route for every lq >= 1 (a workgroup = one (batch, head), up to 8 waves of 32 queries, key blocks of 64).
 * A masked key's score is replaced by -inf (its K row may hold NaN or any finite value); a fully masked batch entry is NaN for that
 * entry only; only rows [0, lq) of out are written.
 * dz_mha_core_limb3_supported (host only, no GPU needed) is 1 exactly when the sizes pass: batch >= 0, lq >= 0, lk >= 1,
 * 1 <= heads <= 65535, batch <= 65535 (the grid's limits).  Anything else, and a null q / k / v / out: DZ_ERR_INVALID with
 * dz_mha_core's wording, before any launch and before a pointer is read.  batch == 0 or lq == 0: DZ_OK, no launch. */
int dz_mha_core_limb3(const float *q, const float *k, const float *v, const uint8_t *key_padding_mask, int batch, int lq, int lk, int heads,
                      float scale, float *out, void *stream);
int dz_mha_core_limb3_supported(int batch, int lq, int lk, int heads);

/* y (rows, cout) = relu?( x (rows, cin) . W (cin, cout_pad) * scale + shift ) — the 1x1 Conv1d/Conv2d
 * + BatchNorm + ReLU stacks of the GRM/PRM PointNet encoders
 * (refining/detzero_refine/models/modules/geometry_transformer.py:34-67), same MFMA engine. */
int dz_linear_forward(const float *x, int rows, int cin, int x_stride, const float *w, int cout, int cout_pad,
                      const float *scale, const float *shift, const float *group_shift, int group_rows, int relu,
                      float *y, int y_stride, void *stream);
/* Opt-in engine of the exact-fp32 mode for these linear layers (csrc/linear_t.hip): dz_linear_forward's row GEMM in the three-limb
 * arithmetic of dz_conv3x3_limb3_forward above - fp32 rows in and out, every operand as three exact bf16 limbs h + m + l, a product
 * as the six terms l.h  h.l  m.m  m.h  h.m  h.h (weight limb . input limb, smallest first) on the bf16 matrix pipe; the dropped terms
 * m.l + l.m + l.l are at most 2^-26 of |x.w|.
 *   x (rows, x_stride) fp32, columns [0, cin) read, cin .. x_stride - 1 never; w_limb = (round_up(cout_pad, 32), cin / 8, 3, 8) bf16:
 *   ops.pack_weight_limb3_generic of the (1, cin, cout_pad) weights of dz_linear_forward (zero rows behind cout_pad).
 *   y = relu?(fma(acc + group_shift[row / group_rows][col], scale[col], shift[col])): group_shift (row groups, cout_pad) fp32 or NULL
 *   goes in once, before scale / shift; group_rows < 1 means 1; the last group may be ragged; scale / shift NULL = 1 / 0.
 * Accumulation order per output element: 16-channel k-steps ascending, the six terms in the order above, one accumulator - whatever
 * the tile or the launch split; no atomics, two launches agree bit for bit.
 * Write contract: columns [0, cout) of rows [0, rows) only (float4 where y_stride % 4 == 0 and y is 16-byte aligned, word by word
 * otherwise); columns cout .. y_stride - 1 and everything behind the last row keep their contents.
 * Rows beyond the 2 GiB buffer window run as several launches over row chunks, aligned to group_rows when there is an addend.
 * max_launch_rows: 0 = the window alone; n > 0 additionally caps the rows of a launch (rounded down to a multiple of group_rows with
 * an addend) - the result does not depend on it.
 * dz_linear_limb3_supported (host only, no GPU needed) is 1 exactly for cin % 32 == 0, cout_pad % 16 == 0, 1 <= cout <= cout_pad,
 * x_stride >= cin, x_stride % 4 == 0, y_stride >= cout and weights below 2 GiB; dz_linear_limb3_forward returns DZ_ERR_UNSUPPORTED,
 * naming the field, for anything else, for one row group beyond the window and for a max_launch_rows below group_rows - before any
 * launch.  Null x / y / w_limb, negative rows or max_launch_rows: DZ_ERR_INVALID.  rows == 0: DZ_OK, no launch.
 * dz_linear_limb3_variant: "k_linear_t<128x128x16>" (cout_pad % 128 == 0), "k_linear_t<128x64x32>" (other cout_pad above 32),
 * "k_linear_t<128x32x32>" (cout_pad 16 or 32) or "none" (cin or cout_pad the engine does not cover). */
int dz_linear_limb3_forward(const float *x, long rows, int cin, int x_stride, const float *w_limb, int cout, int cout_pad,
                            const float *scale, const float *shift, const float *group_shift, int group_rows, int relu,
                            float *y, int y_stride, long max_launch_rows, void *stream);
int dz_linear_limb3_supported(int cin, int x_stride, int cout, int cout_pad, int y_stride);
const char *dz_linear_limb3_variant(int cin, int cout_pad);

/* dz_linear_forward for a few rows against a very long input (the PDV head's first FC layer, pdv_head.py:154-172: 41 472 -> 256 for
 * some hundred RoIs): the input channels are cut into `splits` (1..8, cin % (splits * 32) == 0) groups that run side by side (one
 * grouped launch into the workspace) and are summed in a second pass with scale / shift / ReLU.  Same arguments otherwise. */
size_t dz_linear_splitk_workspace_bytes(int rows, int cout_pad, int splits);
int dz_linear_forward_splitk(const float *x, int rows, int cin, int x_stride, const float *w, int cout, int cout_pad, const float *scale,
                             const float *shift, int relu, float *y, int y_stride, int splits, float *workspace, size_t workspace_bytes,
                             void *stream);

/* out (groups, c) = max over the `len` rows of each group of x (groups*len, c): the point-wise max pooling of
 * the GRM/PRM PointNet encoders (geometry_transformer.py:124,137; position_transformer.py:108,117). */
int dz_group_max(const float *x, int groups, int len, int c, float *out, void *stream);

/* out = LayerNorm(x + y) * gamma + beta over rows of 256 channels (decoder.py:75-88: residual + post-LN);
 * y may be NULL; do_norm == 0 gives the plain sum x + y (with_pos_embed, decoder.py:50-51). */
/* out[i] = 1 when every int of row i of all n (<= 4) row-major int32 tensors t[k] (rows x w[k], w[k] % 4 == 0) is zero: PDV's
 * empty-grid-point mask `(ball_idxs == 0).all(-1)` (pdv_head.py:521-523) over the per-branch ball indices, without concatenating them. */
int dz_rows_all_zero(const int *const *t, const int *w, int n, int rows, unsigned char *out, void *stream);
int dz_add_layernorm(const float *x, const float *y, const float *gamma, const float *beta, int rows, int c,
                     float eps, int do_norm, float *out, void *stream);
/* out = post + (group_skip[row / group_rows] ? post : LayerNorm(x + y)), c = 192: the PDV encoder layer's second normalisation together
 * with COMBINE (pooled + attended features) and the untouched rows of RoIs without points (pdv_head.py:540-560, attention_utils.py:31-44). */
int dz_add_layernorm_combine(const float *x, const float *y, const float *gamma, const float *beta, int rows, int c, float eps, const float *post,
                             const unsigned char *group_skip, int group_rows, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Object features: cropped object points -> inputs of the refining models.
 * Replaces, for inference, WaymoGeometryDataset.extract_track_feature
 * (refining/detzero_refine/datasets/waymo/waymo_geometry_dataset.py:73-131) and WaymoPositionDataset.extract_track_feature
 * (waymo_position_dataset.py:66-155) with their helpers (refining/detzero_refine/utils/data_utils.py:6-113,
 * utils/detzero_utils/box_utils.py:28-53), batched over objects.
 *
 * Common inputs (device): pts (P,4) float64 [x,y,z global, intensity] of all boxes, object-major then frame order;
 * box_offsets (F+1) first point of every box; traj (F,7) float64 global boxes; score (F) float64;
 * obj_box_offsets (B+1) first box of every object.  WHICH points survive the fixed-size selection is the caller's
 * (data_utils.py:12-30 draws with Python's random.sample): index lists, -1 = zero row.
 * ------------------------------------------------------------------------------------------------------------------ */
/* Device-side alternative to the host draw: set s of the call (global id first_set_id + s) keeps, of its counts[s] rows, a
 * uniformly random k-subset in ascending order (all rows when counts[s] < k, padded with -1) - the distribution of
 * sample_points, from a counter-based generator keyed by (seed, set id) instead of Python's random stream.  out_idx (n_sets,k). */
int dz_draw_subsets(const int *counts, int n_sets, int k, unsigned long long seed, int first_set_id, int *out_idx, void *stream);
#define DZ_GRM_XYZ 1
#define DZ_GRM_INTENSITY 2
#define DZ_GRM_P2S 4
#define DZ_GRM_SCORE 8
int dz_grm_feature_channels(int encoding);           /* channels of a memory row for these flags (order: xyz, intensity, p2s, score) */
/* mem_idx (B,mem_n): index into the object's concatenated points; query_box (B,q_max): box id in [0,F) or -1 (padding);
 * query_idx (B,q_max,q_n): index into that box's points.  memory (B,mem_n,channels) and query (B,q_max,q_n,4) float32:
 * points in the frame of their own box (waymo_geometry_dataset.py:75, data_utils.py:62-71). */
int dz_grm_encode_points(const double *pts, const int *box_offsets, const double *traj, const double *score,
                         const int *obj_box_offsets, const int *mem_idx, int mem_n, const int *query_box, const int *query_idx,
                         int q_max, int q_n, int batch, int encoding, float *memory, float *query, void *stream);

#define DZ_PRM_XYZ 0
#define DZ_PRM_INTENSITY 1
#define DZ_PRM_P2CO 2
#define DZ_PRM_SCORE 3
#define DZ_PRM_CLASS 4
int dz_prm_feature_channels(const int *h_encoding, int n_enc);   /* channels of a row for this (host) list of codes, -1 if invalid */
/* q_idx (F,q_n) / m_idx (F,m_n): per box, index into its points.  Outputs: query (B,box_max,q_n,channels), memory
 * (B,box_max,m_n,channels), traj_local (B,box_max,7) and padding_mask (B,box_max) float32, init_box (B,7) float64 - points
 * and boxes in the frame of the object's middle box (waymo_position_dataset.py:72-78, data_utils.py:74-113), boxes past
 * an object's own are zero with mask 1.  anchors: scratch of B*box_max*27 + 2*B doubles.  obj_cls (B) 1-based, may be
 * NULL without the 'class' feature; a class outside 1..3 (0 = unknown) sets none of the three class channels.  At most 40
 * channels per row, counted in whole groups of four (every feature once is 35): a longer list - a repeated 'p2co', say -
 * is refused with DZ_ERR_INVALID. */
int dz_prm_encode_points(const double *pts, const int *box_offsets, const double *traj, const double *score,
                         const int *obj_box_offsets, const int *obj_cls, const int *q_idx, const int *m_idx, int q_n, int m_n,
                         int batch, int box_max, const int *h_encoding, int n_enc, float *query, float *memory,
                         float *traj_local, float *padding_mask, double *init_box, double *anchors, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Test-time augmentation: point transforms of the augmented copies
 * (detection/detzero_det/datasets/augmentor/test_time_augmentor.py:32-83), restore of their boxes
 * (detection/detzero_det/models/centerpoint.py:165-203) and weighted box fusion
 * (detection/detzero_det/utils/ensemble_utils/wbf_3d.py:10-203 as called by ensemble.py:7-33), all on the device.
 * Operations: host arrays of codes + one float parameter each (angle in radians / scale factor, 0 otherwise).
 * ------------------------------------------------------------------------------------------------------------------ */
#define DZ_TTA_ORIGINAL 0
#define DZ_TTA_FLIP_X 1
#define DZ_TTA_FLIP_Y 2
#define DZ_TTA_FLIP_XY 3
#define DZ_TTA_ROT 4
#define DZ_TTA_SCALE 5
/* points (n,c) -> out (n_ops, n, c): copy i = points under operation i (columns >= 3 copied). */
int dz_tta_augment_points(const float *points, int n, int c, const int *h_kind, const float *h_param, int n_ops, float *out,
                          void *stream);
/* boxes (frames, n_ops, m, dim >= 7) in place: rows of copy i back to the original frame (columns >= 7 untouched). */
int dz_tta_restore_boxes(float *boxes, int frames, int n_ops, int m, int dim, const int *h_kind, const float *h_param, void *stream);
size_t dz_wbf_workspace_bytes(int frames, int cand);
/* weighted_boxes_fusion_3d with iou_type '3d' per frame: boxes (frames, cand, 7) float32, scores (frames, cand), labels
 * (frames, cand) in 1..3 (0 = padding); candidate c belongs to model c / per_model (weights: device doubles per model or NULL
 * = 1; weight_sum = their sum).  conf_max: 0 'avg', 1 'max'.  Outputs sorted by fused score: out_boxes (frames, cand, 7) and
 * out_scores (frames, cand) float64 as in the reference, out_labels, out_count (frames). */
int dz_wbf_fuse_3d(const float *boxes, const float *scores, const int *labels, const int *obj_ids, int frames, int cand, int per_model,
                   const double *weights, int n_models, const double *h_iou_thr3, const double *h_skip_thr3, double weight_sum,
                   int conf_max, int allows_overflow, double *out_boxes, double *out_scores, int *out_labels, int *out_obj_ids,
                   int *out_count, void *ws, size_t ws_bytes, void *stream);
/* obj_ids / out_obj_ids (frames, cand), both or neither: weighted_tracking_boxes_fusion_3d (wbf_3d.py:205-265) - a fused box
 * carries the object id of its most confident member that has one (>= 0), else -1. */

/* ------------------------------------------------------------------------------------------------------------------
 * Frame assembly from stored sweeps (DatasetTemplate.merge_sweeps, detection/detzero_det/datasets/dataset.py:164-195):
 * raw (n_total,6) float32 rows [x,y,z,intensity,elongation,NLZ] of n_sweeps sweeps back to back (host offsets,
 * n_sweeps+1 entries); h_transforms: per sweep rows 0..2 of inv(pose_current) @ pose_sweep (12 doubles, row-major);
 * h_time_offsets: seconds.  out (n_total,6) float32 receives the rows with NLZ == -1 in their stored order as
 * [x',y',z',tanh(intensity),elongation,time offset]; *d_count their number. */
size_t dz_merge_sweeps_workspace_bytes(int n_total);
int dz_merge_sweeps(const float *raw, int n_total, const int *h_sweep_offsets, const double *h_transforms, const double *h_time_offsets,
                    int n_sweeps, float *out, int *d_count, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * PDV second stage (detection/detzero_det/models/centerpoint_modules/pdv_head.py:269-637)
 * ------------------------------------------------------------------------------------------------ */
/* voxel_aggregation_utils.get_centroids_per_voxel_layer (:96-157): centroids of the points per voxel of the first feature
 * location's grid (voxel size already multiplied by its stride; grid = trunc((hi - lo) / vsize) as float32, :29-36) and, weighted
 * by the point counts, per voxel of a second location `scaling` times coarser.  points_b (n, 1+c) [b, x, y, z, f...];
 * cen (cap, 1+c) [b, mean x, y, z, f...], coords (cap, 4) int32 [b, z, y, x], counts (cap,), *d_m = number of voxels; rows come
 * in ascending (b, z, y, x) order (the order of torch.unique(dim=0) in the reference).  cen2 .. d_m2 may all be NULL. */
size_t dz_pdv_centroids_workspace_bytes(int n, int batch, int gx, int gy, int gz, int scaling, int cap1);
int dz_pdv_voxel_centroids(const float *points_b, int n, int c, const float *h_range6, const float *h_vsize3, const int *h_grid3,
                           int batch, int scaling, float *cen1, int *coords1, int *counts1, int *d_m1, int cap1, float *cen2,
                           int *coords2, int *counts2, int *d_m2, int cap2, void *ws, size_t ws_bytes, void *stream);
/* voxel_aggregation_utils.get_nonempty_voxel_feature_indices (:59-78) without the dense hash table: out[i] = row of cell
 * coords[i] = [b, z, y, x] in the sparse level (bitmap, prefix of dz_index_*), or -1. */
int dz_index_lookup(const int *coords, const int *d_n, int n, const uint32_t *bitmap, const uint32_t *prefix, int b, int d, int h,
                    int w, int layout, int *out, void *stream);
/* pointnet2_stack ball_query_count (src/ball_query_count_gpu.cu:16-62 + pointnet2_utils.py:78-83,186-189) for points that are
 * voxel centroids: at most one per cell of the (b, d, h, w) bitmap, listed in cell-key order (xyz (np, 3)).  Queries new_xyz
 * (mq, 3), `per_batch` consecutive queries per batch item.  idx (mq, nsample) int32: the first nsample points with d^2 < r^2 in
 * index order (relative to the batch item's first point), padded with the first hit, all 0 for an empty ball; cnt (mq,) hits. */
int dz_pdv_ball_query(const float *new_xyz, int mq, int per_batch, const float *xyz, const uint32_t *bitmap, const uint32_t *prefix,
                      int b, int d, int h, int w, const float *h_lo3, const float *h_vs3, float radius, int nsample, int *idx,
                      int *cnt, void *stream);
/* QueryAndGroup with use_xyz and use_density (pointnet2_utils.py:192-211, kde_utils.py:17-64, bandwidth 0.25): rows
 * (mq * nsample, row_stride) = [offset xyz, KDE density, the point's c features, zeros]. */
int dz_pdv_group_features(const float *new_xyz, int mq, int per_batch, const float *xyz, const float *feats, int c,
                          const uint32_t *bitmap, const uint32_t *prefix, int cells_per_batch, const int *idx, const int *cnt,
                          int nsample, float *rows, int row_stride, void *stream);
/* One branch of StackSAModuleMSGAttention in one kernel (csrc/pdv_sa.hip; pointnet2_modules.py:31-158): grouping as dz_pdv_group_features,
 * two point-wise layers (Conv2d 1x1 + folded BatchNorm + ReLU; w1 (cin_pad, ldw1) / w2 (h1, ldw2) fp32, rows = input channel, scale / shift
 * per output channel) and the max over the ball's nsample rows -> out (mq, h2) fp32.  Exact fp32 (v_mfma_f32_16x16x4_f32).  Instances
 * (dz_pdv_sa_pool_supported): nsample 16, (cin_pad, h1, h2) = (80, 32, 32) or (144, 64, 64), c % 4 == 0, c + 4 <= cin_pad, ReLU on both layers. */
int dz_pdv_sa_pool_supported(int c, int cin_pad, int h1, int h2, int nsample, int relu1, int relu2);
int dz_pdv_sa_pool(const float *new_xyz, int mq, int per_batch, const float *xyz, const float *feats, int c, const uint32_t *bitmap,
                   const uint32_t *prefix, int cells_per_batch, const int *idx, const int *cnt, int nsample, const float *w1, int ldw1,
                   const float *s1, const float *b1, int h1, const float *w2, int ldw2, const float *s2, const float *b2, int h2, int cin_pad,
                   float *out, void *stream);
/* The same branch on pair16 operands (math = DZ_MATH_F16X2 / DZ_MATH_BF16X2; the PDV head's split modes): w1 (h1, ldw1) / w2 (h2, ldw2) are
 * pair16 rows per OUTPUT channel (ld in channels, dz_pair16 packing), features stay fp32 rows (feat_rows x c) and are split in the
 * kernel.  Instances: (c, cin_pad, h1, h2) = (64, 80, 32, 32) and (128, 144, 64, 64), nsample 16.  Same outputs as dz_pdv_sa_pool up
 * to the pair16 product error (~2^-21 relative per product, fp32 accumulation). */
int dz_pdv_sa_pool_split_supported(int c, int cin_pad, int h1, int h2, int nsample, int relu1, int relu2);
int dz_pdv_sa_pool_split(const float *new_xyz, int mq, int per_batch, const float *xyz, const float *feats, long feat_rows, int c,
                         const uint32_t *bitmap, const uint32_t *prefix, int cells_per_batch, const int *idx, const int *cnt, int nsample,
                         const float *w1, int ldw1, const float *s1, const float *b1, int h1, const float *w2, int ldw2, const float *s2,
                         const float *b2, int h2, int cin_pad, int math, float *out, int ldo, void *stream);
/* (ldo: row stride of out in floats, >= h2 - the branches of a head write side by side into one (mq, sum of widths) tensor.  Grid points
 * whose ball is empty skip the arithmetic: their result is the layer stack applied to a zero row, computed once per wave.) */
/* density_utils.find_num_points_per_part_multi (:52-109) on points_in_multi_boxes (roiaware_pool3d_kernel.cu:377-404): counts
 * (batch, o, grid, grid, grid) int32 of the points (n, stride) [b, x, y, z, ...] per cell of every RoI (batch, o, 7), a point
 * counting for the first max_boxes RoIs (in RoI order) that contain it. */
int dz_pdv_part_counts(const float *points_b, int n, int stride, const float *rois, int batch, int o, int grid, int max_boxes,
                       int *counts, void *stream);
/* The same counts, bit for bit, with the RoIs binned on a 64 x 64 BEV grid first (a point then tests the handful of boxes whose
 * footprint circle reaches its cell instead of all o of its frame: ~0.5 ms -> tens of microseconds per 8 frames of 320k points).
 * ws: dz_pdv_part_counts_ws_bytes(batch, o) bytes of device scratch, 64-byte aligned (per frame: grid origin / scale, one 64-byte
 * line of box ids per cell, the staged box table).  More than 4096 RoIs per frame: runs dz_pdv_part_counts. */
size_t dz_pdv_part_counts_ws_bytes(int batch, int o);
int dz_pdv_part_counts_binned(const float *points_b, int n, int stride, const float *rois, int batch, int o, int grid, int max_boxes,
                              int *counts, void *ws, size_t ws_bytes, void *stream);
/* softmax(q k^T * scale + key padding mask) v for r independent sequences of l <= 256 tokens, one head of e <= 256 channels
 * (nn.MultiheadAttention core of attention_utils.TransformerEncoder; q, k, v, out (r, l, e) f32; mask (r, l) bytes or NULL). */
int dz_attention_single_head(const float *q, const float *k, const float *v, const unsigned char *key_padding_mask, int r, int l,
                             int e, float scale, float *out, void *stream);
/* The same layer with the key / value projections folded into its two GEMMs (one head): o' = softmax(q' x^T + mask) x over every group
 * of l consecutive rows, where x (r * l, e) pair16 are the layer's input rows (keys = values) and q' = x (Wq Wk^T) + Wk bq, scaled by
 * log2(e) / sqrt(E), (r * l, e) pair16; the caller applies (Wv Wo, bv Wo + bo) to o' (pdv_modules.py: PDVHead.attention).  e = 192,
 * l <= 224, math = DZ_MATH_F16X2 / DZ_MATH_BF16X2; out (r * l, e) pair16.  A fully masked group gives zero rows. */
/* The rest of the encoder layer around that attention, as two row-chain kernels (csrc/pdv_enc.hip; activations stay in registers):
 *   front: src = feats + (row_add ? W_p2 . ReLU(s0 * (W_p1 . pos_in) + b0) + b1 : 0), q = src . wq + uq          -> (rows, 192) pair16 each
 *   back:  x = LN1(src + op . wo + bo), y = LN2(x + w2 . ReLU(w1 . x + b1) + b2), out = pooled + (row_skip ? pooled : y) -> (rows, 192) fp32
 * Weights are pair16 rows per OUTPUT channel: w0 (96, 16), w1 (192, 96), wq / wo (192, 192), back w1 (128, 192), w2 (192, 128); pos_in
 * (rows, pin) fp32 with pin 4 or 8; feats / pooled (rows, 192) fp32; row_add / row_skip (rows) bytes; math = DZ_MATH_F16X2 / BF16X2. */
int dz_pdv_encoder_front(const float *pos_in, int pin, const float *feats, const unsigned char *row_add, long rows, const float *w0, const float *s0,
                         const float *b0, const float *w1, const float *b1, const float *wq, const float *uq, float *src, float *q, int math,
                         void *stream);
int dz_pdv_encoder_back(const float *op, const float *src, const float *pooled, const unsigned char *row_skip, long rows, const float *wo,
                        const float *bo, const float *g1, const float *be1, float eps1, const float *w1, const float *b1, const float *w2,
                        const float *b2, const float *g2, const float *be2, float eps2, float *out, int out_pair16, int math, void *stream);
/* (out_pair16: the result as pair16 rows - the operand of the head's FC stack - instead of fp32) */
int dz_self_attention_split_supported(int l, int e);
int dz_self_attention_split(const float *q, const float *x, const unsigned char *key_padding_mask, int r, int l, int e, float *out,
                            int math, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Tracking module (csrc/track.hip): the per-track and per-pair arithmetic of tracking/detzero_track/models/tracking_modules
 * (kalman_filter.py KalmanFilter, data_association.py one_stage + distance.py GNN_assignment's masking, track_manager.py
 * overlap_track_merge) on a device-resident track table of ONE sequence.  Frame order, the index bookkeeping of the association
 * stages and linear_sum_assignment stay on the host.
 *
 * dz_track_table: struct of arrays, `cap` rows each, rows [0, n) live, list order = the reference's `tracks` list.  The size and
 * heading of a track are columns 3:7 of its box at every point of the reference's code, so they are not stored twice.
 * A "row buffer" (detections of a frame, log, forward-pass results) is an array of DZ_TRACK_ROW_WORDS 32-bit words per row:
 *   [0:9] box f32 | [9] score f32 | [10] hit i32 | [11] num_points i32 | [12] track id i32 | [13] class code i32 |
 *   [14] frame ordinal i32 | [15] 0
 * All entry points: n == 0 (m == 0) launches nothing; DZ_ERR_UNSUPPORTED where 32-bit offsets would overflow, for more than
 * DZ_TRACK_MAX_CLASSES classes and for an unknown metric. */
#define DZ_TRACK_ROW_WORDS 16
#define DZ_TRACK_MAX_CLASSES 8
typedef struct {
    float *x;            /* (cap,5)  state [x, y, z, vx, vy] */
    float *P;            /* (cap,25) */
    float *Q;            /* (cap,25) */
    float *dt;           /* (cap)    delta_t: F = I with F[0][3] = F[1][4] = dt */
    float *box;          /* (cap,9)  [x, y, z, dx, dy, dz, heading, vx, vy] */
    int *cls;            /* (cap)    class code */
    float *score;        /* (cap) */
    float *update_score; /* (cap) */
    int *num_points;     /* (cap) */
    int *hit;            /* (cap) */
    int *miss;           /* (cap) */
    int *id;             /* (cap) */
    int cap;             /* rows allocated in every array; n (and n + m of dz_track_spawn) beyond it is DZ_ERR_INVALID */
} dz_track_table;
/* KalmanFilter.predict (kalman_filter.py:85-108) on rows [0, n), one thread per track, fp32: class `gate_class` (Vehicle; -1 = no
 * class) with |v| <= max(size) / 2 predicts with v = 0; x = F x, P = F P F^T + Q, Q *= 1.5, miss += 1, hit = 0,
 * box = [x0:3, size, heading, vx, vy]. */
int dz_track_predict(const dz_track_table *t, int n, int gate_class, void *stream);
/* Association cost matrix (data_association.py:36-58 + distance.py:22): out (nr, nc) f32,
 *   aff = metric(row box, col box); 0 where the classes differ (distinguish_class) ; 0 where aff < thr[row class];
 *   cost = 1 - aff; cost >= 1 -> 5000.
 * Rows: row_idx[r] >= 0 is table row row_idx[r] (< n), row_idx[r] < 0 is row (-row_idx[r] - 1) of the row buffer `ext` of n_ext rows
 * (the forward results that join the reverse pass).  Columns: rows col_idx[c] of the row buffer `det` of n_det rows.  A pair with
 * an index outside its buffer reads nothing and costs 5000.  h_thr: host array of n_cls thresholds.  metric: DZ_TRACK_AFF_IOU_BEV (the pair
 * body of dz_boxes_iou_bev), DZ_BOXM_IOU3D, DZ_BOXM_GIOU3D (the pair body of dz_boxes_pairwise_metric): bit-identical to those. */
#define DZ_TRACK_AFF_IOU_BEV 16
int dz_track_affinity(const dz_track_table *t, int n, const int *ext, int n_ext, const int *row_idx, int nr, const int *det, int n_det,
                      const int *col_idx, int nc, int metric, int distinguish_class, const float *h_thr, int n_cls, float *out,
                      void *stream);
/* KalmanFilter.update (kalman_filter.py:110-146) for m matches, one thread each: match (m,3) int32 [table row, det row, stage].
 * Stage 0: S = H P H^T + r I, K = P H^T S^-1 (cofactor inverse), x += K (z - H x), P -= K H P, x[0:3] = z, box = [det 0:7, v],
 * class / score / num_points from the detection, update_score = max(score, 0.03), hit = 1, miss = 0.  Stage 1 (second stage):
 * hit = 2, miss = 0, score and num_points only.  A table row may appear in one match only. */
int dz_track_update(const dz_track_table *t, int n, const int *det, int n_det, const int *match, int m, float r, void *stream);
/* Append m tracks at rows [n, n + m) from rows src_idx (device, each < n_src) of the row buffer `src`, with the
 * constructor's matrices (kalman_filter.py:10-58): P = diag(p0 x3, p1 x2), Q = diag(q0 x3, q1 x2), x = [box 0:3, 0, 0],
 * box = [box 0:7, 0, 0], hit = 1, miss = 0, update_score = score, id = ids[k], delta_t = dt. */
int dz_track_spawn(const dz_track_table *t, int n, const int *src, int n_src, const int *src_idx, const int *ids, int m, float p0,
                   float p1, float q0, float q1, float dt, void *stream);
/* TrackManager.overlap_track_merge (track_manager.py:262-310): bits (n, ceil(n/64)) 64-bit words, bit (i, j) = same class and
 * overlap_bev(i, j) / (dx_i * dy_i + 1e-9) >= thr[class i]; then the reference's greedy sweep in one workgroup (the lowest id of a
 * row's remaining set is kept, the rest of the set is removed, the set's columns are cleared).  removed (n) int32 0 / 1.
 * Workspace: dz_track_merge_workspace_bytes(n).  Every threshold must be > 0 (a cleared column then never passes), n <= 32768. */
size_t dz_track_merge_workspace_bytes(int n);
int dz_track_merge(const dz_track_table *t, int n, const float *h_thr, int n_cls, int *removed, void *ws, size_t ws_bytes, void *stream);
/* Stable removal: rows with removed[i] != 0 (removed may be NULL) or, when death_age != -1, miss >= death_age, are dropped; the
 * survivors are copied in order into `dst` (another table, never `src`).  *d_count (device) = the new count. */
int dz_track_compact(const dz_track_table *src, int n, const int *removed, int death_age, const dz_track_table *dst, int *d_count,
                     void *stream);
/* info() of rows [0, n) (kalman_filter.py:61-72) as rows [log_n, log_n + n) of the row buffer `log`, frame ordinal `frame`. */
int dz_track_log(const dz_track_table *t, int n, int frame, int *log, long log_n, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The AB3DMOT filter (kalman_filter/ab3dmot.py:9-149 over filterpy's KalmanFilter(dim_x=10, dim_z=7)) on the same table, float64.
 * dz_track_ab3d is the companion of a dz_track_table: the same rows, the filter's float64 state beside them.  Its arrays are laid
 * out with the TRACK INDEX FASTEST: element k of track i is at [k * stride + i] (a wave's accesses coalesce); `stride` is the
 * number of rows allocated.  The dz_track_table beside it carries box (the float32 rounding of the float64 box: what
 * dz_track_affinity and dz_track_merge read), cls, score, update_score, num_points (-1), hit, miss, id; its x / P / Q / dt are not used.
 *   state [x y z l w h theta vx vy vz]; F = I + ones at (0,7), (1,8), (2,9); H = the first seven states; R = I;
 *   P0 = diag(10 x7, 10000 x3); Q = diag(1 x7, 0.01 x3).  The config's P, Q, R and DELTA_T are not read, as in the reference.
 * Detections come as a row buffer (score, class, the float32 box) plus a row-major (rows, 7) float64 array of the measurements;
 * the log is a row buffer plus a row-major (rows, 9) float64 array of the boxes.  Word 15 of a log row: bit 0
 * (DZ_TRACK_AB3D_ROW_DROP) = the row fails the output rule of track_manager.py:202-205 and is not part of the results, bit 1
 * (DZ_TRACK_AB3D_ROW_BIRTH) = the row is the track's birth row (its box is the detection rounded to float32). */
#define DZ_TRACK_FILTER_KALMAN 0
#define DZ_TRACK_FILTER_AB3DMOT 1
#define DZ_TRACK_AB3D_WORK 170      /* update's working matrices per track: K (10,7) and (I - K H) P (10,10) */
#define DZ_TRACK_AB3D_ROW_DROP 1
#define DZ_TRACK_AB3D_ROW_BIRTH 2
typedef struct {
    double *x;           /* (10, stride)  */
    double *P;           /* (100, stride) row-major 10 x 10 per track */
    double *box;         /* (9, stride)   the box info() reports: x[0:9], or the birth row's float32 detection */
    double *work;        /* (DZ_TRACK_AB3D_WORK, stride) scratch of dz_track_ab3d_update; not carried by compact */
    int *hits;           /* (stride)      updates + 1 */
    int stride;
} dz_track_ab3d;
/* AB3DMOT.predict (ab3dmot.py:88-109) on rows [0, n): x = F x, P = F P F^T + Q as three row adds and three column adds, theta
 * wrapped once into [-pi, pi), miss += 1, hit = 0, box = x[0:9]. */
int dz_track_ab3d_predict(const dz_track_table *t, const dz_track_ab3d *a, int n, void *stream);
/* AB3DMOT.update (ab3dmot.py:111-149) for m matches, one thread each: match (m,3) int32 [table row, det row, stage]; the stage is
 * ignored (an update is always a full update, hit = 1).  hits += 1, miss = 0, score and class from the row; theta of state and
 * measurement wrapped, the obtuse-angle flip and the >= 3 pi / 2 branch; then y = z - H x, S = H P H^T + R (the leading 7 x 7 block
 * plus I, factored by Cholesky), K = P H^T S^-1, x += K y, P = (I - K H) P (I - K H)^T + K K^T; theta wrapped; box = x[0:9].
 * det64 (n_det, 7) float64 row-major: the measurements.  A table row may appear in one match only. */
int dz_track_ab3d_update(const dz_track_table *t, const dz_track_ab3d *a, int n, const int *det, const double *det64, int n_det,
                         const int *match, int m, void *stream);
/* Append m tracks at rows [n, n + m) (ab3dmot.py:13-86): x = [src64 row, 0, 0, 0], P = P0, hits = 1, hit = 1, miss = 0,
 * num_points = -1, score / class from the row, id = ids[k], box = the row's float32 box with two zero columns. */
int dz_track_ab3d_spawn(const dz_track_table *t, const dz_track_ab3d *a, int n, const int *src, const double *src64, int n_src,
                        const int *src_idx, const int *ids, int m, void *stream);
/* dz_track_compact that carries x, P, box and hits of the companion too (adst: another companion, never asrc). */
int dz_track_ab3d_compact(const dz_track_table *src, const dz_track_ab3d *asrc, int n, const int *removed, int death_age,
                          const dz_track_table *dst, const dz_track_ab3d *adst, int *d_count, void *stream);
/* dz_track_log plus the float64 boxes into rows [log_n, log_n + n) of log64 (rows, 9), and word 15: DZ_TRACK_AB3D_ROW_DROP unless
 * (hits >= birth_age or frame_id < birth_age) and miss < death_age (frame_id = the frame's key as an integer, `frame` its
 * ordinal), DZ_TRACK_AB3D_ROW_BIRTH on a birth row. */
int dz_track_ab3d_log(const dz_track_table *t, const dz_track_ab3d *a, int n, int frame, int frame_id, int birth_age, int death_age,
                      int *log, double *log64, long log_n, void *stream);

/* ---------------------------------------------------------------------------------------------
 * A pass of a sequence as one workgroup (csrc/track_seq.hip): grid = sequences; a workgroup walks its sequence's frames in order
 * and performs per frame what TrackManager.online_track_module (forward) / reverse_tracking_module (reverse = 1) perform through
 * the entry points above, with the assignment on the device (dz_lsa_batch's core): predict, the cost matrices, the index
 * bookkeeping of one_stage / two_stage / only_two_stage, update with the stage flag, spawn with ids counted from init_track_id
 * per sequence, overlap_track_merge + stable removal, the info() log rows, the DEATH_AGE removal.  The per-track and per-pair
 * arithmetic is the same code as the per-op kernels' (csrc/track_body.h).
 *
 * Detections: ONE row buffer `det` for all frames of all sequences; frame g (global index) holds rows [frame_row[g], frame_row[g+1]),
 * sequence s holds frames [seq_frame[s], seq_frame[s+1]) in time order.  det_flags per row: bit 0 = the detection passes the score
 * and point thresholds of the first stage, bit 1 = it has enough points (data_association.py:80-87; computed by the host from the
 * frame's own arrays, whatever their dtype).  one_stage reads no flag.
 * Storage per sequence s: rows [2 s track_cap, 2 (s+1) track_cap) of `tables` (a table and its spare), rows [s log_cap, (s+1) log_cap)
 * of `log` with log_count[s] rows written, one slice of ws (dz_track_seq_ws_bytes).  row_cap >= track_cap bounds the rows of an
 * assignment (reverse: live tracks + the forward rows that join), det_cap the detections of a frame.
 * overflow[s] (sticky, 0 = the pass is complete): DZ_TRACK_SEQ_OVF_TRACKS / _LOG = the capacity ran out (rerun with more),
 * _LSA = an assignment stopped with a status (NaN costs), _DESC = an offset list leaves its buffer or a frame / assignment exceeds
 * det_cap / row_cap.  Such a sequence stops at that frame; the others finish.
 * Reverse: ext = the forward pass's log (ext_cap rows per sequence, ext_count[s] valid); per global frame g the forward rows of
 * that frame in track order, split by the host: going_idx[going_at[g] .. going_at[g+1]) join the association as extra rows,
 * start_idx[start_at[g] .. start_at[g+1]) become reverse tracks after the frame (ids from the rows).  Indices are rows of the
 * sequence's ext slice; one outside it is never followed.
 * Limits: classes <= DZ_TRACK_MAX_CLASSES, track_cap <= DZ_TRACK_SEQ_MAX_TRACKS (the sweep's sets in LDS: 2 x 64 words),
 * det_cap <= DZ_TRACK_SEQ_MAX_DET, row_cap <= 2 x DZ_TRACK_SEQ_MAX_TRACKS (cost slice row_cap x det_cap x 4 <= 32 MiB per sequence);
 * beyond them, and where 32-bit offsets would overflow: DZ_ERR_UNSUPPORTED.  The workgroup keeps 45 KiB of LDS: rect_overlap's
 * scratch, the assignment's vectors up to 512 x 512 (larger ones in ws), the sweep's sets.
 * filter = DZ_TRACK_FILTER_AB3DMOT (forward pass only; reverse = 1 is DZ_ERR_UNSUPPORTED): predict / update / spawn / log / the two
 * removals are those of dz_track_ab3d_* (csrc/track_ab3dmot.h) on io->ab3d beside `tables`, with io->det64, io->frame_id and
 * io->log64; the log rows carry dz_track_ab3d_log's word 15. */
#define DZ_TRACK_SEQ_MAX_TRACKS 4096
#define DZ_TRACK_SEQ_MAX_DET 1024
#define DZ_TRACK_SEQ_OVF_TRACKS 1
#define DZ_TRACK_SEQ_OVF_LOG 2
#define DZ_TRACK_SEQ_OVF_LSA 4
#define DZ_TRACK_SEQ_OVF_DESC 8
typedef struct {
    int metric;              /* DZ_TRACK_AFF_IOU_BEV, DZ_BOXM_IOU3D, DZ_BOXM_GIOU3D */
    int distinguish_class;
    int gate_class;          /* as dz_track_predict */
    int n_cls;
    int two_stage;           /* forward: 0 = one_stage, 1 = two_stage; the reverse pass is only_two_stage */
    int merge_enable;
    int death_age;           /* -1 = off */
    int init_track_id;
    float thr_first[DZ_TRACK_MAX_CLASSES], thr_second[DZ_TRACK_MAX_CLASSES], thr_merge[DZ_TRACK_MAX_CLASSES];
    float p0, p1, q0, q1, r, dt;
    int filter;              /* DZ_TRACK_FILTER_KALMAN (0), DZ_TRACK_FILTER_AB3DMOT: the bodies of dz_track_ab3d_*; forward pass only */
    int birth_age;           /* AB3DMOT: the output rule of dz_track_ab3d_log */
} dz_track_seq_params;
typedef struct {
    const int *det;          /* (n_det_rows, DZ_TRACK_ROW_WORDS) */
    const int *det_flags;    /* (n_det_rows) */
    const int *frame_row;    /* (n_frames + 1) */
    const int *seq_frame;    /* (n_seq + 1) */
    int n_seq, n_frames, n_det_rows;
    int track_cap, row_cap, det_cap, log_cap;
    /* reverse pass only */
    const int *ext;          /* (n_seq, ext_cap, DZ_TRACK_ROW_WORDS) */
    const int *ext_count;    /* (n_seq) */
    const int *going_at;     /* (n_frames + 1) */
    const int *going_idx;    /* (n_going) */
    const int *start_at;     /* (n_frames + 1) */
    const int *start_idx;    /* (n_start) */
    int ext_cap, n_going, n_start;
    /* AB3DMOT only */
    const double *det64;     /* (n_det_rows, 7) the measurements of `det`'s rows */
    const int *frame_id;     /* (n_frames) every frame's key as an integer */
    double *log64;           /* (n_seq, log_cap, 9) the float64 boxes of `log`'s rows */
    dz_track_ab3d ab3d;      /* companion of `tables`: stride >= 2 x track_cap x n_seq, sequence s at the same rows */
} dz_track_seq_io;
size_t dz_track_seq_ws_bytes(int n_seq, int track_cap, int row_cap, int det_cap);
int dz_track_seq_pass(const dz_track_seq_params *p, const dz_track_seq_io *io, int reverse, const dz_track_table *tables, int *log,
                      int *log_count, int *overflow, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Trajectory-pair table of one sequence (csrc/traj_pair.hip): the sums and counts that assign_track_target
 * (tracking/.../tracking_modules/target_assign.py:44-75) and TrackRecall.eval_single_seq (utils/track_recall.py:187-203 through
 * track_calculation.py:84-123) both take per (ground-truth trajectory, track) pair over the frames the two share.
 * Side a = ground-truth trajectories, side b = tracks.
 *   a_box (a_rows,7) f32, a_cls (a_rows) i32 class codes in [0, n_cls).
 *   a_slot (n_frames, n_a) i32, FRAME-MAJOR: a_slot[f * n_a + i] = row of trajectory i at frame ordinal f, or -1 when it has no
 *   box there.  The same for b.  A slot outside [-1, rows) is never followed (the frame counts as absent).
 *   For every (i, j), walking f = 0 .. n_frames-1 ASCENDING, at frames where both slots are >= 0:
 *     v = metric(a row, b row); distinguish_class && classes differ -> v = 0
 *     n_same += 1; sum_all += v            (fp32, one plain add per frame, in frame order: no atomics, the same bytes on every run)
 *     v >= thr[class of the a row] -> n_hit += 1; sum_hit += v
 *   out: sum_all, sum_hit f32 (n_a, n_b); n_hit, n_same i32 (n_a, n_b).
 * metric: DZ_TRACK_AFF_IOU_BEV (v = element of dz_boxes_iou_bev bit for bit) or DZ_BOXM_IOU3D (of dz_boxes_pairwise_metric).
 * h_thr: host array of n_cls (1..DZ_TRACK_MAX_CLASSES) thresholds, every one > 0.  n_a or n_b == 0: no launch, DZ_OK.
 * DZ_ERR_INVALID: another metric, a threshold <= 0, a negative size, n_frames * n_a, n_frames * n_b, rows * 7 or n_a * n_b >= 2^31. */
int dz_traj_pair_table(const float *a_box, const int *a_cls, const int *a_slot, int n_a, int a_rows, const float *b_box,
                       const int *b_cls, const int *b_slot, int n_b, int b_rows, int n_frames, int metric, int distinguish_class,
                       const float *h_thr, int n_cls, float *sum_all, float *sum_hit, int *n_hit, int *n_same, void *stream);
/* Per-frame rows of listed pairs: pairs (n_pairs,2) i32 on the device, [i, j]; rows (n_pairs, n_frames) f32 = the masked v above at
 * the frames the pair shares, 0 elsewhere and for a pair outside the table (the iou_mat_dict[frame][gt, track] the reference reads
 * at target_assign.py:104-111).  n_pairs or n_frames == 0: no launch.  DZ_ERR_INVALID as above and for n_pairs * n_frames >= 2^31. */
int dz_traj_pair_rows(const float *a_box, const int *a_cls, const int *a_slot, int n_a, int a_rows, const float *b_box,
                      const int *b_cls, const int *b_slot, int n_b, int b_rows, int n_frames, int metric, int distinguish_class,
                      const int *pairs, int n_pairs, float *rows, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Linear sum assignment on the device (csrc/lsa.h, csrc/lsa.hip): GNN_assignment (tracking/.../data_association/distance.py:9-41)
 * for a batch of independent problems in one launch, one workgroup per problem.  The solver is the shortest-augmenting-path
 * algorithm of scipy.optimize.linear_sum_assignment: duals and path lengths in double, the fp32 costs widened to double, the
 * problem transposed when rows > cols.  A cost >= threshold counts as 5000; after the assignment a pair whose cost is not
 * < threshold is dropped.  Where the optimum is not unique, which optimal assignment comes out is not scipy's choice by contract.
 *
 *   cost (cost_len) f32: the problems' row-major matrices, anywhere in the buffer.
 *   desc (n_problems, DZ_LSA_DESC_WORDS) int64 on the device, per problem:
 *     [0] rows  [1] cols  [2] offset of its matrix in cost (elements)  [3] offset of its rows in row_to_col / unmatched_rows
 *     [4] offset of its columns in unmatched_cols  [5] byte offset of its slice in ws, a multiple of 16 (read only when
 *     max(rows, cols) > 1024: smaller problems keep their vectors in LDS and dz_lsa_ws_bytes is 0 for them)
 *   row_to_col (rows_len) i32: matched column of each row, -1 = unmatched.
 *   unmatched_rows (rows_len), unmatched_cols (cols_len) i32: ascending lists at the problem's offsets.
 *   counts (n_problems, 4) i32: matched pairs, unmatched rows, unmatched columns, status.
 * Status 0 = solved.  1 = no finite cost left (NaN costs), 2 = a loop bound was reached (at most min(rows, cols) augmentations of at
 * most max(rows, cols) column scans each: every loop of the kernel is bounded by the problem size), 3 = the descriptor leaves a
 * buffer or a limit; such a problem writes its counts only (1, 2: all rows and columns unmatched) and the others finish.
 * A 0 x k or k x 0 problem gives no matches and the full lists.
 * Workspace: ws holds the slices of the problems with a side > 1024, each of dz_lsa_ws_bytes(rows, cols) bytes at the offset its
 * descriptor names (back to back: the sum over the problems).  The kernel checks every slice against ws_bytes; a problem whose
 * slice does not fit gets status 3 and the others finish.  The host checks nothing about ws beyond a null pointer with
 * ws_bytes > 0: the offsets are on the device.
 * Limits: each side <= DZ_LSA_MAX_DIM (max_rows / max_cols, the largest sides of the batch, which may come from different
 * problems; beyond it: DZ_ERR_UNSUPPORTED, as are 2^40 costs or 2^31 rows / columns in one call).  DZ_ERR_INVALID for negative
 * sizes and null pointers.  n_problems == 0: no launch.
 * DZ_LSA_MAX_DIM bounds the time one workgroup can hold a compute unit: a problem makes at most min(rows, cols) x max(rows, cols)
 * column scans, each max(rows, cols) / 256 columns per thread and two barriers, a few microseconds at 4096 columns.  4096 x 4096 is
 * 1.7e7 scans at the bound, of the order of a minute (an estimate); a side of 32768 would be hours.  Measured on one MI355X, one
 * problem per call, host time with the counts read: random 4096 x 4096 matrices 2.2 s (5 % of the costs below the threshold) and
 * 2.8 s (dense, uniform), dense 2048 x 2048 0.37 s. */
#define DZ_LSA_DESC_WORDS 6
#define DZ_LSA_MAX_DIM 4096
size_t dz_lsa_ws_bytes(int rows, int cols);
int dz_lsa_batch(const float *cost, long long cost_len, const long long *desc, int n_problems, int max_rows, int max_cols, double threshold,
                 int *row_to_col, int *unmatched_rows, long long rows_len, int *unmatched_cols, long long cols_len, int *counts, void *ws,
                 size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Waymo-style detection matching on the device (csrc/eval_match.hip): the count table behind AP / APH at every score cutoff, one
 * workgroup per problem.  This is the project's own statement of the protocol; it is not pinned to the official tool.
 *
 * A problem is one (frame, shard): P predictions in descending score order and G ground truths of one object type.
 *   Cutoffs: c_k = (float)(k * 0.01) for k = 0..99, c_100 = 1; a prediction is in cutoff k when score >= c_k; n_k of them are.
 *   Weight: w(p, g) = IoU(p, g) when IoU >= iou_thr[type], else 0.  box_type DZ_EVAL_BOX_3D: the value of dz_boxes_metric's
 *   DZ_BOXM_IOU3D; DZ_EVAL_BOX_BEV: the rotated BEV IoU of the same code.
 *   Matching M_k: a maximum-total-weight matching between the first n_k predictions and all ground truths (cost 1 - w for a pair,
 *   1 for "unmatched", every prediction assigned), pairs with w == 0 then discarded.  The rows enter the shortest-augmenting-path
 *   solver of csrc/lsa.h in score order; after row n - 1 its state is an optimal assignment of rows 0..n-1, so ONE solve passes
 *   through M_k of every cutoff.
 *   Counts per (shard, level L in {1, 2}, k), summed over the problems of the shard:
 *     TP = pairs of M_k whose ground truth has difficulty <= L;  FP = n_k - |M_k|;  FN = #{g: difficulty <= L} - TP;
 *     HA = sum over the TP pairs of 1 - |d| / pi, d = the heading difference wrapped to [-pi, pi], in fixed point with 32
 *     fraction bits, each term rounded to nearest.
 *
 *   pred_box (n_pred, 7) f32, pred_score (n_pred) f32, gt_box (n_gt, 7) f32, gt_difficulty (n_gt) i32.
 *   desc (n_problems, DZ_EVAL_DESC_WORDS) int64 on the device, per problem:
 *     [0] first prediction  [1] P  [2] first ground truth  [3] G  [4] shard  [5] object type, 0..4 (indexes iou_thr)
 *     [6] byte offset of its slice in ws, a multiple of 16; the slice has dz_eval_match_ws_bytes(P, G) bytes
 *   iou_thr: 5 floats on the host.
 *   table (n_shards, 2, 101, 4) int64 [TP, FP, FN, HA]: ADDED to (the caller zeroes it); all terms are integers, so the table is
 *   bit-identical whatever order the workgroups finish in.
 *   scheme DZ_EVAL_ACC_ATOMIC: 64-bit integer atomics on the table.  DZ_EVAL_ACC_SLOTS: each problem fills its own
 *   (2, 101, 4) slot of `slots` (n_problems * 808 int64, zeroed by the call) and a second kernel adds the slots of a shard in
 *   problem order.  slots may be NULL for DZ_EVAL_ACC_ATOMIC.
 *   status (1) i32: OR of DZ_EVAL_ST_DESC (a descriptor leaves its buffers or a limit: that problem contributes nothing, the
 *   others finish) and DZ_EVAL_ST_SOLVER (a solve stopped at a loop bound: its cutoffs from there on are missing).
 * Limits: P + G <= DZ_LSA_MAX_DIM (max_dim = the largest P + G of the batch; beyond it DZ_ERR_UNSUPPORTED), n_pred, n_gt < 2^31 / 7.
 * Every kernel loop is bounded by the problem size or by 101. */
#define DZ_EVAL_DESC_WORDS 7
#define DZ_EVAL_CUTOFFS 101
#define DZ_EVAL_BOX_3D 0
#define DZ_EVAL_BOX_BEV 1
#define DZ_EVAL_ACC_ATOMIC 0
#define DZ_EVAL_ACC_SLOTS 1
#define DZ_EVAL_ST_DESC 1
#define DZ_EVAL_ST_SOLVER 2
size_t dz_eval_match_ws_bytes(int n_pred, int n_gt);
int dz_eval_match_counts(const float *pred_box, const float *pred_score, long long n_pred, const float *gt_box, const int *gt_difficulty,
                         long long n_gt, const long long *desc, int n_problems, int max_dim, int n_shards, int box_type, const float *iou_thr,
                         int scheme, long long *table, long long *slots, int *status, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Waymo-style tracking metrics on the device (csrc/mot_chain.hip): the count table behind MOTA / MOTP at every score cutoff.  This is
 * the project's own statement of the protocol; it is not pinned to the official tool.
 *
 * A prediction is (sequence, frame, object id, box7, type, score), a ground truth (sequence, frame, object id, box7, type,
 * difficulty in {1, 2}).  Types, cutoffs c_k, iou_thr, the weight w(p, g), the box types and the shards are those of
 * dz_eval_match_counts above.  An object id is unique within a frame and side; the host maps ids to dense indices per (sequence, side)
 * and walks the frames of a sequence in ascending frame id.  A problem is one (sequence, frame, shard).
 *   Chain (sequence, shard, cutoff k): its state `last` is a partial bijection between ground-truth ids and prediction ids, empty at
 *   the sequence's first frame and never reset.  Per frame, with P_t the problem's predictions of score >= c_k and G_t its ground truths:
 *     1. carry: for every g in G_t with q = last[g.id] defined, a p in P_t of id q and w(p, g) > 0: the pair (p, g) is kept and both
 *        leave the pools;
 *     2. match: a maximum-total-weight matching of the remaining predictions and ground truths (cost 1 - w, "unmatched" costs 1,
 *        zero-weight pairs discarded), the predictions entering csrc/lsa.h's solver as rows in input order (descending score);
 *     3. update: every new pair (p, g) of step 2 whose last[g.id] is defined and differs from p.id is one mismatch on g, judged on
 *        `last` as the frame found it; then whatever g.id and p.id were paired with is unpaired (through the prediction's side this
 *        is no mismatch) and last[g.id] = p.id.
 *   Counts per (shard, level L in {1, 2}, k), summed over frames and sequences, M = the kept and the new pairs:
 *     TP = #{(p, g) in M: difficulty(g) <= L};  FP = |P_t| - |M|;  MISS = #{g: difficulty <= L} - TP;  MISMATCH = the mismatches on
 *     ground truths of difficulty <= L;  COST = sum over the TP pairs of 1 - w in fixed point with 32 fraction bits, each term
 *     evaluated in double and rounded to nearest.  One chain serves both levels.
 *   Cutoffs that hold the same predictions in every frame of a (sequence, shard) are one chain: with `merge` the kernel runs the
 *   cutoffs some prediction reaches exactly (and the last one) and adds each result to every cutoff down to the next such value.
 *
 * dz_mot_weights: w of every pair of every problem, once for all cutoffs, and each prediction's highest cutoff.
 *   pred_box (n_pred, 7) f32, pred_score (n_pred) f32, gt_box (n_gt, 7) f32, grouped by problem, predictions in descending score.
 *   pdesc (n_problems, DZ_MOT_PDESC_WORDS) int64 on the device, per problem:
 *     [0] first prediction  [1] P  [2] first ground truth  [3] G  [4] object type, 0..4 (indexes iou_thr)
 *     [5] offset of its (P, G) row-major weights in `weights`, in floats
 *   weights (w_len) f32 out, cut (n_pred) i32 out: the highest k with score >= c_k, -1 = none.
 *   status (1) i32: DZ_EVAL_ST_DESC is ORed in when a descriptor leaves its buffers (that problem writes nothing, the others finish).
 * dz_mot_chain_counts: the chains.
 *   pred_id (n_pred) i32 / gt_id (n_gt) i32: dense ids per (sequence, side); gt_difficulty (n_gt) i32.
 *   cdesc (n_chains, DZ_MOT_CDESC_WORDS) int64 on the device, per (sequence, shard):
 *     [0] first entry in `frames`  [1] number of frames  [2] shard  [3] prediction ids of the sequence  [4] ground-truth ids
 *     [5] the largest P + G of its frames  [6] byte offset of its slice in ws, a multiple of 16, dz_mot_chain_ws_bytes([3], [4], [5]) long
 *   frames (n_frames) int64: problem indices, the frames of a chain in walking order (frames without a member are left out).
 *   mapping DZ_MOT_MAP_WAVE: one wavefront per chain; DZ_MOT_MAP_WORKGROUP: 256 threads per chain.  Both give the same bits.
 *   table (n_shards, 2, 101, DZ_MOT_COUNTS) int64 [TP, FP, MISS, MISMATCH, COST * 2^32]: ADDED to with 64-bit integer atomics, zero
 *   terms skipped, so it is bit-identical whatever order the chains finish in.
 *   status (1) i32: OR of DZ_EVAL_ST_DESC (a descriptor or id leaves its buffers or a limit: every descriptor and id of a chain is
 *   checked before anything is followed, such a chain adds nothing and the others finish) and DZ_EVAL_ST_SOLVER (a solve stopped at a
 *   loop bound: the chain adds nothing).
 *   The slice holds, per cutoff, `last` in both directions and the id -> row table of the current frame; when [5] is above
 *   DZ_MOT_LDS_DIM also the per-frame lists and the solver's vectors, which otherwise live in LDS.
 * Limits: per frame P + G <= DZ_LSA_MAX_DIM (max_dim = the largest of the call; beyond it DZ_ERR_UNSUPPORTED, as are 2^31 predictions,
 * ground truths or frame-list entries in one call).  Every kernel loop is
 * bounded by a frame count, a problem size or 101. */
#define DZ_MOT_PDESC_WORDS 6
#define DZ_MOT_CDESC_WORDS 7
#define DZ_MOT_COUNTS 5
#define DZ_MOT_LDS_DIM 192
#define DZ_MOT_MAP_WAVE 0
#define DZ_MOT_MAP_WORKGROUP 1
size_t dz_mot_chain_ws_bytes(long long n_pred_ids, long long n_gt_ids, int max_dim);
int dz_mot_weights(const float *pred_box, const float *pred_score, long long n_pred, const float *gt_box, long long n_gt, const long long *pdesc,
                   int n_problems, int max_dim, int box_type, const float *iou_thr, float *weights, long long w_len, int *cut, int *status,
                   void *stream);
int dz_mot_chain_counts(const float *weights, long long w_len, const int *cut, const int *pred_id, long long n_pred, const int *gt_id,
                        const int *gt_difficulty, long long n_gt, const long long *pdesc, int n_problems, const long long *cdesc, int n_chains,
                        const long long *frames, long long n_frames, int max_dim, int n_shards, int mapping, int merge, long long *table,
                        int *status, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * CenterHead targets and losses on the device (csrc/head_loss.hip).  Reference: center_head.py:107-313,
 * utils/loss_utils.py:143-243, utils/centernet_utils.py:11-71.  One call serves ONE head; every buffer is the caller's.
 *
 * dz_centerhead_targets: heat map, regression targets, cell indices and masks of one head from the batch's ground truth.
 *   gt_boxes (B, M, 8) f32 [x, y, z, dx, dy, dz, heading, class]: class is the 1-based global class, 0 = padding row.
 *     gt_cols != 8 (a `vel` head): DZ_ERR_UNSUPPORTED.
 *   cls_table (n_classes) i32 on the HOST: cls_table[g - 1] = the head's 1-based class of global class g, 0 = not this head.
 *   feat_w x feat_h: the map (x by y); stride = FEATURE_MAP_STRIDE; range_xy = POINT_CLOUD_RANGE[0:2]; voxel_xy = VOXEL_SIZE[0:2].
 *   heatmap (B, ncls, H, W) f32, target_boxes (B, nmax, 8) f32, inds (B, nmax) i64, masks (B, nmax) i64: all four are cleared by the call.
 *   rec (2) i32: [num_pos = cells of the heat map equal to 1.0 over the whole batch, num = sum of masks]; cleared by the call.
 *   Slot k of a frame is the k-th box of this head in gt_boxes order; slots at or beyond min(nmax, count) do not exist; a box with
 *   dx <= 0 or dy <= 0 leaves its slot zero (mask 0) and the slots behind it stay where they are.  Coordinates, the clamp to
 *   [0, size - 0.5], the truncation and gaussian_radius are float32 with every operation rounded on its own; the Gaussian is evaluated
 *   in float64 (sigma = (2r + 1) / 6, values below eps * max cut), rounded to float32 once, clipped to the map and max-accumulated by
 *   integer atomicMax on the bit pattern (exact, order independent).  target_boxes = [cx - int(cx), cy - int(cy), z, log dx, log dy,
 *   log dz, cos, sin]; log / cos / sin are evaluated in float64 and rounded once.
 *   Limits: 1 <= ncls <= 3, 1 <= nmax <= DZ_HEAD_LOSS_MAX_OBJS, 1 <= n_classes <= DZ_HEAD_LOSS_MAX_CLASSES, B * ncls * H * W < 2^31.
 *
 * dz_centerhead_loss: the head's losses and, optionally, their gradient with respect to the head map.
 *   head (B, H*W, 12) f32 channel-last: center 0:2, center_z 2, dim 3:6, rot 6:8, iou 8, hm 9:9+ncls.  Columns 9+ncls..11 are never read.
 *   heatmap / target_boxes / inds / masks / rec: as dz_centerhead_targets writes them (targets of any origin with that layout will do;
 *     a slot whose index is outside [0, H*W) counts as masked out).  rec may be NULL: the call then counts num_pos and num itself.
 *   hm_mask (B, H, W) f32 or NULL: the optional mask of neg_loss_cornernet; with it num_pos is the masked count, summed by the call.
 *   weights (11) doubles on the HOST: [cls_weight, loc_weight, code_weights[8], iou_weight].
 *   out_rec (DZ_HEAD_LOSS_REC) doubles on the device: [0] hm_loss * cls_weight, [1..8] the regression components * code_weights,
 *     [9] loc_loss = loc_weight * sum of [1..8], [10] iou_loss (unweighted; 0 when iou_weight <= 0), [11] total = [0] + [9] +
 *     iou_weight * [10].
 *   grad_head (B, H*W, 12) f32 or NULL: d total / d head, every column written (unwritten head columns get 0).
 *   Focal term: neg_loss_cornernet on p = clamp(sigmoid(x), 1e-4, 1 - 1e-4) (float32 bounds), positives where the target is 1,
 *   negatives weighted (1 - g)^4, divided by num_pos, or -neg undivided when num_pos == 0; the gradient is 0 where the clamp is active.
 *   Regression term: L1 of (pred - target) at inds over the masked slots per component / max(num, 1); gradient sign(.), sign(0) = 0,
 *   slots that share a cell add up.  IoU term (iou_weight > 0): _iou_target - boxes decoded from the prediction at inds and from the
 *   targets, heading atan2(column 6, column 7) on both sides, the paired DZ_BOXM_IOU3D value - L1 against column 8 / max(num, 1).
 *   Every sum is formed in float64 in a fixed order (per-workgroup partials, then a fixed-order pass): two calls give the same bytes.
 *   ws: dz_centerhead_loss_ws_bytes(B, feat_h, feat_w) bytes.  Limits as above.  Nothing is launched when an argument is refused. */
#define DZ_HEAD_LOSS_MAX_OBJS 1024
#define DZ_HEAD_LOSS_MAX_CLASSES 32
#define DZ_HEAD_LOSS_REC 12
int dz_centerhead_targets(const float *gt_boxes, int batch, int max_boxes, int gt_cols, const int *cls_table, int n_classes, int ncls,
                          int feat_h, int feat_w, double stride, const double *range_xy, const double *voxel_xy, int nmax,
                          double gaussian_overlap, int min_radius, float *heatmap, float *target_boxes, long long *inds, long long *masks,
                          int *rec, void *stream);
size_t dz_centerhead_loss_ws_bytes(int batch, int feat_h, int feat_w);
int dz_centerhead_loss(const float *head, const float *heatmap, const float *target_boxes, const long long *inds, const long long *masks,
                       const int *rec, const float *hm_mask, int batch, int feat_h, int feat_w, int ncls, int nmax, const double *weights,
                       double stride, const double *range_xy, const double *voxel_xy, double *out_rec, float *grad_head, void *ws,
                       size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * CenterHead: backward through the head's 3 x 3 convolutions (csrc/head_backward.hip).  The reference leaves this to
 * torch autograd.  One layer is y = relu(scale_c * conv(x, w)_c + shift_c); with g = g_y * [y > 0] the raw weight gradient is
 *   Graw[tap][ci][c] = sum over (b, y, x) of x_img[b, y + ky, x + kx, ci] * g[b, y, x, c],   tap = ky * 3 + kx,
 * x_img the zero-bordered channel-last input, and S_c = sum g_c; the parameter gradients are formed from those two by the caller.
 * The data gradient is dz_conv2d_forward on the g image with flipped, transposed weights: there is no kernel for it here.
 * No floating-point atomics: every sum has a fixed order, two calls give the same bytes whatever the workspace held before.
 * Every entry refuses, before any launch, null pointers and non-positive sizes (DZ_ERR_INVALID), a workspace that is too small
 * (DZ_ERR_WORKSPACE), and shapes outside its limits or an image of 2 GiB or more (DZ_ERR_UNSUPPORTED).
 *
 * dz_conv3x3_wgrad: Graw of one layer by fp32 MFMA (32x32x2), split over pixel chunks, the chunks' partials added in chunk order.
 *   x_img (B, h + 2, w + 2, groups * cin) f32 with its border (read as it is); group q reads channels [q * cin, (q + 1) * cin).
 *   groups == 1: g_img has `cout` channels (cout % 16 == 0); out (9, cin, cout) f32.  g_cout / g_ooff may be NULL (n_g 0).
 *   groups in 2..8: g_img has `cout` channels in all (the head map's 12), group q reads columns [g_ooff[q], g_ooff[q] + g_cout[q]),
 *     1 <= g_cout[q] <= 16, inside [0, cout); out (groups, 9, cin, 16) f32, the pad columns written as 0.  g_cout / g_ooff: n_g
 *     entries on the HOST, n_g == groups.  Columns outside the groups' ranges are never read.
 *   g_border 1: g_img is (B, h + 2, w + 2, cout), its interior read (as dz_relu_grad writes it); 0: dense (B, h, w, cout).
 *   Limits: cin % 16 == 0, 16 <= cin <= 512, cout <= 512, x_img and g_img 16-byte aligned (groups == 1).
 *   A workgroup takes DZ_WGRAD_CHUNK_ROWS rows of a band of DZ_WGRAD_TILE_W pixel columns of one frame (DZ_WGRAD_CHUNK_PIXELS pixels).
 *   ws: dz_conv3x3_wgrad_ws_bytes(batch, h, w, cin, cout, groups) bytes (0 for a shape that is refused).
 *
 * dz_relu_grad: g = g_y where y > 0, else 0 (a select: NaN in y or in a masked g_y does not leak), written into the interior of the
 *   zero-bordered g_img (B, h + 2, w + 2, c) - the border is never written - and sums[c] = S_c in float64 (per-workgroup partials,
 *   then one pass in index order).  y_img (B, h + 2, w + 2, c): the stored activation.  g_y: dense (B, h, w, c) (gy_border 0) or the
 *   interior of a bordered image (gy_border 1; g_img may then be g_y itself).  c % 4 == 0, 4 <= c <= 512.
 *   ws: dz_relu_grad_ws_bytes(batch, h, w, c) bytes.
 *
 * dz_head_final_backward: the grouped output layer (groups hidden slices of c channels -> the head map's 12 columns; no BatchNorm,
 *   no ReLU) of one SeparateHead, both halves.
 *   grad_head (B, h * w, 12) f32: d loss / d head map; columns outside the groups' ranges are never read.
 *   w2 (groups, 9, c, 16) f32: the layer's weights (CenterHead.plan()['heads'][i]['final']['w']).
 *   hidden (B, h + 2, w + 2, groups * c) f32 zero-bordered: the stored activation of the hidden layer (its ReLU mask).
 *   g_hidden (B, h + 2, w + 2, groups * c): interior written with
 *     [hidden > 0] * sum over taps and the group's columns of grad_head[b, y - ky + 1, x - kx + 1, g_ooff + o] * w2[q, tap, ch, o];
 *   sums_hidden (groups * c) f64 = its channel sums; d_w2 (groups, 9, c, 16) f32 = Graw of the layer (dz_conv3x3_wgrad, grouped);
 *   d_bias (groups, 16) f64 = the column sums of grad_head, 0 in the pad columns.
 *   groups in 2..8, c % 16 == 0, 16 <= c <= 128 (and groups * c * 27 * 4 bytes of weights inside 64 KiB of LDS), 1 <= g_cout <= 3.  ws: dz_head_final_backward_ws_bytes(batch, h, w, c, groups). */
#define DZ_WGRAD_TILE_W 32
#define DZ_WGRAD_CHUNK_ROWS 16
#define DZ_WGRAD_CHUNK_PIXELS (DZ_WGRAD_TILE_W * DZ_WGRAD_CHUNK_ROWS)
size_t dz_conv3x3_wgrad_ws_bytes(int batch, int h, int w, int cin, int cout, int groups);
int dz_conv3x3_wgrad(const float *x_img, const float *g_img, int g_border, int batch, int h, int w, int cin, int cout, int groups,
                     const int *g_cout, const int *g_ooff, int n_g, float *out, void *ws, size_t ws_bytes, void *stream);
size_t dz_relu_grad_ws_bytes(int batch, int h, int w, int c);
int dz_relu_grad(const float *g_y, int gy_border, const float *y_img, int batch, int h, int w, int c, float *g_img, double *sums, void *ws,
                 size_t ws_bytes, void *stream);
size_t dz_head_final_backward_ws_bytes(int batch, int h, int w, int c, int groups);
int dz_head_final_backward(const float *grad_head, const float *w2, const float *hidden, int batch, int h, int w, int c, int groups,
                           const int *g_cout, const int *g_ooff, int n_g, float *g_hidden, double *sums_hidden, float *d_w2,
                           double *d_bias, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DETZERO_HIP_H */
