"""Tensor-level wrappers over the C ABI (one Python function per entry point).

Everything here is plumbing: allocate outputs/workspaces as torch tensors on the current device,
pass raw pointers + the current HIP stream to libdetzero_hip, raise on a non-zero status.
Functions whose result size is only known on the device come in two flavours: the plain one
returns tensors sliced to the exact size (one host sync, reference-compatible), ``*_nosync``
returns capacity-sized tensors plus the device count (graph-capturable).
"""
import ctypes
import os
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

from . import lib as L


def _dev():
    return torch.device('cuda', torch.cuda.current_device())


def _ws(nbytes):
    return torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device=_dev())


def grid_size_of(pc_range, voxel_size):
    """round((hi-lo)/voxel) as in data_processor.py:63-65 (float32 range, float64 voxel size)."""
    r = np.asarray(pc_range, dtype=np.float32)
    return np.round((r[3:6] - r[0:3]) / np.array(voxel_size)).astype(np.int64)


# ------------------------------------------------------------------------------------------------
# voxelization
# ------------------------------------------------------------------------------------------------
def voxelize_hard_nosync(points, pc_range, voxel_size, max_points, max_voxels, xy_range_mask=False):
    """points (N,C) f32 cuda -> voxels (max_voxels,max_points,C), coords_zyx (max_voxels,3) i32,
    num_points (max_voxels) i32, d_num (1,) i32 device count."""
    lib = L.load()
    L.require_cuda(points)
    n, c = points.shape
    grid = grid_size_of(pc_range, voxel_size)
    cap = int(min(max_voxels, max(n, 1)))
    voxels = torch.empty((cap, max_points, c), dtype=torch.float32, device=points.device)
    coords = torch.empty((cap, 3), dtype=torch.int32, device=points.device)
    nump = torch.empty((cap,), dtype=torch.int32, device=points.device)
    d_num = torch.zeros((1,), dtype=torch.int32, device=points.device)
    wsb = lib.dz_voxelize_hard_workspace_bytes(n, int(grid[0]), int(grid[1]), int(grid[2]), max_points)
    ws = _ws(wsb)
    rc = lib.dz_voxelize_hard(L.ptr(points), n, c, L.f6(pc_range), L.f3(voxel_size), L.i3(grid),
                              1 if xy_range_mask else 0, max_points, cap, L.ptr(voxels), L.ptr(coords), L.ptr(nump), L.ptr(d_num), L.ptr(ws),
                              ws.numel(), L.stream())
    L.check(rc, 'dz_voxelize_hard')
    return voxels, coords, nump, d_num


def voxelize_hard_mean_into(points, pc_range, voxel_size, max_points, max_voxels, batch_index, feats, coords, d_num,
                            xy_range_mask=False):
    """Fused hard voxelizer + MeanVFE writing into caller-owned slices: feats (cap, C') f32, coords (cap,4) i32
    [b,z,y,x] (pre-filled with -1 by the caller), d_num (1,) i32.  cap = feats.shape[0]."""
    lib = L.load()
    L.require_cuda(points, feats, coords, d_num)
    n, c = points.shape
    grid = grid_size_of(pc_range, voxel_size)
    cap = feats.shape[0]
    ws = _ws(lib.dz_voxelize_hard_workspace_bytes(n, int(grid[0]), int(grid[1]), int(grid[2]), max_points))
    rc = lib.dz_voxelize_hard_mean(L.ptr(points), n, c, L.f6(pc_range), L.f3(voxel_size), L.i3(grid), 1 if xy_range_mask else 0,
                                   max_points, int(min(max_voxels, cap)), int(batch_index), L.ptr(feats), feats.shape[1],
                                   L.ptr(coords), L.ptr(d_num), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, 'dz_voxelize_hard_mean')


def voxelize_hard_mean_batched(points, batch, pc_range, voxel_size, max_points, max_voxels, cap_per_frame, xy_range_mask=False):
    """points (batch*n, C): `batch` equally long frames back to back -> feats (batch*cap, C), coords (batch*cap,4) i32
    [b,z,y,x] with b = -1 on unused rows, d_num (batch,) i32 - one launch chain for the whole batch."""
    lib = L.load()
    L.require_cuda(points)
    n_tot, c = points.shape
    n_per = n_tot // batch
    assert n_per * batch == n_tot
    grid = grid_size_of(pc_range, voxel_size)
    dev = points.device
    feats = torch.empty((batch * cap_per_frame, c), dtype=torch.float32, device=dev)
    coords = torch.full((batch * cap_per_frame, 4), -1, dtype=torch.int32, device=dev)
    d_num = torch.zeros((batch,), dtype=torch.int32, device=dev)
    ws = _ws(lib.dz_voxelize_hard_batched_workspace_bytes(n_per, batch, int(grid[0]), int(grid[1]), int(grid[2]), max_points))
    rc = lib.dz_voxelize_hard_mean_batched(L.ptr(points), n_per, batch, c, L.f6(pc_range), L.f3(voxel_size), L.i3(grid),
                                           1 if xy_range_mask else 0, max_points, int(max_voxels), L.ptr(feats), c, L.ptr(coords),
                                           int(cap_per_frame), L.ptr(d_num), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, 'dz_voxelize_hard_mean_batched')
    return feats, coords, d_num


def voxelize_to_level(points, batch, pc_range, voxel_size, max_points, max_voxels, level_shape, c_dst, math=0, xy_range_mask=False,
                      layout=0):
    """points (batch*n, C), equally long frames back to back, n <= max_voxels -> (SparseLevel of the frames' voxels, level-1
    feature rows (cap, c_dst) fp32 or pair16): hard voxelizer + MeanVFE + sparse-tensor construction in one launch chain."""
    lib = L.load()
    L.require_cuda(points)
    n_tot, c = points.shape
    n_per = n_tot // batch
    assert n_per * batch == n_tot
    grid = grid_size_of(pc_range, voxel_size)
    assert [int(level_shape[1]), int(level_shape[2])] == [int(grid[1]), int(grid[0])], (level_shape, grid)
    cap = batch * max(min(int(max_voxels), n_per), 1)
    lvl = SparseLevel(batch, level_shape, cap, points.device, layout=layout, zero_count=False)
    feats = torch.empty((cap, c_dst), dtype=torch.float32, device=points.device)
    ws = _ws(lib.dz_voxelize_to_level_workspace_bytes(n_per, batch, max_points, cap, *lvl.shape, lvl.layout))
    rc = lib.dz_voxelize_to_level(L.ptr(points), n_per, batch, c, L.f6(pc_range), L.f3(voxel_size), L.i3(grid),
                                  1 if xy_range_mask else 0, max_points, int(max_voxels), lvl.shape[0], lvl.layout, L.ptr(lvl.bitmap),
                                  L.ptr(lvl.prefix), L.ptr(lvl.coords), L.ptr(lvl.d_m), cap, L.ptr(feats), c_dst, storage_math(math),
                                  L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, 'dz_voxelize_to_level')
    lvl.prefix_partial = True
    return lvl, feats


def voxelize_hard(points, pc_range, voxel_size, max_points, max_voxels):
    voxels, coords, nump, d_num = voxelize_hard_nosync(points, pc_range, voxel_size, max_points, max_voxels)
    m = int(d_num.item())
    return voxels[:m], coords[:m], nump[:m]


def mean_vfe(voxels, num_points, c_out=None, d_m=None):
    lib = L.load()
    L.require_cuda(voxels, num_points)
    m, p, c = voxels.shape
    c_out = c if c_out is None else c_out
    out = torch.empty((m, c_out), dtype=torch.float32, device=voxels.device)
    rc = lib.dz_mean_vfe(L.ptr(voxels), L.ptr(num_points), L.ptr(d_m), m, p, c, L.ptr(out), c_out, L.stream())
    L.check(rc, 'dz_mean_vfe')
    return out


def voxelize_dynamic_nosync(points_b, pc_range, voxel_size, batch_size, cap=None, xy_range_mask=False):
    lib = L.load()
    L.require_cuda(points_b)
    n, c1 = points_b.shape
    c = c1 - 1
    grid = grid_size_of(pc_range, voxel_size)
    cap = int(max(n, 1)) if cap is None else int(cap)
    feats = torch.empty((cap, c), dtype=torch.float32, device=points_b.device)
    coords = torch.empty((cap, 4), dtype=torch.int32, device=points_b.device)
    d_num = torch.zeros((1,), dtype=torch.int32, device=points_b.device)
    wsb = lib.dz_voxelize_dynamic_workspace_bytes(n, batch_size, int(grid[0]), int(grid[1]), int(grid[2]), c, cap)
    ws = _ws(wsb)
    rc = lib.dz_voxelize_dynamic_mean(L.ptr(points_b), n, c, L.f6(pc_range), L.f3(voxel_size), L.i3(grid),
                                      1 if xy_range_mask else 0, batch_size, L.ptr(feats), L.ptr(coords), L.ptr(d_num), cap, L.ptr(ws),
                                      ws.numel(), L.stream())
    L.check(rc, 'dz_voxelize_dynamic_mean')
    return feats, coords, d_num


def voxelize_dynamic(points_b, pc_range, voxel_size, batch_size):
    feats, coords, d_num = voxelize_dynamic_nosync(points_b, pc_range, voxel_size, batch_size)
    m = int(d_num.item())
    return feats[:m], coords[:m]


# ------------------------------------------------------------------------------------------------
# sparse index
# ------------------------------------------------------------------------------------------------
LAYOUT_LINEAR, LAYOUT_BRICK = 0, 1


class XWindows(NamedTuple):
    """What build_windows / neighbors_xrun add to a packed submanifold table for the x-run kernels."""
    windows: torch.Tensor                   # per unit of tile_rows output rows and z offset the range of input rows + the tile-queue words
    tile_rows: int                          # the unit: dz_spconv_x_tile_rows(channels, channels)
    sorted_table: Optional[torch.Tensor]    # the table in tap-set order, or None (the kernels then read `words`)
    perm: Optional[torch.Tensor]            # row map of that order, or None


# (what build_tiles adds for the tile-resident convolution: include/detzero_hip.h)
Tiles = NamedTuple('Tiles', [('halo', torch.Tensor), ('tinfo', torch.Tensor), ('ltab', torch.Tensor), ('rowmap', torch.Tensor)])


class NeighborTable:
    """A neighbour table and what was built from it; spconv_route picks the engine from these fields.  words: (kvol, cap) i32 input
    row per tap and output row (-1 = none), or packed the (9, cap) words of a 27-tap table (dz_build_neighbors_packed); kvol: the
    true tap count in both forms; tile_masks: per-32-row tap masks; xwin: None or XWindows; tiles: None or Tiles."""

    def __init__(self, words, kvol=None, packed=False, tile_masks=None, xwin=None, tiles=None):
        self.words, self.packed = words, bool(packed)
        self.kvol = int(kvol) if kvol is not None else 27 if packed else int(words.shape[0])
        self.tile_masks, self.xwin, self.tiles = tile_masks, xwin, tiles

    shape = property(lambda self: self.words.shape)
    device = property(lambda self: self.words.device)

    def numel(self):
        return self.words.numel()

    # the two reads callers written for the tensor form make of a table: its address (L.ptr(table)) and rows of its words (a bare
    # tensor, not a table).  Nothing that acts on a tensor (record_stream, clone, cpu, to) exists here: that goes through tensors()
    def data_ptr(self):
        return self.words.data_ptr()

    def __getitem__(self, index):
        return self.words[index]

    def tensors(self):
        """Every tensor the table owns (what a stream hand-over has to record)."""
        return [t for t in (self.words, self.tile_masks, *(self.xwin or ()), *(self.tiles or ())) if torch.is_tensor(t)]


class SparseLevel:
    """One resolution level of the sparse tensor: bitmap + popcount prefix + coordinates of the rows.
    Plays the role of spconv's SparseConvTensor.indices / indice_dict (backbone3d.py:302-307).
    layout: the cell key that orders the rows (include/detzero_hip.h: DZ_LAYOUT_LINEAR = ascending (b, z, y, x), the canonical
    order of the parity statements; DZ_LAYOUT_BRICK = 8 x 8 columns of the (y, x) plane, the order the backbone computes in)."""

    def __init__(self, batch, shape, cap, device, layout=LAYOUT_LINEAR, zero_count=True):
        lib = L.load()
        self.batch = int(batch)
        self.shape = [int(s) for s in shape]           # (D, H, W)
        self.cap = int(cap)
        self.layout = int(layout)
        nwords = lib.dz_index_words(self.batch, *self.shape, self.layout)
        self.bitmap = torch.empty((nwords,), dtype=torch.int32, device=device)
        self.prefix = torch.empty((nwords,), dtype=torch.int32, device=device)
        self.coords = torch.empty((max(self.cap, 1), 4), dtype=torch.int32, device=device)
        # (zero_count=False: the caller builds the level right away - every build ends with the scan writing the count)
        self.d_m = (torch.zeros if zero_count else torch.empty)((1,), dtype=torch.int32, device=device)
        self.ws = _ws(lib.dz_index_workspace_bytes(self.batch, *self.shape, self.layout))
        self._m_host = None
        # True for levels written by dz_voxelize_to_level: prefix[] is valid only at words that hold a bit, so only ACTIVE cells may
        # be ranked (csrc/common.h: bitmap_rank contract); build_from_coords / downsample write the full prefix
        self.prefix_partial = False
        # power-of-two pre-scale of the feature rows stored on this level (det_modules._Cached.set_prescale): rows hold value * 2^act_exp
        self.act_exp = 0

    def num_active(self):
        """Host copy of the active-site count (one sync; cached)."""
        if self._m_host is None:
            self._m_host = int(self.d_m.item())
        return self._m_host

    def build_from_coords(self, coords, d_n=None, want_rank=True):
        """coords (n,4) i32 [b,z,y,x] any order -> fills the level, returns rank_of_input (n,) i32."""
        lib = L.load()
        L.require_cuda(coords)
        n = coords.shape[0]
        rank = torch.empty((max(n, 1),), dtype=torch.int32, device=coords.device) if want_rank else None
        rc = lib.dz_index_from_coords(L.ptr(coords), L.ptr(d_n), n, self.batch, *self.shape, self.layout, L.ptr(self.bitmap),
                                      L.ptr(self.prefix), L.ptr(self.coords), L.ptr(self.d_m), self.cap,
                                      L.ptr(rank), L.ptr(self.ws), self.ws.numel(), L.stream())
        L.check(rc, 'dz_index_from_coords')
        self._m_host = None
        self.prefix_partial = False
        return rank

    def downsample(self, k, s, p, cap=None):
        """Output level of a strided sparse conv over this level."""
        lib = L.load()
        oshape = [(self.shape[i] + 2 * p[i] - k[i]) // s[i] + 1 for i in range(3)]
        cells = self.batch * oshape[0] * oshape[1] * oshape[2]
        if cap is None:
            per_in = 1
            for i in range(3):
                per_in *= (k[i] + s[i] - 1) // s[i]
            cap = min(cells, self.cap * per_in)
        out = SparseLevel(self.batch, oshape, cap, self.coords.device, layout=self.layout, zero_count=False)
        rc = lib.dz_index_downsample(L.ptr(self.coords), L.ptr(self.d_m), self.cap, self.batch, *self.shape, self.layout,
                                     L.i3(k), L.i3(s), L.i3(p), L.ptr(out.bitmap), L.ptr(out.prefix),
                                     L.ptr(out.coords), L.ptr(out.d_m), out.cap, L.ptr(out.ws), out.ws.numel(),
                                     L.stream())
        L.check(rc, 'dz_index_downsample')
        return out

    def neighbors_to(self, out_level, k, s, p, packed=False):
        """NeighborTable of (kvol, out_level.cap) i32 words, with its tile masks: rows of THIS level feeding each output row.
        packed=True asks for the packed form of a 27-tap table (dz_build_neighbors_packed: (9, cap) words) - what the small-channel
        split-math convolutions read; windows / layouts it does not cover come back unpacked."""
        lib = L.load()
        kvol = k[0] * k[1] * k[2]
        cap = max(out_level.cap, 1)
        masks = torch.empty((lib.dz_tile_masks_words(cap),), dtype=torch.int32, device=self.coords.device)
        args = (L.ptr(out_level.coords), L.ptr(out_level.d_m), out_level.cap, L.ptr(self.bitmap), L.ptr(self.prefix), self.batch,
                *self.shape, self.layout, L.i3(k), L.i3(s), L.i3(p))
        if packed and kvol == 27 and self.layout == LAYOUT_LINEAR and p[2] == 1 and cap < (1 << 29):
            nbr = torch.empty((9, cap), dtype=torch.int32, device=self.coords.device)
            rc = lib.dz_build_neighbors_packed(*args, L.ptr(nbr), L.ptr(masks), L.stream())
            if rc == 0:
                return NeighborTable(nbr, packed=True, tile_masks=masks)
            if rc != L.ERR_UNSUPPORTED:
                L.check(rc, 'dz_build_neighbors_packed')
        nbr = torch.empty((kvol, cap), dtype=torch.int32, device=self.coords.device)
        rc = lib.dz_build_neighbors(*args, L.ptr(nbr), L.ptr(masks), L.stream())
        L.check(rc, 'dz_build_neighbors')
        return NeighborTable(nbr, tile_masks=masks)


FUSED_XWIN = os.environ.get('DZ_TUNE_FUSED_XWIN', '1') != '0'      # development switch: 0 = table and windows by two launches (r04)


def neighbors_xrun(level, channels):
    """Packed submanifold 3 x 3 x 3 table of `level` onto itself WITH the x-run windows (and, from XRUN_SORT_MIN_CHANNELS up, the
    tap-set order) from one launch (dz_build_neighbors_packed_x) - what `build_windows(level.neighbors_to(level, ..., packed=True),
    level, channels)` returns, bit for bit.  Levels / widths the engine does not cover come back as the plain packed / unpacked table."""
    lib = L.load()
    k3, s1, p1 = (3, 3, 3), (1, 1, 1), (1, 1, 1)
    tr = lib.dz_spconv_x_tile_rows(int(channels), int(channels))
    cap = max(level.cap, 1)
    if not FUSED_XWIN or tr == 0 or level.layout != LAYOUT_LINEAR or cap >= (1 << 29):
        return build_windows(level.neighbors_to(level, k3, s1, p1, packed=True), level, channels)
    dev = level.coords.device
    masks = torch.empty((lib.dz_tile_masks_words(cap),), dtype=torch.int32, device=dev)
    nbr = torch.empty((9, cap), dtype=torch.int32, device=dev)
    xwin = _empty_xwin(lib, nbr, tr, channels)
    rc = lib.dz_build_neighbors_packed_x(L.ptr(level.coords), L.ptr(level.d_m), level.cap, L.ptr(level.bitmap), L.ptr(level.prefix), level.batch,
                                         *level.shape, L.ptr(nbr), L.ptr(masks), tr, L.ptr(xwin.windows), L.ptr(xwin.sorted_table),
                                         L.ptr(xwin.perm), L.stream())
    L.check(rc, 'dz_build_neighbors_packed_x')
    return NeighborTable(nbr, packed=True, tile_masks=masks, xwin=xwin)


def _as_table(nbr):
    """`nbr`, or for a bare tensor of table words (a slice, a copy; packed where the caller marked it `.packed = True`, the form
    before NeighborTable) a table of them.  Unmarked (9, n) words are refused: that is the shape of a packed table's slice, which
    must not count as a plain one."""
    if isinstance(nbr, NeighborTable):
        return nbr
    if 'packed' not in vars(nbr) and nbr.shape[0] == 9:
        raise L.DetZeroHipError('bare (9, n) table words: a slice of a packed table? wrap them - NeighborTable(words, packed=True)')
    return NeighborTable(nbr, packed=vars(nbr).get('packed', False))


def unpack_table(nbr):
    """The (27, cap) words of a packed NeighborTable (tests, statistics); the words of other tables are returned as they are."""
    nbr = _as_table(nbr)
    if not nbr.packed:
        return nbr.words
    e = nbr.words.to(torch.int64) & 0xFFFFFFFF
    r = e & 0x1FFFFFFF
    left, cen, right = (e >> 29) & 1, (e >> 30) & 1, (e >> 31) & 1
    minus = torch.full_like(r, -1)
    taps = torch.stack([torch.where(left == 1, r - 1, minus), torch.where(cen == 1, r, minus), torch.where(right == 1, r + cen, minus)], dim=1)
    return taps.reshape(27, nbr.shape[1]).to(torch.int32)


def table_pairs(nbr, m):
    """Number of (input, output) pairs of the first m output rows of a NeighborTable (host sync)."""
    nbr = _as_table(nbr)
    if nbr.packed:
        e = nbr.words[:, :m].to(torch.int64) & 0xFFFFFFFF
        return int((((e >> 29) & 1) + ((e >> 30) & 1) + ((e >> 31) & 1)).sum().item())
    return int((nbr.words[:, :m] >= 0).sum().item())


def build_tiles(nbr, out_level):
    """Tile form of a neighbour table for the tile-resident convolution (dz_spconv_tiles_forward): per tile of
    dz_spconv_tile_rows() output rows the list of distinct input rows (halo), the tile record (slots = non-empty taps, halo
    size, fragment slot masks), the local uint16 table and the tap-set order of the tile's rows (include/detzero_hip.h).
    Filled in as ``nbr.tiles`` (Tiles) - spconv_route picks the tile kernel whenever it is there (split math modes)."""
    lib = L.load()
    kvol, cap = nbr.shape
    tr = lib.dz_spconv_tile_rows()
    ntiles = (cap + tr - 1) // tr
    dev = nbr.device
    halo = torch.empty((ntiles, lib.dz_build_tiles_halo_stride(kvol)), dtype=torch.int32, device=dev)
    tinfo = torch.zeros((ntiles, lib.dz_spconv_tile_info_words()), dtype=torch.int32, device=dev)
    ltab = torch.empty((ntiles, lib.dz_spconv_tile_table_entries()), dtype=torch.int16, device=dev)
    rowmap = torch.empty((ntiles, tr), dtype=torch.int16, device=dev)
    rc = lib.dz_build_tiles(L.ptr(nbr.words), kvol, cap, L.ptr(out_level.d_m), L.ptr(halo), L.ptr(tinfo), L.ptr(ltab), L.ptr(rowmap), L.stream())
    L.check(rc, 'dz_build_tiles')
    nbr.tiles = Tiles(halo, tinfo, ltab, rowmap)
    return nbr


XRUN_SORT = os.environ.get('DZ_TUNE_XRUN_SORT', '1') != '0'       # development switch: rows of a unit in tap-set order
XRUN_SORT_MIN_CHANNELS = int(os.environ.get('DZ_TUNE_XRUN_SORT_MIN', '64'))


def _empty_xwin(lib, words, tr, channels):
    """Unwritten XWindows of a packed (9, cap) table for units of `tr` rows."""
    cap = words.shape[1]
    # (tiles x 3 x 2 window words + the tile-queue words of the convolution kernels)
    win = torch.empty((lib.dz_spconv_x_windows_words(cap, tr),), dtype=torch.int32, device=words.device)
    # the table and the row map in tap-set order (rows of a unit sorted by their neighbour pattern: fewer (fragment, tap) pairs to multiply)
    # (at 32 channels the order saves ~1 % of the kernel - less than sorting a level of 1.8 M rows and writing its table again costs)
    sort = XRUN_SORT and channels >= XRUN_SORT_MIN_CHANNELS
    return XWindows(win, tr, torch.empty_like(words) if sort else None,
                    torch.empty((cap,), dtype=torch.int32, device=words.device) if sort else None)


def build_windows(nbr, out_level, channels):
    """Windows of the x-run convolution (dz_spconv_forward_split_x) for a PACKED submanifold table and the level's channel width:
    per tile of dz_spconv_x_tile_rows(channels, channels) output rows and z offset the contiguous range of input rows its nine taps
    read.  Filled in as ``nbr.xwin`` (XWindows); spconv_route picks an x-run kernel whenever it is there and the layer is
    channels -> channels.  Tables / widths the engine does not cover are returned unchanged."""
    lib = L.load()
    tr = lib.dz_spconv_x_tile_rows(int(channels), int(channels))
    if not nbr.packed or tr == 0:
        return nbr
    xwin = _empty_xwin(lib, nbr.words, tr, channels)
    rc = lib.dz_spconv_x_windows(L.ptr(nbr.words), nbr.shape[1], L.ptr(out_level.d_m), tr, L.ptr(xwin.windows), L.ptr(xwin.sorted_table),
                                 L.ptr(xwin.perm), L.stream())
    L.check(rc, 'dz_spconv_x_windows')
    nbr.xwin = xwin
    return nbr


def scatter_rows(src, rank, c_dst, cap, d_n=None, math=0):
    """dst[rank[i]] = src[i] (zero padded to c_dst channels); with math != 0 the rows are written as pair16."""
    lib = L.load()
    L.require_cuda(src, rank)
    n, c_src = src.shape
    dst = torch.zeros((max(cap, 1), c_dst), dtype=torch.float32, device=src.device)
    if math:
        rc = lib.dz_scatter_rows_split(L.ptr(src), L.ptr(rank), L.ptr(d_n), n, c_src, L.ptr(dst), c_dst, storage_math(math), L.stream())
    else:
        rc = lib.dz_scatter_rows(L.ptr(src), L.ptr(rank), L.ptr(d_n), n, c_src, L.ptr(dst), c_dst, L.stream())
    L.check(rc, 'dz_scatter_rows')
    return dst


def gather_rows(src, idx, d_n, n_cap):
    lib = L.load()
    c = src.shape[1]
    out = torch.zeros((max(n_cap, 1), c), dtype=torch.float32, device=src.device)
    rc = lib.dz_gather_rows(L.ptr(src), L.ptr(idx), L.ptr(d_n), n_cap, c, L.ptr(out), L.stream())
    L.check(rc, 'dz_gather_rows')
    return out


# engines of the sparse backbone's exact-fp32 mode (Backbone3d.set_engine): the gather kernel everywhere; + k_spconv_xf for the submanifold
# convolutions of the 32 / 64 / 128-channel levels; + k_spconv_xt (three bf16 limbs per operand) for those it covers, k_spconv_xf otherwise
SPARSE_F32_ENGINES = ('gather', 'xrun', 'xrun_bf16x3')
# ... and, orthogonal to it, the arithmetic of the convolutions that STAY on the gather path (Backbone3d.set_engine(f32_gather=)):
# 'mfma32' = k_spconv (sparse_conv.hip, fp32 MFMA); 'bf16x3' = k_spconv_gt (sparse_conv_gt.hip, three exact bf16 limbs per operand)
SPARSE_F32_GATHER_ENGINES = ('mfma32', 'bf16x3')
# ... and, on top of either, the kernel of the 16-input-channel layers (conv_input, conv1, conv2's stride-2 layer; set_engine(f32_small=)):
# 'gather' = whatever f32_gather gives them; 'wave_bf16x3' = k_spconv_wt (sparse_conv_wt.hip: wave-private tiles, resident limb weights)
SPARSE_F32_SMALL_ENGINES = ('gather', 'wave_bf16x3')


# what spconv_route returns: a key of _SPCONV_ENGINES; the weight form the engine reads - 'taps' (fp32 (kvol, cin, cout)), 'split'
# (pack_weight_split) or 'limb3' (pack_weight_limb3(w, cout_mult=32)); the library's (cin, cout) -> name of the kernel it launches
SpconvRoute = NamedTuple('SpconvRoute', [('engine', str), ('weights', str), ('variant', Callable)])


def _x_args(t):
    x = t.xwin
    return L.ptr(x.sorted_table if x.perm is not None else t.words), L.ptr(x.perm), L.ptr(x.windows), x.tile_rows


# engine: (weight form, C entry point, its variant-name function, the entry point's arguments between `cin` and `cap`) - in the order
# spconv_route tries them
_SPCONV_ENGINES = {
    'xrun_bf16x3': ('limb3', 'dz_spconv_forward_x_limb3', 'dz_spconv_x_limb3_variant', _x_args),
    'wave_bf16x3': ('limb3', 'dz_spconv_forward_limb3_w', 'dz_spconv_limb3_w_variant', lambda t: (L.ptr(t.words), L.ptr(t.tile_masks), t.kvol)),
    'gather_bf16x3': ('limb3', 'dz_spconv_forward_limb3', 'dz_spconv_limb3_variant', lambda t: (L.ptr(t.words), L.ptr(t.tile_masks), t.kvol)),
    'xrun_f32': ('taps', 'dz_spconv_forward_x_f32', 'dz_spconv_x_f32_variant', _x_args),
    'xrun_split': ('split', 'dz_spconv_forward_split_x', 'dz_spconv_x_variant', _x_args),
    'tiles': ('split', 'dz_spconv_tiles_forward', 'dz_spconv_tiles_variant', lambda t: (*(L.ptr(x) for x in t.tiles), t.kvol)),
    'gather_split_packed': ('split', 'dz_spconv_forward_split_packed', 'dz_spconv_variant_split', lambda t: (L.ptr(t.words), L.ptr(t.tile_masks))),
    'gather_split': ('split', 'dz_spconv_forward_split', 'dz_spconv_variant_split', lambda t: (L.ptr(t.words), L.ptr(t.tile_masks), t.kvol)),
    'gather_f32': ('taps', 'dz_spconv_forward', 'dz_spconv_variant', lambda t: (L.ptr(t.words), t.kvol)),
}


def xrun_unit(cin, cout, math, bf16x3=False):
    """Rows per window unit of the x-run kernel that runs a cin -> cout submanifold layer in this math mode (bf16x3: the three-limb
    kernel of the exact-fp32 mode) from a packed table with windows; 0 = no such kernel.  The one coverage question of the index
    builder (VoxelResBackBone8x.build_pyramid: is a table with windows worth building?) and of spconv_route."""
    lib = L.load()
    cin, cout = int(cin), int(cout)
    rows = lib.dz_spconv_x_limb3_window_rows if bf16x3 else lib.dz_spconv_x_f32_window_rows
    return lib.dz_spconv_x_tile_rows(cin, cout) if cin == cout and (math or rows(cin, cout) > 0) else 0


def spconv_route(table, cin, cout, math, f32_engine=None, f32_gather=None, in_rows=0, f32_small=None):
    """The engine (SpconvRoute) of a cin -> cout convolution over NeighborTable `table`: host logic, the first match wins.
      math 0: 'xrun_bf16x3' for f32_engine 'xrun_bf16x3' on a packed table with windows in the unit of a layer k_spconv_xt covers;
              'wave_bf16x3' for f32_small 'wave_bf16x3' on a plain table with tile masks and a layer k_spconv_wt covers, the table, the
              output and `in_rows` input rows all below 2 GiB (whatever f32_gather says); 'gather_bf16x3' for f32_gather 'bf16x3' on
              such a table and sizes and a layer k_spconv_gt covers; 'xrun_f32' on a packed table with windows in the unit of a layer
              k_spconv_xf covers; 'gather_f32' on any other plain table - no fp32 kernel reads another packed one: an error
      else:   'xrun_split' on a packed table with windows, cin == cout; 'tiles' on a table with tiles, kvol >= 3;
              'gather_split_packed' / 'gather_split' on any other packed / plain table
    A keyword whose engine does not cover the layer falls through (the backbone prefers); spconv_forward, which is explicit, refuses."""
    lib = L.load()
    cin, cout = int(cin), int(cout)
    xwin = table.xwin if table.packed and cin == cout else None
    windows_fit = lambda bf16x3: xwin is not None and 0 != xrun_unit(cin, cout, 0, bf16x3) == xwin.tile_rows
    # what both bf16x3 gather kernels read: a plain table with tile masks; table, output and input rows below 2 GiB
    plain_fits = lambda: (not table.packed and table.tile_masks is not None
                          and 4 * max(table.numel(), table.shape[1] * cout, int(in_rows) * cin) < (1 << 31))
    if math:
        engine = ('xrun_split' if xwin is not None else 'tiles' if table.kvol >= 3 and table.tiles is not None
                  else 'gather_split_packed' if table.packed else 'gather_split')
    elif f32_engine == 'xrun_bf16x3' and windows_fit(True):
        engine = 'xrun_bf16x3'
    elif f32_small == 'wave_bf16x3' and plain_fits() and lib.dz_spconv_limb3_w_tile_rows(cin, cout) > 0:
        engine = 'wave_bf16x3'
    elif f32_gather == 'bf16x3' and plain_fits() and lib.dz_spconv_limb3_tile_rows(cin, cout) > 0:
        engine = 'gather_bf16x3'
    elif windows_fit(False):
        engine = 'xrun_f32'
    elif table.packed:
        raise L.DetZeroHipError('spconv_forward: a packed neighbour table feeds the split-math kernels only - in fp32 an x-run kernel, through windows in '
                                'the unit of a layer it covers (%d -> %d, f32_engine=%r, f32_gather=%r)' % (cin, cout, f32_engine, f32_gather))
    else:
        engine = 'gather_f32'
    form, _, variant, _ = _SPCONV_ENGINES[engine]
    return SpconvRoute(engine, form, getattr(lib, variant))


def spconv_forward(feats, nbr, out_level, w_taps, scale, shift, residual=None, relu=True, out=None, in_level=None, math=0, cout=None,
                   f32_engine=None, f32_gather=None, f32_small=None, *, max_workgroups=0):
    """feats (m_in,cin); nbr: NeighborTable of (kvol,cap); returns (cap,cout), computed by the engine of spconv_route.
    math == 0: fp32 rows, w_taps (kvol,cin,cout) fp32; a packed table with x-run windows (neighbors_xrun / build_windows) runs a
    cin == cout layer of 32 / 64 / 128 channels on the exact-fp32 x-run kernel (dz_spconv_forward_x_f32).
    f32_engine / f32_gather (math 0 only; the split modes ignore them) are explicit - a table or layer the named kernel does not
    cover is an error: 'xrun_bf16x3' = that table and those rows on the three-limb kernel of csrc/sparse_conv_xt.hip; 'bf16x3' = a
    plain table with tile masks on the three-limb gather kernel of csrc/sparse_conv_gt.hip; f32_small 'wave_bf16x3' = such a table
    and a 16 -> 16 or 16 -> 32 layer on the wave-private three-limb kernel of csrc/sparse_conv_wt.hip (it goes before f32_gather;
    max_workgroups, for tests and tools, caps its persistent grid: 0 = as many as fit).  All read `w_taps` in the
    pack_weight_limb3(w, cout_mult=32) layout (kvol, cout_pad, cin * 3 / 2), with `cout=` the true width where it is below 32
    (default: the BatchNorm vector's, else the weights').  None, 'gather', 'xrun', 'mfma32' ask for nothing.
    math != 0: pair16 rows (in, residual, out), w_taps (kvol,cout_pad,cin) pair16 from pack_weight_split."""
    lib = L.load()
    if f32_engine not in (None,) + SPARSE_F32_ENGINES:
        raise L.DetZeroHipError('unknown fp32 sparse engine %r (%s)' % (f32_engine, ' | '.join(SPARSE_F32_ENGINES)))
    if f32_gather not in (None,) + SPARSE_F32_GATHER_ENGINES:
        raise L.DetZeroHipError('unknown fp32 gather arithmetic %r (%s)' % (f32_gather, ' | '.join(SPARSE_F32_GATHER_ENGINES)))
    if f32_small not in (None,) + SPARSE_F32_SMALL_ENGINES:
        raise L.DetZeroHipError('unknown fp32 small-layer engine %r (%s)' % (f32_small, ' | '.join(SPARSE_F32_SMALL_ENGINES)))
    wave = not math and f32_small == 'wave_bf16x3'
    limb = not math and (f32_engine == 'xrun_bf16x3' or f32_gather == 'bf16x3' or wave)
    if math or limb:
        # (split and limb weights are padded to 32 output channels: the true count comes from `cout=`, the BatchNorm vector, else the weights)
        if limb and (w_taps.dim() != 3 or w_taps.shape[0] != nbr.kvol or w_taps.shape[2] % 12 != 0):
            raise L.DetZeroHipError("spconv_forward: the fp32 engines 'xrun_bf16x3' / 'bf16x3' need the (kvol, cout_pad, cin * 3 / 2) limb "
                                    'weights of the layer, not %s' % (tuple(w_taps.shape),))
        cin = w_taps.shape[2] if math else w_taps.shape[2] * 2 // 3
        cout = int(cout) if cout is not None else scale.shape[0] if scale is not None else w_taps.shape[1]
        if limb and w_taps.shape[1] != max(cout, 32):
            raise L.DetZeroHipError("spconv_forward: fp32 arithmetic 'bf16x3' does not cover a %d -> %d layer with %d weight rows"
                                    % (cin, cout, w_taps.shape[1]))
    else:
        cin, cout = w_taps.shape[1], w_taps.shape[2]
    route = spconv_route(nbr, cin, cout, math, f32_engine, f32_gather, feats.shape[0], f32_small)
    if wave and f32_engine != 'xrun_bf16x3' and route.engine != 'wave_bf16x3':
        raise L.DetZeroHipError("spconv_forward: this %s table and %d -> %d layer run on %r - f32_small 'wave_bf16x3' needs a plain table with tile "
                                'masks, a 16 -> 16 or 16 -> 32 layer the library covers and tensors below 2 GiB'
                                % ('packed' if nbr.packed else 'plain', cin, cout, route.engine))
    if max_workgroups and route.engine != 'wave_bf16x3':
        raise L.DetZeroHipError('spconv_forward: max_workgroups caps the grid of the wave_bf16x3 engine only, this layer runs on %r' % (route.engine,))
    if limb and route.engine != ('xrun_bf16x3' if f32_engine == 'xrun_bf16x3' else 'wave_bf16x3' if wave else 'gather_bf16x3'):
        raise L.DetZeroHipError("spconv_forward: this %s table and %d -> %d layer run on %r - f32_engine 'xrun_bf16x3' needs a packed table with x-run "
                                "windows in the unit of a cin == cout layer it covers, f32_gather 'bf16x3' a plain table with tile masks, a layer it "
                                'covers and tensors below 2 GiB' % ('packed' if nbr.packed else 'plain', cin, cout, route.engine))
    L.require_cuda(feats, nbr.words, w_taps, scale, shift, residual)
    assert feats.shape[1] == cin, (feats.shape, w_taps.shape)
    cap = nbr.shape[1]
    if out is None:
        out = torch.empty((cap, cout), dtype=torch.float32, device=feats.device)
    form, entry, _, table_args = _SPCONV_ENGINES[route.engine]

    def launch():
        rc = getattr(lib, entry)(L.ptr(feats), feats.shape[0], cin, *table_args(nbr), cap, L.ptr(out_level.d_m), L.ptr(w_taps), L.ptr(scale),
                                 L.ptr(shift), L.ptr(residual), 1 if relu else 0, L.ptr(out), cout, *((int(math),) if form == 'split' else ()),
                                 *((int(max_workgroups),) if route.engine == 'wave_bf16x3' else ()), L.stream())
        L.check(rc, 'dz_spconv_forward')
    if PROFILER is None:
        launch()
    else:
        # algorithmic work of this launch: 2*pairs*cin*cout FLOP; bytes per BASELINE.md section 3
        m = out_level.num_active()
        pairs = table_pairs(nbr, m)
        flops = 2.0 * pairs * cin * cout
        n_in = in_level.num_active() if in_level is not None else m
        nbytes = 4.0 * (n_in * cin + m * cout + nbr.kvol * cin * cout + (m * cout if residual is not None else 0)) + 8.0 * pairs
        PROFILER.wrap(route.variant(cin, cout).decode(), flops, nbytes, launch)
    return out


def bev_row_index(level, feat_rows, pad=1):
    """(B, H + 2 pad, W + 2 pad, 2) int32: the feature row of every (pixel, z slab) of a two-slab level, -1 = empty / border / past
    `feat_rows` - the sparse-input form of HeightCompression (dz_conv2d_desc.in_rowidx)."""
    lib = L.load()
    d, h, w = level.shape
    idx = torch.empty((level.batch, h + 2 * pad, w + 2 * pad, 2), dtype=torch.int32, device=level.coords.device)
    rc = lib.dz_bev_row_index(L.ptr(level.bitmap), L.ptr(level.prefix), level.batch, d, h, w, level.layout, pad, int(feat_rows), L.ptr(idx), L.stream())
    L.check(rc, 'dz_bev_row_index')
    return idx


def bev_tile_list(ridx, ho, wo, nlists=1):
    """(nlists, words) int32 over a row-index image: row l - 1 holds the two pixel-tile lists of the l-th 3 x 3 layer of the first BEV block
    (dz_bev_tile_cover), each [n to run, n to fill, entries to run, entries to fill].  From word 0 the fixed-grid list: ids of the 8 x 32
    tiles with a pixel less than l + 1 pixels away from any row, ascending, then the skippable ones; from word bev_tile_cover_offset the
    free-offset cover of the same pixels (`bev_tile_cover`) - what the detector launches."""
    lib = L.load()
    b, hp, wp, _ = ridx.shape
    n = lib.dz_bev_tile_cover_words(b, int(ho), int(wo))
    lst = torch.empty((int(nlists), n), dtype=torch.int32, device=ridx.device)
    ws = torch.empty((lib.dz_bev_tile_cover_ws_words(b, int(ho), int(wo), int(nlists)),), dtype=torch.int32, device=ridx.device)
    L.check(lib.dz_bev_tile_cover(L.ptr(ridx), b, hp, wp, int(ho), int(wo), int(nlists), L.ptr(lst), L.ptr(ws), L.stream()), 'dz_bev_tile_cover')
    return lst


def bev_tile_cover(lists, batch, ho, wo):
    """The cover lists of `bev_tile_list`'s rows (a view): [n tiles, n spans, tile entries (bit 31 | b << 21 | ty << 12 | x0), spans (entry of
    (b, ty, xs), xe)].  Tiles start at any pixel column of their 8-row band; spans are the columns of a band outside its tiles."""
    return lists[:, L.load().dz_bev_tile_cover_offset(int(batch), int(ho), int(wo)):]


def bev_fill_empty_tiles(tiles, batch, ho, wo, shift, relu, cout, out, math, zero_resp=None):
    """The pixels that list `tiles` (either list of a `bev_tile_list` row) leaves out of its launch get the layer's zero-input response in the
    zero-bordered pair16 image `out` (B, ho + 2, wo + 2, C): the (1, ho + 2, wo + 2, C) image `zero_resp`, or - None: the first layer - the
    constant ReLU(shift)."""
    lib = L.load()
    L.check(lib.dz_bev_fill_spans(L.ptr(tiles), int(batch), int(ho), int(wo), L.ptr(shift), 1 if relu else 0, int(cout), L.ptr(out), out.shape[1],
                                  out.shape[2], out.shape[3], 0, L.ptr(zero_resp), int(math), L.stream()), 'dz_bev_fill_spans')


BEV_DENSE = not os.environ.get('DZ_BEV_SCATTER')   # development switch: False = zero-fill + scatter (dz_sparse_to_bev_split) for two-slab levels too


def sparse_to_bev(feats, level, c, pad=1, out=None, math=0):
    """-> (B, H+2p, W+2p, C*D) channel-last zero-bordered BEV image (pair16 in, pair16 out when math != 0)."""
    lib = L.load()
    d, h, w = level.shape
    if out is None:
        out = torch.empty((level.batch, h + 2 * pad, w + 2 * pad, c * d), dtype=torch.float32, device=feats.device)
    if math and d == 2 and c % 8 == 0 and BEV_DENSE:
        # two z slabs (the backbone's encoded tensor): the whole image, zeros included, written once from the level's own index
        rc = lib.dz_sparse_to_bev_split_dense(L.ptr(feats), feats.shape[0], L.ptr(level.bitmap), L.ptr(level.prefix), level.batch, c, d, h, w, level.layout,
                                              pad, L.ptr(out), L.stream())
        L.check(rc, 'dz_sparse_to_bev_split_dense')
        return out
    out.zero_()
    fn = lib.dz_sparse_to_bev_split if math else lib.dz_sparse_to_bev
    rc = fn(L.ptr(feats), L.ptr(level.coords), L.ptr(level.d_m), level.cap, c, d, h, w, pad, L.ptr(out), L.stream())
    L.check(rc, 'dz_sparse_to_bev')
    return out


# ------------------------------------------------------------------------------------------------
# split precision (pair16): csrc/hgemm.h
# ------------------------------------------------------------------------------------------------
# 'f16' (3): the tensors of 'f16x2' (fp16 pairs), but every convolution product is ONE fp16 MFMA on the hi halves - plain-fp16
# inputs with fp32 accumulation, a third of the matrix work.  Opt-in fast mode, NOT fp32-class.
MATH_MODES = {'f32': 0, 'f16x2': 1, 'bf16x2': 2, 'f16': 3}


def storage_math(math):
    """The pair16 encoding a math mode keeps its tensors in (3 = 'f16' computes on the tensors of 1 = 'f16x2')."""
    return 1 if int(math) == 3 else int(math)


def math_id(mode):
    if isinstance(mode, str):
        if mode not in MATH_MODES:
            raise L.DetZeroHipError('unknown math mode %r (choose from %s)' % (mode, sorted(MATH_MODES)))
        return MATH_MODES[mode]
    return int(mode)


def pair16_pack(x, math):
    """Host/torch packer (any device): x (..., C) fp32, C % 8 == 0 -> same-shape float32-typed pair16 bits.
    Used for weights at plan time; the device kernels (dz_pair16_from_f32, conv epilogues) do the same split."""
    math = storage_math(math)
    dt = torch.float16 if math == 1 else torch.bfloat16
    x = x.float()
    if math == 1:
        x = x.clamp(-65504.0, 65504.0)
    hi = x.to(dt)
    lo = (x - hi.float()).to(dt)
    shp = x.shape
    g = shp[-1] // 8
    out = torch.stack([hi.reshape(*shp[:-1], g, 8), lo.reshape(*shp[:-1], g, 8)], dim=-2)
    return out.reshape(*shp[:-1], g * 16).contiguous().view(torch.float32)


def pair16_unpack(x, math):
    math = storage_math(math)
    dt = torch.float16 if math == 1 else torch.bfloat16
    shp = x.shape
    g = shp[-1] // 8
    h = x.contiguous().view(dt).reshape(*shp[:-1], g, 2, 8).float()
    return (h[..., 0, :] + h[..., 1, :]).reshape(shp)


def pack_weight_split(w, math, cout_mult=32):
    """(..., cin, cout) fp32 conv weights -> (..., cout_pad, cin) pair16 (cout padded with zero rows)."""
    wt = w.float().transpose(-1, -2)
    co = wt.shape[-2]
    cp = -(-co // cout_mult) * cout_mult
    if cp > co:
        wt = torch.cat([wt, wt.new_zeros(*wt.shape[:-2], cp - co, wt.shape[-1])], dim=-2)
    return pair16_pack(wt.contiguous(), math)


BF16_MAX = 3.3895313892515355e38      # 0x7F7F: the clamp in front of the first rounding of the three-limb split


def _limbs3(x):
    """The three bf16 limbs of fp32 x (csrc/conv3x3_t.hip): h = rn(clamp(x, +-bf16-max)), m = rn(x - h), l = rn(x - h - m) - the last
    rounding is exact for every finite x, so h + m + l == x bit for bit."""
    x = x.float()
    h = x.clamp(-BF16_MAX, BF16_MAX).to(torch.bfloat16)
    r1 = x - h.float()
    m = r1.to(torch.bfloat16)
    l = (r1 - m.float()).to(torch.bfloat16)
    # a zero limb takes the sign of x, so that the limbs of -0 sum to -0 (the value of the limb is that of its remainder either way)
    z = torch.copysign(torch.zeros_like(x), x).to(torch.bfloat16)
    return h, torch.where(m == 0, z, m), torch.where(l == 0, z, l)


def limb3_pack(x):
    """Host/torch packer (any device): x (..., C) fp32, C % 8 == 0 -> (..., C * 3 / 2) float32-typed words: per group of 8 channels
    16 bytes of h limbs, 16 of m, 16 of l (bf16).  The operand format of dz_conv3x3_limb3_forward's weights."""
    shp = x.shape
    if shp[-1] % 8 != 0:
        raise L.DetZeroHipError('limb3_pack: the last dimension (%d) must be a multiple of 8' % shp[-1])
    g = shp[-1] // 8
    out = torch.stack([t.reshape(*shp[:-1], g, 8) for t in _limbs3(x)], dim=-2)
    return out.reshape(*shp[:-1], g * 24).contiguous().view(torch.float32)


def limb3_unpack(x):
    """limb3_pack's inverse, bit for bit: (..., C * 3 / 2) words -> (..., C) fp32 = h + (m + l) (m + l is the exact first remainder:
    summed in this order nothing rounds, and +-fp32-max does not pass through 2^128)."""
    shp = x.shape
    g = shp[-1] // 12
    t = x.contiguous().view(torch.bfloat16).reshape(*shp[:-1], g, 3, 8).float()
    return (t[..., 0, :] + (t[..., 1, :] + t[..., 2, :])).reshape(*shp[:-1], g * 8)


def pack_weight_limb3(w, cout_mult=64):
    """(taps, cin, cout) fp32 conv weights -> (taps, cout_pad, cin * 3 / 2) limb words, output-channel rows (cout padded with zero rows)."""
    wt = w.float().transpose(-1, -2)
    co = wt.shape[-2]
    cp = -(-co // cout_mult) * cout_mult
    if cp > co:
        wt = torch.cat([wt, wt.new_zeros(*wt.shape[:-2], cp - co, wt.shape[-1])], dim=-2)
    return limb3_pack(wt.contiguous())


F16_PAIR_WEIGHT_TOP = 2.0 ** 14      # where the largest |weight| of an output channel is placed before the fp16-pair split


def weight_prescale(w):
    """Exact per-output-channel power-of-two scaling of conv / linear weights (..., cin, cout) for fp16-pair storage.
    An fp16 pair carries 22 significant bits only while its lo half is a NORMAL fp16 (|value| >= 2^-3); checkpoint weights are
    O(1e-2) and would keep ~18.  Every output channel is multiplied by 2^e_c so that its largest |weight| lands in [2^13, 2^15)
    (fp16 tops out at 65504; the products are accumulated in fp32, where a power of two changes nothing), and 2^-e_c goes into the
    layer's per-channel epilogue scale.  Returns (scaled weights, inverse factors (..., cout))."""
    red = (-3, -2) if w.dim() >= 3 else (-2,)
    amax = w.detach().abs().float().amax(dim=red)
    e = torch.floor(torch.log2(F16_PAIR_WEIGHT_TOP / amax.clamp_min(1e-30))).clamp_(-40.0, 40.0)
    e = torch.where(amax > 0, e, torch.zeros_like(e)).to(torch.int32)
    one = torch.ones_like(amax)
    up, down = torch.ldexp(one, e), torch.ldexp(one, -e)
    for _ in red:
        up = up.unsqueeze(-2)
    return w.float() * up, down


def level_rows_f32(rows, level, math=0):
    """Feature rows of a level as plain fp32 values: pair16 decoded, the level's power-of-two pre-scale (SparseLevel.act_exp) removed."""
    plain = pair16_to_f32(rows, math) if math else rows
    e = int(getattr(level, 'act_exp', 0) or 0)
    return plain * (2.0 ** -e) if e else plain


def pair16_from_f32(x, c_dst=None, math=1):
    """device conversion of rows (..., C) fp32 -> (..., c_dst) pair16"""
    lib = L.load()
    L.require_cuda(x)
    x = x.contiguous()
    c = x.shape[-1]
    c_dst = c if c_dst is None else c_dst
    rows = x.numel() // c
    out = torch.empty((*x.shape[:-1], c_dst), dtype=torch.float32, device=x.device)
    L.check(lib.dz_pair16_from_f32(L.ptr(x), rows, c, c_dst, storage_math(math), L.ptr(out), L.stream()), 'dz_pair16_from_f32')
    return out


def pair16_to_f32(x, math=1):
    lib = L.load()
    L.require_cuda(x)
    x = x.contiguous()
    c = x.shape[-1]
    out = torch.empty_like(x)
    L.check(lib.dz_pair16_to_f32(L.ptr(x), x.numel() // c, c, storage_math(math), L.ptr(out), L.stream()), 'dz_pair16_to_f32')
    return out


# ------------------------------------------------------------------------------------------------
# range probe (csrc/range_probe.hip): per-tensor peak / fp16-pair saturation / non-finite counts in device records
# ------------------------------------------------------------------------------------------------
RANGE_DTYPE = np.dtype([('peak', np.float32), ('saturated', np.uint64), ('nonfinite', np.uint64), ('elements', np.uint64)])


def range_table(n_slots, device):
    """Zeroed table of n_slots records (n_slots, 4) int64: [peak bits, saturated, nonfinite, elements] (include/detzero_hip.h)."""
    return torch.zeros((int(n_slots), 4), dtype=torch.int64, device=device)


def range_probe(t, slot_view, *, math, rows=None, d_rows=None, c_off=0, c=None):
    """Add the range of `t` to one record.  t: contiguous float32-typed tensor whose last dimension is the row (fp32 values, or the
    pair16 words of a split mode); slot_view: one row of a `range_table`; math: the storage of t (a mode name or id; 'f16' reads as
    'f16x2').  rows: leading rows to read (default all), d_rows: device int32 count that limits them further; [c_off, c_off + c): the
    channel slice (default: the rest of the row).  Asynchronous on the current stream, no allocation."""
    lib = L.load()
    L.require_cuda(t, slot_view, d_rows)
    if t.dtype != torch.float32 or slot_view.dtype != torch.int64 or slot_view.numel() != 4:
        raise L.DetZeroHipError('range_probe: a float32-typed tensor and a 4-word int64 record are expected')
    stride = int(t.shape[-1])
    cap = t.numel() // max(stride, 1)
    rows = cap if rows is None else int(rows)
    if rows > cap:
        raise L.DetZeroHipError('range_probe: %d rows asked of a tensor of %d' % (rows, cap))
    c = stride - int(c_off) if c is None else int(c)
    L.check(lib.dz_range_probe(L.ptr(t) if rows else None, rows, L.ptr(d_rows), stride, int(c_off), c, storage_math(math_id(math)), L.ptr(slot_view),
                               L.stream()), 'dz_range_probe')


def range_reset(table):
    L.require_cuda(table)
    L.check(L.load().dz_range_reset(L.ptr(table), table.shape[0], L.stream()), 'dz_range_reset')


def range_read(table):
    """The one host copy of a table -> numpy structured array (peak as float32, the three counters as uint64)."""
    raw = table.cpu().numpy().view(np.uint64).reshape(-1, 4)
    out = np.zeros((raw.shape[0],), dtype=RANGE_DTYPE)
    out['peak'] = (raw[:, 0] & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)
    out['saturated'], out['nonfinite'], out['elements'] = raw[:, 1], raw[:, 2], raw[:, 3]
    return out


# ------------------------------------------------------------------------------------------------
# dense conv
# ------------------------------------------------------------------------------------------------
DENSE_F32_ENGINES = ('mfma32', 'bf16x3')
# engine of the layers the 3 x 3 stride-1 kernel does not take (strided 3 x 3, 1 x 1 deblock phases, grouped output layers): csrc/conv2d_t.hip
DENSE_F32_GENERIC_ENGINES = ('mfma32', 'bf16x3')


def _conv2d_desc(desc_kwargs):
    d = L.Conv2dDesc()
    for k, v in desc_kwargs.items():
        if k in ('g_cout', 'g_ooff'):
            arr = getattr(d, k)
            for i, e in enumerate(v):
                arr[i] = int(e)
        else:
            setattr(d, k, v)
    return d


def conv3x3_limb3_supported(desc_kwargs):
    """Whether the bf16x3 engine of the f32 mode (dz_conv3x3_limb3_forward) takes the layer of these dz_conv2d_desc fields.  Host only."""
    return bool(L.load().dz_conv3x3_limb3_supported(ctypes.byref(_conv2d_desc(desc_kwargs))))


def conv2d_limb3_supported(desc_kwargs):
    """Whether the generic bf16x3 engine of the f32 mode (dz_conv2d_limb3_forward, csrc/conv2d_t.hip) takes the layer of these
    dz_conv2d_desc fields.  Host only."""
    return bool(L.load().dz_conv2d_limb3_supported(ctypes.byref(_conv2d_desc(desc_kwargs))))


def pack_weight_limb3_generic(w):
    """(groups, taps, cin, cout_pad) or (taps, cin, cout_pad) fp32 weights of dz_conv2d_forward -> the operand of dz_conv2d_limb3_forward:
    (groups * taps, round_up(cout_pad, 32), cin * 3 / 2) limb words (pack_weight_limb3 with the zero rows k_conv2d_t's tiles read)."""
    return pack_weight_limb3(w.reshape(-1, w.shape[-2], w.shape[-1]), cout_mult=32)


def conv2d(desc_kwargs, math=0, out_f32=False, tiles=None, f32_engine=None, f32_generic=None):
    """One dense-conv launch from a dict of dz_conv2d_desc fields.  math != 0: pair16 input / weights
    (pack_weight_split layout) and pair16 output unless out_f32.  tiles: the tensor behind `in_tiles` (profiling only: the work of
    the launch is that of the tiles it runs).  f32_engine='bf16x3' (math 0 only; the split modes ignore it): the three-limb kernel
    of csrc/conv3x3_t.hip, `w` in the pack_weight_limb3 layout; a layer it does not cover is an error.  f32_generic='bf16x3' (likewise
    math 0 only, and only where f32_engine does not name 'bf16x3'): the generic three-limb kernel of csrc/conv2d_t.hip, `w` in the
    pack_weight_limb3_generic layout; a layer it does not cover is an error."""
    lib = L.load()
    if f32_engine not in (None,) + DENSE_F32_ENGINES:
        raise L.DetZeroHipError('unknown fp32 dense engine %r (%s)' % (f32_engine, ' | '.join(DENSE_F32_ENGINES)))
    if f32_generic not in (None,) + DENSE_F32_GENERIC_ENGINES:
        raise L.DetZeroHipError('unknown generic fp32 dense engine %r (%s)' % (f32_generic, ' | '.join(DENSE_F32_GENERIC_ENGINES)))
    limb3 = f32_engine == 'bf16x3' and not math
    limb3g = f32_generic == 'bf16x3' and not math and not limb3
    d = _conv2d_desc(desc_kwargs)

    def launch():
        if limb3:
            L.check(lib.dz_conv3x3_limb3_forward(ctypes.byref(d), L.stream()), 'dz_conv3x3_limb3_forward')
        elif limb3g:
            L.check(lib.dz_conv2d_limb3_forward(ctypes.byref(d), L.stream()), 'dz_conv2d_limb3_forward')
        elif math:
            L.check(lib.dz_conv2d_forward_split(ctypes.byref(d), int(math), 1 if out_f32 else 0, L.stream()), 'dz_conv2d_forward_split')
        else:
            L.check(lib.dz_conv2d_forward(ctypes.byref(d), L.stream()), 'dz_conv2d_forward')
    if PROFILER is None:
        launch()
        return
    m = d.batch * d.ho * d.wo
    taps = d.kh * d.kw
    cout = sum(d.g_cout[i] for i in range(d.groups))
    flops = 2.0 * m * taps * d.cin * cout
    nbytes = 4.0 * (m * d.cin * (1 if d.phase_groups else d.groups) + m * cout + taps * d.cin * d.cout_pad * d.groups)
    if tiles is not None:
        # zero-response tiles are not run: count the EXECUTED share of the layer (one host sync; profiling passes only), so that the
        # roofline figures of the kernel describe the kernel, not the work it was spared
        # (a cover list counts spans behind its tiles, not tiles: the share is of the layer's 8 x 32 grid)
        share = int(tiles[0]) / float(max(d.batch * (-(-d.ho // 8)) * (-(-d.wo // 32)), 1))
        flops *= share
        nbytes = 4.0 * (share * (m * d.cin + m * cout) + taps * d.cin * d.cout_pad * d.groups)
    if limb3:
        name = lib.dz_conv3x3_limb3_variant(ctypes.byref(d)).decode()
    elif limb3g:
        name = lib.dz_conv2d_limb3_variant(ctypes.byref(d)).decode()
    else:
        name = (lib.dz_conv2d_variant_split(ctypes.byref(d), 1 if out_f32 else 0) if math else lib.dz_conv2d_variant(ctypes.byref(d))).decode()
    PROFILER.wrap(name, flops, nbytes, launch)


LINEAR_F32_ENGINES = ('mfma32', 'bf16x3')


def linear_limb3_supported(cin, x_stride, cout, cout_pad, y_stride):
    """Whether the bf16x3 engine of the f32 mode's linear layers (dz_linear_limb3_forward, csrc/linear_t.hip) takes a layer of these
    sizes.  Host only."""
    return bool(L.load().dz_linear_limb3_supported(int(cin), int(x_stride), int(cout), int(cout_pad), int(y_stride)))


def linear(x, w, scale, shift, relu, cout, out=None, group_shift=None, group_rows=0, f32_engine=None, w_limb=None, max_launch_rows=0):
    """x (rows, cin) @ w (cin, cout_pad) -> (rows, cout); optional per-row-group pre-activation addend.
    f32_engine='bf16x3': the three-limb kernel of csrc/linear_t.hip with w_limb = pack_weight_limb3_generic(w[None]) (w itself only
    gives cout_pad); a layer it does not cover is an error.  max_launch_rows (that engine only): cap on the rows of one launch."""
    lib = L.load()
    if f32_engine not in (None,) + LINEAR_F32_ENGINES:
        raise L.DetZeroHipError('unknown fp32 linear engine %r (%s)' % (f32_engine, ' | '.join(LINEAR_F32_ENGINES)))
    L.require_cuda(x, w, scale, shift, group_shift)
    rows, cin = x.shape
    cout_pad = w.shape[1]
    if out is None:
        out = torch.empty((rows, cout), dtype=torch.float32, device=x.device)
    if f32_engine == 'bf16x3':
        if w_limb is None:
            raise L.DetZeroHipError('linear: f32_engine bf16x3 needs w_limb (pack_weight_limb3_generic of the weights)')
        L.require_cuda(w_limb)
        rc = lib.dz_linear_limb3_forward(L.ptr(x), rows, cin, x.stride(0), L.ptr(w_limb), cout, cout_pad, L.ptr(scale), L.ptr(shift),
                                         L.ptr(group_shift), int(group_rows), 1 if relu else 0, L.ptr(out), out.stride(0),
                                         int(max_launch_rows), L.stream())
        L.check(rc, 'dz_linear_limb3_forward')
        return out
    rc = lib.dz_linear_forward(L.ptr(x), rows, cin, x.stride(0), L.ptr(w), cout, cout_pad, L.ptr(scale),
                               L.ptr(shift), L.ptr(group_shift), int(group_rows), 1 if relu else 0, L.ptr(out),
                               out.stride(0), L.stream())
    L.check(rc, 'dz_linear_forward')
    return out


SPLITK_MAX_ROWS, SPLITK_MIN_CIN = 2048, 4096


def linear_splitk_ok(rows, cin):
    return 0 < rows <= SPLITK_MAX_ROWS and cin >= SPLITK_MIN_CIN and cin % 256 == 0


def linear_splitk(x, w, scale, shift, relu, cout, splits=8):
    """dz_linear_forward_splitk: ops.linear for a few rows against a very long input (cin % (splits * 32) == 0): the input channels in
    `splits` groups side by side, summed in a second pass."""
    lib = L.load()
    L.require_cuda(x, w, scale, shift)
    rows, cin = x.shape
    cout_pad = w.shape[1]
    nbytes = lib.dz_linear_splitk_workspace_bytes(rows, cout_pad, splits)
    ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=x.device)
    out = torch.empty((rows, cout), dtype=torch.float32, device=x.device)
    rc = lib.dz_linear_forward_splitk(L.ptr(x), rows, cin, x.stride(0), L.ptr(w), cout, cout_pad, L.ptr(scale), L.ptr(shift), 1 if relu else 0, L.ptr(out),
                                      out.stride(0), int(splits), L.ptr(ws), nbytes, L.stream())
    L.check(rc, 'dz_linear_forward_splitk')
    return out


def linear_split(x, w, scale, shift, relu, cout, math, out_f32=False, group_shift=None, group_rows=0, group_max=False):
    """dz_linear_forward_split: x (rows, >= cin words) pair16 @ w (cout_pad, cin) pair16 -> (rows, cout) fp32 when out_f32,
    else (rows, cout) pair16 (cout % 32 == 0 so that the result can feed the next layer).
    group_max: -> (rows / group_rows, cout) fp32, the maximum over each group of `group_rows` consecutive rows, taken in the layer's
    epilogue (the PointNet max over an object's points; the (rows, cout) activation is never written)."""
    lib = L.load()
    L.require_cuda(x, w, scale, shift, group_shift)
    rows = x.shape[0]
    cout_pad, cin = w.shape
    if not out_f32 and cout % 32:
        raise L.DetZeroHipError('linear_split: a pair16 result needs cout %% 32 == 0 (got %d)' % cout)
    if group_shift is not None and group_shift.shape[1] != cout_pad:
        raise L.DetZeroHipError('linear_split: group_shift rows must be cout_pad = %d wide' % cout_pad)
    if group_max and (group_rows < 128 or group_rows % 128 or rows % group_rows):
        raise L.DetZeroHipError('linear_split: group_max needs groups of a multiple of 128 rows (got %d rows in groups of %d)' % (rows, group_rows))
    out = torch.empty((rows // group_rows if group_max else rows, cout), dtype=torch.float32, device=x.device)
    rc = lib.dz_linear_forward_split(L.ptr(x), rows, cin, x.stride(0), L.ptr(w), cout, cout_pad, L.ptr(scale), L.ptr(shift),
                                     L.ptr(group_shift), int(group_rows), 1 if relu else 0, L.ptr(out), out.stride(0), int(math),
                                     1 if (out_f32 or group_max) else 0, 1 if group_max else 0, L.stream())
    L.check(rc, 'dz_linear_forward_split')
    return out


def pointnet3(x, layers, group_rows, math, want_tap=False, x_f32=False):
    """dz_pointnet3_forward: x (rows, 32) pair16 - or, with x_f32, (rows, 16 | 32) fp32 rows split inside the kernel - through three
    (w (cout_pad, cin) pair16, scale, shift) layers 32 -> 128 -> 128 -> c3 with ReLU and the max over every `group_rows` rows ->
    (pooled (rows / group_rows, c3) fp32, tap (rows, 128) pair16 or None)."""
    lib = L.load()
    (w1, s1, b1), (w2, s2, b2), (w3, s3, b3) = layers
    L.require_cuda(x, w1, w2, w3, s1, b1, s2, b2, s3, b3)
    rows = x.shape[0]
    c3 = w3.shape[0]
    if tuple(w1.shape) != (128, 32) or tuple(w2.shape) != (128, 128) or w3.shape[1] != 128 or x.shape[1] not in ((16, 32) if x_f32 else (32,)) or rows % group_rows:
        raise L.DetZeroHipError('pointnet3: expects 32 -> 128 -> 128 -> c3 layers on (rows, 32) pair16 input (got %s, %s, %s on %s)' % (
            tuple(w1.shape), tuple(w2.shape), tuple(w3.shape), tuple(x.shape)))
    out = torch.empty((rows // group_rows, c3), dtype=torch.float32, device=x.device)
    tap = torch.empty((rows, 128), dtype=torch.float32, device=x.device) if want_tap else None
    rc = lib.dz_pointnet3_forward(L.ptr(x), rows, L.ptr(w1), L.ptr(s1), L.ptr(b1), L.ptr(w2), L.ptr(s2), L.ptr(b2), L.ptr(w3), L.ptr(s3), L.ptr(b3),
                                  c3, int(group_rows), L.ptr(tap), L.ptr(out), x.shape[1] if x_f32 else 0, storage_math(math), L.stream())
    L.check(rc, 'dz_pointnet3_forward')
    return out, tap


def mlp_chain(x, la, lb, group_shift, group_rows, math, kv=None):
    """dz_mlp_chain_forward: x (rows, 128) pair16 through la = (w (512, 128) pair16, scale, shift) with the per-group pre-BatchNorm addend
    group_shift (groups, >= 512) and lb = (w (256, 512) pair16, scale, shift), both with ReLU -> memory (rows, 256) fp32; with
    kv = (wk (256, 256) pair16, bk, wv, bv) also the key / value projections of the memory -> (memory, k, v)."""
    lib = L.load()
    (wa, sa, ba), (wb, sb, bb) = la, lb
    L.require_cuda(x, wa, sa, ba, wb, sb, bb)
    rows = x.shape[0]
    if tuple(wa.shape) != (512, 128) or tuple(wb.shape) != (256, 512) or x.shape[1] != 128:
        raise L.DetZeroHipError('mlp_chain: expects 128 -> 512 -> 256 layers on (rows, 128) pair16 rows (got %s, %s on %s)' % (
            tuple(wa.shape), tuple(wb.shape), tuple(x.shape)))
    mem = torch.empty((rows, 256), dtype=torch.float32, device=x.device)
    k = v = wk = bk = wv = bv = None
    if kv is not None:
        wk, bk, wv, bv = kv
        if tuple(wk.shape) != (256, 256) or tuple(wv.shape) != (256, 256):
            raise L.DetZeroHipError('mlp_chain: key / value projections must be 256 -> 256')
        k, v = torch.empty_like(mem), torch.empty_like(mem)
    ldg = 0 if group_shift is None else group_shift.stride(0)
    rc = lib.dz_mlp_chain_forward(L.ptr(x), rows, L.ptr(wa), L.ptr(sa), L.ptr(ba), L.ptr(group_shift), ldg, int(group_rows), L.ptr(wb), L.ptr(sb), L.ptr(bb),
                                  L.ptr(wk), L.ptr(bk), L.ptr(wv), L.ptr(bv), L.ptr(mem), L.ptr(k), L.ptr(v), storage_math(math), L.stream())
    L.check(rc, 'dz_mlp_chain_forward')
    return (mem, k, v) if kv is not None else mem


def group_max(x, groups, length):
    """x (groups*length, c) -> (groups, c) max over each group's rows."""
    lib = L.load()
    L.require_cuda(x)
    c = x.shape[1]
    out = torch.empty((groups, c), dtype=torch.float32, device=x.device)
    rc = lib.dz_group_max(L.ptr(x), groups, length, c, L.ptr(out), L.stream())
    L.check(rc, 'dz_group_max')
    return out


def add_layernorm(x, y, gamma, beta, eps=1e-5, norm=True):
    """LayerNorm(x + y) (or x + y when norm=False) over the last dimension."""
    lib = L.load()
    L.require_cuda(x, y, gamma, beta)
    c = x.shape[-1]
    rows = x.numel() // c
    out = torch.empty_like(x)
    rc = lib.dz_add_layernorm(L.ptr(x), L.ptr(y), L.ptr(gamma), L.ptr(beta), rows, c, float(eps), 1 if norm else 0,
                              L.ptr(out), L.stream())
    L.check(rc, 'dz_add_layernorm')
    return out


def rows_all_zero(tensors):
    """(rows,) bool: every int of the row is zero in all of up to four (rows, w) int32 tensors."""
    lib = L.load()
    L.require_cuda(*tensors)
    ts = [t.contiguous() for t in tensors]
    rows = ts[0].shape[0]
    out = torch.empty((rows,), dtype=torch.uint8, device=ts[0].device)
    ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    ws = (ctypes.c_int * len(ts))(*[int(t.shape[1]) for t in ts])
    L.check(lib.dz_rows_all_zero(ptrs, ws, len(ts), rows, L.ptr(out), L.stream()), 'dz_rows_all_zero')
    return out.bool()


def add_layernorm_combine(x, y, gamma, beta, eps, post, group_skip, group_rows):
    """post + (group_skip[row // group_rows] ? post : LayerNorm(x + y)) in one pass (c = 192)."""
    lib = L.load()
    L.require_cuda(x, y, gamma, beta, post, group_skip)
    c = x.shape[-1]
    out = torch.empty_like(x)
    rc = lib.dz_add_layernorm_combine(L.ptr(x), L.ptr(y), L.ptr(gamma), L.ptr(beta), x.numel() // c, c, float(eps), L.ptr(post), L.ptr(group_skip),
                                      int(group_rows), L.ptr(out), L.stream())
    L.check(rc, 'dz_add_layernorm_combine')
    return out


# ------------------------------------------------------------------------------------------------
# head post-processing
# ------------------------------------------------------------------------------------------------
def centerhead_decode(head, h, w, ncls, k, score_thresh, limit6, pc_range, voxel_size, stride, use_iou=True):
    """head (B, H*W, 12) -> boxes (B,K,7), scores (B,K), labels (B,K) i32, counts (B,) i32 (device)."""
    lib = L.load()
    L.require_cuda(head)
    b = head.shape[0]
    dev = head.device
    boxes = torch.zeros((b, k, 7), dtype=torch.float32, device=dev)
    scores = torch.zeros((b, k), dtype=torch.float32, device=dev)
    labels = torch.zeros((b, k), dtype=torch.int32, device=dev)
    counts = torch.zeros((b,), dtype=torch.int32, device=dev)
    ws = _ws(lib.dz_centerhead_decode_workspace_bytes(b, h * w, ncls, k))
    rc = lib.dz_centerhead_decode(L.ptr(head), b, h, w, ncls, k, float(score_thresh), L.f6(limit6),
                                  L.f6(pc_range), L.f3(voxel_size), int(stride), 1 if use_iou else 0,
                                  L.ptr(boxes), L.ptr(scores), L.ptr(labels), L.ptr(counts), L.ptr(ws),
                                  ws.numel(), L.stream())
    L.check(rc, 'dz_centerhead_decode')
    return boxes, scores, labels, counts


def centerhead_select(head, h, w, ncls, k, use_iou=True):
    """First half of centerhead_decode: head (B, H*W, 12), columns 8:12 read -> (ws, cand, ncand).  ws is the decode workspace (hand it
    to centerhead_decode_selected); cand (B, 1024) int64 and ncand (B,) int32 are views of it: the min(K, ncls*HW) selected cells of a
    frame in descending score order as  score bits << 32 | ~(cls * HW + pix)."""
    lib = L.load()
    L.require_cuda(head)
    b = head.shape[0]
    ws = _ws(lib.dz_centerhead_decode_workspace_bytes(b, h * w, ncls, k))
    L.check(lib.dz_centerhead_select(L.ptr(head), b, h, w, ncls, k, 1 if use_iou else 0, L.ptr(ws), ws.numel(), L.stream()), 'dz_centerhead_select')
    o_list = lib.dz_centerhead_candidates_offset(b, h * w, ncls, k, 0)
    o_n = lib.dz_centerhead_candidates_offset(b, h * w, ncls, k, 1)
    cand = ws[o_list:o_list + b * CAND_STRIDE * 8].view(torch.int64).view(b, CAND_STRIDE)
    ncand = ws[o_n:o_n + b * 4].view(torch.int32)
    return ws, cand, ncand


def centerhead_decode_selected(head, h, w, ncls, k, score_thresh, limit6, pc_range, voxel_size, stride, ws):
    """Second half of centerhead_decode on the workspace of centerhead_select: columns 0:8 of head are read at the selected cells only.
    -> boxes (B,K,7), scores (B,K), labels (B,K) i32, counts (B,) i32 (device)."""
    lib = L.load()
    L.require_cuda(head, ws)
    b = head.shape[0]
    dev = head.device
    boxes = torch.zeros((b, k, 7), dtype=torch.float32, device=dev)
    scores = torch.zeros((b, k), dtype=torch.float32, device=dev)
    labels = torch.zeros((b, k), dtype=torch.int32, device=dev)
    counts = torch.zeros((b,), dtype=torch.int32, device=dev)
    rc = lib.dz_centerhead_decode_selected(L.ptr(head), b, h, w, ncls, k, float(score_thresh), L.f6(limit6), L.f6(pc_range), L.f3(voxel_size),
                                           int(stride), L.ptr(boxes), L.ptr(scores), L.ptr(labels), L.ptr(counts), L.ptr(ws), ws.numel(),
                                           L.stream())
    L.check(rc, 'dz_centerhead_decode_selected')
    return boxes, scores, labels, counts


CAND_STRIDE = 1024          # DZ_CENTERHEAD_CAND_STRIDE: candidate words per frame


def head_at_candidates_supported(math, channels):
    return bool(L.load().dz_head_at_candidates_supported(int(math), int(channels)))


def head_at_candidates(shared, cand, ncand, k, w1, s1, b1, w2, s2, b2, g_cout, g_ooff, head, math):
    """The regression branches of a CenterHead at candidate cells (dz_head_at_candidates): shared (B, H+2, W+2, 64) zero-bordered map of
    `math`, cand (B, stride) int64 / ncand (B,) int32 as centerhead_select leaves them, hidden weights whose first 64 * len(g_cout)
    output channels are the branches' - packed (9, cout, 64) in the split modes, (9, 64, cout) in fp32 - and the grouped output layer
    w2 (groups >= len(g_cout), 9, 32, 64), fp32: (groups, 9, 64, 16); writes columns g_ooff[g] .. + g_cout[g] of the candidates' rows
    of head (B, H*W, 12) in place."""
    lib = L.load()
    L.require_cuda(shared, cand, ncand, w1, s1, b1, w2, s2, b2, head)
    b, hp, wp, c = shared.shape
    nbr = len(g_cout)
    w1_cout = w1.shape[-2] if math else w1.shape[-1]
    if (c != 64 or head.shape != (b, (hp - 2) * (wp - 2), 12) or w1.shape[-1 if math else -2] != 64 or w2.shape[0] < nbr
            or tuple(w2.shape[1:]) != ((9, 32, 64) if math else (9, 64, 16))):
        raise L.DetZeroHipError('head_at_candidates: unexpected shapes')
    ia = (ctypes.c_int * 4)(*([int(v) for v in g_cout] + [0] * (4 - nbr)))
    io = (ctypes.c_int * 4)(*([int(v) for v in g_ooff] + [0] * (4 - nbr)))
    rc = lib.dz_head_at_candidates(L.ptr(shared), b, hp - 2, wp - 2, L.ptr(cand), L.ptr(ncand), cand.shape[1], int(k), L.ptr(w1), w1_cout,
                                   L.ptr(s1), L.ptr(b1), L.ptr(w2), L.ptr(s2), L.ptr(b2), nbr, ia, io, L.ptr(head), int(math), L.stream())
    L.check(rc, 'dz_head_at_candidates')
    return head


def nms_rotated_nosync(boxes_sorted, d_n, thresh, post_max):
    """boxes_sorted (n_cap,7) descending score; returns keep (n_cap,) i32, d_num_keep (1,) i32."""
    lib = L.load()
    L.require_cuda(boxes_sorted)
    n_cap = boxes_sorted.shape[0]
    keep = torch.zeros((max(n_cap, 1),), dtype=torch.int32, device=boxes_sorted.device)
    d_nk = torch.zeros((1,), dtype=torch.int32, device=boxes_sorted.device)
    ws = _ws(lib.dz_nms_workspace_bytes(n_cap))
    rc = lib.dz_nms_rotated(L.ptr(boxes_sorted), L.ptr(d_n), n_cap, float(thresh), int(post_max), L.ptr(keep),
                            L.ptr(d_nk), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, 'dz_nms_rotated')
    return keep, d_nk


def nms_rotated_batched_nosync(boxes_sorted, d_n, thresh, post_max):
    """boxes_sorted (B,n_cap,7) descending score per item, d_n (B,) -> keep (B,n_cap) i32, d_num_keep (B,) i32."""
    lib = L.load()
    L.require_cuda(boxes_sorted, d_n)
    b, n_cap = boxes_sorted.shape[0], boxes_sorted.shape[1]
    keep = torch.zeros((b, max(n_cap, 1)), dtype=torch.int32, device=boxes_sorted.device)
    d_nk = torch.zeros((b,), dtype=torch.int32, device=boxes_sorted.device)
    ws = _ws(b * lib.dz_nms_workspace_bytes(n_cap))
    rc = lib.dz_nms_rotated_batched(L.ptr(boxes_sorted), L.ptr(d_n), b, n_cap, float(thresh), int(post_max), L.ptr(keep),
                                    L.ptr(d_nk), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, 'dz_nms_rotated_batched')
    return keep, d_nk


def pack_detections(boxes, scores, labels, keep, d_nk, post_max):
    """(B,K,7),(B,K),(B,K) i32, keep (B,K) i32, d_nk (B,) -> (B,post_max,9) [box7|score|label+1], zero rows after."""
    lib = L.load()
    L.require_cuda(boxes, scores, labels, keep, d_nk)
    b, k = boxes.shape[0], boxes.shape[1]
    out = torch.empty((b, post_max, 9), dtype=torch.float32, device=boxes.device)
    rc = lib.dz_pack_detections(L.ptr(boxes), L.ptr(scores), L.ptr(labels), L.ptr(keep), L.ptr(d_nk), b, k, int(post_max),
                                L.ptr(out), L.stream())
    L.check(rc, 'dz_pack_detections')
    return out


def boxes_pairwise(a, b, iou):
    lib = L.load()
    L.require_cuda(a, b)
    out = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    fn = lib.dz_boxes_iou_bev if iou else lib.dz_boxes_overlap_bev
    rc = fn(L.ptr(a), a.shape[0], L.ptr(b), b.shape[0], L.ptr(out), L.stream())
    L.check(rc, 'dz_boxes_%s_bev' % ('iou' if iou else 'overlap'))
    return out


BOXM_UNION_BEV, BOXM_IOU3D, BOXM_GIOU3D, BOXM_GIOU3D_EXACT = 0, 1, 2, 3        # include/detzero_hip.h


def boxes_pairwise_metric(a, b, metric):
    """a (N,7), b (M,7) f32 -> (N,M) f32 of one of the BOXM_* metrics (one kernel, the final value per pair)."""
    lib = L.load()
    L.require_cuda(a, b)
    out = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    rc = lib.dz_boxes_pairwise_metric(L.ptr(a), a.shape[0], L.ptr(b), b.shape[0], int(metric), L.ptr(out), L.stream())
    L.check(rc, 'dz_boxes_pairwise_metric')
    return out


def boxes_paired_metric(a, b, metric):
    """a, b (N,7) f32 -> (N,) f32, out[i] = metric(a[i], b[i]): the diagonal of boxes_pairwise_metric, bit for bit, without the matrix."""
    lib = L.load()
    L.require_cuda(a, b)
    if a.shape != b.shape:
        raise L.DetZeroHipError('boxes_paired_metric: %s against %s boxes' % (tuple(a.shape), tuple(b.shape)))
    out = torch.empty((a.shape[0],), dtype=torch.float32, device=a.device)
    rc = lib.dz_boxes_paired_metric(L.ptr(a), L.ptr(b), a.shape[0], int(metric), L.ptr(out), L.stream())
    L.check(rc, 'dz_boxes_paired_metric')
    return out


def track_recall_iou3d_nosync(boxes_in, boxes_out, boxes_gt, mask, d_len, thresholds, want_iou=True):
    """Recall table of a batch of tracks (dz_track_recall_iou3d): boxes_* (B,T,7) f32, mask (B,T) uint8, d_len (B,) int32 device
    tensors, thresholds a host sequence of 1..8 numbers.  Returns (counts (B,2,n_thr+1) int32, iou_in, iou_out (B,T) f32 or None)
    on the device, nothing synchronised."""
    lib = L.load()
    L.require_cuda(boxes_in, boxes_out, boxes_gt, mask, d_len)
    b, t = boxes_in.shape[0], boxes_in.shape[1]
    for x in (boxes_in, boxes_out, boxes_gt):
        if tuple(x.shape) != (b, t, 7) or x.dtype != torch.float32:
            raise L.DetZeroHipError('track_recall_iou3d: boxes must be (B,T,7) float32, got %s %s' % (tuple(x.shape), x.dtype))
    if tuple(mask.shape) != (b, t) or mask.dtype != torch.uint8 or tuple(d_len.shape) != (b,) or d_len.dtype != torch.int32:
        raise L.DetZeroHipError('track_recall_iou3d: mask must be (B,T) uint8 and d_len (B,) int32')
    thr = (L.c_double * len(thresholds))(*[float(v) for v in thresholds])
    dev = boxes_in.device
    counts = torch.empty((b, 2, len(thresholds) + 1), dtype=torch.int32, device=dev)
    iou_in = torch.empty((b, t), dtype=torch.float32, device=dev) if want_iou else None
    iou_out = torch.empty((b, t), dtype=torch.float32, device=dev) if want_iou else None
    rc = lib.dz_track_recall_iou3d(L.ptr(boxes_in), L.ptr(boxes_out), L.ptr(boxes_gt), L.ptr(mask), L.ptr(d_len), b, t, thr,
                                   len(thresholds), L.ptr(iou_in), L.ptr(iou_out), L.ptr(counts), L.stream())
    L.check(rc, 'dz_track_recall_iou3d')
    return counts, iou_in, iou_out


def nms_normal_nosync(boxes_sorted, d_n, thresh, post_max):
    """Axis-aligned NMS (heading ignored): boxes_sorted (n_cap,7) descending score; returns keep (n_cap,) i32, d_num_keep (1,) i32."""
    lib = L.load()
    L.require_cuda(boxes_sorted)
    n_cap = boxes_sorted.shape[0]
    keep = torch.zeros((max(n_cap, 1),), dtype=torch.int32, device=boxes_sorted.device)
    d_nk = torch.zeros((1,), dtype=torch.int32, device=boxes_sorted.device)
    ws = _ws(lib.dz_nms_workspace_bytes(n_cap))
    rc = lib.dz_nms_normal(L.ptr(boxes_sorted), L.ptr(d_n), n_cap, float(thresh), int(post_max), L.ptr(keep),
                           L.ptr(d_nk), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, 'dz_nms_normal')
    return keep, d_nk


def nms_normal_batched_nosync(boxes_sorted, d_n, thresh, post_max):
    """boxes_sorted (B,n_cap,7) descending score per item, d_n (B,) -> keep (B,n_cap) i32, d_num_keep (B,) i32."""
    lib = L.load()
    L.require_cuda(boxes_sorted, d_n)
    b, n_cap = boxes_sorted.shape[0], boxes_sorted.shape[1]
    keep = torch.zeros((b, max(n_cap, 1)), dtype=torch.int32, device=boxes_sorted.device)
    d_nk = torch.zeros((b,), dtype=torch.int32, device=boxes_sorted.device)
    ws = _ws(b * lib.dz_nms_workspace_bytes(n_cap))
    rc = lib.dz_nms_normal_batched(L.ptr(boxes_sorted), L.ptr(d_n), b, n_cap, float(thresh), int(post_max), L.ptr(keep),
                                   L.ptr(d_nk), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, 'dz_nms_normal_batched')
    return keep, d_nk


def points_in_boxes_v2(points, boxes):
    """points (B,M,3), boxes (B,T,7) -> (B,T,M) i32."""
    lib = L.load()
    L.require_cuda(points, boxes)
    b, m, _ = points.shape
    t = boxes.shape[1]
    mask = torch.zeros((b, t, m), dtype=torch.int32, device=points.device)
    rc = lib.dz_points_in_boxes_v2(L.ptr(boxes), L.ptr(points), b, t, m, L.ptr(mask), L.stream())
    L.check(rc, 'dz_points_in_boxes_v2')
    return mask


def crop_points_in_boxes_nosync(xyz, boxes, payload, cap):
    """xyz (M,3) f32, boxes (T,7) f32, payload (M,W) any 4-byte-multiple dtype -> (out (cap,W) payload dtype, index (cap,) i32,
    offsets (T+1,) i32, d_total (1,) i32): the rows of the points inside box 0, then box 1, ... (ascending point index)."""
    lib = L.load()
    L.require_cuda(xyz, boxes, payload)
    m, t = xyz.shape[0], boxes.shape[0]
    words = payload.shape[1] * payload.element_size() // 4
    assert payload.shape[0] == m and payload.shape[1] * payload.element_size() % 4 == 0
    dev = xyz.device
    out = torch.empty((max(cap, 1), payload.shape[1]), dtype=payload.dtype, device=dev)
    index = torch.empty((max(cap, 1),), dtype=torch.int32, device=dev)
    offsets = torch.zeros((t + 1,), dtype=torch.int32, device=dev)
    d_total = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = _ws(lib.dz_crop_points_workspace_bytes(m, t, cap))
    rc = lib.dz_crop_points_in_boxes(L.ptr(xyz), m, L.ptr(boxes), t, L.ptr(payload), words, L.ptr(out), L.ptr(index), L.ptr(offsets),
                                     L.ptr(d_total), cap, L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, 'dz_crop_points_in_boxes')
    return out, index, offsets, d_total


def seq_crop_chunk_points():
    """Points per chunk of the sequence crop (one workgroup of dz_seq_crop_count / dz_seq_crop_fill)."""
    return int(L.load().dz_seq_crop_chunk_points())


class SeqCropPlan:
    """Checked geometry of one sequence crop (seq_crop_plan): host arrays, all int32.  `upload(device)` makes the device copies."""

    def __init__(self, m, nb, pt_off, box_off, rank, row_off, chunk_frame, chunk_first):
        self.m, self.nb, self.n_frames = int(m), int(nb), len(pt_off) - 1
        self.pt_off, self.box_off, self.rank, self.row_off = pt_off, box_off, rank, row_off
        self.chunk_frame, self.chunk_first = chunk_frame, chunk_first
        self.n_chunks, self.n_entries = int(chunk_frame.shape[0]), int(row_off[-1])
        self.dev = None

    def upload(self, device):
        if self.dev is None or self.dev[0] != device:
            names = ('pt_off', 'box_off', 'rank', 'row_off', 'chunk_frame', 'chunk_first')
            self.dev = (device, {k: torch.from_numpy(getattr(self, k)).to(device) for k in names})
        return self.dev[1]


def seq_crop_rank(rank, nb):
    """rank (or None for the identity) as a checked int64 permutation of 0..nb-1; DetZeroHipError otherwise."""
    if rank is None:
        return np.arange(nb, dtype=np.int64)
    rk = np.asarray(rank)
    if rk.ndim != 1 or rk.shape[0] != nb or rk.dtype.kind not in 'iu':
        raise L.DetZeroHipError('seq_crop: rank must be a 1-D integer array of %d entries' % nb)
    rk = rk.astype(np.int64)
    if nb and (rk.min() < 0 or rk.max() >= nb or (np.bincount(rk, minlength=nb) != 1).any()):
        raise L.DetZeroHipError('seq_crop: rank is not a permutation of 0..%d' % (nb - 1))
    return rk


def seq_crop_plan(pt_off, box_off, rank, m, nb, chunk=None):
    """Host side of the sequence crop: checks pt_off / box_off (F+1 ascending offsets from 0 to m / nb) and rank (a permutation of
    0..nb-1, or None for the identity), then lays out the chunks (`chunk` consecutive points of one frame that has boxes) and the count
    table (row rank[b] = one entry per chunk of box b's frame).  Raises DetZeroHipError on anything the kernels could not follow safely:
    nothing is launched from an unchecked array.  No device is touched (`chunk` defaults to the library's chunk size)."""
    def bad(msg):
        raise L.DetZeroHipError('seq_crop: ' + msg)
    m, nb = int(m), int(nb)
    if m < 0 or nb < 0:
        bad('negative size (m=%d, boxes=%d)' % (m, nb))
    if m >= 2 ** 31 or nb >= 2 ** 31:
        bad('%d points / %d boxes reach 2^31' % (m, nb))
    offs = []
    for name, off, end in (('pt_off', pt_off, m), ('box_off', box_off, nb)):
        o = np.asarray(off)
        if o.ndim != 1 or o.shape[0] < 1 or o.dtype.kind not in 'iu':
            bad('%s must be a 1-D integer array of F+1 entries' % name)
        o = o.astype(np.int64)
        if o[0] != 0 or (np.diff(o) < 0).any():
            bad('%s does not ascend from 0' % name)
        if o[-1] != end:
            bad('%s ends at %d, not at %d' % (name, o[-1], end))
        offs.append(o)
    p_off, b_off = offs
    if p_off.shape[0] != b_off.shape[0]:
        bad('pt_off has %d frames, box_off %d' % (p_off.shape[0] - 1, b_off.shape[0] - 1))
    nf = p_off.shape[0] - 1
    rk = seq_crop_rank(rank, nb)
    chunk = int(chunk) if chunk is not None else seq_crop_chunk_points()
    n_pts, n_box = np.diff(p_off), np.diff(b_off)
    nch = np.where(n_box > 0, (n_pts + chunk - 1) // chunk, 0)              # frames without boxes (or points) have no chunk
    chunk_first = np.zeros(nf + 1, dtype=np.int64)
    np.cumsum(nch, out=chunk_first[1:])
    frames = np.arange(nf, dtype=np.int64)
    row_len = np.zeros(nb, dtype=np.int64)
    row_len[rk] = np.repeat(nch, n_box)
    row_off = np.zeros(nb + 1, dtype=np.int64)
    np.cumsum(row_len, out=row_off[1:])
    if row_off[-1] >= 2 ** 31 or chunk_first[-1] >= 2 ** 31:
        bad('%d count-table entries / %d chunks reach 2^31: split the sequence' % (row_off[-1], chunk_first[-1]))
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return SeqCropPlan(m, nb, i32(p_off), i32(b_off), i32(rk), i32(row_off), i32(np.repeat(frames, nch)), i32(chunk_first))


def seq_crop(xyz, boxes, payload, plan, want_index=False):
    """xyz (M,3) f32, boxes (B,7) f32 (enlarged, frame-major), payload (M,W) of any 4-byte-multiple dtype, plan = seq_crop_plan(...)
    -> (out (total,W) payload dtype, index (total,) i32 or None, seg_off (B+1,) i32, total): the payload rows of the points inside
    each box, segment rank[b] after segment, ascending point index within a segment.  Two launches around one prefix (torch.cumsum);
    ONE host sync, for the total, and `out` is allocated exactly."""
    lib = L.load()
    L.require_cuda(xyz, boxes, payload)
    if not isinstance(plan, SeqCropPlan):
        raise L.DetZeroHipError('seq_crop: plan must come from seq_crop_plan')
    if xyz.dtype != torch.float32 or boxes.dtype != torch.float32 or xyz.dim() != 2 or boxes.dim() != 2 or payload.dim() != 2:
        raise L.DetZeroHipError('seq_crop: xyz (M,3) and boxes (B,7) must be float32, payload (M,W)')
    if tuple(xyz.shape) != (plan.m, 3) or tuple(boxes.shape) != (plan.nb, 7) or payload.shape[0] != plan.m:
        raise L.DetZeroHipError('seq_crop: %s points / %s boxes / %s payload rows do not match the plan (%d points, %d boxes)'
                                % (tuple(xyz.shape), tuple(boxes.shape), payload.shape[0], plan.m, plan.nb))
    row_bytes = payload.shape[1] * payload.element_size()
    if row_bytes == 0 or row_bytes % 4:
        raise L.DetZeroHipError('seq_crop: payload rows of %d bytes are no whole 32-bit words' % row_bytes)
    dev = xyz.device
    d = plan.upload(dev)
    geom = (L.ptr(xyz), plan.m, L.ptr(d['pt_off']), L.ptr(boxes), plan.nb, L.ptr(d['box_off']), L.ptr(d['rank']), L.ptr(d['row_off']),
            plan.n_frames, L.ptr(d['chunk_frame']), L.ptr(d['chunk_first']), plan.n_chunks)
    index = None
    if plan.n_entries == 0:
        out = torch.empty((0, payload.shape[1]), dtype=payload.dtype, device=dev)
        if want_index:
            index = torch.empty((0,), dtype=torch.int32, device=dev)
        return out, index, torch.zeros((plan.nb + 1,), dtype=torch.int32, device=dev), 0
    counts = torch.zeros((plan.n_entries,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.dz_seq_crop_count(*geom, L.ptr(counts), plan.n_entries, L.stream()), 'dz_seq_crop_count')
        incl = torch.cumsum(counts, 0, dtype=torch.int64)
        total = int(incl[-1].item())                                         # the one sync
        if total >= 2 ** 31:
            raise L.DetZeroHipError('seq_crop: %d kept rows reach 2^31: split the sequence' % total)
        prefix = (incl - counts).to(torch.int32)
        seg_off = torch.cat([prefix, incl[-1:].to(torch.int32)])[d['row_off'].long()].contiguous()
        out = torch.empty((total, payload.shape[1]), dtype=payload.dtype, device=dev)
        if want_index:
            index = torch.empty((total,), dtype=torch.int32, device=dev)
        L.check(lib.dz_seq_crop_fill(*geom, L.ptr(counts), L.ptr(prefix), plan.n_entries, L.ptr(payload), row_bytes // 4, L.ptr(out),
                                     L.ptr(index), total, L.stream()), 'dz_seq_crop_fill')
    return out, index, seg_off, total


ATTENTION_F32_ENGINES = ('mfma32', 'bf16x3')


def mha_core_limb3_supported(batch, lq, lk, heads):
    """Whether the bf16x3 engine of the f32 mode's attention core (dz_mha_core_limb3, csrc/mha_t.hip) takes a call of these sizes.
    Host only."""
    return bool(L.load().dz_mha_core_limb3_supported(int(batch), int(lq), int(lk), int(heads)))


def mha_core(q, k, v, key_padding_mask, heads, scale, math=0, f32_engine=None):
    """q (B,Lq,E), k/v (B,Lk,E), mask (B,Lk) bool/uint8 or None -> (B,Lq,E).  math 0: exact fp32 (dz_mha_core); 1 / 2: operands as
    16-bit pairs on the 16-bit matrix cores (dz_mha_core_split).  The split cores stay within their bound (tests/test_gpu_refine_kernels.py:
    8 x the host emulation of their roundings, 4.0e-3 / 3.2e-3 of sum_j p_j |v_j| for f16x2 / bf16x2) for logits (scale q.k) of standard
    deviation 2^-12 .. 2^8 and |v| of the order 2^-12 .. 2^8 in f16x2 (below |v| ~ 2^-4 the fp16 lo halves of v turn subnormal and the error
    grows from 2e-7 to 5e-5 at 2^-12; |q scale log2 e|, |k|, |v| beyond 65504 saturate) and for logits of standard deviation up to 2^4, any
    v, in bf16x2.  The refiner is well inside: with the synthetic weights on the golden inputs (tests/test_refine.py) its attention layers
    see logits of standard deviation 1.0 - 1.5 (largest 9) and |v| of median 0.6 - 0.8 (largest 5).
    f32_engine (math 0 only): None / 'mfma32' - the dz_mha_core call, word for word; 'bf16x3' - dz_mha_core_limb3 (csrc/mha_t.hip): q, k,
    v and the probabilities as three exact bf16 limbs, all six limb products of both matrix products on the bf16 matrix pipe, fp32
    accumulation and softmax.  It keeps dz_mha_core's own bound (8.0e-5 of sum_j p_j |v_j|, tests/test_gpu_mha_limb3.py) over the
    whole sweep, logits of standard deviation 2^-12 .. 2^8 and |v| of the order 2^-12 .. 2^8 (measured at (2, 40, 130): 2.5e-7 at every
    gain on v; on q.k 1.5e-7 .. 2.5e-7 up to 2^0, 4.8e-6 at 2^4 and 4.6e-5 at 2^8, where the float32 host evaluation is at 4.8e-5 itself); operands
    are clamped to +-3.39e38 (bf16 max) before the first limb only, so every finite fp32 value is carried exactly.  'bf16x3' with a
    split math, or an unknown name: DetZeroHipError."""
    if f32_engine not in (None,) + ATTENTION_F32_ENGINES:
        raise L.DetZeroHipError('unknown fp32 attention engine %r (%s)' % (f32_engine, ' | '.join(ATTENTION_F32_ENGINES)))
    if f32_engine == 'bf16x3' and math:
        raise L.DetZeroHipError('mha_core: f32_engine bf16x3 is an engine of the exact-fp32 mode (math 0), not of split math %r' % (math,))
    lib = L.load()
    L.require_cuda(q, k, v)
    b, lq, e = q.shape
    lk = k.shape[1]
    if e != heads * 32:
        raise L.DetZeroHipError('dz_mha_core supports head_dim 32 only (E=%d, heads=%d)' % (e, heads))
    m8 = None
    if key_padding_mask is not None:
        m8 = key_padding_mask.to(torch.uint8).contiguous()
    out = torch.empty_like(q)
    if math:
        rc = lib.dz_mha_core_split(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(m8), b, lq, lk, heads, float(scale), L.ptr(out), storage_math(math), L.stream())
        L.check(rc, 'dz_mha_core_split')
        return out
    if f32_engine == 'bf16x3':
        rc = lib.dz_mha_core_limb3(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(m8), b, lq, lk, heads, float(scale), L.ptr(out), L.stream())
        L.check(rc, 'dz_mha_core_limb3')
        return out
    rc = lib.dz_mha_core(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(m8), b, lq, lk, heads, float(scale), L.ptr(out),
                         L.stream())
    L.check(rc, 'dz_mha_core')
    return out


def roi_bev_features(boxes, bev_hwc, x_lo, y_lo, voxel_x, voxel_y, stride):
    """dz_roi_bev_features: boxes (n, 7) of one frame, bev_hwc (H, W, C) view with channel stride 1 -> (n, 5 * C) bilinear BEV features at
    the box centre and the four edge middles (center_head.py:408-432,461-486)."""
    lib = L.load()
    if not boxes.is_cuda or not bev_hwc.is_cuda or bev_hwc.stride(2) != 1:
        raise L.DetZeroHipError('roi_bev_features: device tensors, BEV map as an (H, W, C) view with contiguous channels')
    boxes = boxes.float().contiguous()
    n = boxes.shape[0]
    h, w, c = bev_hwc.shape
    out = torch.empty((n, 5 * c), dtype=torch.float32, device=boxes.device)
    rc = lib.dz_roi_bev_features(L.ptr(boxes), n, bev_hwc.data_ptr(), bev_hwc.stride(0), bev_hwc.stride(1), h, w, c, float(x_lo), float(y_lo), float(voxel_x),
                                 float(voxel_y), int(stride), L.ptr(out), L.stream())
    L.check(rc, 'dz_roi_bev_features')
    return out


def xattn_folded_supported(lq, e, heads):
    return bool(L.load().dz_xattn_folded_supported(int(lq), int(e), int(heads)))


def xattn_folded(q, mem, key_padding_mask, wk_oi, wv_io, bv, heads, scale):
    """dz_xattn_folded: q (B,Lq,E) projected queries, mem (B,Lk,E) RAW memory rows, wk_oi = Wk (out, in), wv_io = Wv^T (in, out), bv (E)
    -> (B,Lq,E) attention output before out_proj; the key / value projections of the memory are never formed."""
    lib = L.load()
    L.require_cuda(q, mem, wk_oi, wv_io, bv)
    b, lq, e = q.shape
    lk = mem.shape[1]
    m8 = None if key_padding_mask is None else key_padding_mask.to(torch.uint8).contiguous()
    nbytes = lib.dz_xattn_folded_workspace_bytes(b, lk)
    ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=q.device)
    out = torch.empty_like(q)
    rc = lib.dz_xattn_folded(L.ptr(q), L.ptr(mem), L.ptr(m8), L.ptr(wk_oi), L.ptr(wv_io), L.ptr(bv), b, lq, lk, e, int(heads), float(scale),
                             L.ptr(ws), nbytes, L.ptr(out), L.stream())
    L.check(rc, 'dz_xattn_folded')
    return out


# ------------------------------------------------------------------------------------------------
# per-launch profiling hook (bench.py): HIP events on the stream the kernels are launched on
# ------------------------------------------------------------------------------------------------
class LaunchProfiler:
    """When installed (``ops.PROFILER = LaunchProfiler()``), every dz_conv2d_forward / dz_spconv_forward
    call is bracketed by a pair of timing events recorded on the launch stream; ``summary()`` returns
    per-kernel-variant launch counts, total device time and algorithmic FLOPs / bytes."""

    def __init__(self):
        self.records = []

    def wrap(self, name, flops, nbytes, fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        st = torch.cuda.current_stream()
        e0.record(st)
        fn()
        e1.record(st)
        self.records.append((name, flops, nbytes, e0, e1))

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for name, flops, nbytes, e0, e1 in self.records:
            a = agg.setdefault(name, {'launches': 0, 'ms': 0.0, 'flops': 0.0, 'bytes': 0.0})
            a['launches'] += 1
            a['ms'] += e0.elapsed_time(e1)
            a['flops'] += flops
            a['bytes'] += nbytes
        return agg


# ------------------------------------------------------------------------------------------------
# tracker (csrc/track.hip): a device-resident track table of one sequence and the seven per-frame ops on it
# ------------------------------------------------------------------------------------------------
TRACK_ROW_WORDS = 16                 # include/detzero_hip.h: DZ_TRACK_ROW_WORDS
TRACK_AFF_IOU_BEV = 16               # DZ_TRACK_AFF_IOU_BEV; the other two affinity metrics are BOXM_IOU3D / BOXM_GIOU3D
TRACK_MAX_CLASSES = 8
_TRACK_FIELDS = (('x', 5, torch.float32), ('P', 25, torch.float32), ('Q', 25, torch.float32), ('dt', 1, torch.float32),
                 ('box', 9, torch.float32), ('cls', 1, torch.int32), ('score', 1, torch.float32), ('update_score', 1, torch.float32),
                 ('num_points', 1, torch.int32), ('hit', 1, torch.int32), ('miss', 1, torch.int32), ('id', 1, torch.int32))


class TrackTable:
    """Struct of arrays of ``cap`` tracks on the device (``dz_track_table``); rows [0, n) are live, n is kept by the caller."""

    def __init__(self, cap, device=None):
        self.cap = int(cap)
        self.device = torch.device(device) if device is not None else _dev()
        self.arrays = {name: torch.zeros((self.cap, w) if w > 1 else (self.cap,), dtype=dt, device=self.device) for name, w, dt in _TRACK_FIELDS}
        self.c = L.TrackTable(*[L.ptr(self.arrays[name]) for name, _, _ in _TRACK_FIELDS], self.cap)

    def __getattr__(self, name):
        try:
            return self.__dict__['arrays'][name]
        except KeyError:
            raise AttributeError(name)

    def grown(self, n, need):
        """This table if ``need`` rows fit, else a new one of at least twice the capacity holding rows [0, n)."""
        if need <= self.cap:
            return self
        cap = self.cap
        while cap < need:
            cap *= 2
        new = TrackTable(cap, self.device)
        for name in self.arrays:
            new.arrays[name][:n].copy_(self.arrays[name][:n])
        return new


def _track_rows(buf, what):
    if buf is None:
        return None, 0
    L.require_cuda(buf)
    if buf.dtype != torch.int32 or buf.dim() != 2 or buf.shape[1] != TRACK_ROW_WORDS:
        raise L.DetZeroHipError('%s: a row buffer is (rows, %d) int32, got %s %s' % (what, TRACK_ROW_WORDS, tuple(buf.shape), buf.dtype))
    return buf, buf.shape[0]


def _track_idx(idx, what):
    L.require_cuda(idx)
    if idx.dtype != torch.int32 or idx.dim() != 1:
        raise L.DetZeroHipError('%s: an index list is a 1-d int32 device tensor' % what)
    return idx


def _track_thr(thr):
    return (L.c_float * len(thr))(*[float(v) for v in thr])


def track_predict_nosync(table, n, gate_class):
    """KalmanFilter.predict on rows [0, n) in place; table.box[:n] are the predicted boxes."""
    L.check(L.load().dz_track_predict(ctypes.byref(table.c), int(n), int(gate_class), L.stream()), 'dz_track_predict')


def track_affinity_nosync(table, n, ext, row_idx, det, col_idx, metric, distinguish_class, thr):
    """Cost matrix (len(row_idx), len(col_idx)) f32 of one association stage (dz_track_affinity)."""
    ext, n_ext = _track_rows(ext, 'track_affinity')
    det, n_det = _track_rows(det, 'track_affinity')
    row_idx, col_idx = _track_idx(row_idx, 'track_affinity'), _track_idx(col_idx, 'track_affinity')
    out = torch.empty((row_idx.shape[0], col_idx.shape[0]), dtype=torch.float32, device=row_idx.device)
    rc = L.load().dz_track_affinity(ctypes.byref(table.c), int(n), L.ptr(ext), n_ext, L.ptr(row_idx), row_idx.shape[0], L.ptr(det), n_det,
                                    L.ptr(col_idx), col_idx.shape[0], int(metric), int(bool(distinguish_class)), _track_thr(thr), len(thr),
                                    L.ptr(out), L.stream())
    L.check(rc, 'dz_track_affinity')
    return out


def track_update_nosync(table, n, det, match, r):
    """KalmanFilter.update for match (m,3) int32 rows [table row, det row, stage]."""
    det, n_det = _track_rows(det, 'track_update')
    L.require_cuda(match)
    if match.dtype != torch.int32 or match.dim() != 2 or match.shape[1] != 3:
        raise L.DetZeroHipError('track_update: match is (m, 3) int32')
    L.check(L.load().dz_track_update(ctypes.byref(table.c), int(n), L.ptr(det), n_det, L.ptr(match), match.shape[0], float(r), L.stream()),
            'dz_track_update')


def track_spawn_nosync(table, n, src, src_idx, ids, p, q, dt):
    """Append len(src_idx) tracks at rows [n, n + m) from rows of the row buffer ``src``; p, q = the constructor's (p0, p1), (q0, q1)."""
    src, n_src = _track_rows(src, 'track_spawn')
    src_idx, ids = _track_idx(src_idx, 'track_spawn'), _track_idx(ids, 'track_spawn')
    if ids.shape[0] != src_idx.shape[0] or n + src_idx.shape[0] > table.cap:
        raise L.DetZeroHipError('track_spawn: %d ids for %d rows, %d + %d rows in a table of %d' % (ids.shape[0], src_idx.shape[0], n, src_idx.shape[0], table.cap))
    rc = L.load().dz_track_spawn(ctypes.byref(table.c), int(n), L.ptr(src), n_src, L.ptr(src_idx), L.ptr(ids), src_idx.shape[0], float(p[0]),
                                 float(p[1]), float(q[0]), float(q[1]), float(dt), L.stream())
    L.check(rc, 'dz_track_spawn')


def track_merge_nosync(table, n, thr):
    """overlap_track_merge's verdicts: removed (n,) int32 0 / 1 on the device."""
    lib = L.load()
    removed = torch.empty((max(int(n), 1),), dtype=torch.int32, device=table.device)
    ws = _ws(lib.dz_track_merge_workspace_bytes(int(n)))
    rc = lib.dz_track_merge(ctypes.byref(table.c), int(n), _track_thr(thr), len(thr), L.ptr(removed), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, 'dz_track_merge')
    return removed[:n]


def track_compact_nosync(src, n, removed, death_age, dst):
    """Stable removal into ``dst`` (another TrackTable); returns the new count as a (1,) int32 device tensor."""
    if removed is not None:
        L.require_cuda(removed)
        if removed.dtype != torch.int32 or removed.shape[0] < n:
            raise L.DetZeroHipError('track_compact: removed is (n,) int32')
    d_count = torch.empty((1,), dtype=torch.int32, device=src.device)
    rc = L.load().dz_track_compact(ctypes.byref(src.c), int(n), L.ptr(removed), int(death_age), ctypes.byref(dst.c), L.ptr(d_count), L.stream())
    L.check(rc, 'dz_track_compact')
    return d_count


def track_log_nosync(table, n, frame, log, log_n):
    """info() of rows [0, n) into rows [log_n, log_n + n) of the row buffer ``log``."""
    log, rows = _track_rows(log, 'track_log')
    if log_n + n > rows:
        raise L.DetZeroHipError('track_log: rows %d..%d of a log of %d' % (log_n, log_n + n, rows))
    L.check(L.load().dz_track_log(ctypes.byref(table.c), int(n), int(frame), L.ptr(log), int(log_n), L.stream()), 'dz_track_log')


# ------------------------------------------------------------------------------------------------
# the AB3DMOT filter on the same table (csrc/track_ab3dmot.h): float64 state in a companion of the track table
# ------------------------------------------------------------------------------------------------
TRACK_FILTER_KALMAN, TRACK_FILTER_AB3DMOT = 0, 1     # DZ_TRACK_FILTER_*
TRACK_AB3D_WORK = 170                                # DZ_TRACK_AB3D_WORK
TRACK_AB3D_ROW_DROP, TRACK_AB3D_ROW_BIRTH = 1, 2     # word 15 of a log row
_AB3D_FIELDS = (('x', 10, torch.float64), ('P', 100, torch.float64), ('box', 9, torch.float64), ('work', TRACK_AB3D_WORK, torch.float64),
                ('hits', 1, torch.int32))


class TrackAb3dTable:
    """``dz_track_ab3d``: the float64 companion of a TrackTable of the same capacity.  The arrays are (width, cap) - the track index
    is the fastest one; ``x[:, i]`` is the state of track i, ``P[:, i].reshape(10, 10)`` its covariance."""

    def __init__(self, cap, device=None):
        self.cap = int(cap)
        self.device = torch.device(device) if device is not None else _dev()
        self.arrays = {name: torch.zeros((w, self.cap) if w > 1 else (self.cap,), dtype=dt, device=self.device) for name, w, dt in _AB3D_FIELDS}
        self.c = L.TrackAb3d(*[L.ptr(self.arrays[name]) for name, _, _ in _AB3D_FIELDS], self.cap)

    def __getattr__(self, name):
        try:
            return self.__dict__['arrays'][name]
        except KeyError:
            raise AttributeError(name)

    def grown(self, n, need):
        """This companion if ``need`` rows fit, else a new one of at least twice the capacity holding rows [0, n)."""
        if need <= self.cap:
            return self
        cap = self.cap
        while cap < need:
            cap *= 2
        new = TrackAb3dTable(cap, self.device)
        for name in ('x', 'P', 'box', 'hits'):
            new.arrays[name][..., :n].copy_(self.arrays[name][..., :n])
        return new


def _track_f64(a, rows, width, what):
    L.require_cuda(a)
    if a.dtype != torch.float64 or a.dim() != 2 or a.shape[1] != width or a.shape[0] < rows or not a.is_contiguous():
        raise L.DetZeroHipError('%s: a contiguous (>= %d, %d) float64 device tensor, got %s %s' % (what, rows, width, tuple(a.shape), a.dtype))
    return a


def _ab3d_pair(table, ab, rows, what):
    if ab.cap < rows or table.cap < rows:
        raise L.DetZeroHipError('%s: %d rows in a table of %d / a companion of %d' % (what, rows, table.cap, ab.cap))


def track_ab3d_predict_nosync(table, ab, n):
    """AB3DMOT.predict on rows [0, n) in place; table.box[:n] = the float32 rounding of the predicted boxes."""
    _ab3d_pair(table, ab, n, 'track_ab3d_predict')
    L.check(L.load().dz_track_ab3d_predict(ctypes.byref(table.c), ctypes.byref(ab.c), int(n), L.stream()), 'dz_track_ab3d_predict')


def track_ab3d_update_nosync(table, ab, n, det, det64, match):
    """AB3DMOT.update for match (m,3) int32 rows [table row, det row, stage (ignored)]; det64 (D,7) float64 = the measurements."""
    det, n_det = _track_rows(det, 'track_ab3d_update')
    _ab3d_pair(table, ab, n, 'track_ab3d_update')
    L.require_cuda(match)
    if match.dtype != torch.int32 or match.dim() != 2 or match.shape[1] != 3:
        raise L.DetZeroHipError('track_ab3d_update: match is (m, 3) int32')
    det64 = _track_f64(det64, n_det, 7, 'track_ab3d_update: det64')
    rc = L.load().dz_track_ab3d_update(ctypes.byref(table.c), ctypes.byref(ab.c), int(n), L.ptr(det), L.ptr(det64), n_det, L.ptr(match),
                                       match.shape[0], L.stream())
    L.check(rc, 'dz_track_ab3d_update')


def track_ab3d_spawn_nosync(table, ab, n, src, src64, src_idx, ids):
    """Append len(src_idx) AB3DMOT tracks at rows [n, n + m) from rows of the row buffer ``src`` and their measurements ``src64``."""
    src, n_src = _track_rows(src, 'track_ab3d_spawn')
    src_idx, ids = _track_idx(src_idx, 'track_ab3d_spawn'), _track_idx(ids, 'track_ab3d_spawn')
    if ids.shape[0] != src_idx.shape[0]:
        raise L.DetZeroHipError('track_ab3d_spawn: %d ids for %d rows' % (ids.shape[0], src_idx.shape[0]))
    _ab3d_pair(table, ab, n + src_idx.shape[0], 'track_ab3d_spawn')
    src64 = _track_f64(src64, n_src, 7, 'track_ab3d_spawn: src64')
    rc = L.load().dz_track_ab3d_spawn(ctypes.byref(table.c), ctypes.byref(ab.c), int(n), L.ptr(src), L.ptr(src64), n_src, L.ptr(src_idx),
                                      L.ptr(ids), src_idx.shape[0], L.stream())
    L.check(rc, 'dz_track_ab3d_spawn')


def track_ab3d_compact_nosync(src, asrc, n, removed, death_age, dst, adst):
    """track_compact_nosync carrying the companion: survivors into (dst, adst); returns the new count as a (1,) int32 device tensor."""
    if removed is not None:
        L.require_cuda(removed)
        if removed.dtype != torch.int32 or removed.shape[0] < n:
            raise L.DetZeroHipError('track_ab3d_compact: removed is (n,) int32')
    _ab3d_pair(src, asrc, n, 'track_ab3d_compact')
    _ab3d_pair(dst, adst, n, 'track_ab3d_compact')
    d_count = torch.empty((1,), dtype=torch.int32, device=src.device)
    rc = L.load().dz_track_ab3d_compact(ctypes.byref(src.c), ctypes.byref(asrc.c), int(n), L.ptr(removed), int(death_age), ctypes.byref(dst.c),
                                        ctypes.byref(adst.c), L.ptr(d_count), L.stream())
    L.check(rc, 'dz_track_ab3d_compact')
    return d_count


def track_ab3d_log_nosync(table, ab, n, frame, frame_id, birth_age, death_age, log, log64, log_n):
    """info() of rows [0, n) into rows [log_n, log_n + n) of the row buffer ``log`` and of ``log64`` (rows, 9) float64; word 15 of a
    row carries the output rule's verdict (TRACK_AB3D_ROW_DROP) and the birth flag (TRACK_AB3D_ROW_BIRTH)."""
    log, rows = _track_rows(log, 'track_ab3d_log')
    if log_n + n > rows:
        raise L.DetZeroHipError('track_ab3d_log: rows %d..%d of a log of %d' % (log_n, log_n + n, rows))
    _ab3d_pair(table, ab, n, 'track_ab3d_log')
    log64 = _track_f64(log64, log_n + n, 9, 'track_ab3d_log: log64')
    rc = L.load().dz_track_ab3d_log(ctypes.byref(table.c), ctypes.byref(ab.c), int(n), int(frame), int(frame_id), int(birth_age),
                                    int(death_age), L.ptr(log), L.ptr(log64), int(log_n), L.stream())
    L.check(rc, 'dz_track_ab3d_log')


# ------------------------------------------------------------------------------------------------
# trajectory-pair table (csrc/traj_pair.hip): ground-truth trajectories against tracks over a whole sequence
# ------------------------------------------------------------------------------------------------
def _traj_sides(a_box, a_cls, a_slot, b_box, b_cls, b_slot, n_cls, what):
    """Shapes, dtypes and - one host read for both sides - the index ranges: a slot outside [-1, rows) or a ground-truth class
    outside the threshold table is refused here, before any launch.  -> (n_a, a_rows, n_b, b_rows, n_frames)."""
    L.require_cuda(a_box, a_cls, a_slot, b_box, b_cls, b_slot)
    for box, cls, slot, side in ((a_box, a_cls, a_slot, 'a'), (b_box, b_cls, b_slot, 'b')):
        if box.dtype != torch.float32 or box.dim() != 2 or box.shape[1] != 7:
            raise L.DetZeroHipError('%s: %s_box is (rows, 7) float32, got %s %s' % (what, side, tuple(box.shape), box.dtype))
        if cls.dtype != torch.int32 or cls.dim() != 1 or cls.shape[0] != box.shape[0]:
            raise L.DetZeroHipError('%s: %s_cls is (rows,) int32, one per box' % (what, side))
        if slot.dtype != torch.int32 or slot.dim() != 2:
            raise L.DetZeroHipError('%s: %s_slot is (n_frames, n) int32' % (what, side))
    if a_slot.shape[0] != b_slot.shape[0]:
        raise L.DetZeroHipError('%s: %d frames on side a, %d on side b' % (what, a_slot.shape[0], b_slot.shape[0]))
    probes, names = [], []
    for t, name, hi in ((a_slot, 'a_slot', a_box.shape[0]), (b_slot, 'b_slot', b_box.shape[0]), (a_cls, 'a_cls', n_cls)):
        if t.numel():
            probes += [t.min(), t.max()]
            names.append((name, -1 if name != 'a_cls' else 0, hi))
    if probes:
        seen = torch.stack(probes).cpu().tolist()
        for k, (name, lo, hi) in enumerate(names):
            if seen[2 * k] < lo or seen[2 * k + 1] >= hi:
                raise L.DetZeroHipError('%s: %s holds %d..%d, outside [%d, %d)' % (what, name, seen[2 * k], seen[2 * k + 1], lo, hi))
    return a_slot.shape[1], a_box.shape[0], b_slot.shape[1], b_box.shape[0], a_slot.shape[0]


def _traj_metric(metric, what):
    if int(metric) not in (TRACK_AFF_IOU_BEV, BOXM_IOU3D):
        raise L.DetZeroHipError('%s: metric %s (TRACK_AFF_IOU_BEV or BOXM_IOU3D)' % (what, metric))
    return int(metric)


def traj_pair_table(a_box, a_cls, a_slot, b_box, b_cls, b_slot, metric, distinguish_class, thr):
    """dz_traj_pair_table: a = ground-truth trajectories, b = tracks; *_box (rows,7) f32, *_cls (rows,) i32, *_slot (n_frames, n) i32
    frame-major, -1 = no box at that frame.  -> (sum_all, sum_hit) f32, (n_hit, n_same) i32, each (n_a, n_b), on the device."""
    metric = _traj_metric(metric, 'traj_pair_table')
    thr = [float(v) for v in thr]
    if not 1 <= len(thr) <= TRACK_MAX_CLASSES or not all(v > 0 for v in thr):
        raise L.DetZeroHipError('traj_pair_table: thresholds %s (1..%d of them, every one > 0)' % (thr, TRACK_MAX_CLASSES))
    n_a, a_rows, n_b, b_rows, n_frames = _traj_sides(a_box, a_cls, a_slot, b_box, b_cls, b_slot, len(thr), 'traj_pair_table')
    dev = a_box.device
    sums = torch.zeros((2, n_a, n_b), dtype=torch.float32, device=dev)
    counts = torch.zeros((2, n_a, n_b), dtype=torch.int32, device=dev)
    rc = L.load().dz_traj_pair_table(L.ptr(a_box), L.ptr(a_cls), L.ptr(a_slot), n_a, a_rows, L.ptr(b_box), L.ptr(b_cls), L.ptr(b_slot), n_b,
                                     b_rows, n_frames, metric, int(bool(distinguish_class)), _track_thr(thr), len(thr), L.ptr(sums[0]),
                                     L.ptr(sums[1]), L.ptr(counts[0]), L.ptr(counts[1]), L.stream())
    L.check(rc, 'dz_traj_pair_table')
    return sums[0], sums[1], counts[0], counts[1]


def traj_pair_rows(a_box, a_cls, a_slot, b_box, b_cls, b_slot, metric, distinguish_class, pairs):
    """dz_traj_pair_rows: pairs (n_pairs,2) i32 device [trajectory, track] -> (n_pairs, n_frames) f32, the class-masked per-frame
    value at the frames a pair shares, 0 elsewhere."""
    metric = _traj_metric(metric, 'traj_pair_rows')
    n_a, a_rows, n_b, b_rows, n_frames = _traj_sides(a_box, a_cls, a_slot, b_box, b_cls, b_slot, TRACK_MAX_CLASSES, 'traj_pair_rows')
    L.require_cuda(pairs)
    if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise L.DetZeroHipError('traj_pair_rows: pairs is (n_pairs, 2) int32')
    n_pairs = pairs.shape[0]
    rows = torch.zeros((n_pairs, n_frames), dtype=torch.float32, device=a_box.device)
    if n_pairs:
        lo, hi = torch.stack([pairs.min(dim=0).values, pairs.max(dim=0).values]).cpu().tolist()
        if min(lo) < 0 or hi[0] >= n_a or hi[1] >= n_b:
            raise L.DetZeroHipError('traj_pair_rows: a pair outside the %d x %d table' % (n_a, n_b))
    rc = L.load().dz_traj_pair_rows(L.ptr(a_box), L.ptr(a_cls), L.ptr(a_slot), n_a, a_rows, L.ptr(b_box), L.ptr(b_cls), L.ptr(b_slot), n_b,
                                    b_rows, n_frames, metric, int(bool(distinguish_class)), L.ptr(pairs), n_pairs, L.ptr(rows), L.stream())
    L.check(rc, 'dz_traj_pair_rows')
    return rows


# ------------------------------------------------------------------------------------------------
# a pass of a batch of sequences in one launch (csrc/track_seq.hip)
# ------------------------------------------------------------------------------------------------
TRACK_SEQ_MAX_TRACKS = 4096          # DZ_TRACK_SEQ_MAX_TRACKS
TRACK_SEQ_MAX_DET = 1024             # DZ_TRACK_SEQ_MAX_DET
TRACK_SEQ_OVF_TRACKS, TRACK_SEQ_OVF_LOG, TRACK_SEQ_OVF_LSA, TRACK_SEQ_OVF_DESC = 1, 2, 4, 8


def track_seq_params(metric, distinguish_class, gate_class, n_cls, two_stage, merge_enable, death_age, init_track_id, thr_first, thr_second,
                     thr_merge, p, q, r, dt, filter=TRACK_FILTER_KALMAN, birth_age=1):
    """``dz_track_seq_params`` from the tracker's configuration (threshold lists may be shorter than 8 or None)."""
    def thr(v):
        v = [float(x) for x in (v if v is not None else [])][:TRACK_MAX_CLASSES]
        return L._F8(*(v + [0.] * (TRACK_MAX_CLASSES - len(v))))
    return L.TrackSeqParams(int(metric), int(bool(distinguish_class)), int(gate_class), int(n_cls), int(bool(two_stage)), int(bool(merge_enable)),
                            int(death_age), int(init_track_id), thr(thr_first), thr(thr_second), thr(thr_merge), float(p[0]), float(p[1]),
                            float(q[0]), float(q[1]), float(r), float(dt), int(filter), int(birth_age))


def _seq_i32(t, n, what):
    if t is None:
        if n:
            raise L.DetZeroHipError('track_seq_pass: %s is missing' % what)
        return None
    L.require_cuda(t)
    if t.dtype != torch.int32 or t.numel() < n:
        raise L.DetZeroHipError('track_seq_pass: %s is int32 with at least %d entries, got %s %s' % (what, n, tuple(t.shape), t.dtype))
    return t


def track_seq_pass_nosync(params, det, det_flags, frame_row, seq_frame, track_cap, row_cap, det_cap, log_cap, reverse=None, ab3d=None):
    """One pass (forward, or reverse when ``reverse`` = (ext (S, ext_cap, 16), ext_count (S,), going_at, going_idx, start_at,
    start_idx)) of every sequence in one launch.  det (rows, 16) i32, det_flags (rows,), frame_row (frames + 1,), seq_frame (S + 1,)
    on the device.  -> (log (S, log_cap, 16) i32, log_count (S,) i32, overflow (S,) i32) on the device; nothing is read here.
    With params.filter = TRACK_FILTER_AB3DMOT: ``ab3d`` = (det64 (rows, 7) f64, frame_id (frames,) i32) on the device, and a fourth
    result, log64 (S, log_cap, 9) f64."""
    lib = L.load()
    det, n_rows = _track_rows(det, 'track_seq_pass')
    n_seq, n_frames = seq_frame.shape[0] - 1, frame_row.shape[0] - 1
    _seq_i32(det_flags, n_rows, 'det_flags'), _seq_i32(frame_row, 1, 'frame_row'), _seq_i32(seq_frame, 1, 'seq_frame')
    dev = det.device
    io = L.TrackSeqIO(L.ptr(det), L.ptr(det_flags), L.ptr(frame_row), L.ptr(seq_frame), n_seq, n_frames, n_rows, int(track_cap), int(row_cap),
                      int(det_cap), int(log_cap))
    if reverse is not None:
        ext, ext_count, going_at, going_idx, start_at, start_idx = reverse
        L.require_cuda(ext)
        if ext.dtype != torch.int32 or ext.dim() != 3 or ext.shape[0] != n_seq or ext.shape[2] != TRACK_ROW_WORDS:
            raise L.DetZeroHipError('track_seq_pass: ext is (%d, ext_cap, %d) int32, got %s' % (n_seq, TRACK_ROW_WORDS, tuple(ext.shape)))
        _seq_i32(ext_count, n_seq, 'ext_count'), _seq_i32(going_at, n_frames + 1, 'going_at'), _seq_i32(start_at, n_frames + 1, 'start_at')
        io.ext, io.ext_count, io.going_at, io.start_at = L.ptr(ext), L.ptr(ext_count), L.ptr(going_at), L.ptr(start_at)
        io.going_idx, io.start_idx = L.ptr(_seq_i32(going_idx, 0, 'going_idx')), L.ptr(_seq_i32(start_idx, 0, 'start_idx'))
        io.ext_cap, io.n_going, io.n_start = ext.shape[1], going_idx.numel(), start_idx.numel()
    tables = TrackTable(max(n_seq * 2 * int(track_cap), 1), dev)
    log64 = None
    if params.filter == TRACK_FILTER_AB3DMOT:
        if ab3d is None or reverse is not None:
            raise L.DetZeroHipError('track_seq_pass: the AB3DMOT filter needs (det64, frame_id) and has no reverse pass')
        det64, frame_id = ab3d
        companion = TrackAb3dTable(tables.cap, dev)
        log64 = torch.empty((max(n_seq, 1), max(int(log_cap), 1), 9), dtype=torch.float64, device=dev)
        io.det64 = L.ptr(_track_f64(det64, n_rows, 7, 'track_seq_pass: det64')) if n_rows else None
        io.frame_id, io.log64, io.ab3d = L.ptr(_seq_i32(frame_id, n_frames, 'frame_id')), L.ptr(log64), companion.c
    log = torch.empty((max(n_seq, 1), max(int(log_cap), 1), TRACK_ROW_WORDS), dtype=torch.int32, device=dev)     # rows below log_count are written
    state = torch.zeros((2, max(n_seq, 1)), dtype=torch.int32, device=dev)
    ws = _ws(lib.dz_track_seq_ws_bytes(n_seq, int(track_cap), int(row_cap), int(det_cap)))
    rc = lib.dz_track_seq_pass(ctypes.byref(params), ctypes.byref(io), 0 if reverse is None else 1, ctypes.byref(tables.c), L.ptr(log),
                               L.ptr(state[0]), L.ptr(state[1]), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, 'dz_track_seq_pass')
    if log64 is not None:
        return log[:n_seq], state[0, :n_seq], state[1, :n_seq], log64[:n_seq]
    return log[:n_seq], state[0, :n_seq], state[1, :n_seq]


# ------------------------------------------------------------------------------------------------
# linear sum assignment (csrc/lsa.h, csrc/lsa.hip): GNN_assignment for a batch of problems, one workgroup each
# ------------------------------------------------------------------------------------------------
LSA_MAX_DIM = 4096                 # DZ_LSA_MAX_DIM
LSA_STATUS = {1: 'no finite cost left (NaN costs)', 2: 'a loop bound was reached', 3: 'descriptor outside its buffers'}


def linear_assignment_batch_nosync(cost, shapes, threshold=1.):
    """cost: 1-d float32 device tensor, the row-major matrices of ``shapes`` = [(rows, cols), ...] back to back.
    -> (row_to_col (sum rows,) i32, unmatched_rows (sum rows,) i32, unmatched_cols (sum cols,) i32, counts (P,4) i32
    [matched, unmatched rows, unmatched cols, status]) on the device and the host lists (row_off, col_off) of each problem's
    offsets.  No host read: the caller looks at counts[:, 3] when it reads the results."""
    lib = L.load()
    L.require_cuda(cost)
    if cost.dtype != torch.float32 or cost.dim() != 1:
        raise L.DetZeroHipError('linear_assignment_batch: cost is a 1-d float32 device tensor, got %s %s' % (tuple(cost.shape), cost.dtype))
    shapes = [(int(r), int(c)) for r, c in shapes]
    if any(r < 0 or c < 0 for r, c in shapes):
        raise L.DetZeroHipError('linear_assignment_batch: negative shape in %s' % (shapes,))
    desc = np.zeros((len(shapes), 6), dtype=np.int64)
    cost_at = row_at = col_at = ws_at = 0
    for p, (r, c) in enumerate(shapes):
        desc[p] = (r, c, cost_at, row_at, col_at, ws_at)
        cost_at, row_at, col_at = cost_at + r * c, row_at + r, col_at + c
        if max(r, c) <= LSA_MAX_DIM:        # (a larger side is refused below by the library)
            ws_at += lib.dz_lsa_ws_bytes(r, c)          # 0 for a problem that fits LDS; the slices stand back to back
    if cost_at != cost.shape[0]:
        raise L.DetZeroHipError('linear_assignment_batch: %d costs for shapes that hold %d' % (cost.shape[0], cost_at))
    dev = cost.device
    p = len(shapes)
    row_to_col = torch.empty((max(row_at, 1),), dtype=torch.int32, device=dev)
    rows_free = torch.empty((max(row_at, 1),), dtype=torch.int32, device=dev)
    cols_free = torch.empty((max(col_at, 1),), dtype=torch.int32, device=dev)
    counts = torch.zeros((max(p, 1), 4), dtype=torch.int32, device=dev)
    ws = _ws(ws_at)
    d_desc = torch.from_numpy(desc).to(dev) if p else None
    rc = lib.dz_lsa_batch(L.ptr(cost), cost_at, L.ptr(d_desc), p, max([r for r, _ in shapes] + [0]), max([c for _, c in shapes] + [0]),
                          float(threshold), L.ptr(row_to_col), L.ptr(rows_free), row_at, L.ptr(cols_free), col_at, L.ptr(counts), L.ptr(ws),
                          ws.numel(), L.stream())
    L.check(rc, 'dz_lsa_batch')
    return row_to_col[:row_at], rows_free[:row_at], cols_free[:col_at], counts[:p], desc[:, 3].tolist(), desc[:, 4].tolist()


def linear_assignment_batch(costs, threshold=1.):
    """GNN_assignment (track_models.py) for a list of (rows, cols) float32 device matrices in one launch: a list of
    (matched (K,2) int [row, col] in row order, unmatched rows, unmatched columns) host arrays.  One host read.  The matrices are
    not modified (GNN_assignment writes the 5000 into its argument)."""
    costs = list(costs)
    if not costs:
        return []
    for c in costs:
        L.require_cuda(c)
        if c.dtype != torch.float32 or c.dim() != 2:
            raise L.DetZeroHipError('linear_assignment_batch: a cost matrix is (rows, cols) float32, got %s %s' % (tuple(c.shape), c.dtype))
    flat = torch.cat([c.reshape(-1) for c in costs]) if len(costs) > 1 else costs[0].reshape(-1)
    shapes = [tuple(c.shape) for c in costs]
    row_to_col, rows_free, cols_free, counts, row_off, col_off = linear_assignment_batch_nosync(flat, shapes, threshold)
    row_to_col, rows_free, cols_free, counts = row_to_col.cpu().numpy(), rows_free.cpu().numpy(), cols_free.cpu().numpy(), counts.cpu().numpy()
    out = []
    for p, (r, c) in enumerate(shapes):
        matched, n_rows_free, n_cols_free, status = counts[p].tolist()
        if status != 0:
            raise L.DetZeroHipError('linear_assignment_batch: problem %d (%d x %d): %s' % (p, r, c, LSA_STATUS.get(status, status)))
        r2c = row_to_col[row_off[p]:row_off[p] + r]
        at = np.flatnonzero(r2c >= 0)
        out.append((np.stack([at, r2c[at]], axis=1).astype(int), rows_free[row_off[p]:row_off[p] + n_rows_free].astype(int),
                    cols_free[col_off[p]:col_off[p] + n_cols_free].astype(int)))
    return out


# ------------------------------------------------------------------------------------------------
# detection matching at every score cutoff (csrc/eval_match.hip): the count table behind Waymo-style AP / APH
# ------------------------------------------------------------------------------------------------
EVAL_CUTOFFS = 101                 # DZ_EVAL_CUTOFFS
EVAL_IOU_THR = (0., .7, .5, .5, .5)               # waymo_eval_detection.py:111-115, indexed by object type
EVAL_BOX_TYPES = {'3d': 0, 'bev': 1}              # DZ_EVAL_BOX_*
EVAL_SCHEMES = {'atomic': 0, 'slots': 1}          # DZ_EVAL_ACC_*
EVAL_STATUS = {1: 'a descriptor leaves its buffers or a limit', 2: 'a solve stopped at a loop bound',
               3: 'a descriptor leaves its buffers or a limit; a solve stopped at a loop bound'}
EVAL_FIXED_ONE = float(1 << 32)                   # the tables' HA and COST columns are fixed point with 32 fraction bits
EVAL_HA_ONE = EVAL_FIXED_ONE


def _eval_boxes(what, pred_box, pred_score, gt_box):
    """The box and score arguments the evaluation ops share: (N,7) float32 boxes on the device, one float32 score per prediction."""
    L.require_cuda(pred_box, pred_score, gt_box)
    if any(b.dtype != torch.float32 or b.dim() != 2 or b.shape[1] != 7 for b in (pred_box, gt_box)):
        raise L.DetZeroHipError('%s: boxes are (N,7) float32, got %s %s / %s %s'
                                % (what, tuple(pred_box.shape), pred_box.dtype, tuple(gt_box.shape), gt_box.dtype))
    if pred_score.dtype != torch.float32 or tuple(pred_score.shape) != (pred_box.shape[0],):
        raise L.DetZeroHipError('%s: pred_score is (Np,) float32' % what)


def _eval_thr(what, box_type, iou_thr):
    """-> the five per-type IoU thresholds as the library takes them."""
    if box_type not in EVAL_BOX_TYPES or len(iou_thr) != 5:
        raise L.DetZeroHipError('%s: box_type %r / %d thresholds' % (what, box_type, len(iou_thr)))
    return (ctypes.c_float * 5)(*[float(t) for t in iou_thr])


def _eval_table(table, n_shards, width, dev, what):
    """The (n_shards,2,101,width) int64 count table an op adds to: zeros when None, else the caller's, checked."""
    if table is None:
        return torch.zeros((max(int(n_shards), 1), 2, EVAL_CUTOFFS, width), dtype=torch.int64, device=dev)
    if table.dtype != torch.int64 or tuple(table.shape) != (int(n_shards), 2, EVAL_CUTOFFS, width) or not table.is_cuda or \
            not table.is_contiguous():
        raise L.DetZeroHipError('%s: table is a contiguous (n_shards,2,101,%d) int64 device tensor' % (what, width))
    return table


def _eval_raise(status, what):
    """One host read of a status word; raises when it is set."""
    st = int(status.item())
    if st != 0:
        raise L.DetZeroHipError('%s: %s' % (what, EVAL_STATUS.get(st, st)))


def eval_match_counts_nosync(pred_box, pred_score, gt_box, gt_difficulty, desc, n_shards, box_type='3d', iou_thr=EVAL_IOU_THR,
                             scheme='atomic', table=None, ws_bytes=None):
    """pred_box (Np,7) f32 / pred_score (Np,) f32: the predictions grouped by problem, in descending score order inside each;
    gt_box (Ng,7) f32 / gt_difficulty (Ng,) i32 grouped by problem.  desc: host int64 array (n,6) of
    [first prediction, P, first ground truth, G, shard, object type] - the workspace offsets are added here - or a device tensor
    (n,7) in the library's layout with ``ws_bytes`` given.  -> (table (n_shards,2,101,4) int64 [TP, FP, FN, HA * 2^32], status (1,)
    i32) on the device; ``table`` (zeros when None) is added to.  No host read: the caller looks at status."""
    lib = L.load()
    _eval_boxes('eval_match_counts', pred_box, pred_score, gt_box)
    L.require_cuda(gt_difficulty)
    if gt_difficulty.dtype != torch.int32 or tuple(gt_difficulty.shape) != (gt_box.shape[0],):
        raise L.DetZeroHipError('eval_match_counts: gt_difficulty is (Ng,) int32')
    thr = _eval_thr('eval_match_counts', box_type, iou_thr)
    if scheme not in EVAL_SCHEMES:
        raise L.DetZeroHipError('eval_match_counts: scheme %r' % (scheme,))
    dev = pred_box.device
    if torch.is_tensor(desc):
        L.require_cuda(desc)
        if desc.dtype != torch.int64 or desc.dim() != 2 or desc.shape[1] != 7 or ws_bytes is None:
            raise L.DetZeroHipError('eval_match_counts: a device descriptor table is (n,7) int64 and comes with ws_bytes')
        d_desc, n, max_dim = desc, desc.shape[0], 0
    else:
        desc = np.asarray(desc, dtype=np.int64).reshape(-1, 6)
        n = desc.shape[0]
        dims = desc[:, 1] + desc[:, 3]
        max_dim = int(dims.max()) if n else 0
        full = np.zeros((n, 7), dtype=np.int64)
        full[:, :6] = desc
        if max_dim <= LSA_MAX_DIM and n and desc[:, [1, 3]].min() >= 0:        # (a larger problem is refused below by the library)
            # the library's size, vectorised: weights, cutoff indices and (beyond 1024 columns) the solver's vectors, to 256 bytes
            p, g = desc[:, 1], desc[:, 3]
            c = p + g
            work = np.where(c > 1024, ((2 * c + p) * 8 + (3 * c + p) * 4 + 15) // 16 * 16, 0)
            need = np.where(p > 0, ((p * g * 4 + 15) // 16 * 16 + (p * 4 + 15) // 16 * 16 + work + 255) // 256 * 256, 0)
            full[:, 6] = np.cumsum(need) - need
            ws_bytes = int(need.sum())
        else:
            ws_bytes = 0
        d_desc = torch.from_numpy(full).to(dev) if n else None
    table = _eval_table(table, n_shards, 4, dev, 'eval_match_counts')
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = _ws(ws_bytes)
    slots = torch.empty((max(n, 1) * 2 * EVAL_CUTOFFS * 4,), dtype=torch.int64, device=dev) if scheme == 'slots' else None

    def launch():
        rc = lib.dz_eval_match_counts(L.ptr(pred_box), L.ptr(pred_score), pred_box.shape[0], L.ptr(gt_box), L.ptr(gt_difficulty), gt_box.shape[0],
                                      L.ptr(d_desc), n, max_dim, int(n_shards), EVAL_BOX_TYPES[box_type], thr, EVAL_SCHEMES[scheme],
                                      L.ptr(table), L.ptr(slots), L.ptr(status), L.ptr(ws), int(ws_bytes), L.stream())
        L.check(rc, 'dz_eval_match_counts')

    if PROFILER is None:
        launch()
    else:
        PROFILER.wrap('eval_match[%s,%s]' % (box_type, scheme), 0., 0., launch)
    return table, status


def eval_match_counts(pred_box, pred_score, gt_box, gt_difficulty, desc, n_shards, box_type='3d', iou_thr=EVAL_IOU_THR, scheme='atomic'):
    """eval_match_counts_nosync, then one host read: the table as a host int64 array (n_shards,2,101,4); raises when the status
    word is set."""
    table, status = eval_match_counts_nosync(pred_box, pred_score, gt_box, gt_difficulty, desc, n_shards, box_type, iou_thr, scheme)
    _eval_raise(status, 'eval_match_counts')
    return table.cpu().numpy()[:int(n_shards)]


# ------------------------------------------------------------------------------------------------
# tracking metrics at every score cutoff (csrc/mot_chain.hip): the count table behind Waymo-style MOTA / MOTP
# ------------------------------------------------------------------------------------------------
MOT_COUNTS = 5                     # DZ_MOT_COUNTS: TP, FP, MISS, MISMATCH, COST * 2^32
MOT_LDS_DIM = 192                  # DZ_MOT_LDS_DIM
MOT_MAPPINGS = {'wave': 0, 'workgroup': 1}        # DZ_MOT_MAP_*
MOT_COST_ONE = EVAL_FIXED_ONE


def mot_problem_desc(desc):
    """Host (n,5) [first prediction, P, first ground truth, G, object type] -> (n,6) int64 with the weight offsets (floats, back to
    back), and the length of the weight buffer."""
    desc = np.asarray(desc, dtype=np.int64).reshape(-1, 5)
    full = np.zeros((desc.shape[0], 6), dtype=np.int64)
    full[:, :5] = desc
    size = np.maximum(desc[:, 1], 0) * np.maximum(desc[:, 3], 0)
    full[:, 5] = np.cumsum(size) - size
    return full, int(size.sum())


def mot_chain_ws_bytes(n_pred_ids, n_gt_ids, max_dim):
    """dz_mot_chain_ws_bytes: the workspace slice of one (sequence, shard) descriptor, all 101 cutoffs; 0 for sizes the library refuses."""
    return int(L.load().dz_mot_chain_ws_bytes(int(n_pred_ids), int(n_gt_ids), int(min(max(int(max_dim), -1), 1 << 30))))


def mot_weights(pred_box, pred_score, gt_box, pdesc, w_len, box_type='3d', iou_thr=EVAL_IOU_THR):
    """pred_box (Np,7) f32 / pred_score (Np,) f32 grouped by problem, in descending score order inside each; gt_box (Ng,7) f32
    grouped by problem; pdesc: host (n,6) int64 of mot_problem_desc.  -> (weights (w_len,) f32, cut (Np,) i32) on the device: the
    thresholded IoU of every pair of every problem and each prediction's highest cutoff (-1 = none).  One host read (the status)."""
    lib = L.load()
    _eval_boxes('mot_weights', pred_box, pred_score, gt_box)
    thr = _eval_thr('mot_weights', box_type, iou_thr)
    dev = pred_box.device
    pdesc = np.asarray(pdesc, dtype=np.int64).reshape(-1, 6)
    n = pdesc.shape[0]
    max_dim = int((pdesc[:, 1] + pdesc[:, 3]).max()) if n else 0
    weights = torch.empty((max(int(w_len), 1),), dtype=torch.float32, device=dev)
    cut = torch.full((max(pred_box.shape[0], 1),), -1, dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    d_desc = torch.from_numpy(pdesc).to(dev) if n else None

    def launch():
        rc = lib.dz_mot_weights(L.ptr(pred_box), L.ptr(pred_score), pred_box.shape[0], L.ptr(gt_box), gt_box.shape[0], L.ptr(d_desc), n,
                                max_dim, EVAL_BOX_TYPES[box_type], thr, L.ptr(weights), int(w_len), L.ptr(cut), L.ptr(status), L.stream())
        L.check(rc, 'dz_mot_weights')

    if PROFILER is None:
        launch()
    else:
        PROFILER.wrap('mot_weights[%s]' % box_type, 0., 0., launch)
    _eval_raise(status, 'mot_weights')
    return weights[:int(w_len)], cut[:pred_box.shape[0]]


def mot_chain_counts_nosync(weights, cut, pred_id, gt_id, gt_difficulty, pdesc, cdesc, frames, n_shards, mapping='wave', merge=True,
                            table=None):
    """weights (w_len,) f32 and cut (Np,) i32 as mot_weights gives them (or made by the caller); pred_id (Np,) / gt_id (Ng,) i32
    dense per (sequence, side); gt_difficulty (Ng,) i32; pdesc host (n,6) of mot_problem_desc; cdesc host (c,6) per (sequence,
    shard) of [first entry in frames, number of frames, shard, prediction ids, ground-truth ids, largest P + G] - the workspace
    offsets are added here; frames: host int64 problem indices in walking order.  ``merge=False`` (tests) runs the chain of every
    cutoff instead of one per distinct prediction set.  -> (table (n_shards,2,101,5) int64 [TP, FP, MISS, MISMATCH, COST * 2^32],
    status (1,) i32) on the device; ``table`` (zeros when None) is added to.  No host read: the caller looks at status."""
    lib = L.load()
    L.require_cuda(weights, cut, pred_id, gt_id, gt_difficulty)
    if weights.dtype != torch.float32 or weights.dim() != 1 or any(t.dtype != torch.int32 or t.dim() != 1 for t in (cut, pred_id, gt_id, gt_difficulty)):
        raise L.DetZeroHipError('mot_chain_counts: weights are (w_len,) float32; cut, ids and difficulties (N,) int32')
    if cut.shape != pred_id.shape or gt_id.shape != gt_difficulty.shape:
        raise L.DetZeroHipError('mot_chain_counts: %d cutoff indices for %d prediction ids, %d difficulties for %d ground-truth ids'
                                % (cut.shape[0], pred_id.shape[0], gt_difficulty.shape[0], gt_id.shape[0]))
    if mapping not in MOT_MAPPINGS:
        raise L.DetZeroHipError('mot_chain_counts: mapping %r' % (mapping,))
    dev = weights.device
    pdesc = np.asarray(pdesc, dtype=np.int64).reshape(-1, 6)
    cdesc = np.asarray(cdesc, dtype=np.int64).reshape(-1, 6)
    frames = np.ascontiguousarray(np.asarray(frames, dtype=np.int64).reshape(-1))
    n, nc = pdesc.shape[0], cdesc.shape[0]
    max_dim = int((pdesc[:, 1] + pdesc[:, 3]).max()) if n else 0
    full = np.zeros((nc, 7), dtype=np.int64)
    full[:, :6] = cdesc
    ws_bytes = 0
    for i in range(nc):                                 # (a bad descriptor gets no room: the kernel refuses it by its own check)
        full[i, 6] = ws_bytes
        ws_bytes += mot_chain_ws_bytes(cdesc[i, 3], cdesc[i, 4], cdesc[i, 5])
    table = _eval_table(table, n_shards, MOT_COUNTS, dev, 'mot_chain_counts')
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = _ws(ws_bytes)
    d_pdesc = torch.from_numpy(pdesc).to(dev) if n else None
    d_cdesc = torch.from_numpy(full).to(dev) if nc else None
    d_frames = torch.from_numpy(frames).to(dev) if frames.size else None

    def launch():
        rc = lib.dz_mot_chain_counts(L.ptr(weights), weights.shape[0], L.ptr(cut), L.ptr(pred_id), pred_id.shape[0], L.ptr(gt_id),
                                     L.ptr(gt_difficulty), gt_id.shape[0], L.ptr(d_pdesc), n, L.ptr(d_cdesc), nc, L.ptr(d_frames),
                                     frames.size, max_dim, int(n_shards), MOT_MAPPINGS[mapping], 1 if merge else 0, L.ptr(table),
                                     L.ptr(status), L.ptr(ws), int(ws_bytes), L.stream())
        L.check(rc, 'dz_mot_chain_counts')

    if PROFILER is None:
        launch()
    else:
        PROFILER.wrap('mot_chain[%s]' % mapping, 0., 0., launch)
    return table, status


def mot_chain_counts(weights, cut, pred_id, gt_id, gt_difficulty, pdesc, cdesc, frames, n_shards, mapping='wave', merge=True):
    """mot_chain_counts_nosync, then one host read: the table as a host int64 array (n_shards,2,101,5); raises when the status
    word is set."""
    table, status = mot_chain_counts_nosync(weights, cut, pred_id, gt_id, gt_difficulty, pdesc, cdesc, frames, n_shards, mapping, merge)
    _eval_raise(status, 'mot_chain_counts')
    return table.cpu().numpy()[:int(n_shards)]


# ------------------------------------------------------------------------------------------------
# CenterHead targets and losses (csrc/head_loss.hip)
# ------------------------------------------------------------------------------------------------
HEAD_LOSS_MAX_OBJS = 1024          # DZ_HEAD_LOSS_MAX_OBJS
HEAD_LOSS_REC = 12                 # DZ_HEAD_LOSS_REC: hm, eight regression components, loc, iou, total
HEAD_LOSS_KEYS = ('hm', 'center_x', 'center_y', 'center_z', 'dim_x', 'dim_y', 'dim_z', 'rot_cos', 'rot_sin', 'loc', 'iou', 'total')


def _dbl(values):
    return (ctypes.c_double * len(values))(*[float(v) for v in values])


def centerhead_targets(gt_boxes, cls_table, ncls, feat_h, feat_w, stride, pc_range, voxel_size, num_max_objs=500, gaussian_overlap=0.1,
                       min_radius=2):
    """center_head.py:111-161 for ONE head and the whole batch on the device.  gt_boxes (B, M, 8) f32 [x, y, z, dx, dy, dz, heading,
    1-based global class (0 = padding)]; cls_table[g - 1] = the head's 1-based class of global class g, 0 = not this head.
    -> heatmap (B, ncls, H, W) f32, target_boxes (B, NMAX, 8) f32, inds (B, NMAX) i64, masks (B, NMAX) i64, rec (2,) i32
    [num_pos, num].  No host read."""
    lib = L.load()
    L.require_cuda(gt_boxes)
    if gt_boxes.dtype != torch.float32 or gt_boxes.dim() != 3:
        raise L.DetZeroHipError('centerhead_targets: gt_boxes is (B, M, 8) float32, got %s %s' % (tuple(gt_boxes.shape), gt_boxes.dtype))
    b, m, cols = gt_boxes.shape
    dev = gt_boxes.device
    nmax, ncls = int(num_max_objs), int(ncls)
    shape_ok = 1 <= ncls <= 3 and 1 <= nmax <= HEAD_LOSS_MAX_OBJS and b > 0 and feat_h > 0 and feat_w > 0 and cols == 8
    heat = torch.empty((b, ncls, feat_h, feat_w) if shape_ok else (1,), dtype=torch.float32, device=dev)
    tb = torch.empty((b, nmax, 8) if shape_ok else (8,), dtype=torch.float32, device=dev)
    inds = torch.empty((b, nmax) if shape_ok else (1,), dtype=torch.int64, device=dev)
    masks = torch.empty((b, nmax) if shape_ok else (1,), dtype=torch.int64, device=dev)
    rec = torch.empty((2,), dtype=torch.int32, device=dev)
    table = (ctypes.c_int * max(len(cls_table), 1))(*[int(v) for v in cls_table])

    def launch():
        rc = lib.dz_centerhead_targets(L.ptr(gt_boxes), b, m, cols, table, len(cls_table), ncls, int(feat_h), int(feat_w), float(stride),
                                       _dbl(pc_range[0:2]), _dbl(voxel_size[0:2]), nmax, float(gaussian_overlap), int(min_radius),
                                       L.ptr(heat), L.ptr(tb), L.ptr(inds), L.ptr(masks), L.ptr(rec), L.stream())
        L.check(rc, 'dz_centerhead_targets')

    if PROFILER is None:
        launch()
    else:
        PROFILER.wrap('centerhead_targets', 0., 0., launch)
    return heat, tb, inds, masks, rec


def centerhead_loss_nosync(head, heatmap, target_boxes, inds, masks, rec, feat_h, feat_w, weights, stride, pc_range, voxel_size,
                           hm_mask=None, want_grad=False):
    """The launches of centerhead_loss without autograd: -> (record (12,) f64 on the device in HEAD_LOSS_KEYS order, grad_head
    (B, H*W, 12) f32 or None).  weights = (cls_weight, loc_weight, code_weights[8], iou_weight); rec None: counted by the call."""
    lib = L.load()
    L.require_cuda(head, heatmap, target_boxes, inds, masks, rec, hm_mask)
    if head.dtype != torch.float32 or head.dim() != 3 or head.shape[2] != 12 or head.shape[1] != feat_h * feat_w:
        raise L.DetZeroHipError('centerhead_loss: head is (B, H*W, 12) float32, got %s %s' % (tuple(head.shape), head.dtype))
    b = head.shape[0]
    if heatmap.dtype != torch.float32 or heatmap.dim() != 4 or heatmap.shape[0] != b or tuple(heatmap.shape[2:]) != (feat_h, feat_w):
        raise L.DetZeroHipError('centerhead_loss: heatmap is (B, ncls, H, W) float32, got %s %s' % (tuple(heatmap.shape), heatmap.dtype))
    ncls = heatmap.shape[1]
    if inds.dtype != torch.int64 or masks.dtype != torch.int64 or inds.dim() != 2 or inds.shape[0] != b or masks.shape != inds.shape or \
            target_boxes.dtype != torch.float32 or tuple(target_boxes.shape) != (b, inds.shape[1], 8):
        raise L.DetZeroHipError('centerhead_loss: inds / masks are (B, NMAX) int64 and target_boxes (B, NMAX, 8) float32')
    if rec is not None and (rec.dtype != torch.int32 or rec.numel() != 2):
        raise L.DetZeroHipError('centerhead_loss: rec is (2,) int32')
    if hm_mask is not None and (hm_mask.dtype != torch.float32 or tuple(hm_mask.shape) != (b, feat_h, feat_w)):
        raise L.DetZeroHipError('centerhead_loss: hm_mask is (B, H, W) float32')
    if len(weights) != 11:
        raise L.DetZeroHipError('centerhead_loss: 11 weights (cls, loc, eight code weights, iou), got %d' % len(weights))
    dev = head.device
    nmax = inds.shape[1]
    out = torch.empty((HEAD_LOSS_REC,), dtype=torch.float64, device=dev)
    grad = torch.empty_like(head) if want_grad else None
    ws_bytes = int(lib.dz_centerhead_loss_ws_bytes(b, int(feat_h), int(feat_w)))
    ws = _ws(ws_bytes)

    def launch():
        rc = lib.dz_centerhead_loss(L.ptr(head), L.ptr(heatmap), L.ptr(target_boxes), L.ptr(inds), L.ptr(masks), L.ptr(rec), L.ptr(hm_mask),
                                    b, int(feat_h), int(feat_w), ncls, nmax, _dbl(weights), float(stride), _dbl(pc_range[0:2]),
                                    _dbl(voxel_size[0:2]), L.ptr(out), L.ptr(grad), L.ptr(ws), ws_bytes, L.stream())
        L.check(rc, 'dz_centerhead_loss')

    if PROFILER is None:
        launch()
    else:
        PROFILER.wrap('centerhead_loss', 0., 0., launch)
    return out, grad


class _CenterHeadLoss(torch.autograd.Function):
    """total and record of one head; the fused pass has already formed d total / d head when backward asks for it."""

    @staticmethod
    def forward(ctx, head, args):
        rec, grad = centerhead_loss_nosync(head.detach(), *args, want_grad=True)     # (only applied to a head map that requires grad)
        ctx.grad_head = grad
        ctx.mark_non_differentiable(rec)
        return rec[HEAD_LOSS_REC - 1].to(torch.float32), rec

    @staticmethod
    def backward(ctx, grad_total, _grad_rec):
        if ctx.grad_head is None:
            raise L.DetZeroHipError('centerhead_loss: the head map did not require grad when the loss was formed')
        return ctx.grad_head * grad_total, None


def centerhead_loss(head, heatmap, target_boxes, inds, masks, rec, feat_h, feat_w, weights, stride, pc_range, voxel_size, hm_mask=None):
    """Losses of ONE head (center_head.py:266-313 for one `idx`): head (B, H*W, 12) f32 channel-last as CenterHead.run_head writes
    it, the targets as centerhead_targets gives them.  -> (total, record): total a 0-dim f32 tensor, record (12,) f64 in
    HEAD_LOSS_KEYS order, both on the device.  With a head map that requires grad, total.backward() delivers grad_head * grad_output
    (the gradient buffer is filled by the same pass; without one it is not allocated).  No host read."""
    args = (heatmap, target_boxes, inds, masks, rec, int(feat_h), int(feat_w), tuple(float(w) for w in weights), float(stride),
            tuple(pc_range), tuple(voxel_size), hm_mask)
    if head.requires_grad and torch.is_grad_enabled():
        return _CenterHeadLoss.apply(head, args)
    out, _ = centerhead_loss_nosync(head.detach(), *args, want_grad=False)
    return out[HEAD_LOSS_REC - 1].to(torch.float32), out


# ------------------------------------------------------------------------------------------------
# CenterHead: backward through the head's convolutions (csrc/head_backward.hip)
# ------------------------------------------------------------------------------------------------
WGRAD_TILE_W = 32                  # DZ_WGRAD_TILE_W: pixel columns of a band
WGRAD_CHUNK_ROWS = 16              # DZ_WGRAD_CHUNK_ROWS: rows of a workgroup's chunk
WGRAD_CHUNK_PIXELS = WGRAD_TILE_W * WGRAD_CHUNK_ROWS
WGRAD_GROUP_PAD = 16               # columns of a group in the grouped layout


def _ints(values):
    return (ctypes.c_int * max(len(values), 1))(*[int(v) for v in values])


def _bordered(t, what, c=None):
    """(B, H, W) of a zero-bordered channel-last (B, H + 2, W + 2, C) float32 image."""
    if t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] < 3 or t.shape[2] < 3 or (c is not None and t.shape[3] != c):
        raise L.DetZeroHipError('%s is a zero-bordered (B, H + 2, W + 2, %s) float32 image, got %s %s'
                                % (what, 'C' if c is None else c, tuple(t.shape), t.dtype))
    return t.shape[0], t.shape[1] - 2, t.shape[2] - 2


def conv3x3_wgrad(x_img, g_img, cin, cout, groups=1, g_cout=None, g_ooff=None):
    """Raw weight gradient of a 3 x 3 stride-1 layer: Graw[tap][ci][c] = sum over (b, y, x) of x_img[b, y + ky, x + kx, ci] * g[b, y, x, c].
    x_img (B, H + 2, W + 2, groups * cin) f32 with its border.  groups == 1: g_img (B, H + 2, W + 2, cout) zero-bordered as relu_grad
    writes it, or dense (B, H, W, cout) -> (9, cin, cout) f32.  groups > 1: g_img the dense (B, H * W, cout) or (B, H, W, cout) map
    of which group q reads columns [g_ooff[q], + g_cout[q]) -> (groups, 9, cin, 16) f32, the pad columns 0.  Fixed summation order
    (split over chunks of WGRAD_CHUNK_PIXELS pixels, added in chunk order).  No host read."""
    lib = L.load()
    L.require_cuda(x_img, g_img)
    cin, cout, groups = int(cin), int(cout), int(groups)
    b, h, w = _bordered(x_img, 'conv3x3_wgrad: x_img', groups * cin)
    if g_img.dtype != torch.float32 or g_img.shape[0] != b or g_img.shape[-1] != cout:
        raise L.DetZeroHipError('conv3x3_wgrad: g_img is float32 with %d frames of %d channels, got %s %s' % (b, cout, tuple(g_img.shape), g_img.dtype))
    if g_img.dim() == 4 and tuple(g_img.shape[1:3]) == (h + 2, w + 2) and groups == 1:
        border = 1
    elif (g_img.dim() == 4 and tuple(g_img.shape[1:3]) == (h, w)) or (g_img.dim() == 3 and g_img.shape[1] == h * w):
        border = 0
    else:
        raise L.DetZeroHipError('conv3x3_wgrad: g_img %s does not match the %d x %d map of x_img' % (tuple(g_img.shape), h, w))
    g_cout, g_ooff = list(g_cout or []), list(g_ooff or [])
    if len(g_cout) != len(g_ooff):
        raise L.DetZeroHipError('conv3x3_wgrad: %d g_cout entries but %d g_ooff entries' % (len(g_cout), len(g_ooff)))
    dev = x_img.device
    ws_bytes = int(lib.dz_conv3x3_wgrad_ws_bytes(b, h, w, cin, cout, groups))
    shape_ok = ws_bytes > 0
    shape = ((groups, 9, cin, WGRAD_GROUP_PAD) if groups > 1 else (9, cin, cout)) if shape_ok else (4,)
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    ws = _ws(ws_bytes)

    def launch():
        rc = lib.dz_conv3x3_wgrad(L.ptr(x_img), L.ptr(g_img), border, b, h, w, cin, cout, groups, _ints(g_cout), _ints(g_ooff), len(g_cout),
                                  L.ptr(out), L.ptr(ws), ws.numel(), L.stream())
        L.check(rc, 'dz_conv3x3_wgrad')

    if PROFILER is None:
        launch()
    else:
        cols = sum(g_cout) if groups > 1 else cout
        PROFILER.wrap('k_c3_wgrad', 2.0 * b * h * w * 9 * cin * cols, 4.0 * b * h * w * (groups * cin + cols), launch)
    return out


def relu_grad(g_y, y_img, out=None):
    """The mask pass between two layers: g = g_y where y_img > 0, else 0 (a select) -> (g_img, sums): g_img the zero-bordered
    (B, H + 2, W + 2, C) image (`out`, whose interior is written and whose border is left alone, or a fresh zeroed one; `out` may be
    g_y itself when that is a bordered image), sums (C,) f64 = the channel sums of g in a fixed order.  y_img: the stored activation,
    zero-bordered; g_y: dense (B, H, W, C) or the interior of a bordered image.  No host read."""
    lib = L.load()
    L.require_cuda(g_y, y_img, out)
    b, h, w = _bordered(y_img, 'relu_grad: y_img')
    c = y_img.shape[3]
    if g_y.dtype != torch.float32 or g_y.dim() != 4 or g_y.shape[0] != b or g_y.shape[3] != c or \
            tuple(g_y.shape[1:3]) not in ((h, w), (h + 2, w + 2)):
        raise L.DetZeroHipError('relu_grad: g_y is (B, H, W, C) or (B, H + 2, W + 2, C) float32 like y_img %s, got %s %s'
                                % (tuple(y_img.shape), tuple(g_y.shape), g_y.dtype))
    border = 1 if g_y.shape[1] == h + 2 else 0
    if out is not None and (out.dtype != torch.float32 or out.shape != y_img.shape):
        raise L.DetZeroHipError('relu_grad: out is a float32 image of y_img\'s shape %s, got %s %s' % (tuple(y_img.shape), tuple(out.shape), out.dtype))
    dev = y_img.device
    g_img = out if out is not None else torch.zeros(y_img.shape, dtype=torch.float32, device=dev)
    sums = torch.empty((c,), dtype=torch.float64, device=dev)
    ws_bytes = int(lib.dz_relu_grad_ws_bytes(b, h, w, c))
    ws = _ws(ws_bytes)

    def launch():
        rc = lib.dz_relu_grad(L.ptr(g_y), border, L.ptr(y_img), b, h, w, c, L.ptr(g_img), L.ptr(sums), L.ptr(ws), ws.numel(), L.stream())
        L.check(rc, 'dz_relu_grad')

    if PROFILER is None:
        launch()
    else:
        PROFILER.wrap('k_relu_grad', 0., 12.0 * b * h * w * c, launch)
    return g_img, sums


def conv3x3_dgrad_weights(w_taps, scale=None):
    """(9, cin, cout) forward weights -> the (9, cout, cin) weights of the data gradient: flipped in both spatial axes, cin and cout
    transposed, `scale` (cout,) folded in (w[tap, ci, c] * scale[c]).  Device tensor ops only."""
    if w_taps.dim() != 3 or w_taps.shape[0] != 9:
        raise L.DetZeroHipError('conv3x3_dgrad: w_taps is (9, cin, cout), got %s' % (tuple(w_taps.shape),))
    w = w_taps if scale is None else w_taps * scale.to(w_taps.dtype).reshape(1, 1, -1)
    return w.flip(0).transpose(1, 2).contiguous()


def conv3x3_dgrad(g_img, w_taps, scale=None, out=None):
    """Data gradient of y = scale * conv3x3(x, w) (stride 1, zero padding 1): g_img (B, H + 2, W + 2, cout) zero-bordered, w_taps
    (9, cin, cout) f32 forward weights -> (B, H, W, cin) f32 dense, or written into the interior of the zero-bordered `out`
    (B, H + 2, W + 2, cin).  The weights are flipped and transposed on the device and the layer runs on dz_conv2d_forward (fp32,
    engines off); cin % 16 == 0 and cout % 16 == 0."""
    L.require_cuda(g_img, w_taps, scale, out)
    b, h, w = _bordered(g_img, 'conv3x3_dgrad: g_img')
    cout = g_img.shape[3]
    if w_taps.dtype != torch.float32 or w_taps.dim() != 3 or w_taps.shape[0] != 9 or w_taps.shape[2] != cout:
        raise L.DetZeroHipError('conv3x3_dgrad: w_taps is (9, cin, %d) float32, got %s %s' % (cout, tuple(w_taps.shape), w_taps.dtype))
    cin = w_taps.shape[1]
    if cin % 16 or cout % 16:
        raise L.DetZeroHipError('conv3x3_dgrad: %d -> %d channels (multiples of 16)' % (cin, cout))
    if scale is not None and scale.numel() != cout:
        raise L.DetZeroHipError('conv3x3_dgrad: %d scale entries for %d channels' % (scale.numel(), cout))
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != (b, h + 2, w + 2, cin)):
        raise L.DetZeroHipError('conv3x3_dgrad: out is a zero-bordered (%d, %d, %d, %d) float32 image, got %s %s'
                                % (b, h + 2, w + 2, cin, tuple(out.shape), out.dtype))
    wt = conv3x3_dgrad_weights(w_taps, scale)
    res = out if out is not None else torch.empty((b, h, w, cin), dtype=torch.float32, device=g_img.device)
    pad = 1 if out is not None else 0
    conv2d(dict(inp=g_img.data_ptr(), out=res.data_ptr(), w=wt.data_ptr(), scale=None, shift=None, batch=b, ho=h, wo=w, in_hp=h + 2,
                in_wp=w + 2, in_cstride=cout, in_coff=0, cin=cout, kh=3, kw=3, stride=1, in_off=0, out_hp=h + 2 * pad, out_wp=w + 2 * pad,
                out_cstride=cin, out_coff=0, out_sy=1, out_sx=1, out_dy=pad, out_dx=pad, groups=1, cout_pad=cin, g_cout=[cin], g_ooff=[0],
                relu=0, phase_groups=0, in_rowidx=None, in_row_channels=0, in_rows=0, in_tiles=None), math=0)
    return res


def head_final_backward(grad_head, w2, hidden_img, g_cout, g_ooff, out=None):
    """Both halves of the backward of a SeparateHead's grouped output layer (groups slices of c hidden channels -> the head map's 12
    columns).  grad_head (B, H * W, 12) f32; w2 (groups, 9, c, 16) f32 (plan()['heads'][i]['final']['w']); hidden_img
    (B, H + 2, W + 2, groups * c) f32 zero-bordered: the hidden layer's stored activation.
    -> (g_hidden, sums, d_w2, d_bias): g_hidden the zero-bordered image of the gradient at the hidden layer's pre-activation (the
    layer's ReLU mask applied; `out`, whose border is left alone, or a fresh zeroed image), sums (groups * c,) f64 its channel sums,
    d_w2 (groups, 9, c, 16) f32 the weight gradient (pad columns 0), d_bias (groups, 16) f64 the column sums of grad_head (pad
    columns 0).  Columns of grad_head outside the groups' ranges are never read.  No host read."""
    lib = L.load()
    L.require_cuda(grad_head, w2, hidden_img, out)
    b, h, w = _bordered(hidden_img, 'head_final_backward: hidden_img')
    if grad_head.dtype != torch.float32 or tuple(grad_head.shape) != (b, h * w, 12):
        raise L.DetZeroHipError('head_final_backward: grad_head is (%d, %d, 12) float32, got %s %s' % (b, h * w, tuple(grad_head.shape), grad_head.dtype))
    if w2.dtype != torch.float32 or w2.dim() != 4 or w2.shape[1] != 9 or w2.shape[3] != WGRAD_GROUP_PAD or \
            w2.shape[0] * w2.shape[2] != hidden_img.shape[3]:
        raise L.DetZeroHipError('head_final_backward: w2 is (groups, 9, c, 16) float32 with groups * c = %d, got %s %s'
                                % (hidden_img.shape[3], tuple(w2.shape), w2.dtype))
    groups, c = w2.shape[0], w2.shape[2]
    g_cout, g_ooff = list(g_cout), list(g_ooff)
    if len(g_cout) != len(g_ooff):
        raise L.DetZeroHipError('head_final_backward: %d g_cout entries but %d g_ooff entries' % (len(g_cout), len(g_ooff)))
    if out is not None and (out.dtype != torch.float32 or out.shape != hidden_img.shape):
        raise L.DetZeroHipError('head_final_backward: out is a float32 image of hidden_img\'s shape %s, got %s %s'
                                % (tuple(hidden_img.shape), tuple(out.shape), out.dtype))
    dev = hidden_img.device
    g_hidden = out if out is not None else torch.zeros(hidden_img.shape, dtype=torch.float32, device=dev)
    sums = torch.empty((groups * c,), dtype=torch.float64, device=dev)
    d_w2 = torch.empty(w2.shape, dtype=torch.float32, device=dev)
    d_bias = torch.empty((groups, WGRAD_GROUP_PAD), dtype=torch.float64, device=dev)
    ws_bytes = int(lib.dz_head_final_backward_ws_bytes(b, h, w, c, groups))
    ws = _ws(ws_bytes)

    def launch():
        rc = lib.dz_head_final_backward(L.ptr(grad_head), L.ptr(w2), L.ptr(hidden_img), b, h, w, c, groups, _ints(g_cout), _ints(g_ooff),
                                        len(g_cout), L.ptr(g_hidden), L.ptr(sums), L.ptr(d_w2), L.ptr(d_bias), L.ptr(ws), ws.numel(),
                                        L.stream())
        L.check(rc, 'dz_head_final_backward')

    if PROFILER is None:
        launch()
    else:
        cols = sum(g_cout)
        PROFILER.wrap('head_final_backward', 4.0 * b * h * w * 9 * c * cols, 4.0 * b * h * w * (2 * groups * c + 12), launch)
    return g_hidden, sums, d_w2, d_bias


PROFILER = None


# ------------------------------------------------------------------------------------------------
# device guard: every wrapper above allocates its outputs / workspaces with the current device and launches on its current
# stream, so each public entry runs under torch.cuda.device(<device of its first tensor argument>) - tensors living on a GPU
# other than the current one (one process driving several GPUs) then get their kernels on their own device and stream
# ------------------------------------------------------------------------------------------------
def _guarded(fn):
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        dev = None
        for a in list(args) + list(kwargs.values()):
            a = a.words if isinstance(a, NeighborTable) else a
            if torch.is_tensor(a) and a.is_cuda:
                dev = a.device
                break
            if isinstance(a, SparseLevel):
                dev = a.coords.device
                break
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapper


def _install_guards():
    import types
    g = globals()
    for name, obj in list(g.items()):
        if isinstance(obj, types.FunctionType) and obj.__module__ == __name__ and not name.startswith('_') and name not in ('grid_size_of', 'math_id', 'pair16_pack', 'pair16_unpack', 'limb3_pack', 'limb3_unpack', 'conv3x3_limb3_supported', 'conv2d_limb3_supported', 'mha_core_limb3_supported'):
            g[name] = _guarded(obj)
    for name in ('build_from_coords', 'downsample', 'neighbors_to'):
        setattr(SparseLevel, name, _guarded(getattr(SparseLevel, name)))


_install_guards()
