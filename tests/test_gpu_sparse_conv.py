"""Every sparse-convolution kernel instance against a float64 reference (csrc/sparse_conv.hip, sparse_conv_h.hip, sparse_conv_w.h,
sparse_conv_x.hip, sparse_conv_xf.hip and the bf16x3 x-run kernel k_spconv_xt of sparse_conv_xt.hip; the bf16x3 gather kernel k_spconv_gt
of sparse_conv_gt.hip has its edge table in tests/test_gpu_spconv_gather_limb3.py and joins the detector-launch replay here), the sparse
counterpart of tests/test_gpu_dense_conv.py.

Which kernel runs a layer depends on its channels, on the form of its neighbour table (plain, packed, packed with x-run windows) and
on whether the table comes with tile masks, so every case names the (instance, arm) the dispatch code must report for it and
`test_case_table_covers_every_variant` checks that the table reaches every shipped (instance, math mode, arm) and every edge listed in
EDGES_REQUIRED.  Each instance runs the layer kinds SparseBackbone gives its channels: the submanifold 3 x 3 x 3 convolution of one
level, the stride-2 3 x 3 x 3 down-convolution into a distinct, smaller level (padding (1, 1, 1); 64 -> 128 also (0, 1, 1)) and
conv_out ((3, 1, 1), stride (2, 1, 1)).

Rulebook: the CPU oracle's (oracle.sparse.neighbor_table on the level's coordinates).  The GPU table the kernel reads - plain, packed
(through ops.unpack_table) or in tap-set order (through perm) - must equal it on the rows below m; the convolution is then judged
against the oracle's table alone.  Reference: float64 on the device, on the operands exactly as the kernel sees them (split modes:
rows, residual and weights decoded from their pair16 words), one index_add_ of x[idx] @ w[tap] per tap, the same with absolute values
for sum |x.w|.  Error of an output element = |got - ref| / (|scale| * sum|x.w| + |shift| + |residual|), over EVERY row < m and channel
< cout, a NaN counting as infinity; the bounds are BOUND of tests/test_gpu_dense_conv.py (same arithmetic - igemm.h / hgemm.h - on
shorter sums: at most 27 x 128 products).

Every launch goes twice into a buffer of (cap + TAIL) rows filled with the dense module's sentinel: rows >= m and the tail keep it word
for word, rows < m lose it, the two launches agree bit for bit.  Input rows >= m_in and residual rows >= m are NaN (level buffers come
from torch.empty: an absent neighbour must fetch zeros, never a row).  Every case runs with scale, shift, residual and ReLU all on, and
with all of them off (null pointers, relu = 0).

The bf16x3 kernels (engine keys 'xt', 'gt') read fp32 rows and limb weights that sum to the fp32 weights exactly, so their float64
reference is the fp32 operands' and their bound BOUND['f32'].

The three x-run families switch arm per (unit, z slab) at `window rows <= staging capacity`: the edges 'window=rcap' and 'window=rcap+1'
run each of them on a constructed level (window_coords) whose longest window is exactly the capacity (the last direct-to-LDS run ends
at the slot before the zero row) and exactly one row more (the smallest window of the gather-mode arm); the condition is asserted from
the windows the library built.
"""
import functools
import json
import os
import subprocess
import sys
import types
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from detzero_amd import lib as L
from detzero_amd import ops
from oracle import sparse as osp
from tests.test_gpu_dense_conv import BOUND, SENTINEL
from tests.test_gpu_xrun import K3, P1, S1, _level, _t

MODES = ('f32', 'f16x2', 'bf16x2', 'f16')
SPLIT = ('f16x2', 'bf16x2', 'f16')
S2, P011, P0 = (2, 2, 2), (0, 1, 1), (0, 0, 0)
KINDS = {'subm': (K3, S1, P1), 'down': (K3, S2, P1), 'down011': (K3, S2, P011), 'out': ((3, 1, 1), (2, 1, 1), P0)}
POISON = 0x7FC07FC0            # a NaN as fp32, and as two NaN halves in fp16 and in bf16
TAIL = 64                      # sentinel rows behind the capacity
UNEQUAL = (0.01, 0.9, 0.02, 0.5)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the layers of det_modules.SparseBackbone: (cin, cout, kind)
LAYERS = ((16, 16, 'subm'), (16, 32, 'down'), (32, 32, 'subm'), (32, 64, 'down'), (64, 64, 'subm'), (64, 128, 'down'), (64, 128, 'down011'),
          (128, 128, 'subm'), (128, 128, 'out'))

# ------------------------------------------------------------------------------------------------------------------------
# what the default build can launch: (instance [+ arm of k_spconv_h], arm of the case) per math mode
#   fp32 gather: arm = layer kind; k_spconv_h: ring (tile masks given) / lds (tile_masks = NULL through the C ABI - the small-channel
#   k_spconv_h tiles are reached this way too, k_spconv_w needs the masks); k_spconv_w: plain / packed table;
#   x-run (k_spconv_x, k_spconv_xf, k_spconv_xt): tap-set order or not x staged / gather-mode windows
# ------------------------------------------------------------------------------------------------------------------------
ALL_VARIANTS = {m: set() for m in MODES}
ALL_VARIANTS['f32'] |= {('k_spconv<128x16x16>', 'subm'), ('k_spconv<128x32x16>', 'down'), ('k_spconv<128x32x32>', 'subm'),
                        ('k_spconv<64x64x32>', 'subm'), ('k_spconv<64x64x32>', 'down'), ('k_spconv<64x64x32>', 'down011'),
                        ('k_spconv<64x64x32>', 'out')}
for _m in SPLIT:
    for _arm in ('ring', 'lds'):
        ALL_VARIANTS[_m] |= {('k_spconv_h<256x64x32> ' + _arm, k) for k in ('subm', 'down')}
        ALL_VARIANTS[_m] |= {('k_spconv_h<256x128x32> ' + _arm, k) for k in ('subm', 'down', 'down011', 'out')}
    ALL_VARIANTS[_m] |= {('k_spconv_h<128x32x16> lds', 'subm'), ('k_spconv_h<128x32x16> lds', 'down'), ('k_spconv_h<128x32x32> lds', 'subm')}
    for _t_ in ('plain', 'packed'):
        ALL_VARIANTS[_m] |= {('k_spconv_w<16x16>', _t_), ('k_spconv_w<16x32>', _t_), ('k_spconv_w<32x32>', _t_)}
for _c in (32, 64, 128):
    for _arm in ('sort staged', 'sort gathermode', 'nosort staged', 'nosort gathermode'):
        ALL_VARIANTS['f32'].add(('k_spconv_xf<%d>' % _c, _arm))
        ALL_VARIANTS['f32'].add(('k_spconv_xt<%d>' % _c, _arm))
        for _m in SPLIT:
            ALL_VARIANTS[_m].add(('k_spconv_x<%d>' % _c, _arm))

# edges every engine family must be run at (the m edges are per INSTANCE, in units of its row tile).
#   overflow: a one-word counter holding cap + 5 in place of the level's row count, on a table whose cap rows are all live; the result must
#   equal the m == cap result bit for bit and the sentinel tail behind cap must survive.  It applies to the x-run families too: k_xwin
#   (the window prepass) and k_spconv_x / k_spconv_xf clamp the same counter the same way, m = min(*d_m_out, cap) (sparse_conv_x.hip,
#   sparse_conv_xf.hip) - the case builds its windows from the counter the convolution reads, as the detector does.
#   zero: the counter holds 0 with cap > 0 - nothing may be written.
M_EDGES = ('m=1', 'm=tile-1', 'm=tile', 'm=tile+1')
EDGES_REQUIRED = M_EDGES + ('dead tiles', 'm=cap', 'overflow', 'zero', 'unequal', 'isolated')
XCD_TILES = (1, 16, 17, 127, 128, 129)          # row tiles around the XCD deal of k_spconv_h (XRUN = 16 tiles x 8 XCDs)
FAMILIES = ('k_spconv', 'k_spconv_h', 'k_spconv_w', 'k_spconv_x', 'k_spconv_xf', 'k_spconv_xt')
XRUN_ENGINES = ('x', 'xf', 'xt')                # engine keys of the x-run families (pair16, fp32 MFMA, bf16x3)
LIMB3_ENGINES = ('xt', 'gt')                    # engine keys whose weights are pack_weight_limb3(w, cout_mult=32)
# the staging boundary of the x-run families: the longest (unit, slab) window of the level is exactly the staging capacity / one row more
WINDOW_EDGES = ('window=rcap', 'window=rcap+1')


# ------------------------------------------------------------------------------------------------------------------------
# the dispatch code, restated (csrc/sparse_conv.hip dz_spconv_forward, sparse_conv_h.hip spconv_h_select, sparse_conv_x.hip x_select):
# the instance a launch must report
# ------------------------------------------------------------------------------------------------------------------------
def expected_name(engine, cin, cout, kvol, masks):
    if engine == 'f32':
        return {(16, 16): 'k_spconv<128x16x16>', (16, 32): 'k_spconv<128x32x16>', (32, 32): 'k_spconv<128x32x32>'}.get((cin, cout), 'k_spconv<64x64x32>')
    if engine == 'x':
        return 'k_spconv_x<%d>' % cout
    if engine == 'xf':
        return 'k_spconv_xf<%d>' % cout
    if engine == 'xt':
        return 'k_spconv_xt<%d>' % cout
    if engine == 'packed':
        return 'k_spconv_w<%dx%d>' % (cin, cout)
    cp = max(cout, 32)
    if cp == 32 and masks:
        return 'k_spconv_w<%dx%d>' % (cin, cout)
    if cp == 32:
        return 'k_spconv_h<128x32x%d> lds' % cin
    return 'k_spconv_h<256x%dx32>' % cp + (' ring' if masks else ' lds')


def reported_name(engine, cin, cout, kvol, masks, cap):
    """What the library's own name functions say (host code: no GPU needed)."""
    lib = L.load()
    if engine == 'f32':
        return lib.dz_spconv_variant(cin, cout).decode()
    if engine == 'x':
        return lib.dz_spconv_x_variant(cin, cout).decode()
    if engine == 'xf':
        return lib.dz_spconv_x_f32_variant(cin, cout).decode()
    if engine == 'xt':
        return lib.dz_spconv_x_limb3_variant(cin, cout).decode()
    if engine == 'gt':
        return lib.dz_spconv_limb3_variant(cin, cout).decode()
    if engine == 'packed':
        return lib.dz_spconv_variant_split_packed(cin, cout).decode()
    return lib.dz_spconv_variant_split_arm(cin, cout, kvol, 1 if masks else 0, kvol * max(cap, 1) * 4).decode()


def tile_rows(name, cin=0, cout=0):
    """Row tile of an instance: the first template number of k_spconv / k_spconv_h, 32 per wave for k_spconv_w, the unit of the
    x-run kernels (dz_spconv_x_tile_rows)."""
    if name.startswith('k_spconv_w'):
        return 32
    if name.startswith('k_spconv_x'):
        return L.load().dz_spconv_x_tile_rows(cin, cout)
    return int(name[name.index('<') + 1:].split('x')[0])


def family(name):
    return name[:name.index('<')]


def window_capacity(engine, cin, cout):
    """Staging capacity of an x-run engine's kernel for the width: a (unit, slab) window of more rows runs in gather mode."""
    lib = L.load()
    fn = {'x': lib.dz_spconv_x_window_rows, 'xf': lib.dz_spconv_x_f32_window_rows, 'xt': lib.dz_spconv_x_limb3_window_rows}[engine]
    return fn(cin, cout)


# ------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------
def sp_case(engine, mode, cin, cout, kind, edge, masks=True, sort=False, sweep=False):
    kvol = int(np.prod(KINDS[kind][0]))
    name = expected_name(engine, cin, cout, kvol, masks)
    if engine == 'f32':
        arm = kind
    elif engine == 'packed':
        arm = 'packed'
    elif engine in XRUN_ENGINES:
        arm = ('sort ' if sort else 'nosort ') + ('gathermode' if edge in ('xgather', 'unequal', 'window=rcap+1') else 'staged')
    else:
        arm = 'plain' if name.startswith('k_spconv_w') else kind
    label = '%s %d->%d %s %s%s' % (engine, cin, cout, kind, edge, '' if engine not in XRUN_ENGINES else (' sort' if sort else ' nosort'))
    if engine == 'split':
        label += ' masks' if masks else ' nomasks'
    return types.SimpleNamespace(label=label, engine=engine, mode=mode, cin=cin, cout=cout, kind=kind, kvol=kvol, edge=edge, masks=masks,
                                 sort=sort, expect=name, arm=arm, sweep=sweep)


def _coverage_cases():
    cs = []
    # edges the strided kinds take in turn (their m is whatever the output set is: the exact-m edges are run on the submanifold layer
    # of the same instance) and the ones the submanifold layers take in turn
    strided = ('dead tiles', 'm=cap', 'unequal', 'overflow')
    # (not 'zero': every (layer, mode, arm) of these loops must compute something - the empty level is in the per-instance sweeps below)
    subm = ('unequal', 'dead tiles', 'm=cap', 'overflow', 'isolated', 'plain')
    n = [0]

    def nxt(kind):
        seq = subm if kind == 'subm' else strided
        n[0] += 1
        return seq[n[0] % len(seq)]
    # fp32 gather: every layer; split gather / small-channel: every layer x mode x (tile masks, none)
    for cin, cout, kind in LAYERS:
        cs.append(sp_case('f32', 'f32', cin, cout, kind, nxt(kind)))
        for mode in SPLIT:
            for masks in (True, False):
                cs.append(sp_case('split', mode, cin, cout, kind, nxt(kind), masks=masks))
            if cout <= 32:
                cs.append(sp_case('packed', mode, cin, cout, kind, nxt(kind)))
    # x-run engines: tap-set order or not, on a level of staged windows and on one with windows beyond the staging capacity
    for c in (32, 64, 128):
        for sort in (True, False):
            for edge in ('xgather', 'plain', 'unequal'):
                cs.append(sp_case('xf', 'f32', c, c, 'subm', edge, sort=sort))
                cs.append(sp_case('xt', 'f32', c, c, 'subm', edge, sort=sort))
                for mode in SPLIT:
                    cs.append(sp_case('x', mode, c, c, 'subm', edge, sort=sort))
            # ... and at the staging boundary itself
            for edge in WINDOW_EDGES:
                for engine, mode in (('x', 'f16x2'), ('xf', 'f32'), ('xt', 'f32')):
                    cs.append(sp_case(engine, mode, c, c, 'subm', edge, sort=sort))
    # per instance: the exact-m edges of its row tile and the rest of EDGES_REQUIRED, on its submanifold layer (16 -> 32: the instance
    # has no submanifold layer in the backbone; the kernel does not know - run as one), f32 / f16x2
    inst = {}
    for cin, cout, kind in LAYERS:
        for engine, mode in (('f32', 'f32'), ('split', 'f16x2'), ('packed', 'f16x2'), ('x', 'f16x2'), ('xf', 'f32'), ('xt', 'f32')):
            if engine == 'packed' and cout > 32 or engine in XRUN_ENGINES and (cin != cout or cin < 32):
                continue
            for masks in ((True, False) if engine == 'split' else (True,)):
                name = expected_name(engine, cin, cout, 27, masks)
                inst.setdefault((engine, name, masks), (mode, cin, cout))
    for (engine, name, masks), (mode, cin, cout) in inst.items():
        for edge in M_EDGES + ('dead tiles', 'm=cap', 'overflow', 'zero', 'unequal', 'isolated'):
            cs.append(sp_case(engine, mode, cin, cout, 'subm', edge, masks=masks, sort=cout >= 64, sweep=True))
        if name.startswith('k_spconv_h<256'):
            for t in XCD_TILES:
                cs.append(sp_case(engine, mode, cin, cout, 'subm', 'tiles=%d' % t, masks=masks, sweep=True))
    seen, out = set(), []
    for c in cs:                                    # (the two loops meet in a few cases)
        if (c.label, c.mode) not in seen:
            seen.add((c.label, c.mode))
            out.append(c)
    return out


COVERAGE = _coverage_cases()


def _ids(cases):
    return ['%s [%s]' % (c.label, c.mode) for c in cases]


# ------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ------------------------------------------------------------------------------------------------------------------------
def ref64(x64, tab, w64, m, chunk=1 << 20):
    """float64 evaluation of the rulebook `tab` (kvol, >= m; -1 = absent; indices into the rows of x64) with weights w64 (kvol, cin, cout):
    (sum x.w, sum |x.w|), each (m, cout), on the device of x64.  Per tap one index_add_ of x[idx] @ w[tap], in chunks of rows."""
    kvol, cout = w64.shape[0], w64.shape[2]
    acc = torch.zeros((m, cout), dtype=torch.float64, device=x64.device)
    aacc = torch.zeros_like(acc)
    wa = w64.abs()
    for t in range(kvol):
        idx = tab[t, :m].long()
        rows = torch.nonzero(idx >= 0).squeeze(1)
        for r0 in range(0, rows.numel(), chunk):
            r = rows[r0:r0 + chunk]
            src = x64[idx[r]]
            acc.index_add_(0, r, src @ w64[t])
            aacc.index_add_(0, r, src.abs() @ wa[t])
    return acc, aacc


def normalised_error(got, acc, aacc, scale, shift, res, relu):
    """e per element: |got - ref| / (|scale| * sum|x.w| + |shift| + |residual|); NaN in got -> inf.  Absent operands are None."""
    ref, den = acc, aacc
    if scale is not None:
        ref, den = ref * scale, den * scale.abs()
    if shift is not None:
        ref, den = ref + shift, den + shift.abs()
    if res is not None:
        ref, den = ref + res, den + res.abs()
    if relu:
        ref = ref.clamp_min(0.0)
    err = (got - ref).abs() / den.clamp_min(1e-30)
    return torch.where(torch.isnan(got), torch.full_like(err, float('inf')), err), ref, den


def _decode(x, mode):
    math = ops.math_id(mode)
    return (ops.pair16_unpack(x, math) if math else x).double()


# ------------------------------------------------------------------------------------------------------------------------
# geometry of a case
# ------------------------------------------------------------------------------------------------------------------------
def _coords_exact(rng, m, batch=1):
    """m distinct cells of a 5-slab grid about a third full, canonical order."""
    hw = max(4, int(np.ceil(np.sqrt(3.0 * m / (5 * batch) + 8))))
    shape = [5, hw, hw + 3]
    cells = shape[0] * shape[1] * shape[2]
    lin = np.sort(rng.choice(batch * cells, size=m, replace=False))
    return _lin_to_coords(lin, shape), shape


def _lin_to_coords(lin, shape):
    cells, slab = shape[0] * shape[1] * shape[2], shape[1] * shape[2]
    return np.stack([lin // cells, (lin % cells) // slab, (lin // shape[2]) % shape[1], lin % shape[2]], 1).astype(np.int32)


def _coords_density(rng, batch, shape, d):
    cells = shape[0] * shape[1] * shape[2]
    lin = np.nonzero(rng.random(batch * cells) < d)[0]
    return _lin_to_coords(lin, shape)


def _make_level(coords, batch, shape, cap, dev):
    lvl = ops.SparseLevel(batch, shape, cap, dev)
    lvl.build_from_coords(_t(coords, dev), want_rank=False)
    m = coords.shape[0]
    assert lvl.num_active() == m and torch.equal(lvl.coords[:m].cpu(), torch.from_numpy(coords)), 'level rows are not in canonical order'
    return lvl


def host_windows(coords, shape, unit):
    """Rows of the (unit, z offset) windows of a level's submanifold 3 x 3 x 3 table, on the host: per unit of `unit` consecutive rows
    (canonical order) and z offset the span first .. last input row its nine taps of that offset reference, 0 where there is none - what
    k_xwin computes from the packed table.  (units, 3) int64."""
    m = coords.shape[0]
    c = coords.astype(np.int64)
    d, h, w = shape
    batch = int(c[:, 0].max()) + 1 if m else 1
    grid = np.full(batch * d * h * w, -1, dtype=np.int64)
    grid[((c[:, 0] * d + c[:, 1]) * h + c[:, 2]) * w + c[:, 3]] = np.arange(m)
    units = -(-m // unit)
    out = np.zeros((units, 3), dtype=np.int64)
    first = np.arange(units) * unit
    for tz in range(3):
        lo = np.full(m, np.iinfo(np.int64).max)
        hi = np.full(m, -1)
        z = c[:, 1] + tz - 1
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                y, x = c[:, 2] + dy, c[:, 3] + dx
                ok = (z >= 0) & (z < d) & (y >= 0) & (y < h) & (x >= 0) & (x < w)
                idx = np.where(ok, grid[np.where(ok, ((c[:, 0] * d + z) * h + y) * w + x, 0)], -1)
                lo = np.where(idx >= 0, np.minimum(lo, idx), lo)
                hi = np.maximum(hi, idx)
        ulo, uhi = np.minimum.reduceat(lo, first), np.maximum.reduceat(hi, first)
        out[:, tz] = np.where(uhi >= 0, uhi - ulo + 1, 0)
    return out


@functools.lru_cache(maxsize=None)
def window_coords(rcap, unit, target):
    """A one-frame level of three identical z slabs whose longest (unit, slab) window has exactly `target` (rcap or rcap + 1) rows.
    Every line of a slab holds the cells x < W, so the unit of rows (y0, x0) .. (y1, x1) references, in each slab it has neighbours in,
    the rows (y0 - 1, x0 - 1) .. (y1 + 1, x1 + 1): unit + (cells of line y0 - 1) + (cells of line y1) + 2 of them (one fewer per end
    whose corner lies outside the line).  W = (rcap - unit - 2) / 2 gives rcap; for rcap + 1 one line holds one cell more (the grid is
    W + 1 wide), so a unit that ends in that line or starts in the line after it is one row over and no unit two.  The height and the
    long line are searched on the host model (host_windows) until the longest window is `target` - the GPU's own windows are what the
    case asserts.  Returns (coords, shape)."""
    assert target in (rcap, rcap + 1) and (rcap - unit - 2) % 2 == 0 and rcap - unit - 2 >= 6, (rcap, unit, target)
    w = (rcap - unit - 2) // 2
    h0 = -(-3 * unit // w) + 3
    for h in range(h0, h0 + 6):
        for long_line in ((None,) if target == rcap else range(1, h - 1)):
            shape = [3, h, w + 1]
            cells = [(0, z, y, x) for z in range(3) for y in range(h) for x in range(w + (1 if y == long_line else 0))]
            coords = np.array(cells, dtype=np.int32)
            wins = host_windows(coords, shape, unit)
            if int(wins.max()) == target and int((wins == target).sum()) >= 1:
                return coords, shape
    raise AssertionError(('no level of full slabs with a longest window of %d rows' % target, rcap, unit))


def subm_coords(case, tile, rng):
    """Coordinates of a submanifold case's level (host only): (coords, batch, shape)."""
    edge = case.edge
    batch = 1
    if edge in ('unequal', 'xgather'):
        batch, shape = (2, [4, 40, 56]) if edge == 'unequal' else (1, [4, 48, 64])
        cells, slab = shape[0] * shape[1] * shape[2], shape[1] * shape[2]
        lin = [b * cells + z * slab + np.nonzero(rng.random(slab) < UNEQUAL[(b + z) % 4])[0] for b in range(batch) for z in range(shape[0])]
        coords = _lin_to_coords(np.unique(np.concatenate(lin)), shape)
    elif edge == 'isolated':
        shape = [7, 31, 46]
        g = np.stack(np.meshgrid(np.arange(1, 7, 3), np.arange(1, 31, 3), np.arange(1, 46, 3), indexing='ij'), -1).reshape(-1, 3)
        g = g[rng.random(g.shape[0]) < 0.8]
        coords = np.concatenate([np.zeros((g.shape[0], 1), np.int64), g], 1).astype(np.int32)
    elif edge == 'plain':
        shape = [5, 30, 44]
        coords = _coords_density(rng, 1, shape, 0.25)
    elif edge in WINDOW_EDGES:
        rcap = window_capacity(case.engine, case.cin, case.cout)
        coords, shape = window_coords(rcap, tile, rcap + (1 if edge == 'window=rcap+1' else 0))
    else:
        coords, shape = _coords_exact(rng, edge_rows(edge, tile))
    return coords, batch, shape


def case_rng(case):
    return np.random.default_rng(zlib.crc32(('%s|%s' % (case.label, case.mode)).encode()))


def edge_rows(edge, tile):
    """Rows of the output level an exact-m edge asks for (None: the edge does not fix m)."""
    if edge.startswith('tiles='):
        return (int(edge[6:]) - 1) * tile + 5
    return {'m=1': 1, 'm=tile-1': tile - 1, 'm=tile': tile, 'm=tile+1': tile + 1, 'dead tiles': 3 * tile + 5, 'zero': 2 * tile + 9,
            'm=cap': 2 * tile + 11, 'overflow': 2 * tile}.get(edge)


def build_geometry(case, tile, rng, dev):
    """Levels of a case: (lvl_in, lvl_out, coords_in, coords_out, counter) - counter: the value the launch sees in place of the level's
    own row count (None = the level's)."""
    k, s, p = KINDS[case.kind]
    edge = case.edge
    subm = case.kind == 'subm'
    if subm:
        coords, batch, shape = subm_coords(case, tile, rng)
        m = coords.shape[0]
        cap = m + {'dead tiles': 2 * tile + 3, 'm=cap': 0, 'overflow': 0}.get(edge, 0 if edge.startswith('m=') else 7)
        lvl = _make_level(coords, batch, shape, cap, dev)
        lvl_in, lvl_out, cin_, cout_ = lvl, lvl, coords, coords
    else:
        if edge == 'unequal':
            batch, shape = 2, [9, 40, 48]
            lvl_in, cin_ = _level(rng, batch, shape, UNEQUAL, dev)
            assert torch.equal(lvl_in.coords[:cin_.shape[0]].cpu(), torch.from_numpy(cin_))
        else:
            batch, shape = 1, [11, 48, 64]
            cin_ = _coords_density(rng, 1, shape, 0.05)
            lvl_in = _make_level(cin_, batch, shape, cin_.shape[0] + 7, dev)
        cout_, oshape = osp.conv_out_coords(cin_, shape, k, s, p)
        m = cout_.shape[0]
        cap = m + {'dead tiles': 2 * tile + 3, 'm=cap': 0, 'overflow': 0}.get(edge, 7)
        lvl_out = lvl_in.downsample(k, s, p, cap=cap)
        assert lvl_out.shape == [int(v) for v in oshape] and lvl_out.num_active() == m
        assert torch.equal(lvl_out.coords[:m].cpu(), torch.from_numpy(cout_)), 'output set differs from the oracle'
    if edge == 'dead tiles':
        assert lvl_out.cap - m >= 2 * tile
    if edge in ('m=cap', 'overflow'):
        assert lvl_out.cap == m
    counter = {'overflow': lvl_out.cap + 5, 'zero': 0}.get(edge)
    return lvl_in, lvl_out, cin_, cout_, counter


# ------------------------------------------------------------------------------------------------------------------------
# one launch configuration against the reference
# ------------------------------------------------------------------------------------------------------------------------
def gpu_tables(case, lvl_in, lvl_out, d_m, sort):
    """The table the case's engine reads, built by the library: (nbr, xwin or None)."""
    k, s, p = KINDS[case.kind]
    if case.engine in ('f32', 'split', 'gt'):
        return lvl_in.neighbors_to(lvl_out, k, s, p), None
    nbr = lvl_in.neighbors_to(lvl_out, k, s, p, packed=True)
    assert nbr.packed, 'the library did not build a packed table for this layer'
    if case.engine == 'packed':
        return nbr, None
    saved = ops.XRUN_SORT, ops.XRUN_SORT_MIN_CHANNELS
    try:
        ops.XRUN_SORT, ops.XRUN_SORT_MIN_CHANNELS = True, (0 if sort else 1 << 20)
        # (the windows read the counter the convolution will read)
        nbr = ops.build_windows(nbr, types.SimpleNamespace(d_m=d_m), case.cout)
    finally:
        ops.XRUN_SORT, ops.XRUN_SORT_MIN_CHANNELS = saved
    assert nbr.xwin is not None and (nbr.xwin[3] is not None) == sort
    return nbr, nbr.xwin


def check_tables(case, nbr, xwin, tab, m):
    """The GPU table(s) of the launch against the oracle's `tab` (kvol, m) on the rows < m."""
    if m == 0:
        return
    got = ops.unpack_table(nbr)[:, :m]
    assert torch.equal(got.int(), tab.int()), (case.label, 'the neighbour table differs from the oracle')
    if xwin is not None and xwin[3] is not None:
        perm = xwin[3][:m].long()
        tr = xwin[1]
        pos = torch.arange(m, device=perm.device)
        assert torch.equal(torch.sort(perm).values, pos) and torch.equal(perm // tr, pos // tr), (case.label, 'perm is not a permutation within units')
        srt = ops.NeighborTable(xwin[2][:, :m].clone(), packed=True)
        assert torch.equal(ops.unpack_table(srt).int(), tab[:, perm].int()), (case.label, 'the tap-set-ordered table differs from the oracle')


def launch(case, x, in_rows, nbr, xwin, masks, cap, d_m, w, sc, sh, res, relu, out):
    lib = L.load()
    math = ops.math_id(case.mode)
    p = L.ptr
    if case.engine == 'f32':
        rc = lib.dz_spconv_forward(p(x), in_rows, case.cin, p(nbr.words), case.kvol, cap, p(d_m), p(w), p(sc), p(sh), p(res), relu, p(out), case.cout, L.stream())
    elif case.engine == 'split':
        rc = lib.dz_spconv_forward_split(p(x), in_rows, case.cin, p(nbr.words), p(masks), case.kvol, cap, p(d_m), p(w), p(sc), p(sh), p(res), relu, p(out),
                                         case.cout, math, L.stream())
    elif case.engine == 'packed':
        rc = lib.dz_spconv_forward_split_packed(p(x), in_rows, case.cin, p(nbr.words), p(masks), cap, p(d_m), p(w), p(sc), p(sh), p(res), relu, p(out),
                                                case.cout, math, L.stream())
    elif case.engine == 'gt':
        assert masks is not None and not nbr.packed, (case.label, 'k_spconv_gt reads a plain table with tile masks')
        rc = lib.dz_spconv_forward_limb3(p(x), in_rows, case.cin, p(nbr.words), p(masks), case.kvol, cap, p(d_m), p(w), p(sc), p(sh), p(res), relu, p(out),
                                         case.cout, L.stream())
    else:
        tabx = xwin[2] if xwin[3] is not None else nbr.words
        if case.engine == 'xt':
            rc = lib.dz_spconv_forward_x_limb3(p(x), in_rows, case.cin, p(tabx), p(xwin[3]), p(xwin[0]), xwin[1], cap, p(d_m), p(w), p(sc), p(sh), p(res),
                                               relu, p(out), case.cout, L.stream())
        elif case.engine == 'x':
            rc = lib.dz_spconv_forward_split_x(p(x), in_rows, case.cin, p(tabx), p(xwin[3]), p(xwin[0]), xwin[1], cap, p(d_m), p(w), p(sc), p(sh), p(res),
                                               relu, p(out), case.cout, math, L.stream())
        else:
            rc = lib.dz_spconv_forward_x_f32(p(x), in_rows, case.cin, p(tabx), p(xwin[3]), p(xwin[0]), xwin[1], cap, p(d_m), p(w), p(sc), p(sh), p(res),
                                             relu, p(out), case.cout, L.stream())
    msg = lib.dz_last_error()
    assert rc == 0, (case.label, case.mode, rc, msg.decode() if msg else '')


def convolve_and_check(case, lvl_in, lvl_out, nbr, xwin, tab, m_in, counter, dev, seed=None):
    """`case` on the given levels and GPU table against float64 on the oracle's table `tab` (kvol, m_out) (device, int).  Returns
    (reported name, worst normalised error, tile rows)."""
    mode, math = case.mode, ops.math_id(case.mode)
    cin, cout, kvol = case.cin, case.cout, case.kvol
    cap, in_rows = lvl_out.cap, lvl_in.cap
    masks = nbr.tile_masks if case.masks else None
    name = reported_name(case.engine, cin, cout, kvol, masks is not None, cap)
    if case.expect is not None:
        assert name == case.expect, (case.label, mode, name, case.expect)
    d_m = lvl_out.d_m if counter is None else torch.tensor([counter], dtype=torch.int32, device=dev)
    m_level = lvl_out.num_active()
    m = min(m_level if counter is None else counter, cap)
    if counter is not None and counter > cap:
        assert m_level == cap, 'the overflow case needs a table whose cap rows are all live'
    check_tables(case, nbr, xwin, tab, min(m, m_level))
    assert m == 0 or int(tab[:, :m].max()) < m_in, 'the oracle table points past the live input rows'
    gen = torch.Generator(device=dev)
    gen.manual_seed(zlib.crc32(('%s|%s' % (case.label, mode)).encode()) if seed is None else seed)

    # operands: N(0, 1) rows and weights, the BatchNorm scale sized so that outputs are O(1); poison where nothing may be read
    x32 = torch.randn((in_rows, cin), generator=gen, device=dev)
    r32 = torch.randn((cap, cout), generator=gen, device=dev)
    w32 = torch.randn((kvol, cin, cout), generator=gen, device=dev)
    sc = ((torch.rand(cout, generator=gen, device=dev) + 0.5) / (kvol * cin) ** 0.5).contiguous()
    sh = (torch.randn(cout, generator=gen, device=dev) * 0.5).contiguous()
    if math:
        x, r = ops.pair16_from_f32(x32, math=math), ops.pair16_from_f32(r32, math=math)
        wk = ops.pack_weight_split(w32, ops.storage_math(math))                   # (kvol, cout_pad, cin) pair16
        w64 = _decode(wk, mode).transpose(-1, -2)[..., :cout].contiguous()
    else:
        # (bf16x3: the three limbs of a weight sum to it exactly - the reference is the fp32 operands')
        x, r, wk = x32.clone(), r32.clone(), (ops.pack_weight_limb3(w32, cout_mult=32) if case.engine in LIMB3_ENGINES else w32.contiguous())
        w64 = w32.double()
    del x32, r32
    x.view(torch.int32)[m_in:] = POISON
    r.view(torch.int32)[m:] = POISON
    x64, r64 = _decode(x[:m_in], mode), _decode(r[:m], mode)
    acc, aacc = ref64(x64, tab, w64, m)
    del x64

    worst = 0.0
    results = []
    for on in (True, False):
        outs = [torch.full((cap + TAIL, cout), SENTINEL, dtype=torch.int32, device=dev) for _ in range(2)]
        for o in outs:
            launch(case, x, in_rows, nbr, xwin, masks, cap, d_m, wk, sc if on else None, sh if on else None, r if on else None, 1 if on else 0, o)
        torch.cuda.synchronize(dev)
        what = (case.label, mode, name, 'all on' if on else 'all off')
        assert torch.equal(outs[0], outs[1]), ('two launches differ',) + what
        out = outs[0]
        nbad = int((out[m:] != SENTINEL).sum())
        assert nbad == 0, ('%d words written at or beyond row m = %d (cap %d)' % (nbad, m, cap),) + what
        results.append(out[:m].clone())
        if m == 0:
            continue
        nkept = int((out[:m] == SENTINEL).sum())
        assert nkept == 0, ('%d words below row m = %d were not written' % (nkept, m),) + what
        got = out[:m].contiguous().view(torch.float32)
        got = _decode(got, mode) if math else got.double()
        err, ref, den = normalised_error(got, acc, aacc, sc.double() if on else None, sh.double() if on else None, r64 if on else None, on)
        e = float(err.max())
        if not e <= BOUND[mode]:
            i = int(torch.argmax(err.flatten()))
            raise AssertionError('%s [%s] %s %s: normalised error %.3e > %.3e (row %d channel %d of m = %d: got %r ref %r den %r)' % (
                case.label, mode, name, what[3], e, BOUND[mode], i // cout, i % cout, m, float(got.flatten()[i]), float(ref.flatten()[i]),
                float(den.flatten()[i])))
        worst = max(worst, e)
    if xwin is not None:
        assert not bool(xwin[0][-16:].any()), (case.label, 'the tile-queue words behind the windows are not back at zero')
    tr = tile_rows(name, cin, cout)
    print('  %-44s %-7s %-28s %-18s m %7d cap %7d  worst normalised error %.3e (bound %.1e)' % (case.label, mode, name, case.arm or '-', m, cap, worst,
                                                                                                     BOUND[mode]))
    return name, worst, tr, results


def run_case(case, dev):
    """Build the case's levels and tables, check the tables against the oracle, convolve.  Returns (name, worst e)."""
    name = case.expect
    tile = tile_rows(name, case.cin, case.cout)
    lvl_in, lvl_out, cin_, cout_, counter = build_geometry(case, tile, case_rng(case), dev)
    k, s, p = KINDS[case.kind]
    tab = _t(osp.neighbor_table(cin_, lvl_in.shape, cout_, k, s, p), dev)
    m_in = cin_.shape[0]
    d_m = lvl_out.d_m if counter is None else torch.tensor([counter], dtype=torch.int32, device=dev)
    nbr, xwin = gpu_tables(case, lvl_in, lvl_out, d_m, case.sort)
    if case.engine in XRUN_ENGINES and case.edge in ('xgather', 'unequal', 'plain') + WINDOW_EDGES and counter is None:
        rcap = window_capacity(case.engine, case.cin, case.cout)
        nt = (lvl_out.cap + xwin[1] - 1) // xwin[1]
        wins = xwin[0][:nt * 6].view(-1, 3, 2)[..., 1]
        longest = int(wins.max())
        assert rcap > 0 and (longest > rcap) == ('gathermode' in case.arm), (case.label, longest, rcap)
        if case.edge in WINDOW_EDGES:
            # the staging boundary, read back from the windows the library built
            target = rcap + (1 if case.edge == 'window=rcap+1' else 0)
            hit = int((wins == target).sum())
            print('  %-44s windows of the library: longest %d, %d of exactly %d rows (staging capacity %d)' % (case.label, longest, hit, target, rcap))
            assert hit >= 1, (case.label, 'no window of exactly %d rows' % target, longest, rcap)
            if case.edge == 'window=rcap':
                assert longest == rcap, (case.label, 'a window longer than the staging capacity', longest, rcap)
            host = np.zeros((nt, 3), dtype=np.int64)
            hw = host_windows(cin_, lvl_in.shape, xwin[1])
            host[:hw.shape[0]] = hw
            assert np.array_equal(wins.cpu().numpy().astype(np.int64), host), (case.label, 'the windows differ from the host model')
    name, worst, tr, res = convolve_and_check(case, lvl_in, lvl_out, nbr, xwin, tab, m_in, counter, dev)
    if case.edge == 'overflow':
        # the overflowed counter must give exactly what the exact counter gives
        exact = types.SimpleNamespace(**vars(case))
        nbr2, xwin2 = gpu_tables(exact, lvl_in, lvl_out, lvl_out.d_m, case.sort)
        _, _, _, res2 = convolve_and_check(exact, lvl_in, lvl_out, nbr2, xwin2, tab, m_in, None, dev)
        assert all(torch.equal(a, b) for a, b in zip(res, res2)), (case.label, 'the overflowed counter changed the result')
    return name, worst


# ------------------------------------------------------------------------------------------------------------------------
# no GPU needed: the table, the reference, the bound
# ------------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_every_variant():
    """The name functions report the (instance, arm) every case expects; the cases reach every entry of ALL_VARIANTS in every math mode;
    every engine family is run at every edge of EDGES_REQUIRED, every instance at the four m edges of its row tile, the two
    k_spconv_h production tiles at the tile counts around the XCD deal."""
    reached = {m: set() for m in MODES}
    fam_edges, inst_edges = {}, {}
    for c in COVERAGE:
        name = reported_name(c.engine, c.cin, c.cout, c.kvol, c.masks, 1000)
        assert name == c.expect, (c.label, c.mode, name, c.expect)
        reached[c.mode].add((name, c.arm))
        fam_edges.setdefault(family(name), set()).add(c.edge)
        inst_edges.setdefault(name, set()).add(c.edge)
        t = tile_rows(name, c.cin, c.cout)
        assert t in (32, 64, 128, 256), (name, t)
        rows = edge_rows(c.edge, t)
        if c.edge in M_EDGES:
            assert rows == {'m=1': 1, 'm=tile-1': t - 1, 'm=tile': t, 'm=tile+1': t + 1}[c.edge]
        if c.edge.startswith('tiles='):
            assert -(-rows // t) == int(c.edge[6:])
    for m in MODES:
        print('  %-7s %d (instance, arm) pairs' % (m, len(reached[m])))
        assert reached[m] >= ALL_VARIANTS[m], (m, sorted(ALL_VARIANTS[m] - reached[m]))
        # (beyond ALL_VARIANTS only: arms of edge sweeps that repeat an instance on its submanifold layer)
        assert {n for n, _ in reached[m]} == {n for n, _ in ALL_VARIANTS[m]}, (m, sorted({n for n, _ in reached[m]} ^ {n for n, _ in ALL_VARIANTS[m]}))
    assert set(fam_edges) == set(FAMILIES), sorted(fam_edges)
    for fam in FAMILIES:
        assert fam_edges[fam] >= set(EDGES_REQUIRED), (fam, sorted(set(EDGES_REQUIRED) - fam_edges[fam]))
    for name, edges in inst_edges.items():
        assert edges >= set(M_EDGES), (name, sorted(set(M_EDGES) - edges))
    for name in ('k_spconv_h<256x64x32> ring', 'k_spconv_h<256x128x32> ring', 'k_spconv_h<256x64x32> lds', 'k_spconv_h<256x128x32> lds'):
        assert inst_edges[name] >= {'tiles=%d' % t for t in XCD_TILES}, name
    lib = L.load()
    assert lib.dz_spconv_variant_split(64, 64) == b'k_spconv_h<256x64x32>' and lib.dz_spconv_variant_split(128, 128) == b'k_spconv_h<256x128x32>'
    assert lib.dz_spconv_variant_split(16, 16) == b'k_spconv_w<16x16>' and lib.dz_spconv_variant_split(48, 48) == b'none'


def test_xrun_cases_reach_their_arm_on_the_host_model():
    """The window model of the host (host_windows: first .. last referenced row per unit and z offset) on every x-run case whose arm
    depends on the level: the longest window is above the kernel's staging capacity exactly where the case says 'gathermode'; a
    'window=rcap' level holds a window of exactly the capacity and none longer, a 'window=rcap+1' level one of exactly one row more
    and none longer.  (The GPU cases assert the same from the windows the library builds, and those against this model.)"""
    seen = set()
    for c in COVERAGE:
        if c.engine not in XRUN_ENGINES or c.edge not in ('xgather', 'unequal', 'plain') + WINDOW_EDGES:
            continue
        unit = tile_rows(c.expect, c.cin, c.cout)
        rcap = window_capacity(c.engine, c.cin, c.cout)
        coords, batch, shape = subm_coords(c, unit, case_rng(c))
        wins = host_windows(coords, shape, unit)
        longest = int(wins.max())
        assert rcap > 0 and (longest > rcap) == ('gathermode' in c.arm), (c.label, c.mode, longest, rcap)
        if c.edge in WINDOW_EDGES:
            target = rcap + (1 if c.edge == 'window=rcap+1' else 0)
            assert longest == target and int((wins == target).sum()) >= 1, (c.label, longest, target)
            assert 1000 <= coords.shape[0] <= 8000, (c.label, coords.shape[0])
            seen.add((c.engine, c.cout, c.sort, c.edge))
    assert seen == {(e, w, s, edge) for e in XRUN_ENGINES for w in (32, 64, 128) for s in (True, False) for edge in WINDOW_EDGES}
    # the model itself, on levels small enough to check by hand: one line of 6 cells in units of 2 rows (rows 0, 1 reference rows 0..2,
    # rows 2, 3 rows 1..4, rows 4, 5 rows 3..5); two slabs of one 3-cell line each in units of 3 rows (each slab sees itself and the other)
    line = np.array([(0, 0, 0, x) for x in range(6)], dtype=np.int32)
    assert host_windows(line, [1, 1, 6], 2).tolist() == [[0, 3, 0], [0, 4, 0], [0, 3, 0]]
    slabs = np.array([(0, z, 0, x) for z in range(2) for x in range(3)], dtype=np.int32)
    assert host_windows(slabs, [2, 1, 3], 3).tolist() == [[0, 3, 3], [3, 3, 0]]


# every variable the sparse-convolution launch code once read, at a value that used to select another instance, tile or schedule
REMOVED_ENVS = {'DZ_TUNE_SPCONV64': '1', 'DZ_TUNE_SPCONV128': '1', 'DZ_TUNE_SPCONV_W': '0', 'DZ_TUNE_SPCONV_NOGN': '1', 'DZ_TUNE_W16': '0',
                'DZ_TUNE_W1632': '1', 'DZ_TUNE_SPCONV_D': '1', 'DZ_TUNE_W_DIAG': '1', 'DZ_TUNE_X32': '1', 'DZ_TUNE_XRUN': '1', 'DZ_TUNE_X_STEAL': '0',
                'DZ_TUNE_X_SINGLES': '1', 'DZ_TUNE_X_SLOAD': '0', 'DZ_TUNE_X_DIAG': '1'}
_NAMES_CHILD = """
import json
from detzero_amd import lib as L
from tests import test_gpu_sparse_conv as T
print(json.dumps({'names': [T.reported_name(c.engine, c.cin, c.cout, c.kvol, c.masks, 1000) for c in T.COVERAGE],
                  'unit_rows': [L.load().dz_spconv_x_tile_rows(c, c) for c in (32, 64, 128)]}))
"""


def test_selection_reads_no_environment_variable():
    """The name functions and dz_spconv_x_tile_rows in a child process (the variables were read once per process) started with every
    variable of REMOVED_ENVS set: exactly the defaults, for every case of COVERAGE and for 32 / 64 / 128 channels."""
    e = dict(os.environ)
    e.update(REMOVED_ENVS)
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    p = subprocess.run([sys.executable, '-c', _NAMES_CHILD], env=e, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1])
    assert len(got['names']) == len(COVERAGE)
    for c, name in zip(COVERAGE, got['names']):
        assert name == c.expect, (c.label, c.mode, name, c.expect)
    assert got['unit_rows'] == [256, 256, 128], got['unit_rows']


def test_reference_agrees_with_oracle_and_conv3d():
    """ref64 against oracle.sparse.sparse_conv in float64 and against dense F.conv3d on a small grid, submanifold and strided (both
    paddings of the backbone and conv_out), with in_rows != m."""
    rng = np.random.default_rng(5)
    g = torch.Generator().manual_seed(5)
    shape, cin, cout = [7, 10, 12], 8, 5
    coords = _coords_density(rng, 2, shape, 0.3)
    m_in = coords.shape[0]
    x = torch.randn((m_in + 3, cin), generator=g, dtype=torch.float64)
    x[m_in:] = float('nan')
    dense = torch.zeros((2, cin, *shape), dtype=torch.float64)
    cc = torch.from_numpy(coords.astype(np.int64))
    dense[cc[:, 0], :, cc[:, 1], cc[:, 2], cc[:, 3]] = x[:m_in]
    for kind, (k, s, p) in KINDS.items():
        oc = coords if kind == 'subm' else osp.conv_out_coords(coords, shape, k, s, p)[0]
        m = oc.shape[0]
        assert kind == 'subm' or m != m_in
        kvol = k[0] * k[1] * k[2]
        w = torch.randn((kvol, cin, cout), generator=g, dtype=torch.float64)
        tab = torch.from_numpy(osp.neighbor_table(coords, shape, oc, k, s, p))
        acc, aacc = ref64(x, tab, w, m, chunk=97)
        assert not bool(torch.isnan(acc).any())
        rb = osp.build_rulebook(coords, shape, oc, k, s, p)
        assert torch.allclose(acc, osp.sparse_conv(x[:m_in], rb, w, m), rtol=1e-12, atol=1e-12)
        assert torch.allclose(aacc, osp.sparse_conv(x[:m_in].abs(), rb, w.abs(), m), rtol=1e-12, atol=1e-12)
        w5 = w.reshape(*k, cin, cout).permute(4, 3, 0, 1, 2)
        full = F.conv3d(dense, w5, stride=s, padding=p)
        oo = torch.from_numpy(oc.astype(np.int64))
        assert torch.allclose(acc, full[oo[:, 0], :, oo[:, 1], oo[:, 2], oo[:, 3]], rtol=1e-12, atol=1e-12), kind
        # the metric: exact on the reference itself, infinite on a NaN
        sc, sh, r = torch.rand(cout, dtype=torch.float64) + 0.5, torch.randn(cout, dtype=torch.float64), torch.randn((m, cout), dtype=torch.float64)
        ref = (acc * sc + sh + r).clamp_min(0.0)
        e, _, _ = normalised_error(ref.clone(), acc, aacc, sc, sh, r, True)
        assert float(e.max()) == 0.0
        ref[0, 0] = float('nan')
        assert float(normalised_error(ref, acc, aacc, sc, sh, r, True)[0].max()) == float('inf')


@pytest.mark.parametrize('cin', (16, 32, 64, 128))
def test_bound_detects_a_dropped_unit(cin):
    """The smallest defect each mode's bound catches, shown on the reference itself: one 8-channel group of one tap removed from every
    row (what a skipped 8-channel pair16 group, a skipped LDS fragment or a wrong tap mask bit does).  2000 rows with all 27 taps
    present, N(0, 1) rows and weights and the module's scale / shift / residual, all in the denominator: the worst element is 2^-4.2 (16
    channels) to 2^-7.1 (128 channels) away (printed), above every BOUND - the loosest, 'f16' at 2^-9, sees the group at 128 channels only
    through the MAXIMUM over rows and channels (the median element is at 2^-10.4 there), which is why the metric is a maximum over every
    element.  A whole dropped tap is at 2^-3.8 to 2^-5.3."""
    g = torch.Generator().manual_seed(cin)
    m, cout, kvol = 2000, cin, 27
    x = torch.randn((m + 26, cin), generator=g, dtype=torch.float64)
    tab = (torch.arange(m)[None, :] + torch.arange(kvol)[:, None]).int()            # every tap present, distinct rows
    w = torch.randn((kvol, cin, cout), generator=g, dtype=torch.float64)
    sc = (torch.rand(cout, generator=g, dtype=torch.float64) + 0.5) / (kvol * cin) ** 0.5
    sh = torch.randn(cout, generator=g, dtype=torch.float64) * 0.5
    r = torch.randn((m, cout), generator=g, dtype=torch.float64)
    acc, aacc = ref64(x, tab, w, m)
    wd = w.clone()
    wd[13, 8:16, :] = 0.0                                                       # tap 13, channels 8..15, gone from every row
    unit = acc - ref64(x, tab, wd, m)[0]
    wt = w.clone()
    wt[13] = 0.0
    tap = acc - ref64(x, tab, wt, m)[0]
    for name, d in (('8-channel group', unit), ('whole tap', tap)):
        e = (d * sc).abs() / (aacc * sc.abs() + sh.abs() + r.abs())           # no ReLU: the defect as the epilogue passes it on
        print('  cin %3d dropped %-15s max e = 2^%.1f, median 2^%.1f' % (cin, name, np.log2(float(e.max())), np.log2(float(e.median()))))
        for mode in MODES:
            assert float(e.max()) > BOUND[mode], (name, mode, float(e.max()))


# ------------------------------------------------------------------------------------------------------------------------
# GPU: every instance
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('case', COVERAGE, ids=_ids(COVERAGE))
def test_variant_vs_float64(case, device):
    run_case(case, device)


# ------------------------------------------------------------------------------------------------------------------------
# GPU: more rows than one sweep of the persistent grids
# ------------------------------------------------------------------------------------------------------------------------
def _long_rows(name, dev):
    """Rows beyond which a persistent loop of the instance wraps, from its launch rule (launch_spconv, launch_spconv_h_impl: the grid
    is capped at 2048 row tiles; launch_spconv_w: grid = CUs x max(1, 4 OCC / WAVES) workgroups of WAVES waves, a mask vector covers
    64 tiles of 32 rows per wave)."""
    if name.startswith('k_spconv_w'):
        waves, occ = {'k_spconv_w<16x16>': (4, 3), 'k_spconv_w<16x32>': (6, 3), 'k_spconv_w<32x32>': (12, 3)}[name]
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        grid = (cus * max(1, 4 * occ // waves) + 7) & ~7
        return grid * waves * 64 * 32
    return 2048 * tile_rows(name)


LONG = [sp_case('f32', 'f32', 16, 16, 'subm', 'long'), sp_case('split', 'f16x2', 64, 64, 'subm', 'long'),
        sp_case('split', 'f16x2', 16, 16, 'subm', 'long')]


@pytest.mark.gpu
@pytest.mark.parametrize('case', LONG, ids=_ids(LONG))
def test_long_stream_vs_float64(case, device):
    """Plain random coordinates in the 41 x 1504 x 1504 grid of the 0.1 m detector, more rows than one sweep of the instance's persistent
    grid: k_spconv's strided loop and the XCD deal of k_spconv_h wrap, k_spconv_w reloads its 64-tile mask vector."""
    need = _long_rows(case.expect, device)
    m = need + need // 8 + 1000
    shape = [41, 1504, 1504]
    rng = np.random.default_rng(len(case.expect))
    lin = np.unique(rng.integers(0, shape[0] * shape[1] * shape[2], size=m + m // 16))[:m]
    coords = _lin_to_coords(lin, shape)
    assert coords.shape[0] == m > need, (m, need)
    print('  %s: %d rows, one sweep covers %d' % (case.expect, m, need))
    lvl = _make_level(coords, 1, shape, m + 7, device)
    tab = _t(osp.neighbor_table(coords, shape, coords, K3, S1, P1), device)
    nbr, xwin = gpu_tables(case, lvl, lvl, lvl.d_m, False)
    convolve_and_check(case, lvl, lvl, nbr, xwin, tab, m, None, device)
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------
# GPU: the detector's own 21 launches
# ------------------------------------------------------------------------------------------------------------------------
_ORACLE_TABLES = {}


def _oracle_table(key, lvl_in, lvl_out, k, s, p, dev):
    """Oracle table of a recorded launch from the levels' coordinates (cached per (frames, stage, kind): the index path does not
    depend on the arithmetic or the engine - the cached coordinates are compared, not trusted)."""
    m_in, m = lvl_in.num_active(), min(lvl_out.num_active(), lvl_out.cap)
    ci, co = lvl_in.coords[:m_in], lvl_out.coords[:m]
    hit = _ORACLE_TABLES.get(key)
    if hit is not None and hit[0].shape == ci.shape and hit[1].shape == co.shape and torch.equal(hit[0], ci) and torch.equal(hit[1], co):
        return hit[2]
    cin_, cout_ = ci.cpu().numpy(), co.cpu().numpy()
    if lvl_in is not lvl_out:
        oc, oshape = osp.conv_out_coords(cin_, lvl_in.shape, k, s, p)
        assert list(oshape) == lvl_out.shape
        if lvl_out.num_active() <= lvl_out.cap:
            assert np.array_equal(oc, cout_), 'the output set of a strided stage differs from the oracle'
    tab = _t(osp.neighbor_table(cin_, lvl_in.shape, cout_, k, s, p), dev)
    _ORACLE_TABLES[key] = (ci.clone(), co.clone(), tab)
    return tab


def _infer_geometry(kvol, lvl_in, lvl_out):
    if lvl_in is lvl_out:
        assert kvol == 27
        return 'subm'
    for kind in ('down', 'down011', 'out'):
        k, s, p = KINDS[kind]
        if k[0] * k[1] * k[2] == kvol and osp.out_shape_of(lvl_in.shape, k, s, p) == lvl_out.shape:
            return kind
    raise AssertionError(('unknown layer geometry', kvol, lvl_in.shape, lvl_out.shape))


BACKBONE = [('f32', 'gather'), ('f32', 'xrun'), ('f16x2', 'gather'), ('f16x2', 'xrun'), ('bf16x2', 'gather'), ('bf16x2', 'xrun'),
            ('f16', 'gather'), ('f16', 'xrun')]
# the bf16x3 engines of the f32 mode, 'f32_engine+f32_gather' (no '+': the default gather arithmetic); the last row is the configuration
# DESIGN.md section 8 quotes.  These rows run 40 000-point frames (the tables, perms and calibrated capacities under test have the same
# structure there), one frame and two
BACKBONE_LIMB3 = ('xrun_bf16x3', 'gather+bf16x3', 'xrun_bf16x3+bf16x3')
BACKBONE += [('f32', e) for e in BACKBONE_LIMB3]


@pytest.mark.gpu
@pytest.mark.parametrize('mode,engine', BACKBONE)
def test_backbone_launches_vs_float64(mode, engine, device):
    """The 21 sparse convolutions SparseBackbone.run_pyramid launches for masked_frame(0, 160000) at 0.1 m, one frame (worst-case level
    capacities: m far below cap) and four frames (calibrated capacities): ops.spconv_forward is replaced by a recorder while
    run_pyramid runs, then every recorded launch - the same table object, levels, channel counts, residual and ReLU flags - is replayed
    through convolve_and_check with random operands.  f32: `engine` is the f32_engine.
    The rows of BACKBONE_LIMB3 (f32_engine 'xrun_bf16x3' and / or f32_gather 'bf16x3'): masked_frame(i, 40000), one frame and two; a
    launch the backbone hands one of the two keywords is replayed through that kernel's entry point (k_spconv_xt on the windows and
    tap-set order the pipeline built, k_spconv_gt on the plain table and its tile masks)."""
    from detzero_amd.centerpoint import FramePipeline, set_sparse_engine
    from detzero_amd.synth import VOXEL_SIZE_01
    from tests.util import make_model, masked_frame
    model, cfg, info = make_model(VOXEL_SIZE_01, seed=0)
    model = model.to(device)
    bb = model.backbone3d
    before = (bb.engine, bb.f32_engine, bb.f32_gather)
    math = ops.math_id(mode)
    real = ops.spconv_forward
    limb3 = engine in BACKBONE_LIMB3
    f32_engine, f32_gather = (engine.split('+') + ['mfma32'])[:2]
    try:
        if mode == 'f32':
            set_sparse_engine(model, before[0], f32_engine=f32_engine, f32_gather=f32_gather)
        else:
            set_sparse_engine(model, engine)
        for nb in ((1, 2) if limb3 else (1, 4)):
            frames = [torch.from_numpy(masked_frame(i, 40000 if limb3 else 160000)).to(device) for i in range(nb)]
            pipe = FramePipeline(model, info, math=mode)
            if nb > 1:
                pipe.calibrate(frames[:1], margin=1.5)
            prep = pipe.prepare(frames, overlap=False)
            rec = []

            def recorder(feats, nbr, out_level, w_taps, scale, shift, residual=None, relu=True, out=None, in_level=None, math=0, cout=None,
                         f32_engine=None, f32_gather=None):
                if math:
                    ci, co = w_taps.shape[2], (int(cout) if cout is not None else scale.shape[0])
                elif f32_engine == 'xrun_bf16x3' or f32_gather == 'bf16x3':
                    # limb weights (kvol, cout_pad, cin * 3 / 2), padded to 32 output channels
                    ci, co = w_taps.shape[2] * 2 // 3, (int(cout) if cout is not None else w_taps.shape[1])
                else:
                    ci, co = w_taps.shape[1], w_taps.shape[2]
                rec.append(dict(nbr=nbr, out_level=out_level, in_level=in_level if in_level is not None else out_level, cin=ci, cout=co,
                                residual=residual is not None, relu=bool(relu), math=int(math), in_rows=feats.shape[0],
                                f32_engine=f32_engine, f32_gather=f32_gather))
                return torch.empty((nbr.shape[1], co), dtype=torch.float32, device=feats.device)
            ops.spconv_forward = recorder
            try:
                pipe.backbone_stage(prep)
            finally:
                ops.spconv_forward = real
            torch.cuda.synchronize(device)
            assert len(rec) == 21 and all(r['math'] == math for r in rec)
            print('\n  %d frame(s) [%s, %s]: 21 launches' % (nb, mode, engine))
            stage = {}
            names, launched = set(), []
            for i, r in enumerate(rec):
                nbr, lvl_in, lvl_out = r['nbr'], r['in_level'], r['out_level']
                packed = getattr(nbr, 'packed', False)
                kvol = nbr.kvol if packed else nbr.shape[0]
                kind = _infer_geometry(kvol, lvl_in, lvl_out)
                xwin = getattr(nbr, 'xwin', None) if (packed and r['cin'] == r['cout']) else None
                eng = ('x' if math else 'xf') if xwin is not None else 'packed' if packed else 'split' if math else 'f32'
                assert r['f32_engine'] in (None, 'xrun_bf16x3') and r['f32_gather'] in (None, 'bf16x3') and not (r['f32_engine'] and r['f32_gather'])
                if r['f32_engine'] == 'xrun_bf16x3':
                    assert not math and xwin is not None, 'the bf16x3 x-run engine was asked for on a table without windows'
                    eng = 'xt'
                elif r['f32_gather'] == 'bf16x3':
                    assert not math and not packed and getattr(nbr, 'tile_masks', None) is not None
                    eng = 'gt'
                assert r['in_rows'] == lvl_in.cap or lvl_in is lvl_out
                li = stage.setdefault(id(lvl_out), len(stage))
                case = types.SimpleNamespace(label='backbone %df #%02d %d->%d %s%s%s' % (nb, i, r['cin'], r['cout'], kind, ' +res' if r['residual'] else '',
                                                                                         '' if r['relu'] else ' no relu'),
                                             engine=eng, mode=mode, cin=r['cin'], cout=r['cout'], kind=kind, kvol=kvol, edge='production', masks=True,
                                             sort=xwin is not None and xwin[3] is not None, expect=None, arm=None)
                k, s, p = KINDS[kind]
                tab = _oracle_table((nb, li, kind), lvl_in, lvl_out, k, s, p, device)
                assert r['relu'], 'every layer of the backbone ends in a ReLU'
                name, _, _, _ = convolve_and_check(case, lvl_in, lvl_out, nbr, xwin, tab, lvl_in.num_active(), None, device, seed=1000 * nb + i)
                names.add(name)
                launched.append(name)
            # the engine really was the one asked for
            if limb3:
                nxt = sum(n.startswith('k_spconv_xt<') for n in launched)
                assert nxt == (12 if f32_engine == 'xrun_bf16x3' else 0), launched
                rest = 'k_spconv_gt<' if f32_gather == 'bf16x3' else 'k_spconv<'
                assert all(n.startswith('k_spconv_xt<') or n.startswith(rest) for n in launched), launched
            else:
                assert any(n.startswith('k_spconv_x') for n in names) == (engine == 'xrun'), sorted(names)
            del prep, rec
            torch.cuda.empty_cache()
    finally:
        ops.spconv_forward = real
        set_sparse_engine(model, before[0], f32_engine=before[1], f32_gather=before[2])
