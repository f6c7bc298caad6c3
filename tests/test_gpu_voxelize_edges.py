"""GPU (MI355X): the three voxelizer routes of csrc/voxelize.hip at their edges.

Synthetic geometry throughout: pc_range = [0,0,0,W,H,D], voxel size 1, points at cell centre +- 0.3 - a point's cell is its truncated
coordinate, so the key sets of tests/scan_ref.py place points on the regime edges of the scan.

  * to-level route (ops.voxelize_to_level): the NZ scan (prefix only at non-zero words, early exit of empty chunks, the last chunk's
    end from *d_total) with line flags, in both layouts - bitmap, count, coordinates exact, prefix exact at every non-zero word;
    feature rows against ov.hard_voxelize + ov.mean_vfe bit for bit (pair16 rows against ops.pair16_from_f32 of them).
  * batched hard route (ops.voxelize_hard_mean_batched): rows in first-appearance order per frame against the oracle.
  * dynamic route (ops.voxelize_dynamic_nosync): coordinates exact, means within the derived bound of the fixed-point sums."""
import numpy as np
import pytest
import torch

from tests import scan_ref as sr

pytestmark = pytest.mark.gpu

OUT = -5.0                      # x of a padding point: outside every grid


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _geom(shape):
    d, h, w = (int(s) for s in shape)
    return [0.0, 0.0, 0.0, float(w), float(h), float(d)], [1.0, 1.0, 1.0]


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _points(cells, rng, c):
    """One point per row of cells [b,z,y,x] (b ignored): xyz at the cell centre +- 0.3, the other features random."""
    cells = np.asarray(cells)
    p = rng.uniform(-1, 1, size=(cells.shape[0], c)).astype(np.float32)
    p[:, :3] = cells[:, [3, 2, 1]].astype(np.float32) + np.float32(0.5) + rng.uniform(-0.3, 0.3, size=(cells.shape[0], 3)).astype(np.float32)
    return p


def _pad(n, c):
    p = np.zeros((n, c), np.float32)
    p[:, 0] = OUT
    return p


def _frames_of_cells(cells, batch, rng, c=5, extra=3, first_last=False):
    """Distinct cells [b,z,y,x] in level row order -> equally long frames, padded with out-of-range points.  Even frames keep the key
    order of their cells (runs of one bitmap word over the lanes), odd frames are shuffled; first_last: the padding sits in the
    middle of a frame, so that a frame ends on its last cell and the next one starts on its first."""
    per = [cells[cells[:, 0] == b] for b in range(batch)]
    n_per = max(p.shape[0] for p in per) + extra
    out = []
    for b, cb in enumerate(per):
        pts = _points(cb, rng, c)
        if b % 2 == 1 and not first_last:
            pts = pts[rng.permutation(pts.shape[0])]
        pad = _pad(n_per - pts.shape[0], c)
        cut = pts.shape[0] // 2 if first_last else int(rng.integers(0, pts.shape[0] + 1))
        out.append(np.concatenate([pts[:cut], pad, pts[cut:]], 0))
    return np.concatenate(out, 0), n_per


def _check_level_index(lvl, cells, keys, batch, shape, layout):
    """NZ-scan statement: bitmap, count and coordinates exact, prefix exact at every word that holds a bit."""
    nw = sr.nwords(batch, list(shape), layout)
    bitmap, prefix, order, count = sr.expected_index(keys, nw)
    assert lvl.prefix_partial and lvl.bitmap.numel() == nw
    assert lvl.num_active() == count
    got_b = _u32(lvl.bitmap)
    bad = np.nonzero(got_b != bitmap)[0]
    assert bad.size == 0, ('bitmap', bad[:8], got_b[bad[:8]], bitmap[bad[:8]])
    assert np.array_equal(lvl.coords[:count].cpu().numpy(), cells[order])
    nz = np.nonzero(bitmap)[0]
    got_p = _u32(lvl.prefix[_t(nz, lvl.prefix.device)])
    bad = np.nonzero(got_p != prefix[nz])[0]
    assert bad.size == 0, ('prefix', nz[bad[:8]], got_p[bad[:8]], prefix[nz[bad[:8]]])


def _run_to_level(device, cells, keys, batch, shape, layout, seed=0, first_last=False, c=5):
    from detzero_amd import ops
    rng = np.random.default_rng(seed)
    pts, n_per = _frames_of_cells(cells, batch, rng, c=c, first_last=first_last)
    pc_range, vs = _geom(shape)
    lvl, x = ops.voxelize_to_level(_t(pts, device), batch, pc_range, vs, 5, n_per, list(shape), 8, math=0, layout=layout)
    _check_level_index(lvl, cells, keys, batch, shape, layout)
    # one point per cell: the row of a cell is its point
    valid = pts[pts[:, 0] != OUT]
    cz = np.floor(valid[:, [2, 1, 0]]).astype(np.int64)
    fb = np.repeat(np.arange(batch), n_per)[pts[:, 0] != OUT]
    k = sr.key_of(fb, cz[:, 0], cz[:, 1], cz[:, 2], list(shape), layout)
    o = np.argsort(k, kind='stable')
    m = keys.size
    got = x[:m].cpu().numpy()
    assert np.array_equal(got[:, :c].view(np.uint32), valid[o].view(np.uint32)) and not got[:, c:].any()
    return lvl


# ------------------------------------------------------------------------------------------------
# to-level route: scan side
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', [0, 1])
def test_to_level_word_shared_by_two_frames(device, layout):
    """(3,[3,5,33]): 495 cells per frame, so bitmap word 15 holds the last cells of frame 0 and the first of frame 1 (linear layout);
    the last point of frame f and the first point of frame f + 1 lie in it - neighbouring lanes of k_level_keys' word-run merge.
    48 words: one full line of 32 and a partial one."""
    batch, shape = 3, (3, 5, 33)
    rng = np.random.default_rng(5)
    n = 3 * 5 * 33
    lin = np.unique(np.concatenate([np.nonzero(rng.random(batch * n) < 0.4)[0], [f * n for f in range(batch)],
                                    [f * n + n - 1 for f in range(batch)]]))
    cells = np.stack([lin // n, (lin % n) // (5 * 33), (lin // 33) % 5, lin % 33], 1).astype(np.int32)
    keys = sr.keys_of_coords(cells, list(shape), layout)
    o = np.argsort(keys, kind='stable')
    if layout == 0:
        assert int(keys[o][cells[o][:, 0] == 0][-1]) >> 5 == int(keys[o][cells[o][:, 0] == 1][0]) >> 5 == 15
        assert sr.nwords(batch, list(shape), 0) == 48
    _run_to_level(device, cells[o], keys[o], batch, shape, layout, first_last=True)


@pytest.mark.parametrize('layout', [0, 1])
@pytest.mark.parametrize('batch,last_chunk', [(1, True), (3, True), (3, False)])
def test_to_level_scan_regimes(device, batch, last_chunk, layout):
    """[41,1504,1504] frames: one (four words per thread, one trip) and three (two trips of k_scan_partials), boundary bits of
    tests/scan_ref.py plus a dense stretch and random cells; once more with nothing in the last chunk (its early exit compares
    partial[last] with *d_total)."""
    shape = (41, 1504, 1504)
    cells, keys, surv = sr.edge_case_cells(batch, list(shape), layout, seed=batch)
    assert min(surv.values()) >= 1
    nw = sr.nwords(batch, list(shape), layout)
    wpt, blocks, trips = sr.scan_regime(nw)
    assert (wpt, trips) == (4, 2 if batch == 3 else 1)
    print('to-level grid (%d,%s) layout %d: %d words, %d blocks, %d trips' % (batch, list(shape), layout, nw, blocks, trips))
    last_start = (blocks - 1) * 1024
    in_last = (keys >> np.uint64(5)) >= np.uint64(last_start)
    assert in_last.any()
    if not last_chunk:
        cells, keys = cells[~in_last], keys[~in_last]
    _run_to_level(device, cells, keys, batch, shape, layout, seed=batch)


LINE_GRIDS = [(1, (41, 1504, 1504), 0), (1, (41, 1504, 1504), 1), (2, (5, 9, 70), 0), (2, (5, 9, 70), 1), (3, (3, 5, 33), 0)]


@pytest.mark.parametrize('batch,shape,layout', LINE_GRIDS)
def test_to_level_line_flags(device, batch, shape, layout):
    """Line flags (one byte per 32 words; an unflagged line is never read): lines whose only bit is in their first / in their last
    word, flagged lines on both sides of an unflagged one, and a bit in the last, partial line of a bitmap whose word count is a
    multiple of 8 but not of 32.  No random cells: every other line stays unflagged."""
    nw, last = sr.nwords(batch, list(shape), layout), sr.last_key(batch, list(shape), layout)
    lines = (nw + 31) // 32
    def pick(line, word, bit):
        """a valid cell in word `word` of `line` (ragged brick grids: of the first later line that has one there)"""
        for ln in range(line, lines):
            k = np.arange(32, dtype=np.uint64) + np.uint64((ln * 32 + word) * 32)
            _, ok = sr.cells_of_keys(k, batch, list(shape), layout)
            if ok.any():
                return int(k[bit]) if ok[bit] else int(k[ok][-1])
        raise AssertionError('no valid cell in word %d of any line from %d' % (word, line))

    if lines >= 8:
        a, b, c0 = lines // 7, lines // 3, lines // 2
        cand = [pick(a, 0, 5), pick(b, 31, 31), pick(c0, 9, 0), pick(c0 + 2, 20, 17)]
    else:
        cand = [pick(0, 0, 3), pick(0, 31, 31)]
    cand = np.array(cand, np.uint64)
    if nw % 32:                                        # every cell of the partial line's words (ragged grids: the valid ones)
        tail = np.arange((nw // 32) * 32 * 32, min(nw * 32, last + 1), dtype=np.uint64)
        _, ok = sr.cells_of_keys(tail, batch, list(shape), layout)
        assert ok.any()
        cand = np.concatenate([cand, tail[ok][:1], tail[ok][-1:]])
    else:
        assert tuple(shape) == (41, 1504, 1504)
        cand = np.concatenate([cand] + list(sr.boundary_keys(nw, last).values()))
    cells, ok = sr.cells_of_keys(cand, batch, list(shape), layout)
    assert ok.all()
    cells = np.unique(cells[ok], axis=0)
    keys = sr.keys_of_coords(cells, list(shape), layout)
    o = np.argsort(keys, kind='stable')
    cells, keys = cells[o].astype(np.int32), keys[o]
    words = np.unique((keys >> np.uint64(5)).astype(np.int64))
    assert (words % 32 == 31).any() and (words % 32 == 0).any() and keys.size >= 3
    if nw % 32:
        assert words[-1] >= nw // 32 * 32
    _run_to_level(device, cells, keys, batch, shape, layout, seed=1)


@pytest.mark.parametrize('batch,shape,layout', [(1, (2, 64, 66), 0), (1, (2, 64, 66), 1), (1, (41, 1504, 1504), 0)])
def test_to_level_last_chunk_ends_at_the_total(device, batch, shape, layout):
    """The last chunk of the NZ scan has no partial[blockIdx.x + 1]: its end is *d_total.  The entry point is called with a
    workspace in which every word holds the number of bits below the last chunk - a kernel that read the word behind the chunk
    totals instead of *d_total would see an empty last chunk and leave its coordinates and prefix unwritten."""
    from detzero_amd import lib as L
    from detzero_amd import ops
    lib = L.load()
    cells, keys, _ = sr.edge_case_cells(batch, list(shape), layout, seed=2, n_random=3000)
    nw = sr.nwords(batch, list(shape), layout)
    wpt, blocks, _ = sr.scan_regime(nw)
    below = int(((keys >> np.uint64(5)) < np.uint64((blocks - 1) * 256 * wpt)).sum())
    assert blocks >= 2 and 0 < below < keys.size
    rng = np.random.default_rng(2)
    pts, n_per = _frames_of_cells(cells, batch, rng)
    pc_range, vs = _geom(shape)
    cap = batch * n_per
    lvl = ops.SparseLevel(batch, list(shape), cap, device, layout=layout, zero_count=False)
    lvl.coords.fill_(-7)
    lvl.prefix.fill_(-1)
    feats = torch.empty((cap, 8), dtype=torch.float32, device=device)
    nbytes = lib.dz_voxelize_to_level_workspace_bytes(n_per, batch, 5, cap, *lvl.shape, layout)
    ws = torch.full(((nbytes + 3) // 4 + 64,), below, dtype=torch.int32, device=device)
    p = _t(pts, device)
    rc = lib.dz_voxelize_to_level(L.ptr(p), n_per, batch, 5, L.f6(pc_range), L.f3(vs), L.i3([shape[2], shape[1], shape[0]]), 0, 5, n_per,
                                  lvl.shape[0], layout, L.ptr(lvl.bitmap), L.ptr(lvl.prefix), L.ptr(lvl.coords), L.ptr(lvl.d_m), cap,
                                  L.ptr(feats), 8, 0, L.ptr(ws), ws.numel() * 4, L.stream())
    L.check(rc, 'dz_voxelize_to_level')
    lvl.prefix_partial = True
    _check_level_index(lvl, cells, keys, batch, shape, layout)
    assert bool((lvl.coords[keys.size:] == -7).all())


# ------------------------------------------------------------------------------------------------
# to-level route: feature side
# ------------------------------------------------------------------------------------------------
FSHAPE = (4, 6, 10)
FCELLS = np.array([[1, 2, 3], [1, 2, 4], [3, 5, 9], [0, 0, 0], [2, 2, 3], [1, 3, 3]], np.int64)         # (z, y, x)
FSEQ = [0] * 200 + [1, 0] * 40 + [2] * 7 + [0] * 3 + [3] * 61 + [1] * 5 + [2] * 70 + [4, 3, 4, 3, 4] + [0] * 130 + [1] * 64 + [4] * 64 + [5]


def _feature_frames(c, rng):
    """Two frames: 200 points of one voxel in one run, the same voxel again in later runs, strictly alternating voxels, runs across
    wavefront boundaries, then random voxels; frame 1 is frame 0 reversed.  n_per is no multiple of 64."""
    seq = np.array(FSEQ + list(rng.integers(0, 6, size=300)))
    assert seq.size % 64 != 0
    cz = np.concatenate([np.zeros((seq.size, 1), np.int64), FCELLS[seq]], 1)
    f0 = _points(cz, rng, c)
    return [f0, f0[::-1].copy()], seq.size


def _oracle_rows(frames, shape, layout, max_points, max_voxels, mask=False):
    """(cells [b,z,y,x] in level row order, mean rows) of ov.hard_voxelize + ov.mean_vfe over the frames."""
    from oracle import voxelize as ov
    pc_range, vs = _geom(shape)
    cs, fs = [], []
    for b, f in enumerate(frames):
        with np.errstate(invalid='ignore'):
            if mask:
                f = f[ov.mask_points_by_range(f, pc_range)]
            v, c, n = ov.hard_voxelize(f, pc_range, vs, max_points, max_voxels)
        cs.append(np.concatenate([np.full((c.shape[0], 1), b, np.int32), c], 1))
        fs.append(ov.mean_vfe(v, n))
    cs, fs = np.concatenate(cs, 0), np.concatenate(fs, 0)
    o = np.argsort(sr.keys_of_coords(cs, list(shape), layout), kind='stable')
    return cs[o], fs[o]


@pytest.mark.parametrize('layout', [0, 1])
@pytest.mark.parametrize('max_points', [1, 5, 70])
@pytest.mark.parametrize('c', [3, 5, 6, 9])
def test_to_level_features(device, c, max_points, layout):
    from detzero_amd import ops
    rng = np.random.default_rng(100 + c)
    frames, n_per = _feature_frames(c, rng)
    pc_range, vs = _geom(FSHAPE)
    cells, rows = _oracle_rows(frames, FSHAPE, layout, max_points, n_per)
    m = cells.shape[0]
    assert m == 12
    pts = _t(np.concatenate(frames, 0), device)
    for c_dst in ((8, 16) if c <= 8 else (16,)):
        ref = np.zeros((m, c_dst), np.float32)
        ref[:, :c] = rows
        for math in (0, 1, 2):
            lvl, x = ops.voxelize_to_level(pts, 2, pc_range, vs, max_points, n_per, list(FSHAPE), c_dst, math=math, layout=layout)
            assert lvl.num_active() == m and np.array_equal(lvl.coords[:m].cpu().numpy(), cells)
            if math == 0:
                got = x[:m].cpu().numpy()
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (c_dst, np.abs(got - ref).max())
                assert not got[:, c:].any()                                         # padding channels
            else:
                want = ops.pair16_from_f32(_t(ref, device), c_dst, math=math)
                assert torch.equal(x[:m].view(torch.int32), want.view(torch.int32)), (c_dst, math)


@pytest.mark.parametrize('layout', [0, 1])
@pytest.mark.parametrize('mask', [False, True])
def test_to_level_rejected_points(device, mask, layout):
    """NaN, +-inf, 1e30 in each coordinate and coordinates exactly on the upper range (inside the inclusive xy mask, outside the
    grid), mixed with valid points - against the oracle, which is given the mask itself."""
    from detzero_amd import ops
    shape = FSHAPE
    pc_range, vs = _geom(shape)
    rng = np.random.default_rng(9)
    good = _points(np.concatenate([np.zeros((40, 1), np.int64), FCELLS[rng.integers(0, 6, 40)]], 1), rng, 5)
    bad = []
    for val in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        for axis in range(3):
            p = good[len(bad) % 40].copy()
            p[axis] = val
            bad.append(p)
    for axis, hi in enumerate((shape[2], shape[1], shape[0])):
        p = good[axis].copy()
        p[axis] = hi                                    # exactly the upper range
        bad.append(p)
        p = good[axis + 3].copy()
        p[axis] = np.nextafter(np.float32(hi), np.float32(0))     # the last value inside
        bad.append(p)
    p = good[7].copy(); p[0] = -0.25; bad.append(p)     # floor(-0.25) = -1, not cell 0
    bad = np.array(bad, np.float32)
    f0 = np.concatenate([good, bad], 0)[rng.permutation(40 + bad.shape[0])]
    f1 = np.concatenate([bad, good[:7], _pad(33, 5)], 0)
    assert f0.shape == f1.shape
    cells, rows = _oracle_rows([f0, f1], shape, layout, 5, 1000, mask=mask)
    m = cells.shape[0]
    lvl, x = ops.voxelize_to_level(_t(np.concatenate([f0, f1], 0), device), 2, pc_range, vs, 5, 1000, list(shape), 8, math=0,
                                   xy_range_mask=mask, layout=layout)
    assert lvl.num_active() == m and m >= 8
    assert np.array_equal(lvl.coords[:m].cpu().numpy(), cells)
    assert np.array_equal(x[:m, :5].cpu().numpy().view(np.uint32), rows.view(np.uint32))
    keys = sr.keys_of_coords(cells, list(shape), layout)
    _check_level_index(lvl, cells, keys, 2, shape, layout)


@pytest.mark.parametrize('layout', [0, 1])
def test_to_level_empty_and_refused(device, layout):
    from detzero_amd import lib as L
    from detzero_amd import ops
    shape = FSHAPE
    pc_range, vs = _geom(shape)
    nw = sr.nwords(2, list(shape), layout)
    bad = _pad(70, 5)
    bad[::2, 0] = np.nan
    bad[1::4, 2] = 99.0
    lvl, x = ops.voxelize_to_level(_t(bad, device), 2, pc_range, vs, 5, 1000, list(shape), 8, layout=layout)        # every point invalid
    assert lvl.num_active() == 0 and lvl.bitmap.numel() == nw and int(lvl.bitmap.abs().max()) == 0
    lvl, x = ops.voxelize_to_level(torch.zeros((0, 5), device=device), 2, pc_range, vs, 5, 1000, list(shape), 8, layout=layout)      # n_per == 0
    assert lvl.num_active() == 0 and int(lvl.bitmap.abs().max()) == 0
    with pytest.raises(L.DetZeroHipError):              # 35 points per frame could open more than max_voxels = 34 voxels
        ops.voxelize_to_level(_t(bad, device), 2, pc_range, vs, 5, 34, list(shape), 8, layout=layout)


# ------------------------------------------------------------------------------------------------
# batched hard route
# ------------------------------------------------------------------------------------------------
HSHAPE = (3, 5, 33)


def _check_hard_batched(device, frames, max_points, max_voxels, cap, mask=False):
    from detzero_amd import ops
    from oracle import voxelize as ov
    pc_range, vs = _geom(HSHAPE)
    batch = len(frames)
    feats, coords, d_num = ops.voxelize_hard_mean_batched(_t(np.concatenate(frames, 0), device), batch, pc_range, vs, max_points, max_voxels,
                                                          cap, xy_range_mask=mask)
    feats, coords, d_num = feats.cpu().numpy(), coords.cpu().numpy(), d_num.cpu().numpy()
    counts = []
    for b, f in enumerate(frames):
        with np.errstate(invalid='ignore'):
            ref = f[ov.mask_points_by_range(f, pc_range)] if mask else f
            v, c, n = ov.hard_voxelize(ref, pc_range, vs, max_points, max_voxels)
        m = c.shape[0]
        counts.append(m)
        assert int(d_num[b]) == m, (b, int(d_num[b]), m)
        rows = slice(b * cap, b * cap + m)
        assert np.array_equal(coords[rows, 0], np.full(m, b)) and np.array_equal(coords[rows, 1:], c)      # first-appearance order
        assert np.array_equal(feats[rows].view(np.uint32), ov.mean_vfe(v, n).view(np.uint32))
        assert np.all(coords[b * cap + m:(b + 1) * cap] == -1)
    return counts


def _hard_frame(rng, n, c=5, p_bad=0.0):
    cz = np.stack([np.zeros(n, np.int64), rng.integers(0, HSHAPE[0], n), rng.integers(0, 2, n), rng.integers(0, 4, n)], 1)
    f = _points(cz, rng, c)
    f[rng.random(n) < p_bad, 0] = OUT
    return f


@pytest.mark.parametrize('batch,n_per', [(1, 150), (7, 1), (7, 3), (7, 37), (256, 2)])
def test_hard_batched_frames(device, batch, n_per):
    """One frame; seven frames of 1 / 3 / 37 points (a word of the point bitmap spans frames); 256 frames - k_hard_emit_mean's
    per-frame counts take one thread per frame of a 256-thread block."""
    rng = np.random.default_rng(batch * 100 + n_per)
    frames = [_hard_frame(rng, n_per, p_bad=0.2) for _ in range(batch)]
    counts = _check_hard_batched(device, frames, 5, 1000, n_per)
    assert sum(counts) > batch // 2


def test_hard_batched_refuses_257_frames(device):
    from detzero_amd import lib as L
    from detzero_amd import ops
    pc_range, vs = _geom(HSHAPE)
    rng = np.random.default_rng(3)
    pts = _t(np.concatenate([_hard_frame(rng, 2) for _ in range(257)], 0), device)
    with pytest.raises(L.DetZeroHipError):
        ops.voxelize_hard_mean_batched(pts, 257, pc_range, vs, 5, 1000, 2)


def test_hard_batched_empty_frames_and_cut(device):
    rng = np.random.default_rng(4)
    n = 45
    a, c = _hard_frame(rng, n), _hard_frame(rng, n)
    none = _pad(n, 5)
    none[::3, 1] = np.nan
    late = _hard_frame(rng, n)
    late[0, 0] = OUT                                    # the frame's first point is invalid
    late[1, 2] = np.inf
    counts = _check_hard_batched(device, [a, none, c, late, none], 5, 1000, n)
    assert counts[1] == counts[4] == 0 and min(counts[0], counts[2], counts[3]) > 5
    # max_voxels cuts inside every frame: 3 voxels kept of 9 (points of the refused voxels are dropped, later points of the kept
    # ones still count)
    cells9 = np.array([[0, z, y, x] for z in range(3) for y in range(3) for x in (0, 32)][:9], np.int64)
    seq = np.concatenate([np.arange(9), rng.integers(0, 9, 60)])
    frames = [_points(cells9[seq], rng, 5), _points(cells9[seq[::-1]], rng, 5)]
    counts = _check_hard_batched(device, frames, 5, 3, 69)
    assert counts == [3, 3]
    for mp in (1, 70):
        _check_hard_batched(device, frames, mp, 9, 9)
    _check_hard_batched(device, [late, a], 5, 1000, n, mask=True)


# ------------------------------------------------------------------------------------------------
# dynamic route
# ------------------------------------------------------------------------------------------------
DGRID = (33, 5, 3)                                      # GX, GY, GZ
DRANGE, DVS = [0.0, 0.0, 0.0, 33.0, 5.0, 3.0], [1.0, 1.0, 1.0]


def _dyn_points(rng, n, c, batch, cells=None):
    """points_b (n, 1 + c): [b, x, y, z, features]; features: negative values, magnitudes from 1e-9 to 2^-4 and O(1)."""
    if cells is None:
        cells = np.stack([rng.integers(0, g, n) for g in DGRID], 1)
    p = np.zeros((n, 1 + c), np.float32)
    p[:, 0] = rng.integers(0, batch, n)
    p[:, 1:4] = cells.astype(np.float32) + np.float32(0.5) + rng.uniform(-0.3, 0.3, size=(n, 3)).astype(np.float32)
    if c > 3:
        mag = np.float32(10.0) ** rng.uniform(-9, np.log10(2.0 ** -4), size=(n, c - 3)).astype(np.float32)
        val = np.where(rng.random((n, c - 3)) < 0.5, mag, rng.normal(size=(n, c - 3)) * 3)
        p[:, 4:] = (val * np.where(rng.random((n, c - 3)) < 0.5, -1, 1)).astype(np.float32)
    return p


def _dyn_reference(pb, batch):
    """(coords [b,z,y,x] in ascending x-major key order, float64 means, counts): the oracle's coordinates on the points whose
    truncated batch index is a frame, and the mean of every voxel in float64."""
    from oracle import voxelize as ov
    b = np.trunc(pb[:, 0].astype(np.float64)).astype(np.int64)          # the oracle's int conversion of the batch column
    keep = (b >= 0) & (b < batch)
    pts = pb[keep]
    if pts.shape[0] == 0:
        return np.zeros((0, 4), np.int32), np.zeros((0, pb.shape[1] - 1)), np.zeros((0,), np.int64)
    f32, coords = ov.dynamic_mean_vfe(pts, DRANGE, DVS)
    cx = np.floor(pts[:, 1:4]).astype(np.int64)
    ok = np.all((cx >= 0) & (cx < np.array(DGRID)[None, :]), 1)
    key = sr.key_dynamic(b[keep][ok], cx[ok, 0], cx[ok, 1], cx[ok, 2], DGRID)
    uniq, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    sums = np.zeros((uniq.size, pb.shape[1] - 1), np.float64)
    np.add.at(sums, inv, pts[ok, 1:].astype(np.float64))
    mean = sums / cnt[:, None]
    assert np.array_equal(sr.key_dynamic(coords[:, 0], coords[:, 3], coords[:, 2], coords[:, 1], DGRID), uniq)
    assert np.array_equal(mean.astype(np.float32), f32)
    return coords, mean, cnt


def _dyn_check(got, mean):
    """|got - ref| <= 2^-29 + 2^-23 |ref|: every point is rounded to 2^-28 units (at most 2^-29 each, so at most 2^-29 on the
    mean), then one fp32 rounding of the sum and one of the quotient.  Returns the largest error as a fraction of the bound."""
    bound = 2.0 ** -29 + 2.0 ** -23 * np.abs(mean)
    ratio = np.abs(got.astype(np.float64) - mean) / bound
    worst = float(ratio.max()) if ratio.size else 0.0
    print('dynamic mean: largest error / bound = %.3f over %d values' % (worst, ratio.size))
    assert worst <= 1.0
    return worst


def _dyn_run(device, pb, batch, cap=None):
    from detzero_amd import ops
    feats, coords, d_num = ops.voxelize_dynamic_nosync(_t(pb, device), DRANGE, DVS, batch, cap=cap)
    return feats.cpu().numpy(), coords.cpu().numpy(), int(d_num.item())


@pytest.mark.parametrize('c', [3, 6])
@pytest.mark.parametrize('n', [0, 1, 63, 65, 4000])
def test_dynamic_sizes_and_batch_indices(device, n, c):
    """n around a wavefront; batch column values -1, batch, 1.7 and -0.5 (truncated as the oracle's int conversion does: frame 1 and
    frame 0, the first two outside); coordinates in x-major key order exact, means within the derived bound; the same points
    permuted give the same bits."""
    batch = 2
    rng = np.random.default_rng(n * 10 + c)
    pb = _dyn_points(rng, n, c, batch)
    if n >= 63:
        pb[3::9, 0] = -1.0
        pb[4::9, 0] = float(batch)
        pb[5::9, 0] = 1.7
        pb[6::9, 0] = -0.5
        pb[7::31, 1] = OUT
    coords, mean, cnt = _dyn_reference(pb, batch)
    m = coords.shape[0]
    feats, got_c, d = _dyn_run(device, pb, batch)
    assert d == m and np.array_equal(got_c[:m], coords)
    _dyn_check(feats[:m], mean)
    if n > 1:
        f2, c2, d2 = _dyn_run(device, pb[rng.permutation(n)], batch)
        assert d2 == m and np.array_equal(c2[:m], got_c[:m]) and np.array_equal(f2[:m].view(np.uint32), feats[:m].view(np.uint32))


def test_dynamic_binding_cap(device):
    batch, c = 2, 6
    rng = np.random.default_rng(21)
    pb = _dyn_points(rng, 700, c, batch)
    coords, mean, cnt = _dyn_reference(pb, batch)
    m = coords.shape[0]
    cap = m - 37
    assert cap > 100
    feats, got_c, d = _dyn_run(device, pb, batch, cap=cap)
    assert d == m and feats.shape[0] == cap                         # the full count is reported
    assert np.array_equal(got_c, coords[:cap])
    _dyn_check(feats, mean[:cap])


@pytest.mark.parametrize('runs', [False, True])
def test_dynamic_voxel_of_5000_points(device, runs):
    """One voxel with 5000 points among 3000 others, scattered over the input or in runs longer than a wavefront (the run sums of
    k_dyn_accumulate reach back 63 lanes)."""
    batch, c = 2, 6
    rng = np.random.default_rng(22)
    big = np.tile(np.array([[17, 2, 1]]), (5000, 1))
    pb = np.concatenate([_dyn_points(rng, 5000, c, 1, cells=big), _dyn_points(rng, 3000, c, batch)], 0)
    if runs:
        o = np.concatenate([np.arange(0, 130), 5000 + np.arange(0, 1000), np.arange(130, 4999), 5000 + np.arange(1000, 3000), [4999]])
    else:
        o = rng.permutation(8000)
    pb = pb[o]
    coords, mean, cnt = _dyn_reference(pb, batch)
    m = coords.shape[0]
    assert int(cnt.max()) >= 5000
    feats, got_c, d = _dyn_run(device, pb, batch)
    assert d == m and np.array_equal(got_c[:m], coords)
    _dyn_check(feats[:m], mean)
    f2, c2, d2 = _dyn_run(device, pb[rng.permutation(8000)], batch)
    assert np.array_equal(f2[:m].view(np.uint32), feats[:m].view(np.uint32))
