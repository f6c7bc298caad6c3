"""GPU (MI355X): the three-launch bitmap scan (k_scan_reduce / k_scan_partials / k_scan_down of csrc/sparse_index.hip) through
SparseLevel.build_from_coords, with bits placed on every regime edge - one or four words per thread, the chunk edges of both chunk
sizes, the trips of 8192 chunk totals, keys at and above 2^31, a binding cap_out - against the numpy reference of tests/scan_ref.py.
Everything is exact: count, coordinates, bitmap, prefix at every word, rank of every input row.  The ragged-brick case runs the
index chain (downsamples, neighbour tables, tile masks) on grids whose H or W is no multiple of 8 in the brick layout."""
import functools

import numpy as np
import pytest
import torch

from tests import scan_ref as sr
from tests.util import canon_order, canon_table

pytestmark = pytest.mark.gpu

# (batch, [D,H,W], layouts, trips of k_scan_partials)
GRIDS = [
    (1, (1, 1, 1), (0, 1), 1), (2, (3, 5, 33), (0, 1), 1), (2, (5, 9, 70), (0, 1), 1),           # smallest
    (1, (2, 64, 64), (0, 1), 1), (1, (2, 64, 66), (0, 1), 1),                                     # one block / just over
    (1, (64, 1024, 1024), (0, 1), 1),            # 2^21 words: the last one-word-per-thread size, exactly one trip of 8192 totals
    (1, (64, 1024, 1032), (0, 1), 1),            # the first four-words-per-thread size
    (3, (41, 1504, 1504), (0, 1), 2),            # two trips
    (6, (41, 1504, 1504), (0,), 3),              # three trips
]
CASES = [(b, s, l, t) for b, s, ls, t in GRIDS for l in ls]


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


@functools.lru_cache(maxsize=None)
def _active(batch, shape, layout, frames=None):
    """(distinct cells in reference row order, their keys, shuffled input holding every cell twice, its keys)."""
    cells, keys, surv = sr.edge_case_cells(batch, list(shape), layout, seed=batch + shape[2], random_frames=frames)
    assert min(surv.values()) >= 1
    rng = np.random.default_rng(7)
    p = rng.permutation(2 * keys.size) % keys.size
    for a in (cells, keys):
        a.setflags(write=False)
    return cells, keys, np.ascontiguousarray(cells[p]), keys[p]


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('batch,shape,layout,trips', CASES)
def test_scan_at_regime_edges(device, batch, shape, layout, trips):
    from detzero_amd import ops
    cells, keys, inp, inp_keys = _active(batch, shape, layout)
    nw = sr.nwords(batch, list(shape), layout)
    wpt, blocks, got_trips = sr.scan_regime(nw)
    print('scan grid (%d,%s) layout %d: %d words, %d words/thread, %d blocks, %d trips, %d cells' % (batch, list(shape), layout, nw, wpt,
                                                                                                       blocks, got_trips, keys.size))
    assert got_trips == trips
    bitmap, prefix, order, count = sr.expected_index(inp_keys, nw)
    assert count == keys.size and np.array_equal(inp[order], cells)
    lvl = ops.SparseLevel(batch, list(shape), count + 5, device, layout=layout)
    assert lvl.bitmap.numel() == nw
    rank = lvl.build_from_coords(_t(inp, device))
    assert lvl.num_active() == count
    assert np.array_equal(lvl.coords[:count].cpu().numpy(), inp[order])
    got_b, got_p = _u32(lvl.bitmap), _u32(lvl.prefix)
    bad = np.nonzero(got_b != bitmap)[0]
    assert bad.size == 0, ('bitmap', bad[:8], got_b[bad[:8]], bitmap[bad[:8]])
    bad = np.nonzero(got_p != prefix)[0]
    assert bad.size == 0, ('prefix', bad[:8], got_p[bad[:8]], prefix[bad[:8]])
    assert np.array_equal(rank.cpu().numpy(), sr.rank_of_keys(inp_keys))


def test_scan_keys_above_two_to_the_31(device):
    """24 level-1 frames in the linear layout: 2.23e9 cells, keys of frame 24 at and above 2^31 (LevelGeom::key forms them in int and
    casts).  Neither the bitmap nor the prefix (278 MB each) is downloaded: count, coordinates and rank of every input row, and the
    bitmap and prefix at 10 000 sampled words plus every word that holds a boundary bit or a bit of the dense stretch."""
    from detzero_amd import ops
    batch, shape = 24, (41, 1504, 1504)
    cells, keys, inp, inp_keys = _active(batch, shape, 0, frames=(22, 23))
    assert int((keys >= 2 ** 31).sum()) > 2000 and int(keys[-1]) == sr.last_key(batch, list(shape), 0)
    assert int((cells[:, 0] >= 22).sum()) >= 10000
    nw = sr.nwords(batch, list(shape), 0)
    print('scan grid (24,%s): %d words, regime %s, %d cells' % (list(shape), nw, sr.scan_regime(nw), keys.size))
    lvl = ops.SparseLevel(batch, list(shape), keys.size + 5, device)
    rank = lvl.build_from_coords(_t(inp, device))
    assert lvl.num_active() == keys.size
    assert np.array_equal(lvl.coords[:keys.size].cpu().numpy(), cells)
    assert np.array_equal(rank.cpu().numpy(), sr.rank_of_keys(inp_keys))
    rng = np.random.default_rng(1)
    bwords = np.concatenate(list(sr.boundary_keys(nw, int(keys[-1])).values())).astype(np.int64) >> 5
    words = np.unique(np.concatenate([rng.integers(0, nw, 10000), bwords, sr.dense_stretch_words(nw, int(keys[-1])), [nw - 1],
                                      (keys[rng.integers(0, keys.size, 2000)] >> np.uint64(5)).astype(np.int64)]))
    bitmap, prefix = sr.expected_at_words(keys, words)
    idx = _t(words, device)
    assert np.array_equal(_u32(lvl.bitmap[idx]), bitmap)
    assert np.array_equal(_u32(lvl.prefix[idx]), prefix)
    assert int(prefix[-1]) + int(sr.popcount32(bitmap[-1:])[0]) == keys.size


@pytest.mark.parametrize('layout', [0, 1])
def test_scan_empty_input(device, layout):
    from detzero_amd import ops
    lvl = ops.SparseLevel(2, [5, 9, 70], 16, device, layout=layout)
    lvl.bitmap.fill_(-1); lvl.prefix.fill_(-1); lvl.d_m.fill_(9)
    lvl.build_from_coords(torch.zeros((0, 4), dtype=torch.int32, device=device), want_rank=False)
    assert lvl.num_active() == 0
    assert int(lvl.bitmap.abs().max()) == 0 and int(lvl.prefix.abs().max()) == 0


@pytest.mark.parametrize('layout', [0, 1])
def test_scan_binding_cap(device, layout):
    """cap_out three rows below the count: the first cap rows are right, the rows behind them are not touched (the r < cap_out
    guard of the emission loop), the count is the full one, and every input row still gets its rank."""
    from detzero_amd import ops
    batch, shape = 2, (5, 9, 70)
    cells, keys, inp, inp_keys = _active(batch, shape, layout)
    m = keys.size
    cap = m - 3
    lvl = ops.SparseLevel(batch, list(shape), cap, device, layout=layout)
    big = torch.full((m + 64, 4), -7, dtype=torch.int32, device=device)
    lvl.coords = big[:cap]
    rank = lvl.build_from_coords(_t(inp, device))
    assert lvl.num_active() == m
    got = big.cpu().numpy()
    assert np.array_equal(got[:cap], cells[:cap]) and np.all(got[cap:] == -7)
    assert np.array_equal(rank.cpu().numpy(), sr.rank_of_keys(inp_keys))
    bitmap, prefix, _, _ = sr.expected_index(keys, sr.nwords(batch, list(shape), layout))
    assert np.array_equal(_u32(lvl.bitmap), bitmap) and np.array_equal(_u32(lvl.prefix), prefix)


@pytest.mark.parametrize('shape,fill', [([5, 9, 70], 0.5), ([4, 8, 64], 0.9), ([3, 5, 33], 0.25)])
def test_brick_index_chain_on_ragged_grids(device, shape, fill):
    """The brick layout (scan mode 2, generic neighbour kernel) where H or W is no multiple of 8: level, the three strided
    downsamples of the backbone and the submanifold / strided neighbour tables against the oracle in canonical row order; the
    per-32-row tap masks against the table's own occupancy in storage order."""
    from detzero_amd import ops
    from oracle import sparse as osp
    rng = np.random.default_rng(shape[2])
    batch = 2
    n = shape[0] * shape[1] * shape[2]
    lin = np.nonzero(rng.random(batch * n) < fill)[0]
    lin = np.unique(np.concatenate([lin, [0, 31, 32, batch * n - 1, batch * n - 33]]))
    coords = np.stack([lin // n, (lin % n) // (shape[1] * shape[2]), (lin // shape[2]) % shape[1], lin % shape[2]], 1).astype(np.int32)
    lvl = ops.SparseLevel(batch, shape, coords.shape[0] + 5, device, layout=1)
    inp = coords[rng.permutation(coords.shape[0])]
    rank = lvl.build_from_coords(_t(inp, device))
    m = coords.shape[0]
    assert lvl.num_active() == m
    got = lvl.coords[:m].cpu().numpy()
    assert np.array_equal(got[rank.cpu().numpy()], inp)                              # rank_of_input points at the input's own cell
    bk = sr.keys_of_coords(got, shape, 1)
    assert np.all(np.diff(bk.astype(np.int64)) > 0)                                  # storage rows in ascending brick key
    bitmap, prefix, _, _ = sr.expected_index(sr.keys_of_coords(coords, shape, 1), sr.nwords(batch, shape, 1))
    assert np.array_equal(_u32(lvl.bitmap), bitmap) and np.array_equal(_u32(lvl.prefix), prefix)
    order = canon_order(got, shape)
    assert np.array_equal(got[order], coords)                                         # (np.nonzero order = the canonical order)

    def check(nbr, ref, out_order, in_order):
        mo = out_order.size
        tab = nbr.words[:, :mo].cpu().numpy()
        assert np.array_equal(canon_table(tab, out_order, in_order), ref)
        masks = nbr.tile_masks.cpu().numpy().astype(np.uint32)
        for gi in range(masks.shape[0]):
            blk = tab[:, gi * 32:(gi + 1) * 32]
            want = 0
            for t in range(tab.shape[0]):
                if blk.shape[1] and (blk[t] >= 0).any():
                    want |= 1 << t
            assert int(masks[gi]) == want, (gi, hex(int(masks[gi])), hex(want))

    K3, S1, P1 = (3, 3, 3), (1, 1, 1), (1, 1, 1)
    check(lvl.neighbors_to(lvl, K3, S1, P1), osp.neighbor_table(coords, shape, coords, K3, S1, P1), order, order)
    for k, s, p in [(K3, (2, 2, 2), (1, 1, 1)), (K3, (2, 2, 2), (0, 1, 1)), ((3, 1, 1), (2, 1, 1), (0, 0, 0))]:
        nxt = lvl.downsample(k, s, p)
        oc, oshape = osp.conv_out_coords(coords, shape, k, s, p)
        assert nxt.shape == list(oshape) and nxt.num_active() == oc.shape[0] and nxt.layout == 1
        got_o = nxt.coords[:oc.shape[0]].cpu().numpy()
        assert np.all(np.diff(sr.keys_of_coords(got_o, oshape, 1).astype(np.int64)) > 0)
        o_order = canon_order(got_o, oshape)
        assert np.array_equal(got_o[o_order], oc)
        check(lvl.neighbors_to(nxt, k, s, p), osp.neighbor_table(coords, shape, oc, k, s, p), o_order, order)
        check(nxt.neighbors_to(nxt, K3, S1, P1), osp.neighbor_table(oc, list(oshape), oc, K3, S1, P1), o_order, o_order)
