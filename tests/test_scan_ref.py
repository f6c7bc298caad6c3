"""CPU self-tests of tests/scan_ref.py: the numpy reference the GPU scan and voxelizer edge tests compare against."""
import numpy as np
import pytest

from tests import scan_ref as sr

RAGGED = [(1, [1, 1, 1]), (2, [3, 5, 33]), (2, [5, 9, 70]), (2, [4, 8, 64]), (3, [2, 17, 9])]
# the grids of tests/test_gpu_scan.py: (batch, [D,H,W], layouts)
SCAN_GRIDS = [
    (1, [1, 1, 1], (0, 1)), (2, [3, 5, 33], (0, 1)), (2, [5, 9, 70], (0, 1)),
    (1, [2, 64, 64], (0, 1)), (1, [2, 64, 66], (0, 1)),
    (1, [64, 1024, 1024], (0, 1)), (1, [64, 1024, 1032], (0, 1)),
    (3, [41, 1504, 1504], (0, 1)), (6, [41, 1504, 1504], (0,)), (24, [41, 1504, 1504], (0,)),
]
SMALL = {(1, 1, 1), (3, 5, 33), (5, 9, 70)}         # grids with brick columns that overhang H or W


def _all_cells(batch, shape):
    b, z, y, x = np.meshgrid(np.arange(batch), np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing='ij')
    return np.stack([b.ravel(), z.ravel(), y.ravel(), x.ravel()], 1).astype(np.int64)


@pytest.mark.parametrize('layout', [0, 1])
@pytest.mark.parametrize('batch,shape', RAGGED)
def test_key_round_trip_and_order(batch, shape, layout):
    c = _all_cells(batch, shape)
    k = sr.keys_of_coords(c, shape, layout)
    assert k.dtype == np.uint64 and np.unique(k).size == k.size and int(k.max()) == sr.last_key(batch, shape, layout)
    assert int(k.max()) < sr.cells(batch, shape, layout)
    back, ok = sr.cells_of_keys(k, batch, shape, layout)
    assert ok.all() and np.array_equal(back, c)
    # every key of the key space that is no cell is reported invalid, every other one maps back to itself
    every = np.arange(sr.nwords(batch, shape, layout) * 32, dtype=np.uint64)
    cc, ok = sr.cells_of_keys(every, batch, shape, layout)
    assert int(ok.sum()) == c.shape[0]
    assert np.array_equal(sr.keys_of_coords(cc[ok], shape, layout), every[ok])
    if layout == 0:
        assert ok[:c.shape[0]].all() and not ok[c.shape[0]:].any()
    order = np.argsort(k, kind='stable')
    if layout == 0:
        ref = np.lexsort((c[:, 3], c[:, 2], c[:, 1], c[:, 0]))
    else:       # ascending (b, y/8, x/8, z, y%8, x%8)
        ref = np.lexsort((c[:, 3] % 8, c[:, 2] % 8, c[:, 1], c[:, 3] // 8, c[:, 2] // 8, c[:, 0]))
        bk = ((((c[:, 0] * ((shape[1] + 7) // 8) + c[:, 2] // 8) * ((shape[2] + 7) // 8) + c[:, 3] // 8) * shape[0] + c[:, 1]) * 64
              + (c[:, 2] % 8) * 8 + c[:, 3] % 8)
        assert np.array_equal(bk.astype(np.uint64), k)
    assert np.array_equal(order, ref)


def test_keys_hold_above_two_to_the_31():
    shape = [41, 1504, 1504]
    assert sr.last_key(24, shape, 0) == 24 * 41 * 1504 * 1504 - 1 > 2 ** 31
    c = np.array([[23, 40, 1503, 1503], [23, 10, 0, 1], [22, 0, 0, 0]], np.int64)
    for layout in (0, 1):
        k = sr.keys_of_coords(c, shape, layout)
        assert int(k[0]) == sr.last_key(24, shape, layout) and (layout == 1 or int(k[1]) >= 2 ** 31 > int(k[2]))
        back, ok = sr.cells_of_keys(k, 24, shape, layout)
        assert ok.all() and np.array_equal(back, c)


def test_dynamic_key_is_x_major():
    grid = [33, 5, 3]
    b, x, y, z = np.meshgrid(np.arange(2), np.arange(33), np.arange(5), np.arange(3), indexing='ij')
    k = sr.key_dynamic(b.ravel(), x.ravel(), y.ravel(), z.ravel(), grid)
    assert np.array_equal(k, np.arange(2 * 33 * 5 * 3, dtype=np.uint64))         # (b, x, y, z) row-major


@pytest.mark.parametrize('batch,shape,layouts', SCAN_GRIDS)
def test_nwords_and_regimes(batch, shape, layouts):
    for layout in layouts:
        nw = sr.nwords(batch, shape, layout)
        assert nw % 8 == 0 and nw * 32 >= sr.cells(batch, shape, layout) > (nw - 8) * 32
    want = {(1, 1, 1): 8, (3, 5, 33): 32, (5, 9, 70): 200, (2, 64, 64): 256, (2, 64, 66): 264, (64, 1024, 1024): 1 << 21,
            (64, 1024, 1032): (1 << 21) + 16384}
    if tuple(shape) in want:
        assert sr.nwords(batch, shape, 0) == want[tuple(shape)]
    if shape == [64, 1024, 1024]:
        assert sr.nwords(1, shape, 1) == 1 << 21 and sr.scan_regime(1 << 21) == (1, 8192, 1)
    if shape == [64, 1024, 1032]:
        assert sr.nwords(1, shape, 1) == (1 << 21) + 16384 and sr.scan_regime((1 << 21) + 16384) == (4, 2064, 1)
    if shape == [41, 1504, 1504]:
        assert sr.scan_regime(sr.nwords(batch, shape, 0)) == {3: (4, 8491, 2), 6: (4, 16982, 3), 24: (4, 67927, 9)}[batch]
        assert sr.nwords(batch, shape, 1) == sr.nwords(batch, shape, 0)


@pytest.mark.parametrize('batch,shape,layouts', SCAN_GRIDS)
def test_boundary_keys_realise_every_named_position(batch, shape, layouts):
    for layout in layouts:
        nw, last = sr.nwords(batch, shape, layout), sr.last_key(batch, shape, layout)
        lastword = last >> 5
        pos = sr.boundary_positions(nw, last)
        keys = sr.boundary_keys(nw, last)
        # the named positions: both chunk sizes, every edge that exists, the ragged chunk, first and last cell
        want = {'first', 'last', 'ragged_256', 'ragged_1024'}
        for chunk in sr.CHUNKS:
            for c in sr.EDGE_CHUNKS:
                if c * chunk <= lastword:
                    want.add('edge_%d_%d' % (chunk, c))
        assert set(pos) == want
        assert pos['first'] == [(0, 0)] and pos['last'] == [(lastword, last & 31)]
        for chunk in sr.CHUNKS:
            for c in sr.EDGE_CHUNKS:
                name = 'edge_%d_%d' % (chunk, c)
                if name in pos:
                    e = c * chunk
                    assert [w for w, _ in pos[name]] == [e - 1, e - 1, e, e]
                    assert [b for _, b in pos[name]][:3] == [0, 31, 0] and pos[name][3][1] == (31 if e < lastword else last & 31)
            r = pos['ragged_%d' % chunk]
            assert [w for w, _ in r] == [lastword // chunk * chunk] * 2 + [lastword] * 2 and r[0][1] == 0 and r[2][1] == 0
        for name, k in keys.items():
            assert np.array_equal(k, np.array([w * 32 + b for w, b in pos[name]], np.uint64))
            _, ok = sr.cells_of_keys(k, batch, shape, layout)
            if layout == 0 or tuple(shape) not in SMALL:
                assert ok.all(), (name, layout)                      # nothing may be dropped
            else:
                assert ok.any(), (name, layout)                      # only keys outside H or W are dropped; one per group survives
                c, _ = sr.cells_of_keys(k[~ok], batch, shape, layout)
                assert np.all((c[:, 2] >= shape[1]) | (c[:, 3] >= shape[2])) and np.all(k[~ok] < sr.cells(batch, shape, layout))
        # the dense stretch straddles a chunk edge of both sizes and consists of valid cells only
        w = sr.dense_stretch_words(nw, last)
        if lastword >= 256 + 150:
            assert w.size == 300 and (w[150] % 1024 == 0 or (w[150] == 256 and lastword < 1024 + 150)) and w[-1] <= lastword
            if sr.scan_regime(nw)[2] > 1:
                assert w[150] == sr.TRIP * 1024                      # ... and the edge between two trips where there is one
            if tuple(shape) not in SMALL:
                _, ok = sr.cells_of_keys(sr.dense_stretch_keys(nw, last), batch, shape, layout)
                assert ok.all()


@pytest.mark.parametrize('layout', [0, 1])
@pytest.mark.parametrize('batch,shape', [(2, [5, 9, 70]), (1, [2, 64, 66]), (2, [3, 5, 33])])
def test_expected_index_on_small_grids(batch, shape, layout):
    cells, keys, surv = sr.edge_case_cells(batch, shape, layout, seed=3)
    assert min(surv.values()) >= 1 and np.all(np.diff(keys.astype(np.int64)) > 0)
    nw = sr.nwords(batch, shape, layout)
    rng = np.random.default_rng(0)
    inp = np.concatenate([keys, keys])[rng.permutation(2 * keys.size)]
    bitmap, prefix, order, count = sr.expected_index(inp, nw)
    assert count == keys.size and np.array_equal(inp[order], keys)
    # brute force: one bit per key, prefix by counting
    bits = np.zeros(nw * 32, bool)
    bits[keys.astype(np.int64)] = True
    assert np.array_equal(bitmap, np.packbits(bits.reshape(-1, 32), axis=1, bitorder='little').view('<u4').ravel())
    assert np.array_equal(prefix, np.concatenate([[0], np.cumsum(bits.reshape(-1, 32).sum(1))[:-1]]).astype(np.uint32))
    assert np.array_equal(sr.popcount32(bitmap), bits.reshape(-1, 32).sum(1).astype(np.uint32))
    assert np.array_equal(keys[sr.rank_of_keys(inp)], inp)
    words = np.concatenate([rng.integers(0, nw, 64), [0, nw - 1]])
    bm, pf = sr.expected_at_words(inp, words)
    assert np.array_equal(bm, bitmap[words]) and np.array_equal(pf, prefix[words])


def test_reference_mutations_are_visible():
    """What the GPU tests rely on, shown on the reference: a scan that drops the carry between two trips of 8192 chunk totals, or
    that skips a line's last word, differs from expected_index at positions the boundary keys occupy."""
    batch, shape = 3, [41, 1504, 1504]
    nw, last = sr.nwords(batch, shape, 0), sr.last_key(batch, shape, 0)
    keys = np.concatenate(list(sr.boundary_keys(nw, last).values()))
    bitmap, prefix, _, count = sr.expected_index(keys, nw)
    edge = sr.TRIP * 1024                                             # first word of the second trip
    assert bitmap[edge - 1] and bitmap[edge] and prefix[edge] > 0
    no_carry = prefix.copy()
    no_carry[edge:] -= prefix[edge]                                   # second trip restarted at zero
    assert not np.array_equal(no_carry[bitmap != 0], prefix[bitmap != 0])
    # a line's last word: boundary word 1023 is word 31 of its 32-word line and the line's only occupied word
    line = bitmap[1023 // 32 * 32: 1024]
    assert line[31] and not line[:31].any()
    skipped = bitmap.copy()
    skipped[31::32] = 0
    assert int(sr.popcount32(skipped).sum()) < count
