"""Numpy reference of the bitmap index (test infrastructure): cell keys of both layouts and their inverses, the dynamic voxelizer's
x-major key, the padded word count, the expected bitmap / prefix / row order of a key list, and the key sets that put bits on the
regime edges of the three-launch scan.  Written from the layouts documented in detzero_amd/csrc/common.h (LevelGeom, ScanDims), in
uint64 throughout - a 24-frame level-1 grid has keys at and above 2^31.

    layout 0 (linear): key = ((b*D + z)*H + y)*W + x
    layout 1 (brick):  key = ((((b*NBY + y/8)*NBX + x/8)*D + z) << 6) | (y%8 << 3) | x%8,   NBY = ceil(H/8), NBX = ceil(W/8)
    dynamic (x-major): key = ((b*GX + x)*GY + y)*GZ + z
    words:             ceil(cells / 32) rounded up to a multiple of 8

The scan's regimes (csrc/sparse_index.hip): a workgroup covers a chunk of 256 words (nwords <= 2^21) or of 1024 words (above);
k_scan_partials scans the chunk totals in trips of 8192."""
import numpy as np

U64 = np.uint64
LINEAR, BRICK = 0, 1
CHUNKS = (256, 1024)
ONE_WORD_LIMIT = 1 << 21          # largest nwords scanned with one word per thread
TRIP = 8192                       # chunk totals per trip of k_scan_partials
EDGE_CHUNKS = (1, 2, 1023, 1024, 8191, 8192, 16383, 16384)      # chunk indices whose leading edge carries boundary bits


def _u(a):
    return np.asarray(a).astype(U64)


def key_linear(b, z, y, x, shape):
    d, h, w = (U64(int(s)) for s in shape)
    return ((_u(b) * d + _u(z)) * h + _u(y)) * w + _u(x)


def key_brick(b, z, y, x, shape):
    d, h, w = (int(s) for s in shape)
    nby, nbx = U64((h + 7) // 8), U64((w + 7) // 8)
    y, x = _u(y), _u(x)
    brick = (_u(b) * nby + y // U64(8)) * nbx + x // U64(8)
    return ((brick * U64(d) + _u(z)) << U64(6)) | ((y % U64(8)) << U64(3)) | (x % U64(8))


def key_of(b, z, y, x, shape, layout):
    return key_linear(b, z, y, x, shape) if layout == LINEAR else key_brick(b, z, y, x, shape)


def keys_of_coords(coords, shape, layout):
    c = np.asarray(coords)
    return key_of(c[:, 0], c[:, 1], c[:, 2], c[:, 3], shape, layout)


def key_dynamic(b, x, y, z, grid):
    """DynamicMeanVFE merge key; grid = [GX, GY, GZ]."""
    gx, gy, gz = (U64(int(s)) for s in grid)
    return ((_u(b) * gx + _u(x)) * gy + _u(y)) * gz + _u(z)


def cells(batch, shape, layout):
    d, h, w = (int(s) for s in shape)
    if layout == LINEAR:
        return batch * d * h * w
    return batch * ((h + 7) // 8) * ((w + 7) // 8) * d * 64


def nwords(batch, shape, layout):
    return (((cells(batch, shape, layout) + 31) // 32) + 7) // 8 * 8


def last_key(batch, shape, layout):
    """Key of the last valid cell: both keys are lexicographic in fields that all peak at (B-1, D-1, H-1, W-1)."""
    d, h, w = (int(s) for s in shape)
    return int(key_of(batch - 1, d - 1, h - 1, w - 1, shape, layout))


def cells_of_keys(keys, batch, shape, layout):
    """keys -> ([b,z,y,x] int64 (n,4), valid (n,) bool).  Invalid: keys past `cells`, brick keys whose y or x lies outside H or W."""
    k = _u(keys)
    d, h, w = (int(s) for s in shape)
    if layout == LINEAR:
        x = k % U64(w); t = k // U64(w)
        y = t % U64(h); t = t // U64(h)
        z = t % U64(d); b = t // U64(d)
    else:
        nby, nbx = (h + 7) // 8, (w + 7) // 8
        inner = k & U64(63)
        t = k >> U64(6)
        z = t % U64(d); t = t // U64(d)
        bx = t % U64(nbx); t = t // U64(nbx)
        by = t % U64(nby); b = t // U64(nby)
        y = by * U64(8) + (inner >> U64(3))
        x = bx * U64(8) + (inner & U64(7))
    valid = (k < U64(cells(batch, shape, layout))) & (b < U64(batch)) & (y < U64(h)) & (x < U64(w))
    return np.stack([b, z, y, x], 1).astype(np.int64), valid


def popcount32(words):
    words = np.ascontiguousarray(words, np.uint32)
    if hasattr(np, 'bitwise_count'):
        return np.bitwise_count(words).astype(np.uint32)
    table = np.array([bin(i).count('1') for i in range(256)], np.uint32)
    return table[words.view(np.uint8)].reshape(-1, 4).sum(1, dtype=np.uint32)


def expected_index(keys, n_words):
    """keys (n,) any order, duplicates allowed -> (bitmap uint32[n_words], prefix uint32[n_words] = exclusive sum of the per-word
    popcounts, order = input positions of the distinct keys in ascending key order (the rows of the level), count)."""
    k = _u(keys)
    bitmap = np.zeros(int(n_words), np.uint32)
    np.bitwise_or.at(bitmap, (k >> U64(5)).astype(np.int64), (np.uint32(1) << (k & U64(31)).astype(np.uint32)))
    pop = popcount32(bitmap)
    prefix = np.zeros(int(n_words), np.uint32)
    np.cumsum(pop[:-1], dtype=np.uint32, out=prefix[1:])
    uniq, order = np.unique(k, return_index=True)
    assert int(pop.sum(dtype=np.uint64)) == uniq.size
    return bitmap, prefix, order, int(uniq.size)


def expected_at_words(keys, words):
    """Bitmap and prefix at the listed words only, without the whole arrays (the 24-frame grid): prefix[w] = number of distinct
    keys below 32 * w."""
    uniq = np.unique(_u(keys))
    w = _u(words)
    lo = np.searchsorted(uniq, w << U64(5), side='left')
    hi = np.searchsorted(uniq, (w + U64(1)) << U64(5), side='left')
    bitmap = np.zeros(w.size, np.uint32)
    for i in np.nonzero(hi > lo)[0]:
        bits = (uniq[lo[i]:hi[i]] & U64(31)).astype(np.uint32)
        bitmap[i] = np.bitwise_or.reduce(np.uint32(1) << bits)
    return bitmap, lo.astype(np.uint32)


def rank_of_keys(keys):
    """Row of every input key (duplicates included) among the distinct keys in ascending order."""
    k = _u(keys)
    return np.searchsorted(np.unique(k), k).astype(np.int32)


def scan_regime(n_words):
    """(words per thread, workgroups, trips of k_scan_partials) the scan runs at for n_words."""
    wpt = 1 if n_words <= ONE_WORD_LIMIT else 4
    blocks = (n_words + 256 * wpt - 1) // (256 * wpt)
    return wpt, blocks, (blocks + TRIP - 1) // TRIP


def boundary_positions(n_words, last):
    """Named (word, bit) positions that sit on the scan's regime edges, derived from the word count and the key of the last valid
    cell alone (layout-independent).  Words past the last valid cell's word are padding and hold no position; a bit 31 that would
    lie past the last valid cell (only possible in its word) is moved onto that cell.
    Returns {name: [(word, bit), ...]}."""
    lastword = last >> 5
    assert lastword < n_words
    groups = {'first': [(0, 0)], 'last': [(lastword, last & 31)]}

    def word(w):
        return [(w, 0), (w, min(31, last - 32 * w))]

    for chunk in CHUNKS:
        for c in EDGE_CHUNKS:
            e = c * chunk                       # first word of chunk c: the edge between chunks c - 1 and c
            if e <= lastword:
                groups['edge_%d_%d' % (chunk, c)] = word(e - 1) + word(e)
        groups['ragged_%d' % chunk] = word(lastword // chunk * chunk) + word(lastword)
    return groups


def boundary_keys(n_words, last):
    """{name: uint64 keys} of boundary_positions."""
    return {name: np.array([w * 32 + b for w, b in pos], U64) for name, pos in boundary_positions(n_words, last).items()}


def dense_stretch_words(n_words, last, length=300):
    """`length` consecutive words straddling a chunk edge (the trip edge 8192 * 1024 where the grid has one, else word 1024, else
    word 256); none on grids too small to hold them."""
    lastword = last >> 5
    for e in (TRIP * 1024, 1024, 256):
        if e + length // 2 <= lastword:
            return np.arange(e - length // 2, e + length // 2, dtype=np.int64)
    return np.zeros((0,), np.int64)


def dense_stretch_keys(n_words, last, length=300):
    w = dense_stretch_words(n_words, last, length)
    return (w[:, None] * 32 + np.arange(32)[None, :]).reshape(-1).astype(U64)


def random_cells(rng, batch, shape, n, frames=None):
    """n random cells [b,z,y,x] (duplicates possible); frames: choose b from this list only."""
    d, h, w = (int(s) for s in shape)
    b = rng.integers(0, batch, n) if frames is None else rng.choice(np.asarray(frames), n)
    return np.stack([b, rng.integers(0, d, n), rng.integers(0, h, n), rng.integers(0, w, n)], 1).astype(np.int64)


def edge_case_cells(batch, shape, layout, seed=0, n_random=20000, random_frames=None):
    """The active set of the scan tests: boundary bits, a dense stretch, random cells - as distinct [b,z,y,x] rows (int32) with
    their keys, plus {group name: number of that group's keys that are valid cells}.  Keys that are no cell of the grid (brick
    bricks that overhang H or W) are dropped."""
    nw, last = nwords(batch, shape, layout), last_key(batch, shape, layout)
    groups = boundary_keys(nw, last)
    survivors = {}
    parts = []
    for name, k in groups.items():
        c, ok = cells_of_keys(k, batch, shape, layout)
        survivors[name] = int(ok.sum())
        parts.append(c[ok])
    c, ok = cells_of_keys(dense_stretch_keys(nw, last), batch, shape, layout)
    parts.append(c[ok])
    rng = np.random.default_rng(seed)
    total = batch * int(shape[0]) * int(shape[1]) * int(shape[2])
    n_random = min(n_random, max(1, total // 2))
    if random_frames is None:
        parts.append(random_cells(rng, batch, shape, n_random))
    else:                                   # half of the random cells in the listed frames
        parts.append(random_cells(rng, batch, shape, n_random // 2))
        parts.append(random_cells(rng, batch, shape, n_random - n_random // 2, random_frames))
    cells_ = np.unique(np.concatenate(parts, 0), axis=0)
    keys = keys_of_coords(cells_, shape, layout)
    o = np.argsort(keys, kind='stable')
    return cells_[o].astype(np.int32), keys[o], survivors
