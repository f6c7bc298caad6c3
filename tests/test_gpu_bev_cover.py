"""GPU (MI355X): the free-offset tile cover of the first BEV block (dz_bev_tile_cover, dz_bev_fill_spans, explicit-origin entries in
k_conv3x3_h's tile list) - the planner against a numpy restatement of its rule, the launches over a cover list + the span fill against the
same layer launched over all tiles (bit for bit), and an eager chain against its captured replay on another occupancy.

Shapes: 2 frames of 24 x 70 (three bands, width no multiple of 32, more than two tiles wide) and 20 x 40 (partial last band).  The dense
128-channel instance k_conv3x3_h<8x32x128> takes a layer from 384 grid tiles per launch (conv3x3_h_variant); below that the generic kernel
runs, which ignores the list.  So the dense cases run twice: at 2 frames (the generic kernel computes every pixel, the fill rewrites the
spans) and with the same two occupancies repeated over 44 / 64 frames (396 / 384 tiles), where the instance under test is the one selected -
asserted by name.  The sparse-input instance has no such threshold and runs at 2 frames."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
MODES = [('f16x2', 1), ('bf16x2', 2)]
SIZES = [(24, 70), (20, 40)]
TAG = 0x80000000


def _cases(ho, wo):
    """name -> (2, ho, wo) occupancy."""
    rng = np.random.default_rng(ho * 1000 + wo)
    z = lambda: np.zeros((2, ho, wo), bool)
    c = {'empty': z(), 'full': ~z()}
    corners = z()
    corners[0, [0, 0, -1, -1], [0, -1, 0, -1]] = True          # a single pixel in each corner ...
    corners[1, ho // 2, wo - 1] = True                         # ... and on the last column: a tile clipped at the right edge
    c['corners'] = corners
    straddle = z()
    straddle[0, 10, [28, 36]] = True                           # busy intervals around x = 28 and 36: one tile, two on the 32-column grid
    straddle[1, 3, [30, 33]] = True
    c['straddle'] = straddle
    c['random25'] = rng.random((2, ho, wo)) < 0.25
    half = z()
    half[1] = True
    c['empty_beside_full'] = half
    return c


def _busy(occ_b, y0, l):
    """Busy columns of band [y0, y0 + 8) at layer l: an occupied pixel within rows [y0 - l, y0 + 7 + l] and columns [x - l, x + l]."""
    ho, wo = occ_b.shape
    col = occ_b[max(0, y0 - l):min(ho, y0 + 8 + l)].any(0)
    busy = np.zeros(wo, bool)
    for x in np.nonzero(col)[0]:
        busy[max(0, x - l):x + l + 1] = True
    return busy


def _plan(occ, l):
    """The rule restated: per (b, band) sweep x from 0, a tile [x, x + 32) at the first busy column not yet covered; spans = the maximal
    column intervals outside the tiles.  -> tiles [(b, ty, x0)], spans [(b, ty, xs, xe)], grid tiles to run per (b, band)."""
    nb, ho, wo = occ.shape
    tiles, spans, grid = [], [], []
    for b in range(nb):
        for ty in range(-(-ho // 8)):
            busy = _busy(occ[b], 8 * ty, l)
            cov = np.zeros(wo, bool)
            x = 0
            while x < wo:
                if busy[x]:
                    tiles.append((b, ty, x))
                    cov[x:x + 32] = True
                    x += 32
                else:
                    x += 1
            x = 0
            while x < wo:
                if cov[x]:
                    x += 1
                    continue
                xs = x
                while x < wo and not cov[x]:
                    x += 1
                spans.append((b, ty, xs, x))
            grid.append(sum(bool(busy[32 * tx:32 * tx + 32].any()) for tx in range(-(-wo // 32))))
    return tiles, spans, grid


def _unpack(e):
    assert e & TAG, 'entry without the explicit-origin bit: %#x' % e
    return (e >> 21) & 0x3FF, (e >> 12) & 0x1FF, e & 0xFFF


def _decode(row):
    """A cover list (numpy uint32) -> tiles, spans."""
    n, ns = int(row[0]), int(row[1])
    tiles = [_unpack(int(e)) for e in row[2:2 + n]]
    sp = row[2 + n:2 + n + 2 * ns]
    spans = [_unpack(int(sp[2 * k])) + (int(sp[2 * k + 1]),) for k in range(ns)]
    return tiles, spans


def _ridx(occ, device, rows=None):
    """Row-index image (B, ho + 2, wo + 2, 2) of an occupancy: slab 0 holds a row at every third occupied pixel, slab 1 at the others and at
    some of those too (a pixel is occupied if EITHER slab holds a row).  rows: draw the row numbers below it (else the pixel's number)."""
    nb, ho, wo = occ.shape
    idx = np.full((nb, ho + 2, wo + 2, 2), -1, np.int32)
    pix = np.nonzero(occ)
    k = np.arange(pix[0].size)
    rid = (k * 7 + 3) % rows if rows else k
    s0, s1 = k % 3 == 0, (k % 3 != 0) | (k % 6 == 0)
    idx[pix[0][s0], pix[1][s0] + 1, pix[2][s0] + 1, 0] = rid[s0]
    idx[pix[0][s1], pix[1][s1] + 1, pix[2][s1] + 1, 1] = (rid[s1] * 5 + 1) % rows if rows else rid[s1]
    return torch.from_numpy(idx).to(device)


@pytest.mark.parametrize('ho,wo', SIZES)
def test_planner_equals_the_rule(device, ho, wo):
    from detzero_amd import ops
    ty_n, tx_n = -(-ho // 8), -(-wo // 32)
    for name, occ in _cases(ho, wo).items():
        lists = ops.bev_tile_list(_ridx(occ, device), ho, wo, 6)
        cover = ops.bev_tile_cover(lists, 2, ho, wo).cpu().numpy().view(np.uint32)
        lists = lists.cpu().numpy()
        for l in range(1, 7):
            tiles, spans, grid = _plan(occ, l)
            got_t, got_s = _decode(cover[l - 1])
            assert got_t == tiles and got_s == spans, (name, l, got_t, tiles, got_s, spans)
            # the properties, on what the device wrote
            assert got_t == sorted(got_t), (name, l)                                           # ascending (b, ty, x0)
            cov = np.zeros((2, ty_n, wo + 32), np.int32)
            for b, ty, x0 in got_t:
                assert 0 <= x0 < wo
                cov[b, ty, x0:x0 + 32] += 1
            assert cov.max(initial=0) <= 1, (name, l, 'tiles of a band overlap')
            fill = np.zeros((2, ty_n, wo), np.int32)
            for b, ty, xs, xe in got_s:
                assert 0 <= xs < xe <= wo
                fill[b, ty, xs:xe] += 1
            assert np.array_equal(fill, 1 - cov[:, :, :wo]), (name, l, 'spans are not the complement of the tiles')
            per_band = np.zeros((2, ty_n), np.int32)
            for b, ty, _ in got_t:
                per_band[b, ty] += 1
            for b in range(2):
                for ty in range(ty_n):
                    busy = _busy(occ[b], 8 * ty, l)
                    assert not (busy & ~cov[b, ty, :wo].astype(bool)).any(), (name, l, b, ty, 'a busy column is not covered')
                    assert per_band[b, ty] <= grid[b * ty_n + ty], (name, l, b, ty)
            # the grid list of the same rows: counts and ids of the rule on the fixed 32-column grid
            run = np.array([_busy(occ[b], 8 * ty, l)[32 * tx:32 * tx + 32].any() for b in range(2) for ty in range(ty_n) for tx in range(tx_n)])
            g = lists[l - 1]
            assert g[0] == run.sum() == sum(grid) and g[1] == (~run).sum(), (name, l)
            assert np.array_equal(g[2:2 + g[0]], np.nonzero(run)[0]) and np.array_equal(g[2 + g[0]:2 + g[0] + g[1]], np.nonzero(~run)[0]), (name, l)
            if name == 'empty':
                assert got_t == [] and got_s == [(b, ty, 0, wo) for b in range(2) for ty in range(ty_n)]
            if name == 'full':
                assert got_s == [] and len(got_t) == 2 * ty_n * tx_n
        if name == 'straddle':
            t1, _, g1 = _plan(occ, 1)
            assert [t for t in t1 if t[0] == 0] == [(0, 1, 27)] and g1[1] == 2             # one tile where the grid needs two


def _near(occ, r):
    """Pixels within Chebyshev distance r of an occupied pixel."""
    from scipy.ndimage import maximum_filter
    return np.stack([maximum_filter(o, size=2 * r + 1, mode='constant', cval=False) for o in occ]) if r else occ.copy()


def _bordered(x, device):
    """(B, ho, wo, C) -> zero-bordered (B, ho + 2, wo + 2, C)."""
    out = torch.zeros((x.shape[0], x.shape[1] + 2, x.shape[2] + 2, x.shape[3]), dtype=x.dtype, device=device)
    out[:, 1:-1, 1:-1] = x
    return out


def _nan_interior(shape, device):
    out = torch.full(shape, float('nan'), dtype=torch.float32, device=device)
    out[:, 0], out[:, -1], out[:, :, 0], out[:, :, -1] = 0, 0, 0, 0
    return out


def _border_is_zero(img):
    v = img.view(torch.int32)
    return not (v[:, 0].any() or v[:, -1].any() or v[:, :, 0].any() or v[:, :, -1].any())


def _watch_variant(monkeypatch):
    """Names of the kernels the library selects for the ops.conv2d launches that follow."""
    from detzero_amd import ops
    names, real = [], ops.conv2d

    def conv2d(desc, math=0, out_f32=False, **k):
        names.append(ops.L.load().dz_conv2d_variant_split(ctypes.byref(ops._conv2d_desc(desc)), 1 if out_f32 else 0).decode())
        return real(desc, math=math, out_f32=out_f32, **k)
    monkeypatch.setattr(ops, 'conv2d', conv2d)
    return names


@pytest.mark.parametrize('name,mid', MODES)
@pytest.mark.parametrize('ho,wo', SIZES)
def test_sparse_layer_over_the_cover_equals_all_tiles(device, monkeypatch, ho, wo, name, mid):
    """Layer 1 (SPARSE instance, two slabs of 32-channel rows -> 128): cover list + the constant fill against the list-less launch."""
    from detzero_amd import ops
    from detzero_amd.det_modules import conv_layer
    gen = torch.Generator(device=device).manual_seed(11 * mid + ho)
    c, cout, nrows = 32, 128, 512
    rows = ops.pair16_from_f32(torch.randn((nrows, c), generator=gen, device=device), c, mid)
    w = ops.pack_weight_split(torch.randn((9, 2 * c, cout), generator=gen, device=device) / 24, mid)
    scale = torch.rand(cout, generator=gen, device=device) + 0.5
    shift = torch.randn(cout, generator=gen, device=device) * 0.1
    names = _watch_variant(monkeypatch)
    for case, occ in _cases(ho, wo).items():
        idx = _ridx(occ, device, rows=nrows)
        kw = dict(cin=2 * c, in_cstride=2 * c, ksize=3, stride=1, in_off=0, out_cstride=cout, out_d=(1, 1), ho=ho, wo=wo, batch=2, math=mid,
                  in_rowidx=idx, in_row_channels=c, in_rows=nrows)
        ref = torch.zeros((2, ho + 2, wo + 2, cout), dtype=torch.float32, device=device)
        conv_layer(rows, (ho + 2, wo + 2), w, scale, shift, True, ref, (ho + 2, wo + 2), **kw)
        cover = ops.bev_tile_cover(ops.bev_tile_list(idx, ho, wo, 1), 2, ho, wo)
        out = _nan_interior(ref.shape, device)
        conv_layer(rows, (ho + 2, wo + 2), w, scale, shift, True, out, (ho + 2, wo + 2), in_tiles=cover[0], **kw)
        ops.bev_fill_empty_tiles(cover[0], 2, ho, wo, shift, True, cout, out, mid)
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32)) and _border_is_zero(out), case
    assert names and all(n.startswith('k_conv3x3_h<8x32x128') for n in names), names


@pytest.mark.parametrize('name,mid', MODES)
@pytest.mark.parametrize('ho,wo', SIZES)
def test_dense_layer_over_the_cover_equals_all_tiles(device, monkeypatch, ho, wo, name, mid):
    """Layers 2 and 6 (dense, 32 -> 128).  The layer's input is what the network hands it: the previous layer's zero-input response `zprev`
    (here a fixed non-constant image, so that a fill from the wrong place shows) at every pixel at least l away from any occupied one, data
    elsewhere.  Its own zero-input response = the list-less launch on zprev.  Cover list l + dz_bev_fill_spans against the list-less launch."""
    from detzero_amd import ops
    from detzero_amd.det_modules import conv_layer
    gen = torch.Generator(device=device).manual_seed(13 * mid + wo)
    cin, cout = 32, 128
    big = -(-384 // (-(-ho // 8) * -(-wo // 32)))                       # frames from which the 128-channel instance takes the layer ...
    big += big % 2                                                      # ... as whole pairs of the case's two frames: 44 / 64
    w = ops.pack_weight_split(torch.randn((9, cin, cout), generator=gen, device=device) / 17, mid)
    scale = torch.rand(cout, generator=gen, device=device) + 0.5
    shift = torch.randn(cout, generator=gen, device=device) * 0.1
    zprev = _bordered(ops.pair16_from_f32(torch.randn((1, ho, wo, cin), generator=gen, device=device).view(-1, cin), cin, mid).view(1, ho, wo, cin), device)
    shp = (ho + 2, wo + 2)
    kw = dict(cin=cin, in_cstride=cin, ksize=3, stride=1, in_off=0, out_cstride=cout, out_d=(1, 1), ho=ho, wo=wo, math=mid)
    names = _watch_variant(monkeypatch)
    for nb in (2, big):
        # (from a launch of nb frames: which kernel runs the layer depends on the tile count, and the image must carry ITS bits)
        zero = torch.zeros((nb, ho + 2, wo + 2, cout), dtype=torch.float32, device=device)
        conv_layer(zprev.expand(nb, -1, -1, -1).contiguous(), shp, w, scale, shift, True, zero, shp, batch=nb, **kw)
        zero = zero[:1].clone()
        data = ops.pair16_from_f32(torch.randn((nb * ho * wo, cin), generator=gen, device=device), cin, mid).view(nb, ho, wo, cin)
        for case, occ2 in _cases(ho, wo).items():
            occ = np.concatenate([occ2] * (nb // 2))
            idx = _ridx(occ, device)
            lists = ops.bev_tile_cover(ops.bev_tile_list(idx, ho, wo, 6), nb, ho, wo)
            for l in (2, 6):
                far = torch.from_numpy(~_near(occ, l - 1)).to(device)[..., None]
                x = _bordered(torch.where(far, zprev[:, 1:-1, 1:-1].view(torch.int32), data.view(torch.int32)).view(torch.float32), device)
                ref = torch.zeros((nb, ho + 2, wo + 2, cout), dtype=torch.float32, device=device)
                del names[:]
                conv_layer(x, shp, w, scale, shift, True, ref, shp, batch=nb, **kw)
                out = _nan_interior(ref.shape, device)
                conv_layer(x, shp, w, scale, shift, True, out, shp, batch=nb, in_tiles=lists[l - 1], **kw)
                ops.bev_fill_empty_tiles(lists[l - 1], nb, ho, wo, shift, True, cout, out, mid, zero_resp=zero)
                if nb == big:
                    assert names == ['k_conv3x3_h<8x32x128>'] * 2, names
                assert torch.equal(out.view(torch.int32), ref.view(torch.int32)) and _border_is_zero(out), (case, l, nb)


def test_captured_chain_rebuilds_its_lists(device):
    """Sparse-input layer + one dense layer behind it (128 -> 128, on the resident-tile instance: 44 frames), planner included, eager and
    captured; the graph is replayed after another occupancy was written into its row-index buffer.  Same bits as the eager chain and as
    the chain launched over all tiles: the lists are rebuilt on the device at every replay."""
    from detzero_amd import ops
    from detzero_amd.det_modules import conv_layer
    ho, wo, nb, mid, c, cout, nrows = 24, 70, 44, 1, 32, 128, 512
    gen = torch.Generator(device=device).manual_seed(5)
    rows = ops.pair16_from_f32(torch.randn((nrows, c), generator=gen, device=device), c, mid)
    w1 = ops.pack_weight_split(torch.randn((9, 2 * c, cout), generator=gen, device=device) / 24, mid)
    w2 = ops.pack_weight_split(torch.randn((9, cout, cout), generator=gen, device=device) / 34, mid)
    sc = [torch.rand(cout, generator=gen, device=device) + 0.5 for _ in range(2)]
    sh = [torch.randn(cout, generator=gen, device=device) * 0.1 for _ in range(2)]
    shp = (ho + 2, wo + 2)
    cases = _cases(ho, wo)
    occ_a = np.concatenate([cases['random25'], cases['corners']] * (nb // 4))
    occ_b = np.concatenate([cases['straddle'], cases['empty_beside_full']] * (nb // 4))
    idx_a, idx_b = _ridx(occ_a, device, rows=nrows), _ridx(occ_b, device, rows=nrows)
    k1 = dict(cin=2 * c, in_cstride=2 * c, ksize=3, stride=1, in_off=0, out_cstride=cout, out_d=(1, 1), ho=ho, wo=wo, math=mid,
              in_row_channels=c, in_rows=nrows)
    k2 = dict(cin=cout, in_cstride=cout, ksize=3, stride=1, in_off=0, out_cstride=cout, out_d=(1, 1), ho=ho, wo=wo, batch=nb, math=mid)

    def chain(idx, y1, y2, lists, zero2, batch=nb):
        conv_layer(rows, shp, w1, sc[0], sh[0], True, y1, shp, in_rowidx=idx, batch=batch, in_tiles=None if lists is None else lists[0], **k1)
        if lists is not None:
            ops.bev_fill_empty_tiles(lists[0], batch, ho, wo, sh[0], True, cout, y1, mid)
        conv_layer(y1, shp, w2, sc[1], sh[1], True, y2, shp, in_tiles=None if lists is None else lists[1], **dict(k2, batch=batch))
        if lists is not None:
            ops.bev_fill_empty_tiles(lists[1], batch, ho, wo, sh[1], True, cout, y2, mid, zero_resp=zero2)

    # zero-input response of layer 2: the all-tiles chain on an empty frame
    z1, z2 = (torch.zeros((nb, ho + 2, wo + 2, cout), dtype=torch.float32, device=device) for _ in range(2))
    chain(torch.full_like(idx_a, -1), z1, z2, None, None)
    zero2 = z2[:1].clone()

    def planned(idx, y1, y2):
        chain(idx, y1, y2, ops.bev_tile_cover(ops.bev_tile_list(idx, ho, wo, 2), nb, ho, wo), zero2)

    ref, eager = {}, {}
    for key, idx in (('a', idx_a), ('b', idx_b)):
        y1 = torch.zeros_like(z1)
        ref[key] = torch.zeros_like(z1)
        chain(idx, y1, ref[key], None, None)
        y1, eager[key] = _nan_interior(z1.shape, device), _nan_interior(z1.shape, device)
        planned(idx, y1, eager[key])
        assert torch.equal(eager[key].view(torch.int32), ref[key].view(torch.int32)), key
    static_idx, g1, g2 = idx_a.clone(), _nan_interior(z1.shape, device), _nan_interior(z1.shape, device)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        planned(static_idx, g1, g2)
    for key, idx in (('a', idx_a), ('b', idx_b)):
        static_idx.copy_(idx)
        g2[:, 1:-1, 1:-1] = float('nan')
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g2.view(torch.int32), eager[key].view(torch.int32)), key
    assert not torch.equal(eager['a'].view(torch.int32), eager['b'].view(torch.int32))
