"""GPU (MI355X): the bf16x3 gather-path sparse convolution of the exact-fp32 mode (csrc/sparse_conv_gt.hip, dz_spconv_forward_limb3:
every layer of the sparse backbone from its plain neighbour table and tile masks, every operand as three exact bf16 limbs) against a
float64 evaluation of the same rulebook at its edges, against the fp32 gather kernel's error, its limb terms bit for bit on
one-product outputs, its refusals, and the detector on it.

Geometry, tables, reference and metric are those of tests/test_gpu_sparse_conv.py (imported); the launch is this file's.  The exact-m
edges and the tile counts around the XCD deal need a level of a chosen row count, which only a submanifold table gives: they run on
the submanifold table of the layer's channels (the kernel does not know the layer kind), the other edges on the layer's own kind."""
import types
import zlib

import numpy as np
import pytest
import torch

from detzero_amd import lib as L
from detzero_amd import ops
from oracle import sparse as osp
from tests.test_gpu_conv3x3_limb3 import _patterned, _patterned_tiny, _pow2, _subnormal_report
from tests.test_gpu_sparse_conv import (KINDS, LAYERS, POISON, SENTINEL, TAIL, build_geometry, check_tables, edge_rows, normalised_error,
                                        ref64)
from tests.test_gpu_xrun import K3, P1, S1, _level, _t
from tests.test_gpu_xrun_limb3 import _one_hot_expect, _same_bits

pytestmark = pytest.mark.gpu
BOUND = 2.0 ** -19          # the project's BOUND['f32']: fp32 accumulation of at most 27 x 128 products + 2^-26 for the dropped terms
XRUN = 16                   # k_spconv_gt deals its row tiles to the 8 XCDs in runs of 16 (the deal of k_spconv_h)
XCD_TILES = (1, XRUN, XRUN + 1, 8 * XRUN - 1, 8 * XRUN, 8 * XRUN + 1)
M_EDGES = ('m=1', 'm=tile-1', 'm=tile', 'm=tile+1')
OWN_EDGES = ('dead tiles', 'm=cap', 'overflow', 'zero', 'unequal')
# the selector of csrc/sparse_conv_gt.hip, restated (test_edge_table_is_complete compares it with the library's answer)
INSTANCE = {(16, 16): 'k_spconv_gt<128x32x16>', (16, 32): 'k_spconv_gt<128x32x16>', (32, 32): 'k_spconv_gt<128x32x32>',
            (32, 64): 'k_spconv_gt<128x64x32>', (64, 64): 'k_spconv_gt<128x64x32>', (64, 128): 'k_spconv_gt<128x128x16>',
            (128, 128): 'k_spconv_gt<128x128x16>'}


def _case(cin, cout, kind, edge):
    return types.SimpleNamespace(label='gt %d->%d %s %s' % (cin, cout, kind, edge), engine='f32', mode='f32', cin=cin, cout=cout, kind=kind,
                                 kvol=int(np.prod(KINDS[kind][0])), edge=edge, masks=True, sort=False)


def _edge_cases():
    cs, seen, inst = [], set(), {}
    for cin, cout, kind in LAYERS:
        edges = [(kind, e) for e in OWN_EDGES + (('isolated',) if kind == 'subm' else ())] + [('subm', e) for e in M_EDGES]
        name = INSTANCE[(cin, cout)]
        if name not in inst:
            inst[name] = (cin, cout)
            edges += [('subm', 'tiles=%d' % t) for t in XCD_TILES]
        for k, e in edges:
            c = _case(cin, cout, k, e)
            if c.label not in seen:
                seen.add(c.label)
                cs.append(c)
    return cs


EDGE_CASES = _edge_cases()


def launch(case, x, in_rows, nbr, cap, d_m, wl, sc, sh, res, relu, out, expect_rc=0):
    lib = L.load()
    p = L.ptr
    rc = lib.dz_spconv_forward_limb3(p(x), in_rows, case.cin, p(nbr.words), p(nbr.tile_masks), case.kvol, cap, p(d_m), p(wl), p(sc), p(sh), p(res), relu,
                                     p(out), case.cout, L.stream())
    msg = lib.dz_last_error()
    assert rc == expect_rc, (case.label, rc, msg.decode() if msg else '')


def _operands(case, in_rows, cap, m_in, m, dev, seed):
    """N(0, 1) rows and weights, the BatchNorm scale sized so that outputs are O(1); NaN where nothing may be read."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    cin, cout, kvol = case.cin, case.cout, case.kvol
    x = torch.randn((in_rows, cin), generator=gen, device=dev)
    r = torch.randn((cap, cout), generator=gen, device=dev)
    w = torch.randn((kvol, cin, cout), generator=gen, device=dev)
    sc = ((torch.rand(cout, generator=gen, device=dev) + 0.5) / (kvol * cin) ** 0.5).contiguous()
    sh = (torch.randn(cout, generator=gen, device=dev) * 0.5).contiguous()
    x.view(torch.int32)[m_in:] = POISON
    r.view(torch.int32)[m:] = POISON
    return x, r, w, sc, sh


def convolve(case, lvl_in, lvl_out, nbr, tab, m_in, counter, dev, gather=False):
    """`case` on k_spconv_gt against float64 on the oracle's table: both switch settings, two launches each into a sentinel buffer.
    Returns (rows < m of the two settings, worst e, worst e of k_spconv on the same operands or None)."""
    cin, cout = case.cin, case.cout
    cap, in_rows = lvl_out.cap, lvl_in.cap
    assert nbr.tile_masks is not None and not nbr.packed
    d_m = lvl_out.d_m if counter is None else torch.tensor([counter], dtype=torch.int32, device=dev)
    m_level = lvl_out.num_active()
    m = min(m_level if counter is None else counter, cap)
    if counter is not None and counter > cap:
        assert m_level == cap, 'the overflow case needs a table whose cap rows are all live'
    check_tables(case, nbr, None, tab, min(m, m_level))
    assert m == 0 or int(tab[:, :m].max()) < m_in, 'the oracle table points past the live input rows'
    x, r, w, sc, sh = _operands(case, in_rows, cap, m_in, m, dev, zlib.crc32(case.label.encode()))
    wl = ops.pack_weight_limb3(w, cout_mult=32)
    acc, aacc = ref64(x[:m_in].double(), tab, w.double(), m)
    r64 = r[:m].double()
    worst, worst_g, results = 0.0, (0.0 if gather else None), []
    for on in (True, False):
        outs = [torch.full((cap + TAIL, cout), SENTINEL, dtype=torch.int32, device=dev) for _ in range(2)]
        for o in outs:
            launch(case, x, in_rows, nbr, cap, d_m, wl, sc if on else None, sh if on else None, r if on else None, 1 if on else 0, o)
        torch.cuda.synchronize(dev)
        what = (case.label, 'all on' if on else 'all off')
        assert torch.equal(outs[0], outs[1]), ('two launches differ',) + what
        out = outs[0]
        nbad = int((out[m:] != SENTINEL).sum())
        assert nbad == 0, ('%d words written at or beyond row m = %d (cap %d)' % (nbad, m, cap),) + what
        results.append(out[:m].clone())
        if m == 0:
            continue
        nkept = int((out[:m] == SENTINEL).sum())
        assert nkept == 0, ('%d words below row m = %d were not written' % (nkept, m),) + what
        args = (acc, aacc, sc.double() if on else None, sh.double() if on else None, r64 if on else None, on)
        got = out[:m].contiguous().view(torch.float32).double()
        err, ref, den = normalised_error(got, *args)
        e = float(err.max())
        print('  %-34s %-7s m %6d cap %6d  e = %.3e = %.2f x 2^-24 (bound 2^-19)' % (case.label, what[1], m, cap, e, e * 2 ** 24))
        if not e <= BOUND:
            i = int(torch.argmax(err.flatten()))
            raise AssertionError('%s %s: normalised error %.3e > %.3e (row %d channel %d of m = %d: got %r ref %r den %r)' % (
                case.label, what[1], e, BOUND, i // cout, i % cout, m, float(got.flatten()[i]), float(ref.flatten()[i]), float(den.flatten()[i])))
        worst = max(worst, e)
        if gather:
            # the fp32 gather kernel (k_spconv) on the same operands
            g = ops.spconv_forward(x, nbr, types.SimpleNamespace(d_m=d_m), w, sc if on else None, sh if on else None, r if on else None, relu=on)
            eg = float(normalised_error(g[:m].double(), *args)[0].max())
            print('  %-34s %-7s e(k_spconv) %.3e, e(k_spconv_gt) %.3e: ratio %.2f' % (case.label, what[1], eg, e, e / max(eg, 1e-300)))
            assert eg > 0 and e <= 2.0 * eg, (case.label, what[1], e, eg)
            worst_g = max(worst_g, eg)
    return results, worst, worst_g


def _run(case, dev, gather=False):
    tile = L.load().dz_spconv_limb3_tile_rows(case.cin, case.cout)
    assert tile > 0, ('layer not covered', case.cin, case.cout)
    rng = np.random.default_rng(zlib.crc32(case.label.encode()))
    lvl_in, lvl_out, cin_, cout_, counter = build_geometry(case, tile, rng, dev)
    k, s, p = KINDS[case.kind]
    tab = _t(osp.neighbor_table(cin_, lvl_in.shape, cout_, k, s, p), dev)
    nbr = lvl_in.neighbors_to(lvl_out, k, s, p)
    rows = edge_rows(case.edge, tile)
    if case.kind == 'subm' and rows is not None:
        assert cout_.shape[0] == rows
    res, worst, _ = convolve(case, lvl_in, lvl_out, nbr, tab, cin_.shape[0], counter, dev, gather=gather)
    if case.edge == 'overflow':
        res2, _, _ = convolve(case, lvl_in, lvl_out, nbr, tab, cin_.shape[0], None, dev)
        assert all(torch.equal(a, b) for a, b in zip(res, res2)), (case.label, 'the overflowed counter changed the result')


@pytest.mark.parametrize('case', EDGE_CASES, ids=[c.label for c in EDGE_CASES])
def test_layer_vs_float64_at_its_edges(case, device):
    _run(case, device)


def test_edge_table_is_complete():
    labels = {c.label for c in EDGE_CASES}
    inst = set()
    for cin, cout, kind in LAYERS:
        for e in OWN_EDGES + (('isolated',) if kind == 'subm' else ()):
            assert 'gt %d->%d %s %s' % (cin, cout, kind, e) in labels
        for e in M_EDGES:
            assert 'gt %d->%d subm %s' % (cin, cout, e) in labels
        name = L.load().dz_spconv_limb3_variant(cin, cout).decode()
        assert name == INSTANCE[(cin, cout)] and L.load().dz_spconv_limb3_tile_rows(cin, cout) == int(name[name.index('<') + 1:].split('x')[0])
        inst.add(name)
    for name in inst:
        hit = [c for c in EDGE_CASES if c.edge.startswith('tiles=') and INSTANCE[(c.cin, c.cout)] == name]
        assert {c.edge for c in hit} == {'tiles=%d' % t for t in XCD_TILES}, name


# ------------------------------------------------------------------------------------------------------------------------
# error class: thousands of rows, against the fp32 gather kernel on the same inputs
# ------------------------------------------------------------------------------------------------------------------------
SUBM_SHAPES = (([6, 36, 50], (0.3, 0.35, 0.25), 2), ([4, 48, 64], (0.01, 0.9, 0.02, 0.5), 1), ([3, 20, 33], (0.08,), 1))


@pytest.mark.parametrize('cin,cout,kind', LAYERS, ids=['%d->%d %s' % l for l in LAYERS])
def test_error_class_vs_gather_kernel(cin, cout, kind, device):
    """e(k_spconv_gt) <= 2^-19 and <= 2 x e(k_spconv) > 0 on the same operands: the three level shapes of
    test_xrun_limb3_vs_float64_gather_and_xf for the submanifold layers, the `unequal` and the default down-geometry for the strided."""
    if kind == 'subm':
        for i, (shape, dens, batch) in enumerate(SUBM_SHAPES):
            rng = np.random.default_rng(500 * cin + i)
            lvl, coords = _level(rng, batch, shape, dens, device)
            tab = _t(osp.neighbor_table(coords, lvl.shape, coords, K3, S1, P1), device)
            case = _case(cin, cout, kind, 'class%d' % i)
            convolve(case, lvl, lvl, lvl.neighbors_to(lvl, K3, S1, P1), tab, coords.shape[0], None, device, gather=True)
    else:
        for edge in ('unequal', 'plain'):
            _run(_case(cin, cout, kind, edge), device, gather=True)


# ------------------------------------------------------------------------------------------------------------------------
# limb terms: one product per output, bit for bit
# ------------------------------------------------------------------------------------------------------------------------
ONE_PRODUCT = ((16, 16, 'subm'), (16, 32, 'down'), (64, 128, 'down'), (128, 128, 'out'))


def _geometry(cin, cout, kind, dev, seed):
    case = _case(cin, cout, kind, 'plain')
    rng = np.random.default_rng(seed)
    lvl_in, lvl_out, cin_, cout_, _ = build_geometry(case, L.load().dz_spconv_limb3_tile_rows(cin, cout), rng, dev)
    k, s, p = KINDS[kind]
    nbr = lvl_in.neighbors_to(lvl_out, k, s, p)
    m = cout_.shape[0]
    tab = _t(osp.neighbor_table(cin_, lvl_in.shape, cout_, k, s, p), dev)
    check_tables(case, nbr, None, tab, m)
    return case, lvl_in, lvl_out, cin_, nbr, tab, m


def _gt(case, x, lvl_out, nbr, w):
    out = torch.full((lvl_out.cap, case.cout), float('nan'), device=x.device)
    launch(case, x, x.shape[0], nbr, lvl_out.cap, lvl_out.d_m, ops.pack_weight_limb3(w, cout_mult=32), None, None, None, 0, out)
    return out


def _one_hot_launches(case, x, lvl_out, nbr, tab, m, dev, what, values, k0=0):
    """One non-zero (tap, cin) weight per output channel; over the launches the entries cover every tap x the first and last channel of
    every 8-channel group."""
    cin, cout, kvol = case.cin, case.cout, case.kvol
    edge = [c for g in range(cin // 8) for c in (8 * g, 8 * g + 7)]
    combos = [(t, c) for t in range(kvol) for c in edge]
    order = torch.randperm(len(combos), generator=torch.Generator().manual_seed(cin * 1000 + cout)).tolist()
    for k in range(-(-len(combos) // cout)):
        pick = [combos[order[(k * cout + o) % len(combos)]] for o in range(cout)]
        tap = torch.tensor([p[0] for p in pick], device=dev)
        ci = torch.tensor([p[1] for p in pick], device=dev)
        val = values[(torch.arange(cout, device=dev) + k + k0) % values.numel()]
        w = torch.zeros((kvol, cin, cout), device=dev)
        w[tap, ci, torch.arange(cout, device=dev)] = val
        exp = _one_hot_expect(x, tab[:, :m], tap, ci, val)
        assert bool((exp != 0).any())
        _same_bits(_gt(case, x, lvl_out, nbr, w)[:m], exp, '%s %d->%d %s, launch %d' % (what, cin, cout, case.kind, k))


@pytest.mark.parametrize('cin,cout,kind', ONE_PRODUCT, ids=['%d->%d %s' % l for l in ONE_PRODUCT])
def test_input_limbs_bit_exact(cin, cout, kind, device):
    case, lvl_in, lvl_out, cin_, nbr, tab, m = _geometry(cin, cout, kind, device, 31 * cin + cout)
    gen = torch.Generator(device=device)
    gen.manual_seed(21 + cin)
    m_in = cin_.shape[0]
    x = torch.zeros((lvl_in.cap, cin), device=device)
    x[:m_in] = _patterned((m_in, cin), gen, device)
    _one_hot_launches(case, x, lvl_out, nbr, tab, m, device, 'input limbs', torch.tensor([1.0, -1.0, 0.5, 2.0, -2.0], device=device))
    # the ends of the range and of the mantissa against weight 1: +-fp32-max (h is clamped to bf16-max, the rest goes to m and l),
    # 1 + 2^-23 and 2 - 2^-23 (every limb carries bits)
    special = torch.tensor([3.4028234663852886e38, -3.4028234663852886e38, 1.0 + 2.0 ** -23, 2.0 - 2.0 ** -23], device=device)
    x[:m_in] = special[torch.randint(0, 4, (m_in, cin), generator=gen, device=device)]
    _one_hot_launches(case, x, lvl_out, nbr, tab, m, device, 'range ends', torch.tensor([1.0], device=device))


@pytest.mark.parametrize('cin,cout,kind', ONE_PRODUCT, ids=['%d->%d %s' % l for l in ONE_PRODUCT])
def test_weight_limbs_bit_exact(cin, cout, kind, device):
    """Patterned 24-bit weights; features non-zero only on the input voxels whose (z, y, x) are all multiples of 3, on one channel each
    (a first or last channel of an 8-channel group): the kernel window of an output holds at most one such voxel."""
    case, lvl_in, lvl_out, cin_, nbr, tab, m = _geometry(cin, cout, kind, device, 37 * cin + cout)
    gen = torch.Generator(device=device)
    gen.manual_seed(22 + cin)
    kvol, m_in = case.kvol, cin_.shape[0]
    w = _patterned((kvol, cin, cout), gen, device)
    c = torch.from_numpy(cin_).to(device)
    lattice = ((c[:, 1] % 3 == 0) & (c[:, 2] % 3 == 0) & (c[:, 3] % 3 == 0))
    rows = torch.nonzero(lattice).squeeze(1)
    edge = torch.tensor([ch for g in range(cin // 8) for ch in (8 * g, 8 * g + 7)], device=device)
    values = torch.tensor([1.0, -1.0, 0.5, 2.0, -2.0], device=device)
    ch = edge[torch.arange(rows.numel(), device=device) % edge.numel()]
    val = values[torch.arange(rows.numel(), device=device) % values.numel()]
    x = torch.zeros((lvl_in.cap, cin), device=device)
    x[rows, ch] = val
    row_ch = torch.zeros(m_in, dtype=torch.long, device=device)
    row_val = torch.zeros(m_in, dtype=torch.float64, device=device)
    row_ch[rows], row_val[rows] = ch, val.double()
    tl = tab[:, :m].long()
    e64 = torch.zeros((m, cout), dtype=torch.float64, device=device)
    hits = torch.zeros(m, dtype=torch.long, device=device)
    for t in range(kvol):
        idx = tl[t]
        live = (idx >= 0) & lattice[idx.clamp_min(0)]
        assert bool(live.any()), 'tap %d is reached by no output row' % t
        src = idx.clamp_min(0)
        e64 += torch.where(live.view(-1, 1), w[t].double()[row_ch[src]] * row_val[src].view(-1, 1), torch.zeros_like(e64))
        hits += live.long()
    assert int(hits.max()) == 1                      # never more than one product per output ...
    one = hits == 1
    n_one = int(one.sum())
    print('  weight limbs %d->%d %s: %d of %d outputs rows receive exactly one product' % (cin, cout, kind, n_one, m))
    # ... and a share of the rows receives exactly one.  The leanest case is conv_out: an output's three inputs share (y, x), which lies on
    # the lattice for 1 output in 9, and an existing output has at least one of the three active: at least 1 row in 27 on average - half
    # of that is asked for
    assert n_one >= max(kvol, m // 54), (n_one, m)
    e32 = e64.float()
    assert torch.equal(e32.double(), e64)
    got = _gt(case, x, lvl_out, nbr, w)[:m]
    assert bool((e32[one] != 0).all())               # (patterned weights and values are never zero)
    _same_bits(got[one], e32[one], 'weight limbs %d->%d %s, rows of one product' % (cin, cout, kind))
    assert not bool(got[~one].view(torch.int32).any()), 'rows without a product must be +0'


@pytest.mark.parametrize('cin,cout,kind', ONE_PRODUCT, ids=['%d->%d %s' % l for l in ONE_PRODUCT])
def test_mm_term_bit_exact(cin, cout, kind, device):
    """x = (1 + 2^-10) 2^e, one-hot w = (1 + 2^-10) 2^e': the product (1 + 2^-9 + 2^-20) 2^(e + e') is exact in fp32 and is 2^-20 off
    without the m.m term."""
    case, lvl_in, lvl_out, cin_, nbr, tab, m = _geometry(cin, cout, kind, device, 41 * cin + cout)
    gen = torch.Generator(device=device)
    gen.manual_seed(23 + cin)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=gen, device=device)          # noqa: E731
    one = torch.tensor(1.0 + 2.0 ** -10, device=device)
    kvol, m_in = case.kvol, cin_.shape[0]
    x = torch.zeros((lvl_in.cap, cin), device=device)
    x[:m_in] = one * _pow2(ri(-40, 16, (m_in, cin)))
    tap, ci = ri(0, kvol - 1, (cout,)), ri(0, cin - 1, (cout,))
    n = min(kvol, cout)
    tap[:n] = torch.arange(n, device=device)
    val = one * _pow2(ri(-40, 16, (cout,)))
    w = torch.zeros((kvol, cin, cout), device=device)
    w[tap, ci, torch.arange(cout, device=device)] = val
    exp = _one_hot_expect(x, tab[:, :m], tap, ci, val)
    assert bool((exp != 0).any())
    _same_bits(_gt(case, x, lvl_out, nbr, w)[:m], exp, 'm.m term %d->%d %s' % (cin, cout, kind))


def test_subnormal_limbs_are_measured(device):
    """One one-hot launch of the 64 -> 128 down-convolution with features of exponent [-120, -104]: their m and / or l limbs are bf16
    subnormals while every product (weights +-1, 0.5, 2) stays a normal fp32.  Asserted: |got - x w| <= 2^-124, which holds whether or
    not the matrix pipe flushes subnormal inputs; printed (and recorded in DESIGN.md 2a-ter): the share of bit-exact outputs."""
    cin, cout, kind = 64, 128, 'down'
    case, lvl_in, lvl_out, cin_, nbr, tab, m = _geometry(cin, cout, kind, device, 43 * cin + cout)
    gen = torch.Generator(device=device)
    gen.manual_seed(25 + cin)
    m_in = cin_.shape[0]
    x = torch.zeros((lvl_in.cap, cin), device=device)
    x[:m_in] = _patterned_tiny((m_in, cin), gen, device)
    ar = torch.arange(cout, device=device)
    tap, ci = ar % case.kvol, (ar * 7 + 3) % cin
    val = torch.tensor([1.0, -1.0, 0.5, 2.0, -2.0], device=device)[ar % 5]
    w = torch.zeros((case.kvol, cin, cout), device=device)
    w[tap, ci, ar] = val
    got = _gt(case, x, lvl_out, nbr, w)[:m]
    xsel = _one_hot_expect(x, tab[:, :m], tap, ci, torch.ones_like(val))
    _subnormal_report('k_spconv_gt %d->%d %s' % (cin, cout, kind), got, xsel, val)


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_refusals(device):
    """Uncovered channels, kvol 0 and 28, a null table, buffers at the 2 GiB limit (described, not allocated: the check precedes the
    launch): non-zero return with a message that names the entry point, the output untouched.  In Python: an unknown arithmetic name, a
    packed table."""
    lib = L.load()
    rng = np.random.default_rng(3)
    lvl, coords = _level(rng, 1, [3, 16, 16], (0.3,), device)
    nbr = lvl.neighbors_to(lvl, K3, S1, P1)
    x = torch.zeros((lvl.cap, 256), device=device)
    w = torch.zeros((27 * 256 * 256 * 3 // 2,), device=device)
    out = torch.full((lvl.cap, 256), SENTINEL, dtype=torch.int32, device=device)

    def call(cin, cout, kvol=27, in_rows=None, cap=None, table=nbr.words, masks=nbr.tile_masks):
        rc = lib.dz_spconv_forward_limb3(L.ptr(x), lvl.cap if in_rows is None else in_rows, cin, L.ptr(table), L.ptr(masks), kvol,
                                         lvl.cap if cap is None else cap, L.ptr(lvl.d_m), L.ptr(w), None, None, None, 0, L.ptr(out), cout, L.stream())
        msg = lib.dz_last_error().decode()
        torch.cuda.synchronize(device)
        print('  %3d -> %3d, kvol %d, in_rows %s, cap %s -> rc %d: %s' % (cin, cout, kvol, in_rows, cap, rc, msg))
        assert rc != 0 and 'dz_spconv_forward_limb3' in msg and bool((out == SENTINEL).all())
        return rc, msg
    for cin, cout in ((48, 48), (256, 256), (32, 16)):
        rc, msg = call(cin, cout)
        assert rc == L.ERR_UNSUPPORTED and 'channels' in msg
    assert 'kvol' in call(64, 64, kvol=0)[1]
    assert 'kvol' in call(64, 64, kvol=28)[1]
    assert 'null' in call(64, 64, table=None)[1]
    assert 'null' in call(64, 64, masks=None)[1]
    rc, msg = call(64, 64, in_rows=2 ** 31 // (64 * 4))                  # an input of exactly 2^31 bytes
    assert rc == L.ERR_UNSUPPORTED and '2 GiB' in msg
    rc, msg = call(64, 64, kvol=1, cap=2 ** 31 // (64 * 4))              # an output of exactly 2^31 bytes (its table is 2^25 bytes)
    assert rc == L.ERR_UNSUPPORTED and '2 GiB' in msg
    x64 = x[:, :64].contiguous()
    w64 = torch.zeros((27, 64, 64), device=device)
    wl = ops.pack_weight_limb3(w64, cout_mult=32)
    with pytest.raises(L.DetZeroHipError, match='nonsense'):
        ops.spconv_forward(x64, nbr, lvl, w64, None, None, None, relu=False, f32_gather='nonsense')
    packed = lvl.neighbors_to(lvl, K3, S1, P1, packed=True)
    with pytest.raises(L.DetZeroHipError, match='packed'):
        ops.spconv_forward(x64, packed, lvl, wl, None, None, None, relu=False, f32_gather='bf16x3')
    with pytest.raises(L.DetZeroHipError, match='bf16x3'):               # a layer the library does not cover
        ops.spconv_forward(x[:, :48].contiguous(), nbr, lvl, ops.pack_weight_limb3(torch.zeros((27, 48, 48), device=device), cout_mult=32),
                           None, None, None, relu=False, f32_gather='bf16x3')
    # the split modes ignore the keyword
    xp, wp = ops.pair16_from_f32(x64, 64, 1), ops.pack_weight_split(w64, 1)
    a = ops.spconv_forward(xp, nbr, lvl, wp, None, None, None, relu=False, math=1, cout=64)
    b = ops.spconv_forward(xp, nbr, lvl, wp, None, None, None, relu=False, math=1, cout=64, f32_gather='bf16x3')
    m = lvl.num_active()
    assert torch.equal(a[:m], b[:m])
    # and through the Python entry the kernel computes what the C entry does
    g = torch.Generator(device=device)
    g.manual_seed(5)
    xr = torch.randn((lvl.cap, 64), generator=g, device=device)
    wr = torch.randn((27, 64, 64), generator=g, device=device)
    got = ops.spconv_forward(xr, nbr, lvl, ops.pack_weight_limb3(wr, cout_mult=32), None, None, None, relu=False, f32_gather='bf16x3')
    ref = ops.spconv_forward(xr, nbr, lvl, wr, None, None, None, relu=False)
    assert float((got[:m] - ref[:m]).abs().max()) <= 1e-4 * float(ref[:m].abs().max())


# ------------------------------------------------------------------------------------------------------------------------
# the detector
# ------------------------------------------------------------------------------------------------------------------------
def _sparse_launches(pipe, prep):
    ops.PROFILER = ops.LaunchProfiler()
    try:
        res = pipe.backbone_stage(prep)
        names = [r[0] for r in ops.PROFILER.records if r[0].startswith('k_spconv')]
    finally:
        ops.PROFILER = None
    return res, names


def test_detector_fp32_on_the_gather_limb3_engine_40k(device):
    """The detector at one 40 000-point frame (0.1 m voxels) in exact fp32 with the engine pairs (gather, mfma32), (gather, bf16x3) and
    (xrun_bf16x3, bf16x3): the launch lists, the backbone stages within the fp32 per-stage tolerances of tests/test_gpu_full_parity.py
    of the (gather, mfma32) run, the boxes within 1e-3 of it; 2 frames through a captured FramePipeline (replay == eager, bit for bit);
    a second weight set through load_state_dict equals a fresh model built with it, bit for bit."""
    from detzero_amd.centerpoint import FramePipeline, set_sparse_engine
    from detzero_amd.synth import VOXEL_SIZE_01
    from tests.test_gpu_full_parity import REL
    from tests.test_gpu_xrun_f32 import _stage_rows
    from tests.util import cpu_state_dict, make_model, masked_frame, match_boxes
    model, cfg, info = make_model(VOXEL_SIZE_01, seed=0)
    pts = masked_frame(0, 40000)
    model = model.to(device)
    bb = model.backbone3d
    before = (bb.engine, bb.f32_engine, bb.f32_gather)
    dpts = torch.from_numpy(pts).to(device)
    try:
        # a model that never set the switch
        set_sparse_engine(model, before[0], f32_engine='gather')
        pipe = FramePipeline(model, info, math='f32')
        _, never = _sparse_launches(pipe, pipe.prepare([dpts]))
        assert len(never) == 21 and all(n.startswith('k_spconv<') for n in never), never
        stages, boxes, launches = {}, {}, {}
        for key in (('gather', 'mfma32'), ('gather', 'bf16x3'), ('xrun_bf16x3', 'bf16x3')):
            set_sparse_engine(model, before[0], f32_engine=key[0], f32_gather=key[1])
            pipe = FramePipeline(model, info, math='f32')
            res, launches[key] = _sparse_launches(pipe, pipe.prepare([dpts]))
            stages[key] = _stage_rows(res)
            out, d_n = pipe(dpts)
            k = int(d_n.item())
            boxes[key] = (out[:k, :7].cpu().numpy(), out[:k, 7].cpu().numpy())
            print('  %s: %s' % (key, ', '.join('%s x%d' % (n, launches[key].count(n)) for n in sorted(set(launches[key])))))
        ref_key = ('gather', 'mfma32')
        assert launches[ref_key] == never
        for key in list(launches)[1:]:
            names = launches[key]
            assert len(names) == 21 and not any(n.startswith('k_spconv<') for n in names), names
            assert all(n.startswith('k_spconv_gt<') or n.startswith('k_spconv_xt<') for n in names), names
            nxt = sum(n.startswith('k_spconv_xt<') for n in names)
            assert nxt == (12 if key[0] == 'xrun_bf16x3' else 0), names
        rb, rs = boxes[ref_key]
        n_ref = rb.shape[0]
        for key in list(boxes)[1:]:
            gb, gs = boxes[key]
            nm, worst = match_boxes(rb, rs, gb, gs, tol=1e-3)
            print('%s [f32]: %d boxes, %d/%d within 1e-3 of (gather, mfma32) (worst %.2e)' % (key, gb.shape[0], nm, n_ref, worst))
            assert n_ref > 0 and abs(gb.shape[0] - n_ref) <= 2 and nm >= n_ref - 2, (key, gb.shape[0], n_ref, nm, worst)
            for name in ('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4', 'encoded'):
                g, x = stages[ref_key][name], stages[key][name]
                assert g.shape == x.shape
                amp, err = float(g.std()), float((g - x).abs().max())
                print('  stage %-8s %s vs (gather, mfma32): max abs %.3e = %.2e of the stage std (tolerance %.1e)' % (name, key, err, err / amp, REL[name][0]))
                assert err <= REL[name][0] * amp, (key, name, err, amp)
        # captured, 2 frames, both bf16x3 engines still on
        frames = [torch.from_numpy(masked_frame(20 + i, 40000)).to(device) for i in range(2)]
        pipe = FramePipeline(model, info, math='f32')
        pipe.calibrate(frames, margin=2.0)
        for _ in range(2):
            o1, n1 = pipe(frames)
        torch.cuda.synchronize(device)
        pipe.check_overflow()
        o1, n1 = o1.clone(), n1.clone()
        cp = pipe.capture(frames)
        cp.replay()
        torch.cuda.synchronize(device)
        assert int(n1.sum().item()) > 0
        assert torch.equal(cp.counts, n1.view(-1)) and torch.equal(cp.boxes, o1.view(cp.boxes.shape))
        del cp
        # a second weight set: the cached limb weights go with the plan
        other, _, _ = make_model(VOXEL_SIZE_01, seed=1)
        sd = cpu_state_dict(other)
        other = other.to(device)
        set_sparse_engine(other, before[0], f32_engine='xrun_bf16x3', f32_gather='bf16x3')
        fresh, fn = FramePipeline(other, info, math='f32')(dpts)
        fresh, fn = fresh.clone(), int(fn.item())
        assert any('w_xlimb3' in e for e in (bb.plan()['conv_input'], bb.plan()['conv_out']))
        model.load_state_dict(sd)
        assert bb._plan is None
        again, an = FramePipeline(model, info, math='f32')(dpts)
        assert int(an.item()) == fn > 0 and torch.equal(again[:fn], fresh[:fn])
        assert not torch.equal(again[:fn, :7], out[:fn, :7]) or fn != k
    finally:
        set_sparse_engine(model, before[0], f32_engine=before[1], f32_gather=before[2])
