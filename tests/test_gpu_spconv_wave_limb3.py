"""GPU (MI355X): the wave-private bf16x3 sparse convolution of the exact-fp32 mode's 16-channel layers (csrc/sparse_conv_wt.hip,
dz_spconv_forward_limb3_w: 16 -> 16 and 16 -> 32 from the plain neighbour table and its tile masks, weights of all taps resident as
limbs, three v_mfma_f32_16x16x32_bf16 per tap) against a float64 evaluation of the same rulebook at its edges, on a capped grid,
against the error of the fp32 gather kernel and of k_spconv_gt, its limb terms bit for bit on one-product outputs, its refusals, and
the detector on it.

Geometry, reference, metric, sentinels, poison and the one-product tables are those of tests/test_gpu_spconv_gather_limb3.py: its
helpers and limb tests run here with this file's launch in place of that module's (the `wave` fixture).  The exact-m edges run on the
submanifold table of the layer's channels (the kernel does not know the layer kind), the other edges on the layer's own kind."""
import zlib

import numpy as np
import pytest
import torch

from detzero_amd import lib as L
from detzero_amd import ops
from oracle import sparse as osp
from tests import test_gpu_spconv_gather_limb3 as gt
from tests.test_gpu_conv3x3_limb3 import _patterned_tiny, _subnormal_report
from tests.test_gpu_sparse_conv import KINDS, SENTINEL, build_geometry
from tests.test_gpu_xrun import K3, P1, S1, _level, _t
from tests.test_gpu_xrun_limb3 import _one_hot_expect

pytestmark = pytest.mark.gpu
T = 32                                              # rows of a wave's tile
# the instances of csrc/sparse_conv_wt.hip, restated: (cin, cout) -> (name, waves per workgroup, slots per chunk G, the layer's own kind)
INSTANCES = {(16, 16): ('k_spconv_wt<16x16>', 4, 4, 'subm'), (16, 32): ('k_spconv_wt<16x32>', 12, 3, 'down')}
XRUN = 4                                            # groups per XCD run of the deal: one round = 8 XCDs x 4 runs x R rows
OWN_EDGES = ('dead tiles', 'm=cap', 'overflow', 'zero', 'unequal')


def _rows(cin, cout):
    name, waves, _, _ = INSTANCES[(cin, cout)]
    lib = L.load()
    assert lib.dz_spconv_limb3_w_variant(cin, cout).decode() == name
    r = lib.dz_spconv_limb3_w_tile_rows(cin, cout)
    assert r == T * waves, (cin, cout, r)
    return r


def launch(case, x, in_rows, nbr, cap, d_m, wl, sc, sh, res, relu, out, expect_rc=0):
    lib = L.load()
    p = L.ptr
    rc = lib.dz_spconv_forward_limb3_w(p(x), in_rows, case.cin, p(nbr.words), p(nbr.tile_masks), case.kvol, cap, p(d_m), p(wl), p(sc), p(sh), p(res),
                                       relu, p(out), case.cout, getattr(case, 'max_workgroups', 0), L.stream())
    msg = lib.dz_last_error()
    assert rc == expect_rc, (case.label, rc, msg.decode() if msg else '')


@pytest.fixture
def wave(monkeypatch):
    """The helpers of the sibling file (convolve, _gt and the limb tests built on them) launch k_spconv_wt."""
    monkeypatch.setattr(gt, 'launch', launch)


def _case(cin, cout, kind, edge, label=None, **kw):
    c = gt._case(cin, cout, kind, edge)
    c.label = 'wt %d->%d %s %s' % (cin, cout, kind, label or edge)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _subm_of_rows(case, m, dev):
    """A submanifold level of exactly m rows (cap m + 7) and its tables: build_geometry's `tiles=2` edge is (2 - 1) * tile + 5 rows."""
    assert case.kind == 'subm' and case.edge == 'tiles=2'
    rng = np.random.default_rng(zlib.crc32(case.label.encode()))
    lvl, _, coords, _, counter = build_geometry(case, m - 5, rng, dev)
    assert counter is None and coords.shape[0] == m == lvl.num_active()
    tab = _t(osp.neighbor_table(coords, lvl.shape, coords, K3, S1, P1), dev)
    return lvl, lvl.neighbors_to(lvl, K3, S1, P1), tab


def _m_edges(cin, cout):
    r = T * INSTANCES[(cin, cout)][1]
    rnd = 8 * XRUN * r
    return (('m=1', 1), ('m=15', 15), ('m=16', 16), ('m=17', 17), ('m=T-1', T - 1), ('m=T', T), ('m=T+1', T + 1), ('m=R-1', r - 1), ('m=R', r),
            ('m=R+1', r + 1), ('round-tile', rnd - T), ('round', rnd), ('round+tile', rnd + T))


M_CASES = [(ci, co, lab, m) for ci, co in INSTANCES for lab, m in _m_edges(ci, co)]


@pytest.mark.parametrize('cin,cout,label,m', M_CASES, ids=['%d->%d %s' % c[:3] for c in M_CASES])
def test_exact_row_counts_vs_float64(cin, cout, label, m, device, wave):
    """Everything on and everything off, two launches each into sentinel buffers (equal bit for bit), e <= 2^-19, rows at or beyond m and
    behind cap untouched - at the 16-row half, the wave tile, the workgroup's group and one round of the XCD deal."""
    assert _rows(cin, cout) > 0
    case = _case(cin, cout, 'subm', 'tiles=2', label)
    lvl, nbr, tab = _subm_of_rows(case, m, device)
    gt.convolve(case, lvl, lvl, nbr, tab, m, None, device)


OWN_CASES = [(ci, co, kind, e) for (ci, co), (_, _, _, kind) in INSTANCES.items() for e in OWN_EDGES + (('isolated',) if kind == 'subm' else ('plain',))]


@pytest.mark.parametrize('cin,cout,kind,edge', OWN_CASES, ids=['%d->%d %s %s' % c for c in OWN_CASES])
def test_own_kind_edges_vs_float64(cin, cout, kind, edge, device, wave):
    """Dead tiles, m = cap, a counter above cap (equals the m = cap run) and of 0 (nothing written), slabs of unequal density, isolated
    voxels / the default down-geometry: 16 -> 16 submanifold, 16 -> 32 with stride 2 and padding (1, 1, 1)."""
    case = _case(cin, cout, kind, edge)
    rng = np.random.default_rng(zlib.crc32(case.label.encode()))
    lvl_in, lvl_out, cin_, cout_, counter = build_geometry(case, _rows(cin, cout), rng, device)
    k, s, p = KINDS[kind]
    tab = _t(osp.neighbor_table(cin_, lvl_in.shape, cout_, k, s, p), device)
    nbr = lvl_in.neighbors_to(lvl_out, k, s, p)
    res, _, _ = gt.convolve(case, lvl_in, lvl_out, nbr, tab, cin_.shape[0], counter, device)
    if edge == 'overflow':
        res2, _, _ = gt.convolve(case, lvl_in, lvl_out, nbr, tab, cin_.shape[0], None, device)
        assert all(torch.equal(a, b) for a, b in zip(res, res2)), (case.label, 'the overflowed counter changed the result')
    if edge == 'zero':
        assert all(r.numel() == 0 for r in res)


@pytest.mark.parametrize('cin,cout', list(INSTANCES), ids=['%d->%d' % k for k in INSTANCES])
def test_live_tap_counts_around_the_chunk_vs_float64(cin, cout, device, wave):
    """A level of isolated slabs of 0.3 .. 2 % fill and three slabs half full: wave tiles whose tap list has G - 1, G, G + 1 and 27
    entries (G = slots per chunk: a list that ends one short of, at, and one past a chunk's end), each asserted to occur."""
    g = INSTANCES[(cin, cout)][2]
    case = _case(cin, cout, 'subm', 'taps')
    lvl, coords = _level(np.random.default_rng(7), 1, [16, 64, 96], (0.003, 0, 0.005, 0, 0.008, 0, 0.012, 0, 0.02, 0, 0.5, 0.5, 0.5, 0, 0.004, 0), device)
    m = coords.shape[0]
    nbr = lvl.neighbors_to(lvl, K3, S1, P1)
    tab = _t(osp.neighbor_table(coords, lvl.shape, coords, K3, S1, P1), device)
    masks = nbr.tile_masks[:-(-m // T)].cpu().numpy().astype(np.uint32)
    counts = {int(c) for c in np.unique([bin(int(w)).count('1') for w in masks])}
    print('  live taps per wave tile (%d rows): %s' % (m, sorted(counts)))
    assert {g - 1, g, g + 1, 27} <= counts, (g, sorted(counts))
    gt.convolve(case, lvl, lvl, nbr, tab, m, None, device)


@pytest.mark.parametrize('cin,cout', list(INSTANCES), ids=['%d->%d' % k for k in INSTANCES])
def test_capped_grid_second_mask_batch(cin, cout, device, wave):
    """max_workgroups = 8 on a level of 8 x waves x 64 wave tiles plus one more group: every wave runs 64 tiles, those of the workgroup
    that takes the last group a 65th - the second load of tile masks.  Bit-equal to the default grid, both within the float64 bound."""
    r = _rows(cin, cout)
    m = 8 * 64 * r + r - 3
    case = _case(cin, cout, 'subm', 'tiles=2', 'capped grid', max_workgroups=8)
    lvl, nbr, tab = _subm_of_rows(case, m, device)
    assert -(-m // r) == 8 * 64 + 1
    capped, _, _ = gt.convolve(case, lvl, lvl, nbr, tab, m, None, device)
    case.max_workgroups = 0
    full, _, _ = gt.convolve(case, lvl, lvl, nbr, tab, m, None, device)
    assert all(torch.equal(a, b) for a, b in zip(capped, full)), (case.label, 'the grid changed the result')
    if cout == 16:                                 # (the smaller level: one more grid)
        case.max_workgroups = 13                   # rounded up to 16: two workgroups per XCD, several deal rounds
        odd, _, _ = gt.convolve(case, lvl, lvl, nbr, tab, m, None, device)
        assert all(torch.equal(a, b) for a, b in zip(odd, full)), (case.label, 'the grid changed the result')


@pytest.mark.parametrize('cin,cout', list(INSTANCES), ids=['%d->%d' % k for k in INSTANCES])
def test_error_class_vs_gather_kernels(cin, cout, device, monkeypatch):
    """e(k_spconv_wt) <= 2^-19 and <= 2 x e(k_spconv) > 0 on the same operands (the project's bounds; asserted inside convolve): the
    three level shapes of the sibling file for 16 -> 16, the `unequal` and the default down-geometry for 16 -> 32.  Printed: the ratio
    to k_spconv and to k_spconv_gt."""
    kind = INSTANCES[(cin, cout)][3]
    runs = []
    if kind == 'subm':
        for i, (shape, dens, batch) in enumerate(gt.SUBM_SHAPES):
            lvl, coords = _level(np.random.default_rng(500 * cin + i), batch, shape, dens, device)
            tab = _t(osp.neighbor_table(coords, lvl.shape, coords, K3, S1, P1), device)
            runs.append((_case(cin, cout, kind, 'class%d' % i), lvl, lvl, lvl.neighbors_to(lvl, K3, S1, P1), tab, coords.shape[0], None))
    else:
        for edge in ('unequal', 'plain'):
            case = _case(cin, cout, kind, edge, 'class ' + edge)
            rng = np.random.default_rng(zlib.crc32(case.label.encode()))
            lvl_in, lvl_out, cin_, cout_, counter = build_geometry(case, _rows(cin, cout), rng, device)
            k, s, p = KINDS[kind]
            tab = _t(osp.neighbor_table(cin_, lvl_in.shape, cout_, k, s, p), device)
            runs.append((case, lvl_in, lvl_out, lvl_in.neighbors_to(lvl_out, k, s, p), tab, cin_.shape[0], counter))
    for run in runs:
        _, e_gt, _ = gt.convolve(*run, device, gather=False)                # the module's own launch: k_spconv_gt
        with monkeypatch.context() as mp:
            mp.setattr(gt, 'launch', launch)
            _, e_wt, e_g = gt.convolve(*run, device, gather=True)
        print('  %-30s e(k_spconv_wt) %.3e = %.2f x e(k_spconv) = %.2f x e(k_spconv_gt)' % (run[0].label, e_wt, e_wt / e_g, e_wt / max(e_gt, 1e-300)))
        assert 0 < e_wt <= gt.BOUND and e_wt <= 2.0 * e_g


# ------------------------------------------------------------------------------------------------------------------------
# limb terms: one product per output, bit for bit (the sibling's tables and checks, this file's launch)
# ------------------------------------------------------------------------------------------------------------------------
ONE_PRODUCT = ((16, 16, 'subm'), (16, 32, 'down'))


@pytest.mark.parametrize('cin,cout,kind', ONE_PRODUCT, ids=['%d->%d %s' % l for l in ONE_PRODUCT])
def test_input_limbs_bit_exact(cin, cout, kind, device, wave):
    """Every tap x channels 0, 7, 8, 15 - one of each of the four channel quads a row's four lanes hold."""
    gt.test_input_limbs_bit_exact(cin, cout, kind, device)


@pytest.mark.parametrize('cin,cout,kind', ONE_PRODUCT, ids=['%d->%d %s' % l for l in ONE_PRODUCT])
def test_weight_limbs_bit_exact(cin, cout, kind, device, wave):
    gt.test_weight_limbs_bit_exact(cin, cout, kind, device)


@pytest.mark.parametrize('cin,cout,kind', ONE_PRODUCT, ids=['%d->%d %s' % l for l in ONE_PRODUCT])
def test_mm_term_bit_exact(cin, cout, kind, device, wave):
    gt.test_mm_term_bit_exact(cin, cout, kind, device)


def test_subnormal_limbs_are_measured(device, wave):
    """One one-hot launch of the 16 -> 32 down-convolution with features of exponent [-120, -104] (bf16-subnormal m and / or l limbs,
    normal fp32 products).  Asserted: |got - x w| <= 2^-124; printed: the share of bit-exact outputs."""
    cin, cout, kind = 16, 32, 'down'
    case, lvl_in, lvl_out, cin_, nbr, tab, m = gt._geometry(cin, cout, kind, device, 43 * cin + cout)
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
    got = gt._gt(case, x, lvl_out, nbr, w)[:m]
    xsel = _one_hot_expect(x, tab[:, :m], tap, ci, torch.ones_like(val))
    _subnormal_report('k_spconv_wt %d->%d %s' % (cin, cout, kind), got, xsel, val)


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_refusals(device):
    """Uncovered channels, kvol 0 and 28, a null table or masks, a negative workgroup cap, buffers at the 2 GiB limit (described, not
    allocated: the check precedes the launch): non-zero return with a message that names the entry point, the output untouched.  In
    Python: an unknown name, a packed table, an uncovered layer; the split modes ignore the keyword."""
    lib = L.load()
    rng = np.random.default_rng(3)
    lvl, coords = _level(rng, 1, [3, 16, 16], (0.3,), device)
    nbr = lvl.neighbors_to(lvl, K3, S1, P1)
    x = torch.zeros((lvl.cap, 64), device=device)
    w = torch.zeros((27 * 64 * 64 * 3 // 2,), device=device)
    out = torch.full((lvl.cap, 64), SENTINEL, dtype=torch.int32, device=device)

    def call(cin, cout, kvol=27, in_rows=None, cap=None, table=nbr.words, masks=nbr.tile_masks, wgs=0):
        rc = lib.dz_spconv_forward_limb3_w(L.ptr(x), lvl.cap if in_rows is None else in_rows, cin, L.ptr(table), L.ptr(masks), kvol,
                                           lvl.cap if cap is None else cap, L.ptr(lvl.d_m), L.ptr(w), None, None, None, 0, L.ptr(out), cout, wgs,
                                           L.stream())
        msg = lib.dz_last_error().decode()
        torch.cuda.synchronize(device)
        print('  %3d -> %3d, kvol %d, in_rows %s, cap %s, workgroups %d -> rc %d: %s' % (cin, cout, kvol, in_rows, cap, wgs, rc, msg))
        assert rc != 0 and 'dz_spconv_forward_limb3_w' in msg and bool((out == SENTINEL).all())
        return rc, msg
    for cin, cout in ((32, 32), (16, 64), (48, 48), (32, 16), (64, 64)):
        rc, msg = call(cin, cout)
        assert rc == L.ERR_UNSUPPORTED and 'channels' in msg
    assert 'kvol' in call(16, 16, kvol=0)[1]
    assert 'kvol' in call(16, 32, kvol=28)[1]
    assert 'null' in call(16, 16, table=None)[1]
    assert 'null' in call(16, 32, masks=None)[1]
    assert 'workgroup' in call(16, 16, wgs=-8)[1]
    rc, msg = call(16, 16, in_rows=2 ** 31 // (16 * 4))                  # an input of exactly 2^31 bytes
    assert rc == L.ERR_UNSUPPORTED and '2 GiB' in msg
    rc, msg = call(16, 32, kvol=1, cap=2 ** 31 // (32 * 4))              # an output of exactly 2^31 bytes (its table is 2^26 bytes)
    assert rc == L.ERR_UNSUPPORTED and '2 GiB' in msg
    rc, msg = call(16, 16, kvol=27, cap=2 ** 31 // (27 * 4) + 1)         # a table just over 2^31 bytes (its output is smaller)
    assert rc == L.ERR_UNSUPPORTED and '2 GiB' in msg
    x16 = x[:, :16].contiguous()
    w16 = torch.zeros((27, 16, 16), device=device)
    wl = ops.pack_weight_limb3(w16, cout_mult=32)
    with pytest.raises(L.DetZeroHipError, match='nonsense'):
        ops.spconv_forward(x16, nbr, lvl, w16, None, None, None, relu=False, f32_small='nonsense')
    packed = lvl.neighbors_to(lvl, K3, S1, P1, packed=True)
    with pytest.raises(L.DetZeroHipError, match='packed'):
        ops.spconv_forward(x16, packed, lvl, wl, None, None, None, relu=False, cout=16, f32_small='wave_bf16x3')
    with pytest.raises(L.DetZeroHipError, match='wave_bf16x3'):          # a layer the kernel does not cover
        ops.spconv_forward(x[:, :32].contiguous(), nbr, lvl, ops.pack_weight_limb3(torch.zeros((27, 32, 32), device=device), cout_mult=32),
                           None, None, None, relu=False, f32_small='wave_bf16x3')
    # the split modes ignore the keyword
    xp, wp = ops.pair16_from_f32(x16, 16, 1), ops.pack_weight_split(w16, 1)
    a = ops.spconv_forward(xp, nbr, lvl, wp, None, None, None, relu=False, math=1, cout=16)
    b = ops.spconv_forward(xp, nbr, lvl, wp, None, None, None, relu=False, math=1, cout=16, f32_small='wave_bf16x3')
    m = lvl.num_active()
    assert torch.equal(a[:m], b[:m])
    # and through the Python entry the kernel computes what the C entry does, with and without a grid cap
    g = torch.Generator(device=device)
    g.manual_seed(5)
    xr = torch.randn((lvl.cap, 16), generator=g, device=device)
    for cout in (16, 32):
        wr = torch.randn((27, 16, cout), generator=g, device=device)
        wrl = ops.pack_weight_limb3(wr, cout_mult=32)
        got = ops.spconv_forward(xr, nbr, lvl, wrl, None, None, None, relu=False, cout=cout, f32_small='wave_bf16x3')
        ref = ops.spconv_forward(xr, nbr, lvl, wr, None, None, None, relu=False)
        assert got.shape == ref.shape and float((got[:m] - ref[:m]).abs().max()) <= 1e-4 * float(ref[:m].abs().max())
        cap8 = ops.spconv_forward(xr, nbr, lvl, wrl, None, None, None, relu=False, cout=cout, f32_small='wave_bf16x3', max_workgroups=8)
        assert torch.equal(cap8[:m], got[:m])
        # it goes before the gather arithmetic
        both = ops.spconv_forward(xr, nbr, lvl, wrl, None, None, None, relu=False, cout=cout, f32_gather='bf16x3', f32_small='wave_bf16x3')
        assert torch.equal(both[:m], got[:m])


# ------------------------------------------------------------------------------------------------------------------------
# the detector
# ------------------------------------------------------------------------------------------------------------------------
def _count(names, prefix):
    return sum(n.startswith(prefix) for n in names)


def test_detector_fp32_on_the_wave_limb3_engine_40k(device):
    """The detector at one 40 000-point frame (0.1 m voxels) in exact fp32.  With f32_small never set the launch lists of the three
    engine pairs of the sibling test are those it states; with 'wave_bf16x3' the six 16-input-channel convolutions move to k_spconv_wt
    under either gather arithmetic.  Backbone stages within the fp32 per-stage tolerances of tests/test_gpu_full_parity.py of the
    (gather, mfma32) run, boxes within 1e-3 of it; 2 frames through a captured FramePipeline (replay == eager, bit for bit); a second
    weight set through load_state_dict equals a fresh model built with it, bit for bit."""
    from detzero_amd.centerpoint import FramePipeline, set_sparse_engine
    from detzero_amd.synth import VOXEL_SIZE_01
    from tests.test_gpu_full_parity import REL
    from tests.test_gpu_xrun_f32 import _stage_rows
    from tests.util import cpu_state_dict, make_model, masked_frame, match_boxes
    model, cfg, info = make_model(VOXEL_SIZE_01, seed=0)
    pts = masked_frame(0, 40000)
    model = model.to(device)
    bb = model.backbone3d
    before = (bb.engine, bb.f32_engine, bb.f32_gather, bb.f32_small)
    assert before[3] == 'gather'
    dpts = torch.from_numpy(pts).to(device)
    pairs = (('gather', 'mfma32'), ('gather', 'bf16x3'), ('xrun_bf16x3', 'bf16x3'))
    # (k_spconv<, k_spconv_gt<, k_spconv_xt<, k_spconv_wt<) launches of a pass
    today = {pairs[0]: (21, 0, 0, 0), pairs[1]: (0, 21, 0, 0), pairs[2]: (0, 9, 12, 0)}
    wave = {pairs[0]: (15, 0, 0, 6), pairs[2]: (0, 3, 12, 6)}
    census = lambda names: tuple(_count(names, p) for p in ('k_spconv<', 'k_spconv_gt<', 'k_spconv_xt<', 'k_spconv_wt<'))      # noqa: E731
    try:
        stages, boxes, launches = {}, {}, {}
        for key in pairs:
            # a model that never set the switch, then the switch at its default by name
            set_sparse_engine(model, before[0], f32_engine=key[0], f32_gather=key[1])
            pipe = FramePipeline(model, info, math='f32')
            res, names = gt._sparse_launches(pipe, pipe.prepare([dpts]))
            assert len(names) == 21 and census(names) == today[key], (key, names)
            set_sparse_engine(model, before[0], f32_small='gather')
            pipe = FramePipeline(model, info, math='f32')
            assert gt._sparse_launches(pipe, pipe.prepare([dpts]))[1] == names, key
            if key == pairs[0]:
                stages[key] = _stage_rows(res)
                out, d_n = pipe(dpts)
                k = int(d_n.item())
                boxes[key] = (out[:k, :7].cpu().numpy(), out[:k, 7].cpu().numpy())
        for pair in wave:
            key = pair + ('wave_bf16x3',)
            set_sparse_engine(model, before[0], f32_engine=key[0], f32_gather=key[1], f32_small=key[2])
            pipe = FramePipeline(model, info, math='f32')
            res, launches[key] = gt._sparse_launches(pipe, pipe.prepare([dpts]))
            names = launches[key]
            print('  %s: %s' % (key, ', '.join('%s x%d' % (n, names.count(n)) for n in sorted(set(names)))))
            assert len(names) == 21 and census(names) == wave[pair], (key, names)
            assert {n for n in names if n.startswith('k_spconv_wt<')} == {'k_spconv_wt<16x16>', 'k_spconv_wt<16x32>'}
            stages[key] = _stage_rows(res)
            out, d_n = pipe(dpts)
            k = int(d_n.item())
            boxes[key] = (out[:k, :7].cpu().numpy(), out[:k, 7].cpu().numpy())
        ref_key = pairs[0]
        rb, rs = boxes[ref_key]
        n_ref = rb.shape[0]
        assert len(boxes) == len(stages) == 3
        for key in launches:
            gb, gs = boxes[key]
            nm, worst = match_boxes(rb, rs, gb, gs, tol=1e-3)
            print('%s [f32]: %d boxes, %d/%d within 1e-3 of (gather, mfma32) (worst %.2e)' % (key, gb.shape[0], nm, n_ref, worst))
            assert n_ref > 0 and abs(gb.shape[0] - n_ref) <= 2 and nm >= n_ref - 2, (key, gb.shape[0], n_ref, nm, worst)
            for name in ('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4', 'encoded'):
                g, x = stages[ref_key][name], stages[key][name]
                assert g.shape == x.shape
                amp, err = float(g.std()), float((g - x).abs().max())
                print('  stage %-8s %s vs (gather, mfma32): max abs %.3e = %.2e of the stage std (tolerance %.1e)'
                      % (name, key, err, err / amp, REL[name][0]))
                assert err <= REL[name][0] * amp, (key, name, err, amp)
            # another arithmetic in six layers: the stage behind them differs from the fp32 MFMA's in its last bits, not at all
            assert not torch.equal(stages[ref_key]['x_conv1'], stages[key]['x_conv1']), key
        # captured, 2 frames, every bf16x3 sparse engine on
        assert (bb.f32_engine, bb.f32_gather, bb.f32_small) == ('xrun_bf16x3', 'bf16x3', 'wave_bf16x3')
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
        set_sparse_engine(other, before[0], f32_engine='xrun_bf16x3', f32_gather='bf16x3', f32_small='wave_bf16x3')
        fresh, fn = FramePipeline(other, info, math='f32')(dpts)
        fresh, fn = fresh.clone(), int(fn.item())
        assert 'w_xlimb3' in bb.plan()['conv_input'] and 'w_xlimb3' in bb.plan()['conv2']['down']
        model.load_state_dict(sd)
        assert bb._plan is None
        again, an = FramePipeline(model, info, math='f32')(dpts)
        assert int(an.item()) == fn > 0 and torch.equal(again[:fn], fresh[:fn])
        assert not torch.equal(again[:fn, :7], out[:fn, :7]) or fn != k
    finally:
        set_sparse_engine(model, before[0], f32_engine=before[1], f32_gather=before[2], f32_small=before[3])
    assert (bb.engine, bb.f32_engine, bb.f32_gather, bb.f32_small) == before
