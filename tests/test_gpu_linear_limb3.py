"""GPU: the three-limb (bf16x3) engine of the f32 mode's linear layers (csrc/linear_t.hip, dz_linear_limb3_forward) - every instance
at its edges against float64 next to dz_linear_forward on the same operands, row-chunked launches bit for bit, the error class on the
refiner's layer shapes, the limb terms and the addend bit exact, refusals that write nothing, and GRM / PRM / the PDV head with the
switch on against the goldens of the reference's classes.

Bounds: BOUND['f32'] (the fp32 engine's own, normalised by what was summed into an element) for both engines; the rule of the sibling
engines for the error class (k_linear_t <= BOUND['f32'] and <= 2 x dz_linear_forward's worst error on the same operands).  The limb
tests have ONE non-zero product per output element and compare bits."""
import numpy as np
import pytest
import torch

from detzero_amd import lib as L
from detzero_amd import ops
from oracle import refine as R
from tests.test_gpu_conv3x3_limb3 import _patterned, _pow2
from tests.test_gpu_refine_kernels import BOUND, LINEAR_CASES, Out, assert_within, dev, embed, linear_inputs, worst_ratio

BP = 128
INST = {'A': 'k_linear_t<128x128x16>', 'B': 'k_linear_t<128x64x32>', 'C': 'k_linear_t<128x32x32>'}
BC = {'A': 128, 'B': 64, 'C': 32}

#        rows cin x_extra cout cout_pad y_extra group_rows relu null scale/shift
EXTRA = [(1, 32, 0, 128, 128, 0, 0, True, False),               # A: cout_pad % 128 == 0
         (127, 96, 4, 250, 256, 5, 37, False, False),
         (128, 512, 0, 128, 128, 4, 0, False, True),
         (129, 32, 8, 300, 384, 0, 50, True, True),
         (400, 96, 0, 384, 384, 0, 129, True, False),
         (1, 32, 0, 64, 64, 0, 0, True, False),                 # B: other widths above 32
         (127, 96, 4, 90, 96, 3, 37, False, False),
         (128, 512, 0, 48, 48, 0, 0, False, True),
         (129, 32, 8, 180, 192, 0, 50, True, True),
         (400, 96, 0, 160, 160, 4, 129, True, False),
         (127, 96, 4, 30, 32, 3, 37, False, False),             # C: cout_pad 16 / 32 (rows 1 is LINEAR_CASES' first)
         (128, 512, 0, 32, 32, 0, 0, False, True),
         (129, 32, 8, 9, 16, 0, 50, True, True),
         (400, 96, 0, 20, 32, 4, 129, True, False)]
EDGE_CASES = [c + (False,) for c in LINEAR_CASES] + EXTRA


def _cid(c):
    return '-'.join(str(int(v)) for v in c)


def _inst(cout_pad):
    return 'A' if cout_pad % 128 == 0 else 'B' if cout_pad > 32 else 'C'


def _edges(case):
    """The edges a case reaches, from its parameters alone."""
    rows, cin, x_extra, cout, cp, y_extra, gr, relu, null_ss = case
    e = {'rows %d' % rows} if rows in (1, BP - 1, BP, BP + 1) else set()
    if rows > 2 * BP:
        e.add('several row tiles')
    if cin in (32, 96, 512):
        e.add('cin %d' % cin)
    e.add('ntiles %d' % -(-((cp + 31) // 32 * 32) // BC[_inst(cp)]))
    if cout < cp:
        e.add('cout < cout_pad')
    if x_extra:
        e.add('x_extra')
    if y_extra:
        e.add('y_extra')
    e.add('float4 stores' if (cout + y_extra) % 4 == 0 else 'word stores')
    if gr and gr % BP and rows > gr and rows % gr:
        e.add('group boundary inside a tile, ragged last group')
    if not gr:
        e.add('no addend')
    if null_ss:
        e.add('null scale / shift')
    e.add('relu' if relu else 'no relu')
    return e


COMMON = {'rows 1', 'rows 127', 'rows 128', 'rows 129', 'several row tiles', 'cin 32', 'cin 96', 'cin 512', 'ntiles 1', 'cout < cout_pad',
          'x_extra', 'y_extra', 'float4 stores', 'word stores', 'group boundary inside a tile, ragged last group', 'no addend',
          'null scale / shift', 'relu', 'no relu'}
# (the 32-wide tile has one channel tile by construction: cout_pad 16 / 32)
REQUIRED = {'A': COMMON | {'ntiles 2', 'ntiles 3'}, 'B': COMMON | {'ntiles 2', 'ntiles 3'}, 'C': COMMON}


def test_edge_table_is_complete():
    lib = L.load()
    reached = {k: set() for k in INST}
    for c in EDGE_CASES:
        rows, cin, x_extra, cout, cp, y_extra, gr, relu, null_ss = c
        assert lib.dz_linear_limb3_supported(cin, cin + x_extra, cout, cp, cout + y_extra) == 1, c
        k = _inst(cp)
        assert lib.dz_linear_limb3_variant(cin, cp).decode() == INST[k], c
        reached[k] |= _edges(c)
    for k in INST:
        assert REQUIRED[k] <= reached[k], (k, sorted(REQUIRED[k] - reached[k]))
    assert {c[1] for c in LINEAR_CASES} <= {32, 64, 96}


def _limb_w(w, device):
    return ops.pack_weight_limb3_generic(dev(w, device)[None])


def _fwd(engine, dx, rows, cin, xs, dw, dwl, cout, cp, ds, db, dgs, gr, relu, out, ys, mlr=0):
    lib = L.load()
    if engine == 'bf16x3':
        L.check(lib.dz_linear_limb3_forward(L.ptr(dx), rows, cin, xs, L.ptr(dwl), cout, cp, L.ptr(ds), L.ptr(db), L.ptr(dgs), gr, 1 if relu else 0,
                                            out.ptr, ys, mlr, L.stream()), 'dz_linear_limb3_forward')
    else:
        L.check(lib.dz_linear_forward(L.ptr(dx), rows, cin, xs, L.ptr(dw), cout, cp, L.ptr(ds), L.ptr(db), L.ptr(dgs), gr, 1 if relu else 0,
                                      out.ptr, ys, L.stream()), 'dz_linear_forward')


def _run_case(device, case, engine, mlr=0, seed=None, twice=True):
    rows, cin, x_extra, cout, cp, y_extra, gr, relu, null_ss = case
    x, w, s, b, gs = linear_inputs(rows + cin if seed is None else seed, rows, cin, cp, gr)
    if null_ss:
        s = b = None
    dx, dw, ds, db, dgs = dev(embed(x, x_extra, np.nan), device), dev(w, device), dev(s, device), dev(b, device), dev(gs, device)
    dwl = _limb_w(w, device)
    out = Out(rows, cout + y_extra, device)
    launch = lambda: _fwd(engine, dx, rows, cin, cin + x_extra, dw, dwl, cout, cp, ds, db, dgs, gr, relu, out, cout + y_extra, mlr)   # noqa: E731
    if twice:
        out.run_twice(launch)
    else:
        launch()
    out.check(cout)
    sl = lambda v: None if v is None else v[..., :cout]            # noqa: E731
    want, den = R.linear(x, w[:, :cout], sl(s), sl(b), relu, sl(gs), max(gr, 1), with_den=True)
    return out, want, den


@pytest.mark.gpu
@pytest.mark.parametrize('case', EDGE_CASES, ids=[_cid(c) for c in EDGE_CASES])
def test_edges_against_float64(device, case):
    """Both engines on the same operands within BOUND['f32'] of float64: cout < cout_pad, NaN in the unused input columns, sentinel
    columns beside the result and rows behind it, group boundaries inside a tile, NULL scale / shift; two launches, the same bits."""
    for engine in ('bf16x3', 'mfma32'):
        out, want, den = _run_case(device, case, engine)
        assert_within(out.f32(case[3]).cpu().numpy(), want, BOUND['f32'] * den, '%s %s' % (engine, _cid(case)), BOUND['f32'])


@pytest.mark.gpu
@pytest.mark.parametrize('case,mlr', [((300, 64, 16, 250, 256, 6, 37, True, False), 100), ((300, 64, 16, 250, 256, 6, 0, True, False), 128),
                                      ((300, 96, 0, 30, 32, 3, 37, False, True), 100), ((300, 32, 4, 90, 96, 0, 0, True, False), 128)],
                         ids=['addend-100', 'plain-128', 'addend-100-C', 'plain-128-B'])
def test_chunked_launches_equal_one_launch(device, case, mlr):
    """max_launch_rows: 300 rows in groups of 37 capped at 100 run as three launches of 74 rows and one of 78 (the cap rounded down to
    whole groups, the addend advanced with them); without addend 128 + 128 + 44.  Bit-identical to the single launch."""
    one, want, den = _run_case(device, case, 'bf16x3')
    many, _, _ = _run_case(device, case, 'bf16x3', mlr=mlr)
    assert torch.equal(one.raw, many.raw)
    assert_within(many.f32(case[3]).cpu().numpy(), want, BOUND['f32'] * den, 'chunked %s' % _cid(case), BOUND['f32'])


CLASSES = {'32 -> 128': (32, 128, 0), '128 -> 128': (128, 128, 0), '128 -> 512 + addend': (128, 512, 128), '512 -> 256': (512, 256, 0),
           '256 -> 256': (256, 256, 0)}


@pytest.mark.gpu
@pytest.mark.parametrize('kind', list(CLASSES))
def test_error_class_vs_dz_linear_forward(device, kind):
    """The layer classes of tools/bench_linear.py at about 2 200 rows: the sibling engines' rule."""
    cin, cout, gr = CLASSES[kind]
    case = (2203, cin, 0, cout, cout, 0, gr, True, False)
    errs = {}
    for engine in ('bf16x3', 'mfma32'):
        out, want, den = _run_case(device, case, engine, seed=17, twice=False)
        errs[engine] = worst_ratio(out.f32(cout).cpu().numpy(), want, den)           # worst normalised error
    et, ec = errs['bf16x3'], errs['mfma32']
    print('  %-22s %-24s k_linear_t %.3e (%.2f x 2^-24)   dz_linear_forward %.3e (%.2f x 2^-24)   ratio %.2f' % (
        kind, L.load().dz_linear_limb3_variant(cin, cout).decode(), et, et * 2 ** 24, ec, ec * 2 ** 24, et / max(ec, 1e-30)))
    assert ec > 0
    assert et <= BOUND['f32'], (kind, et)
    assert et <= 2.0 * ec, (kind, et, ec)


# ------------------------------------------------------------------------------------------------------------------------
# limb terms: one product per output, bit exact.  One case per instance: (cin, cout_pad); 130 rows = two row tiles
# ------------------------------------------------------------------------------------------------------------------------
LIMB_CASES = {'A': (64, 128), 'B': (64, 64), 'C': (32, 16)}
LIMB_ROWS = 130
ONE_HOT_VALUES = (1.0, -1.0, 0.5, 2.0, -2.0)


def _group_edges(cin):
    """The first and last channel of every 8-channel group."""
    return [c for g in range(cin // 8) for c in (8 * g, 8 * g + 7)]


def _limb_launch(device, x, w, gs=None, gr=0, scale=None):
    rows, cin = x.shape
    cp = w.shape[1]
    out = Out(rows, cp, device)
    wl = ops.pack_weight_limb3_generic(w[None].contiguous())
    out.run_twice(lambda: _fwd('bf16x3', x, rows, cin, cin, None, wl, cp, cp, scale, None, gs, gr, False, out, cp))
    out.check()
    return out.f32()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, exp, what):
    bad = _bits(got) != _bits(exp)
    assert not bool(bad.any()), (what, int(bad.sum()), got[bad][:4].tolist(), exp[bad][:4].tolist())


def _one_hot_w(cin, cp, combos, k, device):
    """(cin, cp) weights with one non-zero entry per output column: column c of launch k takes combo (k * cp + c) % len(combos)."""
    w = torch.zeros((cin, cp), device=device)
    pick = [combos[(k * cp + c) % len(combos)] for c in range(cp)]
    ch = torch.tensor([p[0] for p in pick], device=device)
    val = torch.tensor([p[1] for p in pick], dtype=torch.float32, device=device)
    w[ch, torch.arange(cp, device=device)] = val
    return w, ch, val


@pytest.mark.gpu
@pytest.mark.parametrize('inst', list(LIMB_CASES))
def test_input_limbs_bit_exact(device, inst):
    """One-hot weights (+-1, 0.5, +-2) against patterned 24-bit inputs: every output is one input value times a power of two, which
    only comes out bit for bit if h, m and l of the input all arrive (terms h.h, h.m, h.l).  Every (group edge channel, value) pair."""
    cin, cp = LIMB_CASES[inst]
    assert L.load().dz_linear_limb3_variant(cin, cp).decode() == INST[inst]
    gen = torch.Generator(device=device).manual_seed(3)
    x = _patterned((LIMB_ROWS, cin), gen, device)
    combos = [(c, v) for v in ONE_HOT_VALUES for c in _group_edges(cin)]
    seen = set()
    for k in range(-(-len(combos) // cp)):
        w, ch, val = _one_hot_w(cin, cp, combos, k, device)
        seen |= set(zip(ch.tolist(), val.tolist()))
        _same_bits(_limb_launch(device, x, w), x[:, ch] * val, '%s launch %d' % (inst, k))
    assert seen == set(combos)


@pytest.mark.gpu
@pytest.mark.parametrize('inst', list(LIMB_CASES))
def test_range_ends_bit_exact(device, inst):
    """+-fp32-max (clamped before the first rounding only: no inf limb), 1 + 2^-23 and 2 - 2^-23 against weight 1."""
    cin, cp = LIMB_CASES[inst]
    fmax = float(np.finfo(np.float32).max)
    vals = torch.tensor([fmax, -fmax, 1.0 + 2.0 ** -23, 2.0 - 2.0 ** -23, -(1.0 + 2.0 ** -23), -(2.0 - 2.0 ** -23)], device=device)
    gen = torch.Generator(device=device).manual_seed(4)
    x = vals[torch.randint(0, vals.numel(), (LIMB_ROWS, cin), generator=gen, device=device)]
    w, ch, _ = _one_hot_w(cin, cp, [(c, 1.0) for c in _group_edges(cin)], 0, device)
    _same_bits(_limb_launch(device, x, w), x[:, ch], inst)


@pytest.mark.gpu
@pytest.mark.parametrize('inst', list(LIMB_CASES))
def test_weight_limbs_bit_exact(device, inst):
    """Patterned 24-bit weights against one-hot inputs (+-1, 0.5, +-2): the weight's h, m and l (terms h.h, m.h, l.h)."""
    cin, cp = LIMB_CASES[inst]
    gen = torch.Generator(device=device).manual_seed(5)
    w = _patterned((cin, cp), gen, device)
    edges = _group_edges(cin)
    ch = torch.tensor([edges[r % len(edges)] for r in range(LIMB_ROWS)], device=device)
    val = torch.tensor([ONE_HOT_VALUES[(r // len(edges)) % len(ONE_HOT_VALUES)] for r in range(LIMB_ROWS)], device=device)
    x = torch.zeros((LIMB_ROWS, cin), device=device)
    x[torch.arange(LIMB_ROWS, device=device), ch] = val
    _same_bits(_limb_launch(device, x, w), w[ch] * val[:, None], inst)


@pytest.mark.gpu
@pytest.mark.parametrize('inst', list(LIMB_CASES))
def test_mm_term_bit_exact(device, inst):
    """(1 + 2^-10) 2^a times (1 + 2^-10) 2^b = (1 + 2^-9 + 2^-20) 2^(a + b): both operands have h = 2^e and m = 2^(e - 10), so the
    2^-20 comes from the m.m term alone."""
    cin, cp = LIMB_CASES[inst]
    gen = torch.Generator(device=device).manual_seed(6)
    f = 1.0 + 2.0 ** -10
    x = f * _pow2(torch.randint(-30, 31, (LIMB_ROWS, cin), generator=gen, device=device))
    b = torch.randint(-30, 31, (cp,), generator=gen, device=device)
    w, ch, _ = _one_hot_w(cin, cp, [(c, 1.0) for c in _group_edges(cin)], 0, device)
    w = w * (f * _pow2(b))[None, :]
    exp = (x[:, ch].double() * (f * _pow2(b)).double()[None, :]).float()
    assert torch.equal(exp.double(), x[:, ch].double() * (f * _pow2(b)).double()[None, :])          # exact in fp32: 21 bits
    _same_bits(_limb_launch(device, x, w), exp, inst)


@pytest.mark.gpu
@pytest.mark.parametrize('inst', list(LIMB_CASES))
def test_addend_enters_once_before_the_scale(device, inst):
    """One exact product p per output and a group_shift value g with p + g exact (integers below 2^12): the output is p + g bit for
    bit with scale NULL, and (p + g) s with a power-of-two scale - not p s + g, and not p + 2 g.  Groups of 37 rows: boundaries inside
    both row tiles, the last group ragged."""
    cin, cp = LIMB_CASES[inst]
    gen = torch.Generator(device=device).manual_seed(7)
    x = torch.randint(-2048, 2049, (LIMB_ROWS, cin), generator=gen, device=device).float()
    w, ch, val = _one_hot_w(cin, cp, [(c, v) for v in (1.0, -1.0) for c in _group_edges(cin)], 0, device)
    gr = 37
    gs = torch.randint(-2048, 2049, (-(-LIMB_ROWS // gr), cp), generator=gen, device=device).float()
    gs = torch.where(gs == 0, torch.ones_like(gs), gs)
    grp = torch.arange(LIMB_ROWS, device=device) // gr
    p = x[:, ch] * val
    _same_bits(_limb_launch(device, x, w, gs, gr), p + gs[grp], inst + ' no scale')
    s = _pow2(torch.randint(-3, 4, (cp,), generator=gen, device=device))
    s = torch.where(s == 1, 4 * torch.ones_like(s), s)
    got = _limb_launch(device, x, w, gs, gr, scale=s)
    _same_bits(got, (p + gs[grp]) * s, inst + ' scale')
    assert not torch.equal(got, p * s + gs[grp])


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
#           cin cout cout_pad out columns  word
OPS_REFUSED = [(16, 64, 64, 64, 'cin (a'), (48, 64, 64, 64, 'cin (a'), (64, 24, 24, 24, 'cout_pad (a'), (64, 8, 8, 8, 'cout_pad (a'),
               (64, 65, 64, 65, 'cout (1'), (64, 64, 64, 63, 'y_stride (at')]


@pytest.mark.gpu
@pytest.mark.parametrize('cin,cout,cp,ycols,word', OPS_REFUSED, ids=['%d-%d-%d-%d' % r[:4] for r in OPS_REFUSED])
def test_refusals_through_ops_linear_write_nothing(device, cin, cout, cp, ycols, word):
    rows = 5
    x, w = torch.randn(rows, cin, device=device), torch.randn(cin, cp, device=device)
    wl = torch.zeros((1, (cp + 31) // 32 * 32, max(cin // 8 * 12, 12)), device=device)
    out = Out(rows, ycols, device)
    with pytest.raises(L.DetZeroHipError) as e:
        ops.linear(x, w, None, None, False, cout, out=out.raw.view(torch.float32)[:rows], f32_engine='bf16x3', w_limb=wl)
    assert word in str(e.value) and 'dz_linear_limb3_forward' in str(e.value), str(e.value)
    assert out.untouched()
    if word.startswith(('cin', 'cout_pad')):
        assert L.load().dz_linear_limb3_variant(cin, cp) == b'none'
    with pytest.raises(L.DetZeroHipError):
        ops.linear(x, w, None, None, False, cout, f32_engine='bf16x3')           # no limb weights


@pytest.mark.gpu
def test_refusals_through_the_abi_write_nothing(device):
    """The fields ops.linear cannot express (it passes the stride of a contiguous tensor), null pointers, negative counts, a cap below
    one row group."""
    lib = L.load()
    rows, cin, cp = 5, 64, 64
    x, wl = torch.randn(rows, cin, device=device), torch.zeros((1, cp, cin * 3 // 2), device=device)
    gs = torch.zeros((1, cp), device=device)
    out = Out(rows, cp, device)

    def call(word, rc_want, **kw):
        a = dict(x=L.ptr(x), rows=rows, cin=cin, xs=cin, w=L.ptr(wl), cout=cp, cp=cp, gs=None, gr=0, y=out.ptr, ys=cp, mlr=0)
        a.update(kw)
        rc = lib.dz_linear_limb3_forward(a['x'], a['rows'], a['cin'], a['xs'], a['w'], a['cout'], a['cp'], None, None, a['gs'], a['gr'], 0, a['y'],
                                         a['ys'], a['mlr'], L.stream())
        assert rc == rc_want and word in lib.dz_last_error().decode(), (kw, rc, lib.dz_last_error())
        with pytest.raises(L.DetZeroHipError):
            L.check(rc, 'dz_linear_limb3_forward')
        torch.cuda.synchronize()
        assert out.untouched(), kw
    call('x_stride (at', -4, xs=60)
    call('x_stride (at', -4, xs=66)
    call('cin (a', -4, cin=0, xs=0)
    call('cout_pad (a', -4, cp=0, cout=0)
    call('cout (1', -4, cout=0)
    call('null', -1, x=None)
    call('null', -1, y=None)
    call('null', -1, w=None)
    call('rows', -1, rows=-1)
    call('max_launch_rows', -1, mlr=-1)
    call('max_launch_rows', -4, mlr=4, gs=L.ptr(gs), gr=5)
    assert lib.dz_linear_limb3_variant(0, 64) == b'none' and lib.dz_linear_limb3_variant(64, 0) == b'none'
    assert lib.dz_linear_limb3_forward(L.ptr(x), 0, cin, cin, L.ptr(wl), cp, cp, None, None, None, 0, 0, out.ptr, cp, 0, L.stream()) == 0
    torch.cuda.synchronize()
    assert out.untouched()


# ------------------------------------------------------------------------------------------------------------------------
# through the models
# ------------------------------------------------------------------------------------------------------------------------
class _Spy:
    """Stands in for ops.linear: records (cin, x_stride, cout, cout_pad, relu, addend, engine) of every call and makes it."""

    def __init__(self, monkeypatch):
        self.real, self.calls = ops.linear, []
        monkeypatch.setattr(ops, 'linear', self)

    def __call__(self, x, w, scale, shift, relu, cout, *a, **kw):
        self.calls.append((x.shape[1], x.stride(0), cout, w.shape[1], bool(relu), kw.get('group_shift') is not None, kw.get('f32_engine'),
                           kw.get('w_limb') is not None))
        return self.real(x, w, scale, shift, relu, cout, *a, **kw)

    def take(self):
        out, self.calls = self.calls, []
        return out


def _check_routing(calls, on):
    """With the switch on in f32: a call ran on dz_linear_limb3_forward exactly when the predicate covers it; every other call, and
    every call with the switch off, is the plain one (no engine keyword at all).  Returns the covered calls."""
    covered = []
    assert calls
    for cin, xs, cout, cp, relu, addend, engine, has_wl in calls:
        want = on and ops.linear_limb3_supported(cin, xs, cout, cp, cout)
        assert (engine == 'bf16x3') == want and has_wl == want and engine in (None, 'bf16x3'), (cin, xs, cout, cp, engine, on)
        if want:
            covered.append((cin, cout, relu, addend))
    return covered


def _refiner(device, which, golden):
    from detzero_amd.synth import synth_state_dict
    from tests.test_refine import _models
    model = _models()[0 if which == 'grm' else 1]
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=5 if which == 'grm' else 6), strict=True)
    data = lambda: {k[len(which) + 4:]: torch.from_numpy(golden[k]).to(device) for k in golden.files if k.startswith(which + '_in_')}   # noqa: E731
    return model.to(device), data


def _refiner_outputs(model, res, which):
    keys = ('geometry_cls', 'geometry_reg') if which == 'grm' else ('center_reg', 'heading_cls', 'heading_reg')
    return [res['memory'].clone(), res['query'].clone(), res['batch_box_preds'].clone()] + [model.preds_dict[k].clone() for k in keys]


@pytest.fixture(scope='module')
def refine_golden(golden_dir):
    import os
    return np.load(os.path.join(golden_dir, 'refine_golden.npz'))


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['grm', 'prm'])
def test_refiner_with_the_switch_on(device, refine_golden, which, monkeypatch):
    """GRM / PRM in f32 with set_linear_engine('bf16x3'): the reference golden at the tolerances of test_grm_matches_reference /
    test_prm_matches_reference; the routing; the parent's bits again after switching back; f16x2 untouched by the switch."""
    g = refine_golden
    model, data = _refiner(device, which, g)
    spy = _Spy(monkeypatch)
    model.set_math('f32')
    off = _refiner_outputs(model, model(data()), which)
    assert _check_routing(spy.take(), False) == []
    assert model.set_linear_engine('bf16x3') is model
    res = model(data())
    covered = _check_routing(spy.take(), True)
    close = torch.testing.assert_close
    t = lambda k: torch.from_numpy(g[which + '_' + k])           # noqa: E731
    if which == 'grm':
        close(res['memory'].cpu(), t('memory'), rtol=1e-3, atol=1e-4)
        close(res['query'].cpu(), t('query'), rtol=1e-3, atol=1e-4)
        close(model.preds_dict['geometry_cls'].cpu(), t('cls'), rtol=1e-3, atol=2e-4)
        close(model.preds_dict['geometry_reg'].cpu(), t('reg'), rtol=1e-3, atol=2e-4)
        close(res['batch_box_preds'].cpu(), t('boxes'), rtol=1e-3, atol=1e-3)
        # (its encoders read 16-column rows - 11 and 4 point dims padded: the first layer stays on dz_linear_forward)
        assert {(128, 128, True, False), (128, 512, True, False)} <= set(covered)
    else:
        close(res['query'].cpu(), t('query'), rtol=1e-3, atol=1e-4)
        close(res['memory'].cpu()[:, :, ::16], t('memory'), rtol=1e-3, atol=1e-4)
        valid = torch.from_numpy(g['prm_in_padding_mask']) == 0
        for k in ('center_reg', 'heading_cls', 'heading_reg'):
            close(model.preds_dict[k].cpu()[valid], t(k)[valid], rtol=1e-3, atol=2e-4)
        close(res['batch_box_preds'].cpu()[valid], t('boxes')[valid], rtol=1e-3, atol=1e-3)
        assert {(32, 128, True, False), (128, 128, True, False), (128, 256, True, False)} <= set(covered)       # the three encoder layers
    assert (128, 512, True, True) in covered                                           # the group_shift layer of the memory MLP
    assert (512, 256, True, False) in covered
    assert covered.count((256, 256, False, False)) >= 5                                # Q / K / V / O of the self-attention, Q / O of the cross-attention, FFN 2
    assert (256, 256, True, False) in covered                                          # the feed-forward block's first layer
    assert (256, 64, True, False) in covered and any(c[0] == 64 for c in covered)      # the prediction heads
    on = _refiner_outputs(model, res, which)
    assert any(not torch.equal(a, b) for a, b in zip(off, on))                         # (another accumulation order: not the same bits)
    model.set_linear_engine('mfma32')
    back = _refiner_outputs(model, model(data()), which)
    assert _check_routing(spy.take(), False) == []
    assert all(torch.equal(a, b) for a, b in zip(off, back))
    # the split modes ignore the switch
    monkeypatch.setattr(__import__('detzero_amd.refine_modules', fromlist=['x']), 'SPLIT_MIN_ROWS', 1)
    model.set_math('f16x2')
    s_off = _refiner_outputs(model, model(data()), which)
    model.set_linear_engine('bf16x3')
    s_on = _refiner_outputs(model, model(data()), which)
    assert _check_routing(spy.take(), False) is not None
    assert all(torch.equal(a, b) for a, b in zip(s_off, s_on))


@pytest.mark.gpu
def test_pdv_head_with_the_switch_on(device, golden_dir, monkeypatch):
    """The PDV head in f32 with centerpoint.set_linear_engine(.., 'bf16x3'): its golden at the tolerances of
    test_final_boxes_and_confidences and test_pooled_features_positional_input_and_attention, and the routing.
    Bits: the head's front (voxel centroids) sums with float atomics in arrival order, so two passes of the WHOLE head are not the same
    bits whatever the switch says (printed below); everything behind the pooled features is a fixed-order function of them.  The
    switch-back and split-mode checks therefore run the encoder layer and the FC stacks - every linear of the head - on the pooled
    features, positional input and mask of ONE pass."""
    import os
    from detzero_amd.centerpoint import set_linear_engine
    from detzero_amd.refine_modules import _run_stack
    from tests.test_pdv import _batch, _head
    g = np.load(os.path.join(golden_dir, 'pdv_golden.npz'))
    head = _head().to(device)
    spy = _Spy(monkeypatch)

    def run():
        out = head(_batch(g, device))
        return [out['batch_box_preds'].clone(), out['batch_cls_preds'].clone(), head.forward_ret_dict['attention_output'].clone()]
    off = run()
    assert _check_routing(spy.take(), False) == []
    r = head.forward_ret_dict
    pooled, pos_in, mask = r['pooled_features'].clone(), r['positional_input'].clone(), r['key_padding_mask'].clone()
    print('  two whole-head passes with the switch off, same bits:', all(torch.equal(a, b) for a, b in zip(off, run())))
    spy.take()

    def tail():
        """forward() behind roi_grid_pool, on the kept tensors."""
        p, kw = head.plan(), dict(math=head.stack_math(), engine=head.f32_linear_engine)
        att = head.attention(pooled, pos_in, mask, combine=bool(head.pool_cfg.ATTENTION.get('COMBINE')))
        shared, _ = _run_stack(att.reshape(att.shape[0], -1).contiguous(), p['shared'], **kw)
        return [att.clone(), _run_stack(shared, p['reg'], **kw)[0].clone(), _run_stack(shared, p['cls'], **kw)[0].clone()]
    t_off = tail()
    assert _check_routing(spy.take(), False) == []
    set_linear_engine(head, 'bf16x3')
    assert head.f32_linear_engine == 'bf16x3'
    on = run()
    covered = _check_routing(spy.take(), True)
    torch.testing.assert_close(on[0].cpu(), torch.from_numpy(g['batch_box_preds']), rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(on[1].cpu(), torch.from_numpy(g['batch_cls_preds']), rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(on[2][g['roi_subset']].cpu(), torch.from_numpy(g['pooled'] + g['attention']), rtol=2e-3, atol=2e-3)
    assert covered.count((192, 192, False, False)) >= 4                                # Q / K / V / O of the encoder layer
    assert any(c[0] == 192 and c[2] for c in covered) and (256, 256, True, False) in covered       # its feed-forward block, the FC stacks
    t_on = tail()
    assert sorted(_check_routing(spy.take(), True)) == sorted(covered)                 # the tail makes every linear call of the head
    assert any(not torch.equal(a, b) for a, b in zip(t_off, t_on))
    set_linear_engine(head, 'mfma32')
    t_back = tail()
    assert _check_routing(spy.take(), False) == []
    assert all(torch.equal(a, b) for a, b in zip(t_off, t_back))
    head.set_math('f16x2')
    s_off = tail()
    set_linear_engine(head, 'bf16x3')
    s_on = tail()
    assert all(c[6] is None for c in spy.take())
    assert all(torch.equal(a, b) for a, b in zip(s_off, s_on))
