"""GPU: the three-limb (bf16x3) engine of the f32 mode's attention core (csrc/mha_t.hip, dz_mha_core_limb3) against the float64
reference oracle.refine.attention - on every case of dz_mha_core's own table (tests/test_gpu_refine_kernels.py, the fp32 core's bound),
on an edge table for its 32-key tile / 64-key block geometry, over the gain sweep, in its exact properties, limb by limb, next to
dz_mha_core for the error class, in its refusals and through GRM / PRM with the switch on.  Every output sits in a buffer with
sentinel rows behind it; every case is launched twice and must give the same bits.  tests/test_mha_limb3_build.py holds the host
emulation, the edge table and the allowances."""
import numpy as np
import pytest
import torch

from detzero_amd import lib as L
from detzero_amd import ops
from oracle import refine as R
from tests.test_gpu_refine_kernels import (ATT_BOUND, MHA_CASES, SENT_F, SWEEP, Out, assert_within, attention_inputs, dev, f32_baseline, mha_case,
                                           sweep_case, worst_ratio)
from tests.test_mha_limb3_build import EDGE_CASES, LONG_RISE, edge_allowance, edge_case, edge_id, emulation_error

F64, F32 = np.float64, np.float32
FLT_MAX = 3.4028234663852886e38
POISONS = (np.nan, 1e30, FLT_MAX)


def poison3(k, mask, turn=0):
    """A copy of k with the rows of the masked keys NaN, 1e30 and FLT_MAX in turn by key position, starting with POISONS[turn]: over
    turn 0, 1, 2 every masked key holds each of the three."""
    if mask is None:
        return k
    k = k.copy()
    bi, ki = np.nonzero(mask)
    k[bi, ki, :] = np.asarray(POISONS, F32)[(ki + turn) % 3][:, None]
    return k


def run(device, case, engine='bf16x3', poison=True, turn=0):
    """dz_mha_core_limb3 (or dz_mha_core) on a case, masked keys poisoned, in a sentinel buffer, twice -> (b, lq, e) float32."""
    lib = L.load()
    b, lq, e = case['q'].shape
    lk = case['k'].shape[1]
    dq, dk, dv = dev(case['q'], device), dev(poison3(case['k'], case['mask'], turn) if poison else case['k'], device), dev(case['v'], device)
    dm = dev(case['mask'], device)
    out = Out(b * lq, e, device)
    fn = lib.dz_mha_core_limb3 if engine == 'bf16x3' else lib.dz_mha_core

    def launch():
        L.check(fn(L.ptr(dq), L.ptr(dk), L.ptr(dv), L.ptr(dm), b, lq, lk, case['heads'], case['scale'], out.ptr, L.stream()), 'attention')
    out.run_twice(launch)
    out.check()
    return out.f32().cpu().numpy().reshape(b, lq, e)


def run_turns(device, case):
    """`run` once per poison turn (masked cases: three runs, every masked K row holds NaN, 1e30 and FLT_MAX once); the results must be
    the same bits - a masked row shows in nothing - and the first is returned."""
    got = run(device, case)
    if case['mask'] is not None:
        for turn in (1, 2):
            assert np.array_equal(run(device, case, turn=turn).view(np.int32), got.view(np.int32)), ('poison turn', turn)
    return got


def case_of(q, k, v, mask, heads, scale=32 ** -0.5):
    return {'q': q, 'k': k, 'v': v, 'mask': mask, 'heads': heads, 'scale': scale}


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(MHA_CASES)), ids=['-'.join(str(x) for x in c) for c in MHA_CASES])
def test_mha_cases(device, i):
    """dz_mha_core_limb3 on MHA_CASES[i] within the fp32 core's own bound."""
    c = mha_case(i)
    got = run_turns(device, c)
    assert_within(got, c['want'], ATT_BOUND['f32'] * c['nat'], 'dz_mha_core_limb3 %s' % '-'.join(str(x) for x in MHA_CASES[i]), ATT_BOUND['f32'])


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(EDGE_CASES)), ids=[edge_id(c) for c in EDGE_CASES])
def test_edge_cases(device, i):
    """The edge table of the tile / block geometry; ATT_BOUND['f32'], the 1000-key rising case 8 x its host allowance."""
    c = edge_case(i)
    bound = 8.0 * edge_allowance(i) if i == LONG_RISE else ATT_BOUND['f32']
    assert bound >= ATT_BOUND['f32']
    got = run_turns(device, c)
    assert_within(got, c['want'], bound * c['nat'], 'dz_mha_core_limb3 edge %s' % edge_id(EDGE_CASES[i]), bound)


@pytest.mark.gpu
def test_gain_sweep(device):
    """Gains 2^-12 .. 2^8 on q.k and on v at (2, 40, 130): the kernel, the host emulation and the float32 host baseline side by side;
    the kernel within max(ATT_BOUND['f32'], 8 x the emulation)."""
    for kind in ('qk', 'v'):
        line, plain, rows = [], [], []
        for k2, g in SWEEP:
            if k2 != kind:
                continue
            c = sweep_case(kind, g)
            got = run(device, c)
            err, emu, base = worst_ratio(got, c['want'], c['nat']), emulation_error(c), f32_baseline(c)
            line.append('2^%d %.1e (emulation %.1e, float32 host %.1e)' % (g, err, emu, base))
            rows.append((g, err, emu))
            if err <= ATT_BOUND['f32']:
                plain.append(g)
        print('  dz_mha_core_limb3, gain on %s: ' % kind + ', '.join(line))
        print('  the plain bound %.1e holds at gains 2^%s' % (ATT_BOUND['f32'], plain))
        for g, err, emu in rows:
            assert err <= max(ATT_BOUND['f32'], 8.0 * emu), (kind, g, err, emu)


@pytest.mark.gpu
@pytest.mark.parametrize('lq', [17, 64, 300])
def test_exact_properties(device, lq):
    """No tolerance: a masked tail of random keys up to 160 and 192 (the next multiples of 32 and 64) gives the bits of the unpadded
    call, with and without a mask of its own; permuting batch entries and heads permutes the output; v times 2^+-20 scales it."""
    b, lk, heads = 3, 129, 8
    q, k, v, mask = attention_inputs(5000 + lq, b, lq, lk, heads, 32, 'randn', 'rand')
    rng = np.random.default_rng(lq)
    go = lambda q_, k_, v_, m_: run(device, case_of(q_, k_, v_, m_, heads))          # noqa: E731
    for m in (None, mask):
        base = go(q, k, v, m)
        for lkp in (160, 192):
            kp = np.concatenate([k, rng.standard_normal((b, lkp - lk, heads * 32)).astype(F32)], 1)
            vp = np.concatenate([v, rng.standard_normal((b, lkp - lk, heads * 32)).astype(F32)], 1)
            mp = np.ones((b, lkp), np.uint8)
            mp[:, :lk] = 0 if m is None else m
            assert np.array_equal(go(q, kp, vp, mp).view(np.int32), base.view(np.int32)), ('padding', lkp, m is None)
    base = go(q, k, v, mask)
    pb, ph = np.array([2, 0, 1]), rng.permutation(heads)
    hp = lambda a: np.ascontiguousarray(a.reshape(a.shape[0], a.shape[1], heads, 32)[:, :, ph].reshape(a.shape))        # noqa: E731
    assert np.array_equal(go(q[pb], k[pb], v[pb], mask[pb]).view(np.int32), base[pb].view(np.int32)), 'batch permutation'
    assert np.array_equal(go(hp(q), hp(k), hp(v), mask).view(np.int32), hp(base).view(np.int32)), 'head permutation'
    for g in (2.0 ** 20, 2.0 ** -20):
        assert np.array_equal(go(q, k, v * F32(g), mask).view(np.int32), (base * F32(g)).view(np.int32)), ('v gain', g)


@pytest.mark.gpu
@pytest.mark.parametrize('lq', [17, 64, 300])
def test_fully_masked_entry_is_nan_for_that_entry_only(device, lq):
    b, lk, heads = 3, 70, 8
    q, k, v, mask = attention_inputs(6000 + lq, b, lq, lk, heads, 32, 'randn', 'rand')
    mask[1] = 1
    want, nat = R.attention(q, k, v, mask, heads, 32 ** -0.5)
    assert np.isnan(want[1]).all() and np.isfinite(want[[0, 2]]).all()
    got = run(device, case_of(q, k, v, mask, heads))
    assert_within(got, want, ATT_BOUND['f32'] * nat, 'fully masked entry, lq %d' % lq, ATT_BOUND['f32'])


# ------------------------------------------------------------------------------------------------------------------------
# limb fidelity, bit exact
# ------------------------------------------------------------------------------------------------------------------------
def unit_log2_scale():
    """A float32 `scale` with scale * float32(log2 e) == 1.0 in float32: the kernel's q * (scale * log2 e) is then q itself."""
    log2e = F32(1.44269504088896340736)
    s = F32(1.0) / log2e
    for cand in (s, np.nextafter(s, F32(0)), np.nextafter(s, F32(2))):
        if F32(cand * log2e) == F32(1.0):
            return float(cand)
    raise AssertionError('no float32 scale gives scale * log2(e) == 1')


def full24(rng, n, lo_exp, hi_exp):
    """n float32 values with 24 significant bits (odd significands), random signs, exponents in [lo_exp, hi_exp)."""
    sig = (1 << 23) + 2 * rng.integers(0, 1 << 22, n) + 1
    return (rng.choice([-1.0, 1.0], n) * sig * np.exp2(rng.integers(lo_exp, hi_exp, n).astype(F64) - 23)).astype(F32)


def test_unit_scale_exists():
    assert F32(F32(unit_log2_scale()) * F32(1.44269504088896340736)) == F32(1.0)


@pytest.mark.gpu
def test_limb_fidelity_scores(device):
    """(1, 32, 32, 1).  Query i is one-hot in channel i with a power of two 2^e_i (scale * log2 e == 1), so score(i, j) = k[j, i] * 2^e_i:
    ONE product, exact in the six terms exactly when all three limbs of k arrive (q has one limb; l.h + m.h + h.h rebuild k).  Keys 0 .. 3
    are live with k[j, i] = X_i - n_j 2^-e_i, n = 0, 1, 2, 2, X_i a 24-bit significand with three fraction bits: in exact arithmetic
    score - max = -n, p = 1, 1/2, 1/4, 1/4, their sum 2, and with v = the identity pattern the output row is 1/2, 1/4, 1/8, 1/8, 0 ... bit
    for bit (2^integer is exact on v_exp_f32).  Any lost limb moves a score by at least 2^-16 of 2^20 and the differences are no
    integers any more.  Query 31: k = M 2^-133 (M odd, 24 bits: the low limb is a bf16 subnormal) against q = 2^127.  The masked rows hold
    +-FLT_MAX, NaN and 1e30."""
    rng = np.random.default_rng(11)
    e = rng.integers(0, 4, 32)
    q = np.zeros((1, 32, 32), F32)
    q[0, np.arange(32), np.arange(32)] = np.exp2(e).astype(F32)
    n = np.array([0, 1, 2, 2], F64)
    k = np.zeros((1, 32, 32), F32)
    for i in range(31):
        x = float(rng.choice([-1.0, 1.0])) * float((1 << 23) + 2 * int(rng.integers(0, 1 << 22)) + 1) * 2.0 ** -3
        k[0, :4, i] = (x - n * 2.0 ** -float(e[i])).astype(F32)
        assert (k[0, :4, i].astype(F64) == x - n * 2.0 ** -float(e[i])).all()               # representable: 24 bits each
    q[0, 31, 31] = F32(2.0 ** 127)
    m31 = (1 << 23) + 2 * int(rng.integers(0, 1 << 22)) + 1
    k[0, :4, 31] = ((m31 - 64.0 * n) * 2.0 ** -133).astype(F32)
    assert (k[0, :4, 31].astype(F64) * 2.0 ** 127 == (m31 - 64.0 * n) * 2.0 ** -6).all()
    from tests.test_mha_limb3_build import limbs3
    low = limbs3(k[0, :4, 31])[2]
    assert (low != 0).all() and (np.abs(low) < F32(2.0 ** -126)).all()                      # a subnormal low limb
    mask = np.ones((1, 32), np.uint8)
    mask[0, :4] = 0
    fill = np.array([FLT_MAX, -FLT_MAX, np.nan, 1e30], F32)
    k[0, 4:, :] = fill[np.arange(28) % 4][:, None]
    v = np.eye(32, dtype=F32)[None]
    got = run(device, case_of(q, k, v, mask, 1, unit_log2_scale()), poison=False)
    want = np.zeros((1, 32, 32), F32)
    want[0, :, :4] = [0.5, 0.25, 0.125, 0.125]
    bad = np.nonzero((got.view(np.int32) != want.view(np.int32)).any(-1)[0])[0]
    assert bad.size == 0, (bad, got[0, bad[0], :6])


@pytest.mark.gpu
def test_limb_fidelity_pv(device):
    """(1, 32, 32, 1), one live key: p = 1 (one limb), so O = v_l + v_m + v_h in that order, and the output row is that key's v row bit
    for bit - for entries with full 24-bit significands from 2^-100 to 2^100, +-FLT_MAX and one with a subnormal low limb.  A dropped V
    limb or a dropped term shows here."""
    rng = np.random.default_rng(12)
    q, k, v, _ = attention_inputs(12, 1, 32, 32, 1, 32, 'randn', None)
    live = 17
    v[0] = full24(rng, 32 * 32, -20, 20).reshape(32, 32)
    v[0, live] = full24(rng, 32, -100, 100)
    v[0, live, :3] = [FLT_MAX, -FLT_MAX, float(((1 << 23) + 12345) * 2.0 ** -133)]
    mask = np.ones((1, 32), np.uint8)
    mask[0, live] = 0
    got = run(device, case_of(q, k, v, mask, 1))
    assert np.array_equal(got.view(np.int32), np.broadcast_to(v[0, live], (1, 32, 32)).view(np.int32))


@pytest.mark.gpu
def test_error_class_vs_dz_mha_core(device):
    """randn shapes: the new engine's worst normalised error against float64 is at most 2 x the fp32 core's on the same inputs."""
    for n, (b, lq, lk, heads) in enumerate([(3, 64, 200, 8), (1, 300, 129, 8), (2, 33, 1000, 1)]):
        q, k, v, mask = attention_inputs(8000 + n, b, lq, lk, heads, 32, 'randn', 'rand' if n else None)
        want, nat = R.attention(q, k, v, mask, heads, 32 ** -0.5)
        c = case_of(q, k, v, mask, heads)
        e3, e32 = worst_ratio(run(device, c), want, nat), worst_ratio(run(device, c, engine='mfma32'), want, nat)
        print('  %-18s dz_mha_core_limb3 %.3e   dz_mha_core %.3e   ratio %.2f' % ((b, lq, lk, heads), e3, e32, e3 / e32))
        assert e3 <= 2.0 * e32 and e3 <= ATT_BOUND['f32'], ((b, lq, lk, heads), e3, e32)


@pytest.mark.gpu
def test_refusals_write_nothing(device):
    from detzero_amd.lib import DetZeroHipError
    lib, st = L.load(), L.stream()
    z = torch.zeros((64, 256), device=device)
    p = z.data_ptr()
    out = Out(64, 256, device)

    def refused(rc, word):
        torch.cuda.synchronize()
        assert rc == -1 and word in lib.dz_last_error().decode() and out.untouched(), (rc, word, lib.dz_last_error())
    call = lambda sizes, q=p, k=p, v=p, o=out.ptr: lib.dz_mha_core_limb3(q, k, v, None, *sizes, 1.0, o, st)          # noqa: E731
    refused(call((2, 4, 0, 8)), 'bad sizes')
    for sizes in ((-1, 4, 8, 8), (2, -4, 8, 8), (2, 4, -8, 8), (2, 4, 8, 0), (2, 4, 8, -1), (65536, 4, 8, 8), (2, 4, 8, 65536)):
        refused(call(sizes), 'bad sizes')
    for kw in (dict(q=None), dict(k=None), dict(v=None)):
        refused(call((2, 4, 8, 8), **kw), 'null pointer')
    assert call((2, 4, 8, 8), o=None) == -1 and 'null pointer' in lib.dz_last_error().decode()
    assert call((0, 4, 8, 8)) == 0 and call((2, 0, 8, 8)) == 0
    torch.cuda.synchronize()
    assert out.untouched()
    # through ops.mha_core: nothing is launched, the inputs keep their bits
    q = torch.full((2, 4, 256), SENT_F, device=device)
    k0 = torch.full((2, 0, 256), SENT_F, device=device)
    k8 = torch.full((2, 8, 256), SENT_F, device=device)
    for kv, kw in ((k0, dict(f32_engine='bf16x3')), (k8, dict(math=1, f32_engine='bf16x3')), (k8, dict(math=2, f32_engine='bf16x3')),
                   (k8, dict(f32_engine='limbs'))):
        with pytest.raises(DetZeroHipError):
            ops.mha_core(q, kv, kv, None, 8, 1.0, **kw)
    torch.cuda.synchronize()
    sent = torch.full((1,), SENT_F).view(torch.int32).item()                        # (the sentinel is a NaN pattern: compare the words)
    assert bool((q.view(torch.int32) == sent).all()) and bool((k8.view(torch.int32) == sent).all())


# ------------------------------------------------------------------------------------------------------------------------
# through the models
# ------------------------------------------------------------------------------------------------------------------------
class _Spy:
    """Stands in for ops.mha_core: records (lq, lk, math, f32_engine, whether an engine keyword was passed) of every call and makes it."""

    def __init__(self, monkeypatch):
        self.real, self.calls = ops.mha_core, []
        monkeypatch.setattr(ops, 'mha_core', self)

    def __call__(self, q, k, v, mask, heads, scale, *a, **kw):
        math = a[0] if a else kw.get('math', 0)
        self.calls.append((q.shape[1], k.shape[1], math, kw.get('f32_engine'), 'f32_engine' in kw or len(a) > 1))
        return self.real(q, k, v, mask, heads, scale, *a, **kw)

    def take(self):
        out, self.calls = self.calls, []
        return out


@pytest.fixture(scope='module')
def refine_golden(golden_dir):
    import os
    return np.load(os.path.join(golden_dir, 'refine_golden.npz'))


def _golden_holds(model, res, g, which):
    close = torch.testing.assert_close
    t = lambda k: torch.from_numpy(g[which + '_' + k])           # noqa: E731
    if which == 'grm':
        close(res['memory'].cpu(), t('memory'), rtol=1e-3, atol=1e-4)
        close(res['query'].cpu(), t('query'), rtol=1e-3, atol=1e-4)
        close(model.preds_dict['geometry_cls'].cpu(), t('cls'), rtol=1e-3, atol=2e-4)
        close(model.preds_dict['geometry_reg'].cpu(), t('reg'), rtol=1e-3, atol=2e-4)
        close(res['batch_box_preds'].cpu(), t('boxes'), rtol=1e-3, atol=1e-3)
    else:
        close(res['query'].cpu(), t('query'), rtol=1e-3, atol=1e-4)
        close(res['memory'].cpu()[:, :, ::16], t('memory'), rtol=1e-3, atol=1e-4)
        valid = torch.from_numpy(g['prm_in_padding_mask']) == 0
        for k in ('center_reg', 'heading_cls', 'heading_reg'):
            close(model.preds_dict[k].cpu()[valid], t(k)[valid], rtol=1e-3, atol=2e-4)
        close(res['batch_box_preds'].cpu()[valid], t('boxes')[valid], rtol=1e-3, atol=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['grm', 'prm'])
def test_refiner_with_the_switch_on(device, refine_golden, which, monkeypatch):
    """GRM / PRM in f32 with set_attention_engine('bf16x3') (LIMB3_ATTN_MIN_KEYS patched to 0): the reference golden at the tolerances of
    test_grm_matches_reference / test_prm_matches_reference; the routing; the parent's bits with the switch off and again after
    switching back; nothing routed above the threshold; f16x2 untouched by the switch; both bf16x3 switches together."""
    from detzero_amd import refine_modules as rm
    from tests.test_gpu_linear_limb3 import _refiner, _refiner_outputs
    g = refine_golden
    model, data = _refiner(device, which, g)
    spy = _Spy(monkeypatch)
    monkeypatch.setattr(rm, 'LIMB3_ATTN_MIN_KEYS', 0)
    model.set_math('f32')
    same = lambda a, b: all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))          # noqa: E731
    off = _refiner_outputs(model, model(data()), which)
    calls = spy.take()
    assert calls and all(c[2] == 0 and c[3] is None and not c[4] for c in calls), calls            # no call carries an engine
    assert model.set_attention_engine('bf16x3') is model
    res = model(data())
    calls_on = spy.take()
    assert [c[:2] for c in calls_on] == [c[:2] for c in calls]
    assert all(c[2] == 0 and c[3] == 'bf16x3' for c in calls_on), calls_on                      # every math-0 call carries the engine
    print('  %s: attention calls (lq, lk) on the bf16x3 engine: %s' % (which, sorted({c[:2] for c in calls_on})))
    _golden_holds(model, res, g, which)
    on = _refiner_outputs(model, res, which)
    assert not same(off, on)                                                                     # (another arithmetic: not the same bits)
    # above the threshold nothing routes, and the outputs are the parent's bits
    monkeypatch.setattr(rm, 'LIMB3_ATTN_MIN_KEYS', max(c[1] for c in calls) + 1)
    high = _refiner_outputs(model, model(data()), which)
    assert all(c[3] is None and not c[4] for c in spy.take()) and same(off, high)
    monkeypatch.setattr(rm, 'LIMB3_ATTN_MIN_KEYS', 0)
    # both switches together
    model.set_linear_engine('bf16x3')
    res = model(data())
    assert all(c[3] == 'bf16x3' for c in spy.take())
    _golden_holds(model, res, g, which)
    model.set_linear_engine('mfma32').set_attention_engine('mfma32')
    back = _refiner_outputs(model, model(data()), which)
    assert all(c[3] is None and not c[4] for c in spy.take()) and same(off, back)
    # the split modes ignore the switch
    monkeypatch.setattr(rm, 'SPLIT_MIN_ROWS', 1)
    model.set_math('f16x2')
    s_off = _refiner_outputs(model, model(data()), which)
    spy.take()
    model.set_attention_engine('bf16x3')
    s_on = _refiner_outputs(model, model(data()), which)
    assert all(c[3] is None and not c[4] for c in spy.take()) and same(s_off, s_on)
