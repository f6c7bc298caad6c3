"""The three-limb (bf16x3) engine of the f32 mode's dense 3x3 layers (csrc/conv3x3_t.hip) on the GPU.

Float64 cases: the normalised error, bound and sentinel discipline of tests/test_gpu_dense_conv.py (|got - ref| / (|scale| * sum|x.w| +
|shift|) <= 2^-19, the f32 engine's bound), each case the smallest shape that reaches a distinct failure point; the f32 engine
(k_conv2d) runs on the same operands and its worst error is printed beside the new kernel's.

Limb-term cases: a 2^-19 bound cannot see a dropped h.l term (at most 2^-18 of ONE product, averaged down over a sum), so these are
one-hot and BIT-exact: every output is a single product whose six limb terms sum without rounding in any order.
  input limbs:  x = +-(A 2^16 + B 2^8 + C) 2^e, A in [128, 255], B, C in [0, 127] (limbs A 2^16, ~B 2^8, ~C: all three non-trivial),
                one (tap, cin) weight per output channel with value 1, -2 or 0.5;
  weight limbs: the same values in the weights, one non-zero input pixel per 3 x 3 window;
  m.m:          x = (1 + 2^-10) 2^a, w = (1 + 2^-10) 2^b: the product 1 + 2^-9 + 2^-20 is exact in fp32 and is 2^-20 off without m.m.

Every float64 case prints its worst normalised error (in units of 2^-24 too) beside the f32 engine's on the same operands.

Launch rule and epilogue arms: launch_t3 runs a layer of three channel tiles as two launches (2 + 1 tiles, the second starting at
channel tile 2) from 5000 (pixel tile, channel tile) pairs on and as one launch of 30 workgroups per XCD below; cases e - g sit on
both sides of that threshold at both tile widths, and assert which side from the descriptor (limb3_launches of
tests/test_gpu_dense_conv.py, the rule restated).  Cases h - m reach the epilogue's scalar arm (g_cout not a multiple of 4, an output
row stride or channel offset that is not 16-byte aligned), in_off = 1 and a 1 x 1-pixel image; batch = 0 returns 0 and writes nothing.

Subnormal limbs (test_subnormal_limbs_are_measured): inputs of exponent [-120, -104], whose m and l limbs are bf16 subnormals, against
one-hot weights - asserted to 2^-124 (what holds whether or not the matrix pipe flushes them), the share of bit-exact outputs printed.
"""
import ctypes

import pytest
import torch

from detzero_amd import lib as L
from detzero_amd import ops
from tests.test_gpu_dense_conv import BOUND, SENTINEL, _cdesc, conv_case, conv_ref, limb3_launches

pytestmark = pytest.mark.gpu

V128, V64 = 'k_conv3x3_t<8x32x128>', 'k_conv3x3_t<8x32x64>'
CASES = [
    # one chunk, one ragged tile
    conv_case('a 1x9x13 32->64', 'f32', 1, 9, 13, 32, 64, expect=V64),
    # odd chunk count, 400 tiles (more than the workgroups: the persistent loop and the weight stream wrap), channel offsets
    conv_case('b 40x37x45 96->128 offsets', 'f32', 40, 37, 45, 96, 128, in_coff=32, in_cextra=32, out_coff=64, out_cextra=64, expect=V128),
    # the BC = 64 tile with three channel tiles, pad channels beyond g_cout, identity epilogue
    conv_case('c 24x29x61 64->192 g_cout 184', 'f32', 24, 29, 61, 64, 192, g_cout=[184], scale=False, shift=False, relu=False, expect=V64),
    # exactly one full tile per frame, no ragged edge
    conv_case('d 2x8x32 128->64', 'f32', 2, 8, 32, 128, 64, expect=V64),
    # three channel tiles above the two-launch threshold (7 x 8 x 30 = 1680 ragged pixel tiles, 5040 pairs): the second launch starts at
    # channel tile 2; at the 128- and at the 64-channel tile
    conv_case('e 7x61x950 32->384 two launches', 'f32', 7, 61, 950, 32, 384, expect=V128),
    conv_case('f 7x61x950 32->192 two launches', 'f32', 7, 61, 950, 32, 192, expect=V64),
    # the same layer just below it (7 x 7 x 34 = 1666 pixel tiles, 4998 pairs): one launch, 30 of the 32 workgroups of an XCD
    conv_case('g 7x53x1070 32->384 one launch', 'f32', 7, 53, 1070, 32, 384, expect=V128),
    # epilogue: g_cout not a multiple of 4 in an aligned row of 184 words (quad stores, then the scalar tail and the channel predicate inside the last quad) ...
    conv_case('h 2x9x40 32->192 g_cout 181', 'f32', 2, 9, 40, 32, 192, g_cout=[181], out_cextra=3, expect=V64),
    # ... an output row stride that is not a multiple of 4 words, an aligned stride with an unaligned channel offset (vec false both ways)
    conv_case('i 2x9x40 32->64 out stride 67', 'f32', 2, 9, 40, 32, 64, out_coff=1, out_cextra=2, expect=V64),
    conv_case('j 2x9x40 32->64 out offset 2 g_cout 61', 'f32', 2, 9, 40, 32, 64, g_cout=[61], out_coff=2, out_cextra=1, expect=V64),
    # the input read from pixel (1, 1) on
    conv_case('k 2x9x40 32->64 in_off 1', 'f32', 2, 9, 40, 32, 64, in_off=1, expect=V64),
    # one pixel
    conv_case('m 1x1x1 32->64', 'f32', 1, 1, 1, 32, 64, expect=V64),
]
# (launches, workgroups per XCD of each) launch_t3 must give the cases around its two-launch threshold
LAUNCHES = {'e 7x61x950 32->384 two launches': (2, [32, 32]), 'f 7x61x950 32->192 two launches': (2, [32, 32]),
            'g 7x53x1070 32->384 one launch': (1, [30])}


def _launch(desc, ptrs, engine):
    lib = L.load()
    d = _cdesc(desc, ptrs)
    fn = lib.dz_conv3x3_limb3_forward if engine == 'bf16x3' else lib.dz_conv2d_forward
    rc = fn(ctypes.byref(d), L.stream())
    msg = lib.dz_last_error()
    return rc, (msg.decode() if msg else '')


def _region(dd):
    o0 = dd['out_coff'] + dd['g_ooff'][0]
    return (slice(None), slice(dd['out_dy'], dd['out_dy'] + dd['ho']), slice(dd['out_dx'], dd['out_dx'] + dd['wo']), slice(o0, o0 + dd['g_cout'][0]))


def _run(dd, inp, w32, sc, sh, engine, dev, twice=True):
    """Launch into sentinel-filled buffers (twice: same bits); nothing outside the descriptor's region may be written.
    Returns the written region as fp32 (batch, ho, wo, g_cout)."""
    wk = ops.pack_weight_limb3(w32) if engine == 'bf16x3' else w32.contiguous()
    B = dd['batch']
    nout = B * dd['out_hp'] * dd['out_wp'] * dd['out_cstride']
    outs = [torch.full((nout,), SENTINEL, dtype=torch.int32, device=dev) for _ in range(2 if twice else 1)]
    for o in outs:
        ptrs = dict(inp=inp.data_ptr(), out=o.data_ptr(), w=wk.data_ptr())
        if sc is not None:
            ptrs['scale'] = sc.data_ptr()
        if sh is not None:
            ptrs['shift'] = sh.data_ptr()
        rc, msg = _launch(dd, ptrs, engine)
        assert rc == 0, (engine, rc, msg)
    torch.cuda.synchronize(dev)
    if twice:
        assert torch.equal(outs[0], outs[1]), ('two launches differ', engine)
    out = outs[0].view(B, dd['out_hp'], dd['out_wp'], dd['out_cstride'])
    touched = torch.zeros(out.shape, dtype=torch.bool, device=dev)
    touched[_region(dd)] = True
    bad = (out != SENTINEL) & ~touched
    assert not bool(bad.any()), ('%d words written outside the output region, first at (b, y, x, channel) = %s' % (int(bad.sum()), torch.nonzero(bad)[0].tolist()), engine)
    return out[_region(dd)].contiguous().view(torch.float32)


@pytest.mark.parametrize('case', CASES, ids=[c.label for c in CASES])
def test_against_float64(device, case):
    dev, dd = device, case.desc
    lib = L.load()
    assert lib.dz_conv3x3_limb3_supported(ctypes.byref(_cdesc(dd))) == 1
    assert lib.dz_conv3x3_limb3_variant(ctypes.byref(_cdesc(dd))).decode() == case.expect
    nl, pair_tiles, per_xcd = limb3_launches(dd)
    if case.label in LAUNCHES:
        # which side of the launcher's threshold the case is on, from the descriptor: a change of the rule shows here
        print('  %-32s %d pair tiles -> %d launch(es) of %s workgroups per XCD' % (case.label, pair_tiles, nl, per_xcd))
        assert (nl, per_xcd) == LAUNCHES[case.label], (case.label, pair_tiles, nl, per_xcd)
        assert abs(pair_tiles - 5000) <= 40, (case.label, pair_tiles)
    else:
        assert nl == 1, (case.label, pair_tiles)
    vec = ((dd['out_cstride'] | (dd['out_coff'] + dd['g_ooff'][0])) & 3) == 0
    assert vec == (case.label[0] not in 'ij') and (dd['g_cout'][0] % 4 != 0) == (case.label[0] in 'hj'), case.label
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    B, ho, wo, cin, cp, gc = dd['batch'], dd['ho'], dd['wo'], dd['cin'], dd['cout_pad'], dd['g_cout'][0]
    inp = torch.randn((B, dd['in_hp'], dd['in_wp'], dd['in_cstride']), generator=gen, device=dev)
    w32 = torch.randn((9, cin, cp), generator=gen, device=dev)
    sc = (torch.rand(cp, generator=gen, device=dev) + 0.5) / (9 * cin) ** 0.5 if case.scale else None
    sh = torch.randn(cp, generator=gen, device=dev) * 0.5 if case.shift else None
    # float64 on the fp32 operands, once for both engines
    x = inp[:, dd['in_off']:, dd['in_off']:, dd['in_coff']:dd['in_coff'] + cin].double()
    acc, aacc = conv_ref(x, w32.double().view(3, 3, cin, cp), 1, ho, wo)
    scv = sc[:gc].double() if sc is not None else torch.ones(gc, dtype=torch.float64, device=dev)
    shv = sh[:gc].double() if sh is not None else torch.zeros(gc, dtype=torch.float64, device=dev)
    ref = acc[..., :gc] * scv + shv
    if dd['relu']:
        ref = ref.clamp_min(0.0)
    den = (aacc[..., :gc] * scv.abs() + shv.abs()).clamp_min(1e-30)
    worst = {}
    for engine in ('bf16x3', 'mfma32'):
        got = _run(dd, inp, w32, sc, sh, engine, dev).double()
        err = (got - ref).abs() / den
        err = torch.where(torch.isnan(got), torch.full_like(err, float('inf')), err)
        worst[engine] = float(err.max())
    print('  %-32s %-22s normalised error: bf16x3 %.3e (%.2f x 2^-24)   f32 engine %.3e (%.2f x 2^-24)   bound %.1e' % (
        case.label, case.expect, worst['bf16x3'], worst['bf16x3'] * 2 ** 24, worst['mfma32'], worst['mfma32'] * 2 ** 24, BOUND['f32']))
    assert worst['bf16x3'] <= BOUND['f32'], (case.label, worst)
    assert worst['mfma32'] <= BOUND['f32'], (case.label, worst)


def test_batch_zero_writes_nothing(device):
    """batch = 0: dz_conv3x3_limb3_forward returns 0 and not one word of the output buffer changes."""
    dd = dict(conv_case('batch 0', 'f32', 1, 9, 40, 32, 64).desc)
    inp = torch.zeros((1, dd['in_hp'], dd['in_wp'], dd['in_cstride']), device=device)
    wk = ops.pack_weight_limb3(torch.ones((9, 32, 64), device=device))
    out = torch.full((dd['out_hp'] * dd['out_wp'] * dd['out_cstride'],), SENTINEL, dtype=torch.int32, device=device)
    dd['batch'] = 0
    assert L.load().dz_conv3x3_limb3_supported(ctypes.byref(_cdesc(dd))) == 1
    rc, msg = _launch(dd, dict(inp=inp.data_ptr(), out=out.data_ptr(), w=wk.data_ptr()), 'bf16x3')
    torch.cuda.synchronize(device)
    assert rc == 0, (rc, msg)
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------
# limb-term cases: one product per output, bit-exact
# ------------------------------------------------------------------------------------------------------------------------
def _pow2(e):
    """2^e as fp32 from the exponent field (|e| <= 126): exact by construction.  torch.ldexp multiplies by pow(2, e), which the
    device evaluates to within an ulp, not exactly."""
    assert int(e.min()) >= -126 and int(e.max()) <= 127
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def _patterned(shape, gen, dev, e_lo=-40, e_hi=16):
    """+-(A 2^16 + B 2^8 + C) 2^e as fp32 (exact: 24 bits), A in [128, 255], B, C in [0, 127], e in [e_lo, e_hi]."""
    ri = lambda lo, hi: torch.randint(lo, hi + 1, shape, generator=gen, device=dev)
    mant = ri(128, 255) * 65536 + ri(0, 127) * 256 + ri(0, 127)
    sign = ri(0, 1) * 2 - 1
    e = ri(e_lo, e_hi)
    f = (mant * sign).float() * _pow2(e)             # a 24-bit integer times a power of two in the normal range: no rounding
    m2, e2 = torch.frexp(f.double())                 # checked in integers: mant is in [2^23, 2^24), so f = (+-mant 2^-24) 2^(e + 24)
    assert torch.equal((m2 * 2 ** 24).long(), mant * sign) and torch.equal(e2.long(), e + 24)
    return f


def _one_hot_weights(cin, cp, values, gen, dev):
    """(9, cin, cp) weights with ONE non-zero (tap, cin) entry per output channel: the first output channels cover all nine taps x
    the first and last channel of every 32-channel chunk, the rest draw theirs at random.  Returns (w, tap, ci, value) per channel."""
    edge = [c for k in range(cin // 32) for c in (32 * k, 32 * k + 31)]
    combos = [(t, c) for t in range(9) for c in edge]
    g = torch.Generator().manual_seed(int(torch.randint(0, 1 << 30, (1,), generator=gen, device=dev)))
    perm = torch.randperm(len(combos), generator=g).tolist()
    tap = torch.empty(cp, dtype=torch.long)
    ci = torch.empty(cp, dtype=torch.long)
    for o in range(cp):
        if o < len(combos):
            tap[o], ci[o] = combos[perm[o]]
        else:
            tap[o], ci[o] = int(torch.randint(0, 9, (1,), generator=g)), int(torch.randint(0, cin, (1,), generator=g))
    val = values[torch.arange(cp) % values.numel()]
    w = torch.zeros((9, cin, cp), dtype=torch.float32)
    w[tap, ci, torch.arange(cp)] = val
    return w.to(dev), tap, ci, val.to(dev)


def _expect_one_hot(inp, dd, tap, ci, val):
    """float64 products in[y + ky, x + kx, ci_o] * val_o -> fp32 (they are exact there by construction; checked)."""
    ho, wo = dd['ho'], dd['wo']
    cols = []
    for o in range(tap.numel()):
        ky, kx = int(tap[o]) // 3, int(tap[o]) % 3
        cols.append(inp[:, ky:ky + ho, kx:kx + wo, int(ci[o])].double() * val[o].double())
    e64 = torch.stack(cols, dim=-1)
    e32 = e64.float()
    assert torch.equal(e32.double(), e64)
    return e32


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same_bits(got, exp, what):
    diff = _bits(got) != _bits(exp)
    if bool(diff.any()):
        i = torch.nonzero(diff)[0].tolist()
        raise AssertionError('%s: %d of %d outputs differ in bits, first at (b, y, x, channel) = %s: got %r, expected %r' % (
            what, int(diff.sum()), diff.numel(), i, float(got[tuple(i)]), float(exp[tuple(i)])))


ONE_HOT = [(64, 64, 9, 40), (96, 128, 11, 70)]        # (cin, cout_pad, ho, wo): both instances, ragged tiles in x and y, 2 and 3 chunks


@pytest.mark.parametrize('cin,cp,ho,wo', ONE_HOT)
def test_input_limbs_bit_exact(device, cin, cp, ho, wo):
    dev = device
    dd = conv_case('input limbs', 'f32', 2, ho, wo, cin, cp, scale=False, shift=False, relu=False).desc
    gen = torch.Generator(device=dev)
    gen.manual_seed(21)
    inp = _patterned((2, dd['in_hp'], dd['in_wp'], cin), gen, dev)
    w, tap, ci, val = _one_hot_weights(cin, cp, torch.tensor([1.0, -2.0, 0.5]), gen, dev)
    got = _run(dd, inp, w, None, None, 'bf16x3', dev, twice=False)
    _assert_same_bits(got, _expect_one_hot(inp, dd, tap, ci, val), 'input limbs %d->%d' % (cin, cp))


@pytest.mark.parametrize('cin,cp,ho,wo', ONE_HOT)
def test_weight_limbs_bit_exact(device, cin, cp, ho, wo):
    """The weights carry the patterned 24-bit values; the input has one non-zero pixel per 3 x 3 window (a 3-pixel lattice), on one
    channel - a first or last channel of a chunk - with value +-1, 0.5 or 2: every output is one product, every tap is reached."""
    dev = device
    dd = conv_case('weight limbs', 'f32', 2, ho, wo, cin, cp, scale=False, shift=False, relu=False).desc
    gen = torch.Generator(device=dev)
    gen.manual_seed(22)
    hp, wp = dd['in_hp'], dd['in_wp']
    w = _patterned((9, cin, cp), gen, dev)
    edge = torch.tensor([c for k in range(cin // 32) for c in (32 * k, 32 * k + 31)], device=dev)
    vals = torch.tensor([1.0, -1.0, 0.5, 2.0], device=dev)
    yy, xx = torch.meshgrid(torch.arange(hp, device=dev), torch.arange(wp, device=dev), indexing='ij')
    on = (yy % 3 == 1) & (xx % 3 == 2)
    chan = edge[torch.randint(0, edge.numel(), (2, hp, wp), generator=gen, device=dev)]
    pv = vals[torch.randint(0, 4, (2, hp, wp), generator=gen, device=dev)] * on
    inp = torch.zeros((2, hp, wp, cin), device=dev)
    inp.scatter_(3, chan.unsqueeze(-1), pv.unsqueeze(-1))
    got = _run(dd, inp, w, None, None, 'bf16x3', dev, twice=False)
    # every term but one is an exact zero: the float64 convolution IS the single product
    acc, _ = conv_ref(inp.double(), w.double().view(3, 3, cin, cp), 1, ho, wo)
    exp = acc.float()
    assert torch.equal(exp.double(), acc) and bool((exp != 0).all())
    _assert_same_bits(got, exp, 'weight limbs %d->%d' % (cin, cp))


@pytest.mark.parametrize('cin,cp,ho,wo', ONE_HOT)
def test_mm_term_bit_exact(device, cin, cp, ho, wo):
    dev = device
    dd = conv_case('m.m', 'f32', 2, ho, wo, cin, cp, scale=False, shift=False, relu=False).desc
    gen = torch.Generator(device=dev)
    gen.manual_seed(23)
    shp = (2, dd['in_hp'], dd['in_wp'], cin)
    inp = (1 + 2.0 ** -10) * _pow2(torch.randint(-20, 21, shp, generator=gen, device=dev))
    wv = (1 + 2.0 ** -10) * _pow2(torch.randint(-20, 21, (cp,)))
    w, tap, ci, val = _one_hot_weights(cin, cp, wv, gen, dev)
    got = _run(dd, inp, w, None, None, 'bf16x3', dev, twice=False)
    exp = _expect_one_hot(inp, dd, tap, ci, val)
    # the product is (1 + 2^-9 + 2^-20) 2^(a + b): its last bit is the m.m term
    mant = torch.frexp(exp)[0] * 2
    assert torch.equal(mant, torch.full_like(mant, 1 + 2.0 ** -9 + 2.0 ** -20))
    _assert_same_bits(got, exp, 'm.m %d->%d' % (cin, cp))


# ------------------------------------------------------------------------------------------------------------------------
# subnormal limbs: measured, not required
# ------------------------------------------------------------------------------------------------------------------------
TINY_BOUND = 2.0 ** -124        # two flushed limbs, each below 2^-126 (the smallest normal bf16), times |w| <= 2


def _patterned_tiny(shape, gen, dev, e_lo=-120, e_hi=-104):
    """_patterned's 24-bit values scaled to +-[1, 2) 2^e, e in [e_lo, e_hi]: normal fp32 whose m and / or l limbs (at most 2^(e - 9) and
    2^(e - 17)) lie below 2^-126, the smallest normal bf16.  Exact: two multiplications by powers of two with normal results."""
    e = torch.randint(e_lo, e_hi + 1, shape, generator=gen, device=dev)
    f = _patterned(shape, gen, dev, 0, 0) * _pow2(torch.full_like(e, -23)) * _pow2(e)
    assert torch.equal(torch.frexp(f.double())[1].long(), e + 1)
    return f


def _subnormal_report(what, got, xsel, val):
    """`got` (..., C) against the single product xsel * val behind every output (xsel (..., C): the input value, val (C,): +-1, 0.5, 2).
    Asserts |got - x w| <= 2^-124, which holds whether the matrix pipe keeps or flushes subnormal bf16 inputs; prints the share of
    outputs that are bit-exact, and the share that equals each of the two predictions made from the host's limb split
    (ops._limbs3, on the CPU): every limb kept, and the limbs below 2^-126 dropped.  (Below exponent -110 the 24 bits of a value
    reach under 2^-133, the smallest bf16 subnormal: there the three limbs do not hold all of x even when kept.)  Returns the
    shares (exact, kept, flushed) over the outputs whose input has a subnormal limb."""
    x64, v64 = xsel.double().cpu(), val.double().cpu()
    g64 = got.double().cpu()
    exact = x64 * v64
    assert torch.equal(exact.float().double(), exact) and not bool(torch.isnan(g64).any())
    err = float((g64 - exact).abs().max())
    h, m, l = (t.double() for t in ops._limbs3(xsel.cpu()))
    sub = lambda t: (t != 0) & (t.abs() < 2.0 ** -126)          # noqa: E731
    has = sub(m) | sub(l)
    kept = (h + (m + l)) * v64
    flushed = (h + (torch.where(sub(m), torch.zeros_like(m), m) + torch.where(sub(l), torch.zeros_like(l), l))) * v64
    n = max(int(has.sum()), 1)
    share = lambda ref: float(((g64 == ref) & has).sum()) / n   # noqa: E731
    s_exact, s_kept, s_flushed = share(exact), share(kept), share(flushed)
    held = has & (kept == exact)                                # the three limbs hold all of x
    s_held = float(((g64 == exact) & held).sum()) / max(int(held.sum()), 1)
    print('  %-28s %d outputs, %d with a subnormal input limb: max |got - x w| = 2^%.1f (bound 2^-124); of those bit-exact %.4f (%.4f of the '
          '%d whose limbs hold all of x), = limbs kept %.4f, = subnormal limbs flushed %.4f'
          % (what, has.numel(), int(has.sum()), torch.log2(torch.tensor(max(err, 2.0 ** -200))).item(), s_exact, s_held, int(held.sum()), s_kept,
             s_flushed))
    assert int(has.sum()) >= 256, 'the inputs do not reach subnormal limbs'
    assert err <= TINY_BOUND, (what, err)
    return s_exact, s_kept, s_flushed


def test_subnormal_limbs_are_measured(device):
    """k_conv3x3_t on inputs whose m / l limbs are bf16 subnormals (see _subnormal_report): a measurement of whether the bf16 matrix
    pipe keeps them (recorded in DESIGN.md 2a-ter), asserted only to the bound that holds either way."""
    dev = device
    cin, cp, ho, wo = ONE_HOT[0]
    dd = conv_case('subnormal limbs', 'f32', 2, ho, wo, cin, cp, scale=False, shift=False, relu=False).desc
    gen = torch.Generator(device=dev)
    gen.manual_seed(24)
    inp = _patterned_tiny((2, dd['in_hp'], dd['in_wp'], cin), gen, dev)
    w, tap, ci, val = _one_hot_weights(cin, cp, torch.tensor([1.0, -1.0, 0.5, 2.0, -2.0]), gen, dev)
    got = _run(dd, inp, w, None, None, 'bf16x3', dev, twice=False)
    xsel = _expect_one_hot(inp, dd, tap, ci, torch.ones_like(val))
    _subnormal_report('k_conv3x3_t %d->%d' % (cin, cp), got, xsel, val)


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
REFUSED = [dict(kh=1), dict(kw=1), dict(stride=2), dict(groups=2), dict(cin=48), dict(cout_pad=32), dict(phase_groups=1), dict(in_rowidx=True),
           dict(in_tiles=True), dict(group_shift=True), dict(group_max=1), dict(batch=4096, in_hp=192, in_wp=192)]


@pytest.mark.parametrize('field', REFUSED, ids=[' '.join('%s=%s' % kv for kv in f.items()) for f in REFUSED])
def test_refusals_leave_the_output_untouched(device, field):
    dev = device
    dd = dict(conv_case('refused', 'f32', 1, 9, 13, 64, 64).desc)
    inp = torch.zeros((1, dd['in_hp'], dd['in_wp'], dd['in_cstride']), device=dev)
    wk = torch.zeros((9, 64, 96), device=dev)
    aux = torch.zeros(4096, dtype=torch.int32, device=dev)
    out = torch.full((dd['out_hp'] * dd['out_wp'] * dd['out_cstride'],), SENTINEL, dtype=torch.int32, device=dev)
    ptrs = dict(inp=inp.data_ptr(), out=out.data_ptr(), w=wk.data_ptr())
    d = _cdesc(dd, ptrs)
    for k, v in field.items():
        setattr(d, k, aux.data_ptr() if v is True else v)
    lib = L.load()
    assert lib.dz_conv3x3_limb3_supported(ctypes.byref(d)) == 0
    assert lib.dz_conv3x3_limb3_variant(ctypes.byref(d)) == b'none'
    rc = lib.dz_conv3x3_limb3_forward(ctypes.byref(d), L.stream())
    torch.cuda.synchronize(dev)
    assert rc == L.ERR_UNSUPPORTED, (field, rc)
    assert bool((out == SENTINEL).all()), field
