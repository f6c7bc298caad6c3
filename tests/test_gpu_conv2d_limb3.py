"""The generic three-limb (bf16x3) engine of the f32 mode's dense layers (csrc/conv2d_t.hip, dz_conv2d_limb3_forward) on the GPU.

Float64 cases: the normalised error, bound and sentinel discipline of tests/test_gpu_dense_conv.py (|got - ref| / (|scale| * sum|x.w| +
|shift|) <= 2^-19, the f32 engine's bound; every word outside the region the descriptor names keeps the sentinel; two launches give
the same bits), per kernel instance at every edge of the skeleton: the row count around one tile, a ragged tile across two frames,
3 x 3 stride 2 on odd and even input extents, the deblock mappings (1 x 1 with in_off 1 into a channel slice of a wider image; the
four output-stride-2 phases), the head's grouped 12-column output layer, channel offsets, one and several chunks, 1 - 3 channel
tiles, the identity epilogue, ReLU on and off.  `test_edge_table_is_complete` derives each case's edges from its descriptor and
asserts that every instance meets every edge that exists for it.

Error class: the four production layer classes at their production channels on a crop, k_conv2d_t against k_conv2d on the same
operands (<= 2 x the fp32 engine's error, the rule of the sparse sibling).

Limb-term cases (bit exact; a 2^-19 bound cannot see a dropped h.l term): one product per output - one-hot weights against patterned
24-bit inputs, the ends of the fp32 range, patterned weights against a 3-pixel lattice of inputs, and the m.m term - on a 3 x 3
stride-2 layer, a 1 x 1 phase and the grouped layer (one per instance).

Through the detector (fixture of tests/test_gpu_dense_engine.py): routing with the switch off / alone / with the 3 x 3 engine, the
default path's bits after switching off again, the stage error against float64, boxes and graph replay.
"""
import ctypes

import pytest
import torch

from detzero_amd import lib as L
from detzero_amd import ops
from tests.test_gpu_conv3x3_limb3 import _patterned, _patterned_tiny, _pow2, _subnormal_report
from tests.test_gpu_dense_conv import BOUND, SENTINEL, _cdesc, conv_case, conv_ref, production_cases
from tests.test_gpu_dense_engine import BOX_TOL_F32, _bev, _boxes, _dense_stage, _dense_stage_f64, small  # noqa: F401  (small: fixture)
from tests.util import match_boxes

BP = 128
FP32_MAX = 3.4028234663852886e38
INST = {
    'A': dict(name='k_conv2d_t<128x128x16>', bc=128, kc=16, cps=(128, 256, 384)),
    'B': dict(name='k_conv2d_t<128x64x32>', bc=64, kc=32, cps=(64, 96, 192)),
    'C': dict(name='k_conv2d_t<128x32x32>', bc=32, kc=32, cps=(32, 32, 32)),
}
HEAD_GC, HEAD_OOFF = [2, 1, 3, 2, 1, 3], [0, 2, 3, 6, 8, 9]


def _phase(case, py, px):
    """The output mapping of phase (py, px) of a ConvTranspose2d with kernel == stride == 2 into the zero-bordered full-size image."""
    d = case.desc
    d.update(out_sy=2, out_sx=2, out_hp=2 * d['ho'] + 2, out_wp=2 * d['wo'] + 2, out_dy=1 + py, out_dx=1 + px)
    return case


def _exact_fit(case):
    """A stride-2 layer whose last tap is the image's last row / column: odd input extents (conv_case leaves one more: even)."""
    case.desc.update(in_hp=case.desc['in_hp'] - 1, in_wp=case.desc['in_wp'] - 1)
    return case


def _head_case(label, cp=16, **kw):
    return conv_case(label, 'f32', 2, 9, 13, 64, cp, groups=6, g_cout=HEAD_GC, g_ooff=HEAD_OOFF, out_pad=0, out_f32=True, relu=False,
                     scale=False, **kw)


def _edge_cases():
    cs = []
    for key, inst in INST.items():
        c1, c2, c3 = inst['cps']
        c = lambda label, *a, **k: conv_case('%s %s' % (key, label), 'f32', *a, expect=inst['name'], **k)      # noqa: E731
        cs += [
            c('m=1 1x1', 1, 1, 1, 64, c1, k=1),
            c('m=127 3x3', 1, 1, 127, 64, c1),
            c('m=128 3x3', 1, 8, 16, 64, c1),
            c('m=129 1x1', 1, 3, 43, 64, c1, k=1),
            c('ragged two frames in_coff', 2, 9, 13, 64, c1, in_coff=32, in_cextra=32),
            c('s2 even extents min cin', 1, 11, 15, 32, c1, s=2),
            _exact_fit(c('s2 odd extents 3 chunks+', 2, 12, 16, 96, c2, s=2)),
            c('deblock1 1x1 in_off 1 out_coff', 2, 9, 13, 64, c1, k=1, out_coff=c1, out_cextra=32),
            _phase(c('phase 00', 1, 9, 13, 64, c1, k=1), 0, 0),
            _phase(c('phase 01 no scale/shift', 1, 9, 13, 64, c1, k=1, scale=False, shift=False), 0, 1),
            _phase(c('phase 10 relu off', 1, 9, 13, 64, c1, k=1, relu=False, out_coff=64, out_cextra=64), 1, 0),
            _phase(c('phase 11', 2, 9, 13, 128, c3, k=1), 1, 1),
        ]
    cs += [_head_case('C grouped head 6x64->12', expect=INST['C']['name']),
           _head_case('C grouped head cout_pad 32 with shift off', cp=32, shift=False, expect=INST['C']['name'])]
    return cs


EDGE_CASES = _edge_cases()


def _edges(case):
    """The edges a case meets, from its descriptor alone."""
    d = case.desc
    inst = next(i for i in INST.values() if i['name'] == case.expect)
    m = d['batch'] * d['ho'] * d['wo']
    tags = {'relu %d' % d['relu'], 'ntiles %d' % -(-(-(-d['cout_pad'] // 32) * 32) // inst['bc'])}
    for n, t in ((1, 'm=1'), (BP - 1, 'm=BP-1'), (BP, 'm=BP'), (BP + 1, 'm=BP+1')):
        if m == n:
            tags.add(t)
    if d['batch'] == 2 and m > BP and m % BP and (d['ho'] * d['wo']) % BP:
        tags.add('ragged two frames')
    if d['kh'] == 3 and d['stride'] == 2:
        tags.add('s2 %s' % ('odd' if d['in_hp'] % 2 and d['in_wp'] % 2 else 'even'))
        assert (d['in_hp'] % 2) == (d['in_wp'] % 2)
    gc_span = max(o + c for o, c in zip(d['g_ooff'], d['g_cout']))
    if d['kh'] == 1 and d['in_off'] == 1 and d['out_sy'] == 1 and d['out_coff'] > 0 and d['out_cstride'] > d['out_coff'] + gc_span:
        tags.add('deblock1')
    if d['kh'] == 1 and d['in_off'] == 1 and d['out_sy'] == 2 and d['out_sx'] == 2:
        tags.add('phase %d%d' % (d['out_dy'] - 1, d['out_dx'] - 1))
    if d['groups'] == 6 and d['cin'] == 64 and d['in_cstride'] == 384 and d['out_cstride'] == 12 and d['g_cout'] == HEAD_GC and not case.scale \
            and not d['relu'] and d['out_dy'] == 0:
        tags.add('grouped head' if d['cout_pad'] == 16 else 'grouped head cout_pad 32')
    if d['in_coff'] != 0 and d['in_cstride'] > d['in_coff'] + d['groups'] * d['cin']:
        tags.add('in_coff')
    if d['cin'] == 32:
        tags.add('min cin')               # one 32-channel chunk; two chunks at KC = 16, whose instance has no one-chunk layer (cin % 32 == 0)
    if d['cin'] // inst['kc'] >= 3:
        tags.add('several chunks')
    if not case.scale and not case.shift:
        tags.add('no scale/shift')
    return tags


COMMON = {'m=1', 'm=BP-1', 'm=BP', 'm=BP+1', 'ragged two frames', 's2 even', 's2 odd', 'deblock1', 'phase 00', 'phase 01', 'phase 10',
          'phase 11', 'in_coff', 'min cin', 'several chunks', 'no scale/shift', 'relu 0', 'relu 1', 'ntiles 1'}
REQUIRED = {'A': COMMON | {'ntiles 2', 'ntiles 3'}, 'B': COMMON | {'ntiles 2', 'ntiles 3'},
            'C': COMMON | {'grouped head', 'grouped head cout_pad 32'}}      # (cout_pad 16 / 32: one channel tile is all there is)


def test_edge_table_is_complete():
    """Host only: every case runs on the instance it names, and every instance meets every edge that exists for it."""
    lib = L.load()
    reached = {k: set() for k in INST}
    for case in EDGE_CASES:
        d = _cdesc(case.desc)
        assert lib.dz_conv2d_limb3_supported(ctypes.byref(d)) == 1, case.label
        assert lib.dz_conv2d_limb3_variant(ctypes.byref(d)).decode() == case.expect, case.label
        key = next(k for k, i in INST.items() if i['name'] == case.expect)
        assert case.label.startswith(key + ' ')
        reached[key] |= _edges(case)
    for key in INST:
        assert REQUIRED[key] <= reached[key], (key, sorted(REQUIRED[key] - reached[key]))


# ------------------------------------------------------------------------------------------------------------------------
# launches and references
# ------------------------------------------------------------------------------------------------------------------------
def _launch(dd, ptrs, engine):
    lib = L.load()
    d = _cdesc(dd, ptrs)
    fn = lib.dz_conv2d_limb3_forward if engine == 'bf16x3' else lib.dz_conv2d_forward
    rc = fn(ctypes.byref(d), L.stream())
    msg = lib.dz_last_error()
    return rc, (msg.decode() if msg else '')


def _regions(dd):
    """Per group: the slices of the (batch, out_hp, out_wp, out_cstride) buffer the descriptor names."""
    ys = slice(dd['out_dy'], dd['out_dy'] + (dd['ho'] - 1) * dd['out_sy'] + 1, dd['out_sy'])
    xs = slice(dd['out_dx'], dd['out_dx'] + (dd['wo'] - 1) * dd['out_sx'] + 1, dd['out_sx'])
    return [(slice(None), ys, xs, slice(dd['out_coff'] + dd['g_ooff'][g], dd['out_coff'] + dd['g_ooff'][g] + dd['g_cout'][g]))
            for g in range(dd['groups'])]


def _run(dd, inp, w32, sc, sh, engine, dev, twice=True):
    """Launch into sentinel-filled buffers (twice: same bits); nothing outside the descriptor's regions may be written.  w32: (groups,
    taps, cin, cout_pad).  Returns the written regions as fp32, one (batch, ho, wo, g_cout) tensor per group."""
    wk = ops.pack_weight_limb3_generic(w32) if engine == 'bf16x3' else w32.contiguous()
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
    for r in _regions(dd):
        touched[r] = True
    bad = (out != SENTINEL) & ~touched
    assert not bool(bad.any()), ('%d words written outside the output region, first at (b, y, x, channel) = %s' % (
        int(bad.sum()), torch.nonzero(bad)[0].tolist()), engine)
    return [out[r].contiguous().view(torch.float32) for r in _regions(dd)]


def _window(dd, inp, g):
    """The input pixels and channels group g reads: (batch, rows, cols, cin)."""
    k, s, off = dd['kh'], dd['stride'], dd['in_off']
    c0 = dd['in_coff'] + g * dd['cin']
    return inp[:, off:off + (dd['ho'] - 1) * s + k, off:off + (dd['wo'] - 1) * s + k, c0:c0 + dd['cin']]


def _operands(case, dev, seed=11):
    dd = case.desc
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    taps, cin, cp, groups = dd['kh'] * dd['kw'], dd['cin'], dd['cout_pad'], dd['groups']
    inp = torch.randn((dd['batch'], dd['in_hp'], dd['in_wp'], dd['in_cstride']), generator=gen, device=dev)
    w32 = torch.randn((groups, taps, cin, cp), generator=gen, device=dev)
    sc = (torch.rand(groups * cp, generator=gen, device=dev) + 0.5) / (taps * cin) ** 0.5 if case.scale else None
    sh = torch.randn(groups * cp, generator=gen, device=dev) * 0.5 if case.shift else None
    return inp, w32, sc, sh


def _reference(dd, inp, w32, sc, sh, on_device=False):
    """Per group (ref, den) in float64 on the operands as given, (batch, ho, wo, g_cout) on the device."""
    dev = inp.device
    k, cin, cp = dd['kh'], dd['cin'], dd['cout_pad']
    res = []
    for g in range(dd['groups']):
        x = _window(dd, inp, g).double()
        w = w32[g].double().view(k, k, cin, cp)
        if not on_device:
            x, w = x.cpu(), w.cpu()
        acc, aacc = conv_ref(x, w, dd['stride'], dd['ho'], dd['wo'])
        gc = dd['g_cout'][g]
        acc, aacc = acc[..., :gc].to(dev), aacc[..., :gc].to(dev)
        scv = sc[g * cp:g * cp + gc].double() if sc is not None else torch.ones(gc, dtype=torch.float64, device=dev)
        shv = sh[g * cp:g * cp + gc].double() if sh is not None else torch.zeros(gc, dtype=torch.float64, device=dev)
        ref = acc * scv + shv
        if dd['relu']:
            ref = ref.clamp_min(0.0)
        res.append((ref, (aacc * scv.abs() + shv.abs()).clamp_min(1e-30)))
    return res


def _worst(gots, refs):
    worst = 0.0
    for got, (ref, den) in zip(gots, refs):
        err = (got.double() - ref).abs() / den
        err = torch.where(torch.isnan(got), torch.full_like(err, float('inf')), err)
        worst = max(worst, float(err.max()))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('case', EDGE_CASES, ids=[c.label for c in EDGE_CASES])
def test_edges_against_float64(device, case):
    dev, dd = device, case.desc
    lib = L.load()
    assert lib.dz_conv2d_limb3_variant(ctypes.byref(_cdesc(dd))).decode() == case.expect
    inp, w32, sc, sh = _operands(case, dev)
    refs = _reference(dd, inp, w32, sc, sh)
    worst = {e: _worst(_run(dd, inp, w32, sc, sh, e, dev), refs) for e in ('bf16x3', 'mfma32')}
    print('  %-44s %-24s normalised error: bf16x3 %.3e (%.2f x 2^-24)   f32 engine %.3e (%.2f x 2^-24)   bound %.1e' % (
        case.label, case.expect, worst['bf16x3'], worst['bf16x3'] * 2 ** 24, worst['mfma32'], worst['mfma32'] * 2 ** 24, BOUND['f32']))
    assert worst['bf16x3'] <= BOUND['f32'], (case.label, worst)
    assert worst['mfma32'] <= BOUND['f32'], (case.label, worst)


@pytest.mark.gpu
def test_four_phases_fill_one_interleaved_image(device):
    """The four phase launches of a ConvTranspose2d (kernel == stride == 2) into ONE image: its interior is written exactly once, the
    border keeps the sentinel, and the whole is the float64 transposed convolution."""
    dev = device
    b, h, w, cin, cout = 2, 9, 13, 64, 128
    gen = torch.Generator(device=dev).manual_seed(12)
    x = torch.randn((b, h + 2, w + 2, cin), generator=gen, device=dev)
    wt = torch.randn((cin, cout, 2, 2), generator=gen, device=dev)
    sc = (torch.rand(cout, generator=gen, device=dev) + 0.5) / cin ** 0.5
    sh = torch.randn(cout, generator=gen, device=dev) * 0.5
    out = torch.full((b, 2 * h + 2, 2 * w + 2, cout), SENTINEL, dtype=torch.int32, device=dev)
    packs = []
    for py in range(2):
        for px in range(2):
            dd = _phase(conv_case('phase', 'f32', b, h, w, cin, cout, k=1), py, px).desc
            dd.update(in_hp=h + 2, in_wp=w + 2)                 # (the level's image with its whole border, as the detector holds it)
            wk = ops.pack_weight_limb3_generic(wt[:, :, py, px].contiguous().view(1, 1, cin, cout))
            packs.append(wk)
            rc, msg = _launch(dd, dict(inp=x.data_ptr(), out=out.data_ptr(), w=wk.data_ptr(), scale=sc.data_ptr(), shift=sh.data_ptr()), 'bf16x3')
            assert rc == 0, (rc, msg)
    torch.cuda.synchronize(dev)
    border = out.clone()
    border[:, 1:-1, 1:-1, :] = SENTINEL
    assert bool((border == SENTINEL).all()), 'a phase wrote into the zero border'
    xd, wd = x[:, 1:-1, 1:-1, :].double().cpu().permute(0, 3, 1, 2), wt.double().cpu()
    ref = torch.nn.functional.conv_transpose2d(xd, wd, stride=2).permute(0, 2, 3, 1)
    den = torch.nn.functional.conv_transpose2d(xd.abs(), wd.abs(), stride=2).permute(0, 2, 3, 1)
    scd, shd = sc.double().cpu(), sh.double().cpu()
    ref, den = (ref * scd + shd).clamp_min(0.0), den * scd + shd.abs()
    got = out[:, 1:-1, 1:-1, :].contiguous().view(torch.float32).double().cpu()
    err = float(((got - ref).abs() / den).max())
    print('  four phases into one image vs float64 conv_transpose2d: worst normalised error %.3e' % err)
    assert err <= BOUND['f32'], err


# ------------------------------------------------------------------------------------------------------------------------
# error class against k_conv2d on the production layers
# ------------------------------------------------------------------------------------------------------------------------
def _production_classes():
    """One case per class the 3 x 3 stride-1 engine refuses (strided, deblock 1, a deblock-2 phase, the grouped output layer), with the
    production channels, cropped to 47 x 47 output pixels (2209 rows) of one frame."""
    lib = L.load()
    picked = {}
    for c in production_cases('f32', 'single'):
        d = c.desc
        if lib.dz_conv3x3_limb3_supported(ctypes.byref(_cdesc(d))):
            continue
        kind = 'strided' if d['stride'] == 2 else 'grouped' if d['groups'] > 1 else 'deblock2' if d['out_sy'] == 2 else 'deblock1'
        if kind in picked:
            continue
        n, dd = 47, dict(d)
        ext = d['in_off'] + (n - 1) * d['stride'] + d['kh'] + 1
        dd.update(batch=1, ho=n, wo=n, in_hp=ext, in_wp=ext, out_hp=(n - 1) * d['out_sy'] + d['out_dy'] + 2,
                  out_wp=(n - 1) * d['out_sx'] + d['out_dx'] + 2, g_cout=list(d['g_cout'])[:d['groups']], g_ooff=list(d['g_ooff'])[:d['groups']])
        picked[kind] = type(c)(label='%s (%s)' % (kind, c.label), desc=dd, scale=c.scale, shift=c.shift)
    return picked


def test_production_classes_are_the_four():
    p = _production_classes()
    assert sorted(p) == ['deblock1', 'deblock2', 'grouped', 'strided'], sorted(p)
    assert (p['strided'].desc['cin'], p['strided'].desc['cout_pad']) == (128, 256) and p['deblock2'].desc['cin'] == 256
    assert p['grouped'].desc['cout_pad'] == 16 and p['grouped'].desc['out_cstride'] == 12 and not p['grouped'].scale


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['strided', 'deblock1', 'deblock2', 'grouped'])
def test_error_class_vs_k_conv2d(device, kind):
    dev = device
    case = _production_classes()[kind]
    dd = case.desc
    inp, w32, sc, sh = _operands(case, dev, seed=13)
    refs = _reference(dd, inp, w32, sc, sh, on_device=True)
    et = _worst(_run(dd, inp, w32, sc, sh, 'bf16x3', dev), refs)
    ec = _worst(_run(dd, inp, w32, sc, sh, 'mfma32', dev), refs)
    name = L.load().dz_conv2d_limb3_variant(ctypes.byref(_cdesc(dd))).decode()
    print('  %-70s %-24s k_conv2d_t %.3e (%.2f x 2^-24)   k_conv2d %.3e (%.2f x 2^-24)   ratio %.2f' % (
        case.label, name, et, et * 2 ** 24, ec, ec * 2 ** 24, et / max(ec, 1e-30)))
    assert ec > 0
    assert et <= BOUND['f32'], (kind, et)
    assert et <= 2.0 * ec, (kind, et, ec)


# ------------------------------------------------------------------------------------------------------------------------
# limb-term cases: one product per output, bit exact
# ------------------------------------------------------------------------------------------------------------------------
def _limb_cases():
    off = dict(scale=False, shift=False, relu=False)
    return [conv_case('3x3 stride 2', 'f32', 2, 9, 13, 64, 128, s=2, expect=INST['A']['name'], **off),
            _phase(conv_case('1x1 phase 10', 'f32', 2, 9, 13, 64, 64, k=1, expect=INST['B']['name'], **off), 1, 0),
            _head_case('grouped head', shift=False, expect=INST['C']['name'])]


LIMB_CASES = _limb_cases()
LIMB_IDS = [c.label for c in LIMB_CASES]
ONE_HOT_VALUES = (1.0, -1.0, 0.5, 2.0, -2.0)


def _combos(dd):
    """(tap, channel) pairs to cover: every tap x the first and last channel of every 8-channel group (one LDS limb group)."""
    return [(t, c) for t in range(dd['kh'] * dd['kw']) for g8 in range(dd['cin'] // 8) for c in (8 * g8, 8 * g8 + 7)]


def _one_hot(dd, launch, values, dev):
    """(groups, taps, cin, cout_pad) weights with ONE non-zero (tap, cin) entry per live output channel: channel number n of launch
    number `launch` takes pair (launch * n_out + n) % len(combos), value values[(launch + n) % len(values)].
    Returns (w, [(group, column, tap, ci, value)])."""
    combos = _combos(dd)
    nout = sum(dd['g_cout'])
    w = torch.zeros((dd['groups'], dd['kh'] * dd['kw'], dd['cin'], dd['cout_pad']), dtype=torch.float32)
    sel, n = [], 0
    for g in range(dd['groups']):
        for o in range(dd['g_cout'][g]):
            t, c = combos[(launch * nout + n) % len(combos)]
            v = float(values[(launch + n) % len(values)])
            w[g, t, c, o] = v
            sel.append((g, o, t, c, v))
            n += 1
    return w.to(dev), sel


def _expect_one_hot(inp, dd, sel, unit=False):
    """Per group the products in[window of (ky, kx), ci] * value as fp32 (exact there by construction; checked); unit: value 1."""
    k, s, ho, wo = dd['kh'], dd['stride'], dd['ho'], dd['wo']
    out = [torch.empty((dd['batch'], ho, wo, dd['g_cout'][g]), dtype=torch.float32, device=inp.device) for g in range(dd['groups'])]
    for g, o, t, c, v in sel:
        ky, kx = t // k, t % k
        xs = _window(dd, inp, g)[:, ky:ky + (ho - 1) * s + 1:s, kx:kx + (wo - 1) * s + 1:s, c].double()
        e64 = xs if unit else xs * v
        e32 = e64.float()
        assert torch.equal(e32.double(), e64)
        out[g][..., o] = e32
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same_bits(gots, exps, what):
    for g, (got, exp) in enumerate(zip(gots, exps)):
        diff = _bits(got) != _bits(exp)
        if bool(diff.any()):
            i = torch.nonzero(diff)[0].tolist()
            raise AssertionError('%s, group %d: %d of %d outputs differ in bits, first at (b, y, x, channel) = %s: got %r, expected %r' % (
                what, g, int(diff.sum()), diff.numel(), i, float(got[tuple(i)]), float(exp[tuple(i)])))


def test_one_hot_launches_cover_every_tap_and_group_edge():
    """Host only: over its launches every limb case reaches every (tap, first / last channel of an 8-channel group) pair and every value."""
    for case in LIMB_CASES:
        dd = case.desc
        combos, nout = _combos(dd), sum(dd['g_cout'])
        seen, vals = set(), set()
        for launch in range(-(-len(combos) // nout)):
            for g, o, t, c, v in _one_hot(dd, launch, ONE_HOT_VALUES, 'cpu')[1]:
                seen.add((t, c))
                vals.add(v)
        assert seen == set(combos), (case.label, len(seen), len(combos))
        assert vals == set(ONE_HOT_VALUES) or nout * -(-len(combos) // nout) < len(ONE_HOT_VALUES), case.label


@pytest.mark.gpu
@pytest.mark.parametrize('case', LIMB_CASES, ids=LIMB_IDS)
def test_input_limbs_bit_exact(device, case):
    dev, dd = device, case.desc
    assert L.load().dz_conv2d_limb3_variant(ctypes.byref(_cdesc(dd))).decode() == case.expect
    gen = torch.Generator(device=dev)
    gen.manual_seed(21)
    inp = _patterned((dd['batch'], dd['in_hp'], dd['in_wp'], dd['in_cstride']), gen, dev)
    for launch in range(-(-len(_combos(dd)) // sum(dd['g_cout']))):
        w, sel = _one_hot(dd, launch, ONE_HOT_VALUES, dev)
        got = _run(dd, inp, w, None, None, 'bf16x3', dev, twice=False)
        _assert_same_bits(got, _expect_one_hot(inp, dd, sel), 'input limbs, %s, launch %d' % (case.label, launch))


@pytest.mark.gpu
@pytest.mark.parametrize('case', LIMB_CASES, ids=LIMB_IDS)
def test_range_ends_bit_exact(device, case):
    """+-fp32-max (no inf limb: the clamp before the first rounding), 1 + 2^-23 and 2 - 2^-23 (all 24 bits set) against weight 1."""
    dev, dd = device, case.desc
    shp = (dd['batch'], dd['in_hp'], dd['in_wp'], dd['in_cstride'])
    special = torch.tensor([FP32_MAX, -FP32_MAX, 1 + 2.0 ** -23, 2 - 2.0 ** -23], dtype=torch.float32, device=dev)
    n = shp[0] * shp[1] * shp[2] * shp[3]
    inp = special[(torch.arange(n, device=dev) * 7 + torch.arange(n, device=dev) // 5) % 4].view(shp)
    w, sel = _one_hot(dd, 0, (1.0,), dev)
    got = _run(dd, inp, w, None, None, 'bf16x3', dev, twice=False)
    exp = _expect_one_hot(inp, dd, sel)
    assert all(bool((e.abs() == FP32_MAX).any()) and bool((e == 1 + 2.0 ** -23).any()) and bool((e == 2 - 2.0 ** -23).any()) for e in exp)
    _assert_same_bits(got, exp, 'range ends, %s' % case.label)


@pytest.mark.gpu
@pytest.mark.parametrize('case', LIMB_CASES, ids=LIMB_IDS)
def test_weight_limbs_bit_exact(device, case):
    """Patterned 24-bit weights; the input is non-zero on the pixels whose unpadded (y, x) are both multiples of 3 - in ONE channel of
    every group's slice, value +-1, 0.5 or 2 - so a 3 x 3 window holds at most one such pixel and an output is one product or none.
    One-product outputs equal the product bit for bit, the others are +0.  The one-product outputs are counted: for the 3 x 3 layers at
    least every output whose window lies wholly inside the unpadded image, for the 1 x 1 layer exactly the lattice pixels; every tap
    is behind some one-product output."""
    dev, dd = device, case.desc
    gen = torch.Generator(device=dev)
    gen.manual_seed(22)
    k, s, ho, wo, cin, cp, groups = dd['kh'], dd['stride'], dd['ho'], dd['wo'], dd['cin'], dd['cout_pad'], dd['groups']
    hp, wp = dd['in_hp'], dd['in_wp']
    w = _patterned((groups, k * k, cin, cp), gen, dev)
    vals = torch.tensor([1.0, -1.0, 0.5, 2.0], device=dev)
    yy, xx = torch.meshgrid(torch.arange(hp, device=dev), torch.arange(wp, device=dev), indexing='ij')
    inside = (yy >= 1) & (yy <= hp - 2) & (xx >= 1) & (xx <= wp - 2)                 # the unpadded image: one border pixel all around
    on = inside & ((yy - 1) % 3 == 0) & ((xx - 1) % 3 == 0)
    inp = torch.zeros((dd['batch'], hp, wp, dd['in_cstride']), device=dev)
    edge = torch.tensor([c for g8 in range(cin // 8) for c in (8 * g8, 8 * g8 + 7)], device=dev)
    for g in range(groups):
        chan = dd['in_coff'] + g * cin + edge[torch.randint(0, edge.numel(), (dd['batch'], hp, wp), generator=gen, device=dev)]
        pv = vals[torch.randint(0, 4, (dd['batch'], hp, wp), generator=gen, device=dev)] * on
        inp.scatter_(3, chan.unsqueeze(-1), pv.unsqueeze(-1))
    got = _run(dd, inp, w, None, None, 'bf16x3', dev, twice=False)
    # which tap a window's lattice pixel sits on, and which windows lie wholly inside: a one-channel float64 convolution of the masks
    tapw = (torch.arange(k * k, dtype=torch.float64) + 1).view(k, k, 1, 1)
    geo = lambda m, wt: conv_ref(_window(dd, m.double().view(1, hp, wp, 1).expand(1, hp, wp, dd['in_cstride']).cpu(), 0)[..., :1], wt, s, ho, wo)[0][0, :, :, 0]   # noqa: E731
    npix = geo(on, torch.ones(k, k, 1, 1, dtype=torch.float64))
    tap_of = geo(on, tapw)
    whole = geo(inside, torch.ones(k, k, 1, 1, dtype=torch.float64)) == k * k
    assert float(npix.max()) == 1.0
    assert set(int(t) - 1 for t in tap_of[npix == 1].tolist()) == set(range(k * k)), 'the lattice does not reach every tap'
    if k == 3:
        assert bool((npix[whole] == 1).all()) and int(whole.sum()) > 0
    for g in range(groups):
        x64 = _window(dd, inp, g).double().cpu()
        acc, _ = conv_ref(x64, w[g].double().cpu().view(k, k, cin, cp), s, ho, wo)
        cnt, _ = conv_ref((x64 != 0).double(), torch.ones(k, k, cin, cp, dtype=torch.float64), s, ho, wo)
        gc = dd['g_cout'][g]
        acc, cnt = acc[..., :gc].to(dev), cnt[..., :gc].to(dev)
        exp = acc.float()
        assert torch.equal(exp.double(), acc) and float(cnt.max()) == 1.0
        one = cnt == 1
        assert bool((exp[one] != 0).all()) and bool((exp[~one] == 0).all())
        n_one = int(one[..., 0].sum())
        assert n_one == dd['batch'] * int((npix == 1).sum()) and n_one >= dd['batch'] * (int(whole.sum()) if k == 3 else int(on.sum())), (n_one, g)
        exp = torch.where(one, exp, torch.zeros_like(exp))                              # none: +0
        _assert_same_bits([got[g]], [exp], 'weight limbs, %s, group %d (%d one-product outputs per channel)' % (case.label, g, n_one))


@pytest.mark.gpu
@pytest.mark.parametrize('case', LIMB_CASES, ids=LIMB_IDS)
def test_mm_term_bit_exact(device, case):
    """x = (1 + 2^-10) 2^a against w = (1 + 2^-10) 2^b: the product (1 + 2^-9 + 2^-20) 2^(a + b) is exact in fp32 and 2^-20 off without m.m."""
    dev, dd = device, case.desc
    gen = torch.Generator(device=dev)
    gen.manual_seed(23)
    shp = (dd['batch'], dd['in_hp'], dd['in_wp'], dd['in_cstride'])
    inp = (1 + 2.0 ** -10) * _pow2(torch.randint(-20, 21, shp, generator=gen, device=dev))
    wv = ((1 + 2.0 ** -10) * _pow2(torch.randint(-20, 21, (7,)))).tolist()
    w, sel = _one_hot(dd, 0, wv, dev)
    got = _run(dd, inp, w, None, None, 'bf16x3', dev, twice=False)
    exp = _expect_one_hot(inp, dd, sel)
    for e in exp:
        mant = torch.frexp(e)[0] * 2
        assert torch.equal(mant, torch.full_like(mant, 1 + 2.0 ** -9 + 2.0 ** -20))
    _assert_same_bits(got, exp, 'm.m, %s' % case.label)


@pytest.mark.gpu
def test_subnormal_limbs_are_measured(device):
    """k_conv2d_t on inputs whose m / l limbs are bf16 subnormals (exponent [-120, -104], the sibling test's inputs) against one-hot
    weights +-1, 0.5, +-2: asserted to 2^-124, what holds whether or not the matrix pipe flushes them; the kept / flushed shares are
    printed."""
    dev = device
    case = LIMB_CASES[0]
    dd = case.desc
    gen = torch.Generator(device=dev)
    gen.manual_seed(24)
    inp = _patterned_tiny((dd['batch'], dd['in_hp'], dd['in_wp'], dd['in_cstride']), gen, dev)
    w, sel = _one_hot(dd, 0, ONE_HOT_VALUES, dev)
    got = _run(dd, inp, w, None, None, 'bf16x3', dev, twice=False)
    xsel = _expect_one_hot(inp, dd, sel, unit=True)
    val = torch.tensor([v for *_, v in sel], device=dev)
    _subnormal_report('k_conv2d_t %s' % case.label, got[0], xsel[0], val)


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
REFUSED = [(dict(group_shift=True), 'group_shift'), (dict(group_max=1), 'group_max'), (dict(phase_groups=1), 'phase_groups'),
           (dict(in_rowidx=True), 'in_rowidx'), (dict(in_tiles=True), 'in_tiles'), (dict(batch=4096, in_hp=192, in_wp=192), '2 GiB'),
           (dict(cin=48), 'cin'), (dict(cout_pad=24), 'cout_pad'), (dict(kh=5, kw=5), 'kh'), (dict(kw=1), 'kh'), (dict(stride=3), 'stride'),
           (dict(groups=9), 'groups')]


@pytest.mark.gpu
@pytest.mark.parametrize('field,word', REFUSED, ids=[' '.join('%s=%s' % kv for kv in f.items()) for f, _ in REFUSED])
def test_refusals_leave_the_output_untouched(device, field, word):
    """ops.conv2d(..., f32_generic='bf16x3') on a layer the engine does not cover: DetZeroHipError naming the field, before any launch."""
    dev = device
    dd = dict(conv_case('refused', 'f32', 1, 9, 13, 64, 64, s=2).desc)
    inp = torch.zeros((1, dd['in_hp'], dd['in_wp'], dd['in_cstride']), device=dev)
    wk = torch.zeros((9, 64, 96), device=dev)
    aux = torch.zeros(4096, dtype=torch.int32, device=dev)
    out = torch.full((dd['out_hp'] * dd['out_wp'] * dd['out_cstride'],), SENTINEL, dtype=torch.int32, device=dev)
    dd.update(inp=inp.data_ptr(), out=out.data_ptr(), w=wk.data_ptr())
    assert ops.conv2d_limb3_supported(dd)
    for k, v in field.items():
        dd[k] = aux.data_ptr() if v is True else v
    assert not ops.conv2d_limb3_supported(dd)
    assert L.load().dz_conv2d_limb3_variant(ctypes.byref(ops._conv2d_desc(dd))) == b'none'
    with pytest.raises(L.DetZeroHipError) as exc:
        ops.conv2d(dd, f32_generic='bf16x3')
    torch.cuda.synchronize(dev)
    assert word in str(exc.value), (field, str(exc.value))
    assert bool((out == SENTINEL).all()), field


@pytest.mark.gpu
def test_split_modes_ignore_the_keyword(device):
    dev = device
    dd = dict(conv_case('split', 'f16x2', 1, 9, 13, 32, 64, k=1).desc)
    gen = torch.Generator(device=dev).manual_seed(14)
    x = ops.pair16_from_f32(torch.randn((1, dd['in_hp'], dd['in_wp'], dd['in_cstride']), generator=gen, device=dev), math=1)
    wk = ops.pack_weight_split(torch.randn((1, 1, 32, 64), generator=gen, device=dev), 1)
    outs = []
    for kw in ({}, {'f32_generic': 'bf16x3'}, {'f32_generic': 'mfma32'}):
        out = torch.full((dd['out_hp'] * dd['out_wp'] * dd['out_cstride'],), SENTINEL, dtype=torch.int32, device=dev)
        ops.conv2d(dict(dd, inp=x.data_ptr(), out=out.data_ptr(), w=wk.data_ptr()), math=1, **kw)
        outs.append(out)
    torch.cuda.synchronize(dev)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and not bool((outs[0] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------
# through the detector
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def engines(small):  # noqa: F811
    """set_dense_engine(model, f32_engine, f32_generic) on the module's model, both back to the default afterwards."""
    from detzero_amd.centerpoint import set_dense_engine, set_math
    model = small[0]
    set_math(model, 'f32')
    set_dense_engine(model, 'mfma32', f32_generic='mfma32')
    yield lambda name, generic: set_dense_engine(model, name, f32_generic=generic)
    set_dense_engine(model, 'mfma32', f32_generic='mfma32')


@pytest.mark.gpu
def test_routing_and_the_default_path(small, device, engines, monkeypatch):  # noqa: F811
    bd = _bev(small, device)
    calls = []
    real = ops.conv2d

    def spy(desc, **kw):
        calls.append((dict(desc), kw.get('f32_engine'), kw.get('f32_generic')))
        return real(desc, **kw)
    monkeypatch.setattr(ops, 'conv2d', spy)

    def profiled():
        del calls[:]
        ops.PROFILER = ops.LaunchProfiler()
        try:
            out = _dense_stage(small, bd)
            names = [r[0] for r in ops.PROFILER.records]
            return list(calls), names, ops.PROFILER.summary(), out
        finally:
            ops.PROFILER = None
    tot = lambda s, key: sum(v[key] for v in s.values())          # noqa: E731

    def same_work(s):
        assert tot(s0, 'launches') == tot(s, 'launches')
        for key in ('flops', 'bytes'):
            assert abs(tot(s0, key) - tot(s, key)) <= 1e-9 * tot(s0, key), key
    # switch off: today's launches
    c0, n0, s0, out0 = profiled()
    assert len(c0) == len(n0) == 20 and all(n.startswith('k_conv2d<') for n in n0) and all(e is None and g is None for _, e, g in c0)
    # the generic engine alone: every layer it covers, and no k_conv3x3_t
    engines('mfma32', 'bf16x3')
    c1, n1, s1, _ = profiled()
    assert len(c1) == len(n1) == len(c0)
    for (desc, eng, gen), name, name0 in zip(c1, n1, n0):
        ok = ops.conv2d_limb3_supported(desc)
        assert eng is None and (gen == 'bf16x3') == ok
        assert name.startswith('k_conv2d_t<') == ok and (ok or name == name0) and not name.startswith('k_conv3x3_t<'), (name, name0, desc)
    assert sum(n.startswith('k_conv2d_t<') for n in n1) == 20
    same_work(s1)
    print('  generic alone:  ' + ', '.join('%s x%d' % (k, v['launches']) for k, v in sorted(s1.items())))
    # both: 13 plain layers on k_conv3x3_t, the other 7 on k_conv2d_t, nothing left on the fp32 matrix pipe
    engines('bf16x3', 'bf16x3')
    c2, n2, s2, _ = profiled()
    assert sum(n.startswith('k_conv3x3_t<') for n in n2) == 13 and sum(n.startswith('k_conv2d_t<') for n in n2) == 7
    assert not any(n.startswith('k_conv2d<') for n in n2) and len(n2) == 20
    for (desc, eng, gen), name in zip(c2, n2):
        assert name.startswith('k_conv3x3_t<') == ops.conv3x3_limb3_supported(desc) == (eng == 'bf16x3'), (name, desc)
    same_work(s2)
    print('  both engines:   ' + ', '.join('%s x%d' % (k, v['launches']) for k, v in sorted(s2.items())))
    # everything off again: the first run's names and bits
    engines('mfma32', 'mfma32')
    c3, n3, s3, out3 = profiled()
    assert n3 == n0 and all(e is None and g is None for _, e, g in c3)
    for k in out0:
        assert torch.equal(out0[k], out3[k]), k


@pytest.mark.gpu
def test_stage_error_against_float64(small, device, engines):  # noqa: F811
    model = small[0]
    bd = _bev(small, device)
    yard = _dense_stage_f64(model, bd['spatial_features'])
    f32 = _dense_stage(small, bd)
    engines('bf16x3', 'bf16x3')
    l3 = _dense_stage(small, bd)
    engines('mfma32', 'mfma32')
    err = lambda t, k: float((t[k].double() - yard[k]).abs().max()) / float(yard[k].std())      # noqa: E731
    print('\n  dense stage, max |error| against float64, in units of the stage standard deviation')
    print('  %-22s %12s %12s %12s' % ('stage', 'f32 engine', 'all bf16x3', 'ratio'))
    for k in yard:
        e32, e3 = err(f32, k), err(l3, k)
        print('  %-22s %12.2e %12.2e %12.2f' % (k, e32, e3, e3 / max(e32, 1e-30)))
    for k in yard:
        e32, e3 = err(f32, k), err(l3, k)
        assert e3 <= 2.0 * e32, (k, e3, e32)


@pytest.mark.gpu
def test_detector_boxes_and_graph_replay(small, device, engines):  # noqa: F811
    """FramePipeline(math='f32') on the 20k-point frame with both engines on: the default's box count, every box within BOX_TOL_F32;
    a captured graph of that pass replays to the eager bits."""
    _, ref, n = _boxes(small, device)
    assert n > 20
    engines('bf16x3', 'bf16x3')
    pipe, got, m = _boxes(small, device)
    a, b = ref[:n].cpu().numpy(), got[:m].cpu().numpy()
    nm, worst = match_boxes(a[:, :7], a[:, 7], b[:, :7], b[:, 7], tol=BOX_TOL_F32)
    print('  boxes: %d default / %d all bf16x3, %d matched within %.0e (worst %.2e)' % (n, m, nm, BOX_TOL_F32, worst))
    assert m == n and nm == n, (n, m, nm, worst)
    static_in = torch.from_numpy(small[3]).to(device)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):
            pipe(static_in)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_out, g_n = pipe(static_in)
    g.replay()
    torch.cuda.synchronize()
    assert int(g_n.item()) == m and torch.equal(g_out[:m], got[:m])
