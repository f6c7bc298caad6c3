"""Every dense-convolution kernel instance against a float64 reference (csrc/conv2d.hip, conv2d_h.hip, conv3x3_h.hip; the bf16x3 engine
of the f32 mode, k_conv3x3_t of csrc/conv3x3_t.hip, has its cases in tests/test_gpu_conv3x3_limb3.py and joins the production replay
here: test_production_layers_on_the_bf16x3_engine).

Which instance runs a layer depends on the launch's size, not only on the layer (conv2d_select, conv2d_h_select and
conv3x3_h_variant score tile counts against the chip), so the cases here are chosen by shape: every case names the variant
the selector must report for it, and `test_case_table_covers_every_variant` checks that the table reaches every shipped
instance in every math mode it is compiled for.  The production layers are taken from the detector itself: the
descriptors BaseBEVBackbone / CenterHead hand to ops.conv2d in FramePipeline.dense_stage, recorded on the meta device.

Reference: float64 on the operands exactly as the kernel sees them (split modes: input and weights decoded from their
pair16 form), small cases with CPU F.conv2d, large ones on the device as one float64 matmul per tap over frame chunks.
Error per output element = |got - ref| / (|scale| * sum|x.w| + |shift|): normalised by the magnitude of what was summed,
so that a dropped tap or K chunk cannot hide under a large output.  Every word of the output buffer outside the region the
descriptor names must keep the sentinel it was filled with, and two launches must give the same bits.
"""
import ctypes
import functools
import types
import zlib

import pytest
import torch
import torch.nn.functional as F

from detzero_amd import lib as L
from detzero_amd import ops

MODES = ('f32', 'f16x2', 'bf16x2', 'f16')
SENTINEL = 0x7FBADBAD          # a NaN as fp32; as two fp16 halves NaN (0x7FBA) and a normal - never a plausible result

# Bounds on the normalised error per math mode, a few times the worst value observed on an MI355X over every case of this
# module (printed by each test; worst seen: f32 5.2e-7, f16x2 2.9e-7, bf16x2 7.8e-6, f16 4.2e-4).
#   f32: fp32 MFMA accumulation of exact fp32 products, 2^-24-class per addition.  Looser than one rounding: the error grows
#        with the length of the sum (up to 9 x 3 x 3 x 512 products), worst seen 8.7 x 2^-24.
#   f16x2: the dropped lo.lo product (2^-22 of |x.w|) plus the pair16 output rounding (2^-22 of the value) and fp32 sums.
#   bf16x2: the same with 8-bit halves: the 2^-16 class.
#   f16: one product on the hi halves while the reference keeps hi + lo: the dropped hi.lo + lo.hi terms, 2^-11 of |x.w| each.
BOUND = {'f32': 2.0 ** -19, 'f16x2': 2.0 ** -20, 'bf16x2': 2.0 ** -15, 'f16': 2.0 ** -9}

ALL_VARIANTS = {
    'f32': {'k_conv2d<64x64x16>', 'k_conv2d<128x16x16>', 'k_conv2d<128x64x32>', 'k_conv2d<96x64x32>', 'k_conv2d<64x64x32>',
            'k_conv2d<48x64x32>', 'k_conv2d<128x32x32>', 'k_conv2d<128x16x32>'},
}
for _m in ('f16x2', 'bf16x2', 'f16'):
    ALL_VARIANTS[_m] = {'k_conv2d_h<128x128x32>', 'k_conv2d_h<128x64x32>', 'k_conv2d_h<64x128x32>', 'k_conv2d_h<64x64x32>',
                        'k_conv2d_h<128x32x32>', 'k_conv3x3_h<8x32x128>', 'k_conv3x3_h<8x32x64>', 'k_conv3x3_h<16x32x32>'}

# ------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------
def conv_case(label, mode, batch, ho, wo, cin, cout_pad, *, k=3, s=1, in_off=None, groups=1, g_cout=None, g_ooff=None,
              in_cextra=0, in_coff=0, out_cextra=0, out_coff=0, out_pad=1, out_f32=False, relu=True, scale=True, shift=True,
              phase=False, tiles=False, sparse=False, expect=None):
    """A dz_conv2d_desc (geometry only) in the layout of the detector: channel-last images, the input read from in_off on,
    the output written at (y * out_s + out_pad, x * out_s + out_pad) inside a border of out_pad pixels."""
    if in_off is None:
        in_off = 1 if k == 1 else 0
    g_cout = list(g_cout or [cout_pad] * groups)
    g_ooff = list(g_ooff or ([0] * groups if phase else [g * cout_pad for g in range(groups)]))
    out_s = 1
    if phase:
        out_s = int(round(groups ** 0.5))
        assert out_s * out_s == groups
    in_groups = 1 if phase else groups
    in_hp = in_off + (ho - 1) * s + k + (1 if s > 1 else 0)
    in_wp = in_off + (wo - 1) * s + k + (1 if s > 1 else 0)
    span = max(o + c for o, c in zip(g_ooff, g_cout))
    desc = dict(batch=batch, ho=ho, wo=wo, in_hp=in_hp, in_wp=in_wp, in_cstride=in_coff + in_groups * cin + in_cextra,
                in_coff=in_coff, cin=cin, kh=k, kw=k, stride=s, in_off=in_off,
                out_hp=ho * out_s + 2 * out_pad, out_wp=wo * out_s + 2 * out_pad, out_cstride=out_coff + span + out_cextra,
                out_coff=out_coff, out_sy=out_s, out_sx=out_s, out_dy=out_pad, out_dx=out_pad, groups=groups, cout_pad=cout_pad,
                g_cout=g_cout, g_ooff=g_ooff, relu=1 if relu else 0, phase_groups=1 if phase else 0)
    return types.SimpleNamespace(label=label, mode=mode, desc=desc, out_f32=out_f32, scale=scale, shift=shift, tiles=tiles,
                                 sparse=sparse, in_rows=0, expect=expect)


def _coverage_cases():
    """One or more cases per (instance, math mode), each also exercising an edge where tiled kernels go wrong."""
    cs = []
    c = conv_case
    # fp32 engine (conv2d.hip): the tile is picked by cin % 32, cout_pad % 64 and the chip-fill score
    cs += [
        c('f32 cin48 ragged 3x3', 'f32', 1, 19, 21, 48, 64, expect='k_conv2d<64x64x16>'),
        c('f32 cin48 grouped g_cout 13/5 in_coff', 'f32', 2, 11, 37, 48, 16, groups=2, g_cout=[13, 5], g_ooff=[0, 13], in_coff=4,
          in_cextra=8, out_coff=3, out_cextra=2, out_pad=0, out_f32=True, relu=False, expect='k_conv2d<128x16x16>'),
        c('f32 1x1 cout192', 'f32', 2, 64, 64, 32, 192, k=1, expect='k_conv2d<128x64x32>'),
        c('f32 1x1 cout256 47x47', 'f32', 2, 47, 47, 32, 256, k=1, expect='k_conv2d<96x64x32>'),
        c('f32 1x1 cout256 40x40 no scale/shift', 'f32', 2, 40, 40, 32, 256, k=1, scale=False, shift=False, expect='k_conv2d<64x64x32>'),
        c('f32 3x3 small out_coff', 'f32', 1, 9, 13, 64, 64, out_coff=64, out_cextra=32, relu=False, expect='k_conv2d<48x64x32>'),
        c('f32 stride2 in_off1 cout96', 'f32', 1, 23, 29, 64, 96, s=2, in_off=1, g_cout=[90], expect='k_conv2d<128x32x32>'),
        c('f32 cout16 head-like g_cout 3', 'f32', 1, 17, 45, 64, 16, groups=3, g_cout=[3, 1, 2], g_ooff=[0, 3, 4], out_pad=0,
          out_f32=True, relu=False, scale=False, expect='k_conv2d<128x16x32>'),
    ]
    for m in ('f16x2', 'bf16x2', 'f16'):
        cs += [
            # generic split kernel (conv2d_h.hip)
            c('split 1x1 2x128x128', m, 2, 128, 128, 32, 256, k=1, expect='k_conv2d_h<128x128x32>'),
            c('split stride2 in_off1 16 frames', m, 16, 60, 59, 64, 128, s=2, in_off=1, in_coff=32, in_cextra=32,
              expect='k_conv2d_h<128x128x32>'),
            c('split 1x1 94x94 no scale/shift relu off', m, 1, 94, 94, 32, 256, k=1, scale=False, shift=False, relu=False,
              expect='k_conv2d_h<128x64x32>'),
            c('split 1x1 cout384 ragged M', m, 1, 7, 3109, 32, 384, k=1, out_pad=0, expect='k_conv2d_h<64x128x32>'),
            c('split 3x3 small out_coff', m, 1, 13, 19, 64, 64, out_coff=64, out_cextra=64, expect='k_conv2d_h<64x64x32>'),
            c('split cout32 g_cout 24', m, 1, 21, 23, 96, 32, g_cout=[24], expect='k_conv2d_h<128x32x32>'),
            c('split cout32 fp32 out grouped g_cout 5/3', m, 1, 15, 17, 32, 32, groups=2, g_cout=[5, 3], g_ooff=[0, 5], out_pad=0,
              out_f32=True, relu=False, expect='k_conv2d_h<128x32x32>'),
            c('split 1x1 fp32 out', m, 2, 40, 40, 64, 64, k=1, out_f32=True, out_pad=0, expect='k_conv2d_h<64x64x32>'),
            # resident-tile 3x3 kernel (conv3x3_h.hip): ragged in wo % 32, ho % 8 and ho % 16
            c('resident 128 ragged', m, 40, 37, 45, 64, 128, in_coff=32, in_cextra=32, out_coff=64, out_cextra=64,
              expect='k_conv3x3_h<8x32x128>'),
            c('resident 64 ragged no scale/shift relu off', m, 24, 29, 61, 96, 192, scale=False, shift=False, relu=False,
              g_cout=[184], expect='k_conv3x3_h<8x32x64>'),
            c('resident 32 ragged', m, 64, 37, 45, 64, 32, g_cout=[24], expect='k_conv3x3_h<16x32x32>'),
            c('resident 32 fp32 out grouped g_cout 2/7/3', m, 32, 21, 50, 32, 32, groups=3, g_cout=[2, 7, 3], g_ooff=[0, 2, 9],
              out_pad=0, out_f32=True, relu=False, scale=False, expect='k_conv3x3_h<16x32x32>'),
            # a layer the 128-channel resident tile takes (384 tiles), with fp32 output: that exists at 32-channel tiles only, so
            # the generic kernel runs it - and the report must say so
            c('resident-size 128 fp32 out', m, 16, 61, 70, 64, 128, g_cout=[122], out_pad=0, out_f32=True, relu=False,
              expect='k_conv2d_h<64x64x32>'),
            # in_tiles: listed 8 x 32 tiles computed, the others untouched
            c('resident 128 tile list', m, 12, 93, 90, 64, 128, tiles=True, expect='k_conv3x3_h<8x32x128>'),
            c('resident 64 tile list', m, 18, 61, 70, 64, 64, tiles=True, expect='k_conv3x3_h<8x32x64>'),
            # deblock phases: ConvTranspose2d with kernel == stride, s = 2, as the 4 groups of one launch
            c('phase groups s2', m, 3, 23, 41, 64, 64, k=1, groups=4, phase=True, out_coff=64, out_cextra=32,
              expect='k_conv2d_h<64x64x32>'),
        ]
        sp = c('sparse input 16 frames', m, 16, 188, 188, 256, 128, sparse=True, tiles=True, expect='k_conv3x3_h<8x32x128>')
        sp.in_rows = 300000
        cs.append(sp)
    return cs


COVERAGE = _coverage_cases()


def _ids(cases):
    return ['%s [%s]' % (c.label, c.mode) for c in cases]


# ------------------------------------------------------------------------------------------------------------------------
# descriptors, selectors, launches
# ------------------------------------------------------------------------------------------------------------------------
def _cdesc(desc, ptrs=None):
    d = L.Conv2dDesc()
    ptrs = ptrs or {}
    for k, v in desc.items():
        if k in ('g_cout', 'g_ooff'):
            for i, x in enumerate(v):
                getattr(d, k)[i] = int(x)
        else:
            setattr(d, k, v)
    for k in ('inp', 'out', 'w'):
        setattr(d, k, ptrs.get(k, 16))            # (a dummy non-null address for the host-side selectors)
    for k in ('scale', 'shift', 'in_rowidx', 'in_tiles'):
        if k in ptrs:
            setattr(d, k, ptrs[k])
    if desc.get('in_row_channels') and 'in_rowidx' not in ptrs:
        d.in_rowidx = 16
    return d


def selected_variant(case):
    d = _cdesc(case.desc)
    if case.sparse:
        d.in_rowidx, d.in_row_channels, d.in_rows = 16, case.desc['cin'] // 2, case.in_rows
    lib = L.load()
    if ops.math_id(case.mode):
        return lib.dz_conv2d_variant_split(ctypes.byref(d), 1 if case.out_f32 else 0).decode()
    return lib.dz_conv2d_variant(ctypes.byref(d)).decode()


LIMB3_VARIANTS = {'k_conv3x3_t<8x32x128>', 'k_conv3x3_t<8x32x64>'}


def _limb3(case):
    """The case runs on the bf16x3 engine of the f32 mode (production replay: the launches recorded with f32_engine='bf16x3')."""
    return getattr(case, 'f32_engine', None) == 'bf16x3'


def _launch(case, ptrs, math):
    lib = L.load()
    d = _cdesc(case.desc, ptrs)
    if case.sparse:
        d.in_row_channels, d.in_rows = case.desc['cin'] // 2, case.in_rows
    if _limb3(case):
        assert not math
        rc = lib.dz_conv3x3_limb3_forward(ctypes.byref(d), L.stream())
    elif math:
        rc = lib.dz_conv2d_forward_split(ctypes.byref(d), math, 1 if case.out_f32 else 0, L.stream())
    else:
        rc = lib.dz_conv2d_forward(ctypes.byref(d), L.stream())
    msg = lib.dz_last_error()
    return rc, (msg.decode() if msg else '')


# the launch rule of the bf16x3 engine, restated (csrc/conv3x3_t.hip launch_t3; test_limb3_launch_rule_is_the_library_s reads the
# constants back from the source): 32 workgroup slots per XCD; a layer of `nty` channel tiles that does not divide them and has at
# least LIMB3_SPLIT_PAIR_TILES (pixel tile, channel tile) pairs runs as two launches over 2^k and nty - 2^k channel tiles
LIMB3_SLOTS, LIMB3_SPLIT_PAIR_TILES = 32, 5000


def limb3_launches(desc):
    """(launches, pair tiles, workgroups per XCD of each launch) of dz_conv3x3_limb3_forward for a descriptor it supports."""
    bc = 128 if desc['cout_pad'] % 128 == 0 else 64
    nty = desc['cout_pad'] // bc
    pair_tiles = desc['batch'] * -(-desc['wo'] // 32) * -(-desc['ho'] // 8) * nty
    parts = [nty]
    if LIMB3_SLOTS % nty != 0 and nty < LIMB3_SLOTS and pair_tiles >= LIMB3_SPLIT_PAIR_TILES:
        a = 1
        while a * 2 <= nty:
            a *= 2
        if LIMB3_SLOTS % a == 0 and LIMB3_SLOTS % (nty - a) == 0:
            parts = [a, nty - a]
    return len(parts), pair_tiles, [max(LIMB3_SLOTS // ny * ny, ny) for ny in parts]


def test_limb3_launch_rule_is_the_library_s():
    """limb3_launches restates launch_t3: its two constants are the source's, and the rule gives the head's 64 -> 384 layer two launches
    from 5000 pair tiles on and one launch of 30 workgroups per XCD below."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), 'csrc', 'conv3x3_t.hip')).read()
    assert 'const int slots = %d;' % LIMB3_SLOTS in src and 'pair_tiles >= %d)' % LIMB3_SPLIT_PAIR_TILES in src
    d = dict(cout_pad=384, batch=7, ho=64, wo=960)
    assert limb3_launches(d) == (2, 5040, [32, 32])
    assert limb3_launches(dict(d, batch=1, ho=8 * 34 * 7 * 7, wo=32)) == (1, 4998, [30])
    assert limb3_launches(dict(d, cout_pad=192)) == (2, 5040, [32, 32]) and limb3_launches(dict(d, cout_pad=256)) == (1, 3360, [32])


# ------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ------------------------------------------------------------------------------------------------------------------------
def conv_ref(x, w, stride, ho, wo):
    """x (n, Hw, Ww, cin) float64, w (kh, kw, cin, cout) float64 -> (sum x.w, sum |x.w|), each (n, ho, wo, cout).
    CPU: F.conv2d; device: one float64 matmul per tap (the unfolded input of that tap)."""
    kh, kw = w.shape[0], w.shape[1]
    if x.device.type == 'cpu':
        xc, wc = x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1)
        acc = F.conv2d(xc, wc, stride=stride)[:, :, :ho, :wo]
        aacc = F.conv2d(xc.abs(), wc.abs(), stride=stride)[:, :, :ho, :wo]
        return acc.permute(0, 2, 3, 1), aacc.permute(0, 2, 3, 1)
    n, cin, cout = x.shape[0], x.shape[3], w.shape[3]
    acc = torch.zeros((n * ho * wo, cout), dtype=torch.float64, device=x.device)
    aacc = torch.zeros_like(acc)
    for ky in range(kh):
        for kx in range(kw):
            xt = x[:, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride, :].reshape(-1, cin)
            acc.addmm_(xt, w[ky, kx])
            aacc.addmm_(xt.abs(), w[ky, kx].abs())
    return acc.view(n, ho, wo, cout), aacc.view(n, ho, wo, cout)


def _tile_list(batch, ho, wo, gen, dev):
    """A dz_bev_tile_list-format list over 8 x 32-pixel tiles: [n run, n skipped, run ids ascending, skipped ids], about 60 % run;
    and the (batch, ho, wo) mask of the pixels the listed tiles cover."""
    tx, ty = -(-wo // 32), -(-ho // 8)
    n = batch * tx * ty
    run = torch.rand(n, generator=gen, device=dev) < 0.6
    ids = torch.arange(n, device=dev, dtype=torch.int32)
    lst = torch.cat([torch.tensor([int(run.sum()), int((~run).sum())], dtype=torch.int32, device=dev), ids[run], ids[~run]])
    pix = run.view(batch, ty, 1, tx, 1).expand(batch, ty, 8, tx, 32).reshape(batch, ty * 8, tx * 32)[:, :ho, :wo]
    return lst.contiguous(), pix.contiguous()


def _decode(x, mode):
    """Operand as the kernel sees it, float64: fp32 as is, split modes hi + lo of the pair16 words."""
    math = ops.math_id(mode)
    return (ops.pair16_unpack(x, math) if math else x).double()


def run_case(case, dev, seed=None):
    """Launch `case` twice into sentinel-filled buffers; check determinism, the result against float64 and the sentinel outside
    the written region.  Returns (variant, worst normalised error)."""
    mode, math, dd = case.mode, ops.math_id(case.mode), case.desc
    if _limb3(case):
        assert L.load().dz_conv3x3_limb3_supported(ctypes.byref(_cdesc(dd))) == 1, case.label
        name = L.load().dz_conv3x3_limb3_variant(ctypes.byref(_cdesc(dd))).decode()
    else:
        name = selected_variant(case)
    if case.expect is not None:
        assert name == case.expect, (case.label, mode, name, case.expect)
    assert name in (LIMB3_VARIANTS if _limb3(case) else ALL_VARIANTS[mode]), (case.label, mode, name)
    gen = torch.Generator(device=dev)
    gen.manual_seed(zlib.crc32(('%s|%s' % (case.label, mode)).encode()) if seed is None else seed)
    B, ho, wo, cin, groups, cp = dd['batch'], dd['ho'], dd['wo'], dd['cin'], dd['groups'], dd['cout_pad']
    kh, kw, s, in_off = dd['kh'], dd['kw'], dd['stride'], dd['in_off']
    phase = bool(dd['phase_groups'])
    sv = ops.storage_math(math)

    # operands
    if case.sparse:
        crow = cin // 2
        rows32 = torch.randn((case.in_rows, crow), generator=gen, device=dev)
        rows = ops.pair16_from_f32(rows32, math=math)
        rows_dec = _decode(rows, mode)
        ridx = torch.randint(0, case.in_rows, (B, dd['in_hp'], dd['in_wp'], 2), generator=gen, device=dev, dtype=torch.int32)
        ridx[torch.rand(ridx.shape, generator=gen, device=dev) < 0.35] = -1
        inp = rows

        def frames(b0, b1):
            idx = ridx[b0:b1].long()
            g = rows_dec[idx.clamp(min=0)] * (idx >= 0).unsqueeze(-1)
            return g.reshape(b1 - b0, dd['in_hp'], dd['in_wp'], cin)
    else:
        img = torch.randn((B, dd['in_hp'], dd['in_wp'], dd['in_cstride']), generator=gen, device=dev)
        inp = ops.pair16_from_f32(img, math=math) if math else img
        del img

        def frames(b0, b1):
            return _decode(inp[b0:b1], mode)
    taps = kh * kw
    w32 = torch.randn((groups, taps, cin, cp), generator=gen, device=dev)
    if math:
        wk = ops.pack_weight_split(w32, sv, cout_mult=cp)                    # (groups, taps, cp, cin) pair16
        w64 = _decode(wk, mode).transpose(-1, -2)
    else:
        # (bf16x3: the three limbs of a weight sum to it exactly - the reference is the fp32 operands')
        wk = ops.pack_weight_limb3(w32[0]) if _limb3(case) else w32.contiguous()
        w64 = w32.double()
    w64 = w64.reshape(groups, kh, kw, cin, cp)
    nss = cp if phase else groups * cp
    sc = (torch.rand(nss, generator=gen, device=dev) + 0.5) / (taps * cin) ** 0.5 if case.scale else None
    sh = torch.randn(nss, generator=gen, device=dev) * 0.5 if case.shift else None
    tl = pix = None
    if case.tiles:
        tl, pix = _tile_list(B, ho, wo, gen, dev)
        if name not in ('k_conv3x3_h<8x32x128>', 'k_conv3x3_h<8x32x64>'):
            pix = None          # the generic kernel ignores the list and computes every pixel (dz_conv2d_desc.in_tiles)

    # two launches into sentinel-filled buffers
    nout = B * dd['out_hp'] * dd['out_wp'] * dd['out_cstride']
    outs = [torch.full((nout,), SENTINEL, dtype=torch.int32, device=dev) for _ in range(2)]
    for o in outs:
        ptrs = dict(inp=inp.data_ptr(), out=o.data_ptr(), w=wk.data_ptr())
        if sc is not None:
            ptrs['scale'] = sc.data_ptr()
        if sh is not None:
            ptrs['shift'] = sh.data_ptr()
        if case.sparse:
            ptrs['in_rowidx'] = ridx.data_ptr()
        if tl is not None:
            ptrs['in_tiles'] = tl.data_ptr()
        rc, msg = _launch(case, ptrs, math)
        assert rc == 0, (case.label, mode, rc, msg)
    torch.cuda.synchronize(dev)
    assert torch.equal(outs[0], outs[1]), ('two launches differ', case.label, mode, name)
    out = outs[0].view(B, dd['out_hp'], dd['out_wp'], dd['out_cstride'])
    del outs[1]

    # compare the written region with float64, frame chunk by frame chunk; mark it
    touched = torch.zeros(out.shape, dtype=torch.bool, device=dev)
    big = B * ho * wo * cin * taps * cp * groups > 2e8
    chunk = max(1, (1 << 28) // max(1, ho * wo * max(cin, cp) * 8))
    worst = 0.0
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        xall = frames(b0, b1)
        if not big:
            xall = xall.cpu()
        for g in range(groups):
            c0 = dd['in_coff'] + (0 if phase else g * cin)
            x = xall[:, in_off:in_off + (ho - 1) * s + kh, in_off:in_off + (wo - 1) * s + kw, c0:c0 + cin]
            gc = dd['g_cout'][g]
            acc, aacc = conv_ref(x, w64[g].to(x.device), s, ho, wo)
            acc, aacc = acc[..., :gc].to(dev), aacc[..., :gc].to(dev)
            si = 0 if phase else g * cp
            scv = sc[si:si + gc].double() if sc is not None else torch.ones(gc, dtype=torch.float64, device=dev)
            shv = sh[si:si + gc].double() if sh is not None else torch.zeros(gc, dtype=torch.float64, device=dev)
            ref = acc * scv + shv
            if dd['relu']:
                ref = ref.clamp_min(0.0)
            den = aacc * scv.abs() + shv.abs()
            dy = dd['out_dy'] + (g // dd['out_sx'] if phase else 0)
            dx = dd['out_dx'] + (g % dd['out_sx'] if phase else 0)
            o0 = dd['out_coff'] + dd['g_ooff'][g]
            sl = (slice(b0, b1), slice(dy, dy + (ho - 1) * dd['out_sy'] + 1, dd['out_sy']),
                  slice(dx, dx + (wo - 1) * dd['out_sx'] + 1, dd['out_sx']), slice(o0, o0 + gc))
            words = out[sl].contiguous()
            got = words.view(torch.float32).double() if (case.out_f32 or not math) else _decode(words.view(torch.float32), mode)
            err = (got - ref).abs() / den.clamp_min(1e-30)
            err = torch.where(torch.isnan(got), torch.full_like(err, float('inf')), err)
            if pix is not None:
                m = pix[b0:b1].unsqueeze(-1)
                err = torch.where(m, err, torch.zeros_like(err))
                touched[sl] = m.expand(-1, -1, -1, gc)
            else:
                touched[sl] = True
            e = float(err.max())
            if not e <= BOUND[mode]:
                i = int(torch.argmax(err.flatten()))
                raise AssertionError('%s [%s] %s: normalised error %.3e > %.3e (group %d, frame chunk %d, flat index %d: got %r ref %r den %r)' % (
                    case.label, mode, name, e, BOUND[mode], g, b0, i, float(got.flatten()[i]), float(ref.flatten()[i]), float(den.flatten()[i])))
            worst = max(worst, e)
        del xall
    # nothing outside the region: zero borders, other channels, pad channels beyond g_cout, other phases, skipped tiles
    bad = (out != SENTINEL) & ~touched
    nbad = int(bad.sum())
    if nbad:
        i = torch.nonzero(bad)[0].tolist()
        raise AssertionError('%s [%s] %s: %d words written outside the output region (first at (b, y, x, channel) = %s)' % (
            case.label, mode, name, nbad, i))
    print('  %-46s %-7s %-24s worst normalised error %.3e (bound %.1e)' % (case.label, mode, name, worst, BOUND[mode]))
    return name, worst


# ------------------------------------------------------------------------------------------------------------------------
# the table: no GPU needed (the selectors are host code)
# ------------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_every_variant():
    """Every case's selector reports the variant the case names, and the cases reach every instance of kConvVariantName,
    kConvHVariantName and the three k_conv3x3_h tiles in every math mode it is compiled for."""
    reached = {m: set() for m in MODES}
    for c in COVERAGE:
        name = selected_variant(c)
        assert name == c.expect, (c.label, c.mode, name, c.expect)
        reached[c.mode].add(name)
    for m in MODES:
        print('  %-7s %s' % (m, ' '.join(sorted(reached[m]))))
        assert reached[m] == ALL_VARIANTS[m], (m, sorted(ALL_VARIANTS[m] - reached[m]), sorted(reached[m] - ALL_VARIANTS[m]))


def test_refused_descriptors_report_none():
    """A layer dz_conv2d_forward_split refuses is reported as "none", not as the kernel it would have reached: a tile list on a
    32-channel tile layer (its tiles are 16 x 32, the list's 8 x 32), and sparse input with fp32 output."""
    tiled = next(c for c in COVERAGE if c.label == 'resident 32 ragged' and c.mode == 'f16x2')
    assert selected_variant(tiled) == 'k_conv3x3_h<16x32x32>'
    d = _cdesc(tiled.desc, dict(in_tiles=16))
    assert L.load().dz_conv2d_variant_split(ctypes.byref(d), 0).decode() == 'none'
    sparse = next(c for c in COVERAGE if c.sparse and c.mode == 'f16x2')
    assert selected_variant(sparse) == 'k_conv3x3_h<8x32x128>'
    d = _cdesc(sparse.desc)
    d.in_rowidx, d.in_row_channels, d.in_rows = 16, sparse.desc['cin'] // 2, sparse.in_rows
    assert L.load().dz_conv2d_variant_split(ctypes.byref(d), 1).decode() == 'none'


def test_reference_paths_agree():
    """The two float64 reference paths (CPU F.conv2d, per-tap matmul) agree, and the phase-group mapping of the reference is a
    float64 ConvTranspose2d (kernel == stride)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 13, 17, 24), generator=g, dtype=torch.float64)
    w = torch.randn((3, 3, 24, 16), generator=g, dtype=torch.float64)
    a, aa = conv_ref(x, w, 2, 6, 8)
    n, cin, cout = 2, 24, 16
    acc = torch.zeros((n * 6 * 8, cout), dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            acc += x[:, ky:ky + 11:2, kx:kx + 15:2, :].reshape(-1, cin) @ w[ky, kx]
    assert torch.allclose(a.reshape(-1, cout), acc, rtol=1e-12, atol=1e-12)
    assert bool((aa >= a.abs() - 1e-12).all())
    wt = torch.randn((24, 16, 2, 2), generator=g, dtype=torch.float64)           # ConvTranspose2d weight (cin, cout, s, s)
    ct = F.conv_transpose2d(x.permute(0, 3, 1, 2), wt, stride=2).permute(0, 2, 3, 1)
    for ph in range(4):
        dy, dx = ph // 2, ph % 2
        p, _ = conv_ref(x, wt[:, :, dy, dx].reshape(1, 1, 24, 16), 1, 13, 17)
        assert torch.allclose(ct[:, dy::2, dx::2, :], p, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------------------
# GPU: every instance
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('case', COVERAGE, ids=_ids(COVERAGE))
def test_variant_vs_float64(case, device):
    run_case(case, device)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ('f16x2', 'bf16x2'))
def test_phase_groups_vs_conv_transpose2d(mode, device):
    """The fused-phase deblock (dz_conv2d_desc.phase_groups, s = 2) against a float64 torch ConvTranspose2d of the decoded operands."""
    math = ops.math_id(mode)
    gen = torch.Generator(device=device).manual_seed(11)
    b, h, w, cin, cout, s = 2, 21, 35, 64, 64, 2
    x32 = torch.randn((b, h + 2, w + 2, cin), generator=gen, device=device)
    xp = ops.pair16_from_f32(x32, math=math)
    wt = torch.randn((cin, cout, s, s), generator=gen, device=device)
    w_ph = wt.permute(2, 3, 0, 1).reshape(s * s, 1, cin, cout)                   # phase g = (g // s, g % s): BaseBEVBackbone.plan
    wk = ops.pack_weight_split(w_ph, math)
    sc = torch.rand(cout, generator=gen, device=device) + 0.5
    sh = torch.randn(cout, generator=gen, device=device)
    out = torch.full((b, h * s + 2, w * s + 2, cout), SENTINEL, dtype=torch.int32, device=device)
    ops.conv2d(dict(inp=xp.data_ptr(), out=out.data_ptr(), w=wk.data_ptr(), scale=sc.data_ptr(), shift=sh.data_ptr(), batch=b, ho=h, wo=w,
                    in_hp=h + 2, in_wp=w + 2, in_cstride=cin, in_coff=0, cin=cin, kh=1, kw=1, stride=1, in_off=1, out_hp=h * s + 2,
                    out_wp=w * s + 2, out_cstride=cout, out_coff=0, out_sy=s, out_sx=s, out_dy=1, out_dx=1, groups=s * s, cout_pad=cout,
                    g_cout=[cout] * 4, g_ooff=[0] * 4, relu=1, phase_groups=1), math=math)
    xd = _decode(xp, mode)[:, 1:-1, 1:-1, :].cpu().permute(0, 3, 1, 2)
    wd = _decode(wk, mode).transpose(-1, -2).reshape(s, s, cin, cout).permute(2, 3, 0, 1).cpu()
    ref = F.conv_transpose2d(xd, wd, stride=s).permute(0, 2, 3, 1)
    den = F.conv_transpose2d(xd.abs(), wd.abs(), stride=s).permute(0, 2, 3, 1)
    scd, shd = sc.double().cpu(), sh.double().cpu()
    ref = (ref * scd + shd).clamp_min(0.0)
    den = den * scd.abs() + shd.abs()
    got = _decode(out[:, 1:-1, 1:-1, :].contiguous().view(torch.float32), mode).cpu()
    err = float(((got - ref).abs() / den).max())
    print('  phase groups s=2 [%s] vs float64 conv_transpose2d: worst normalised error %.3e' % (mode, err))
    assert err <= BOUND[mode], err
    border = out.clone()
    border[:, 1:-1, 1:-1, :] = SENTINEL
    assert bool((border == SENTINEL).all()), 'the deblock wrote into the zero border'


# ------------------------------------------------------------------------------------------------------------------------
# GPU: the detector's own dense layers at the frame counts it runs them at
# ------------------------------------------------------------------------------------------------------------------------
# frames per pass: one frame (the parity tests), bench.py's ref_batch leg (BATCH_SIZE_PER_GPU = 8 of the reference config),
# FramePipeline.dense_group (frames per dense pass) and a sub-pass of bench.py's default 64-frame step (two concurrent passes
# of 32 frames: the first and second BEV blocks over all 32, the deblocks and the head in dense_group frames)
FRAMES = ('single', 'ref_batch', 'dense_group', 'sub_pass')


@functools.lru_cache(maxsize=None)
def production_cases(mode, frames, dense_engine='mfma32', full_head=False):
    """The dense layers FramePipeline.dense_stage launches for a pass of the 0.1 m Waymo detector (188 x 188 BEV),
    recorded as the descriptors det_modules.conv_layer hands to ops.conv2d (the images live on the meta device: nothing runs),
    distinct geometries only.  Split modes read the first convolution's input as sparse rows (in_rowidx) with tile lists.
    dense_engine: the f32 mode's engine of the 3 x 3 stride-1 layers (centerpoint.set_dense_engine); a launch the detector hands
    f32_engine='bf16x3' is recorded as such (case.f32_engine) and replayed through dz_conv3x3_limb3_forward.
    full_head: the pass with FramePipeline.head_at_candidates off - the head writes full maps, so all six branches' hidden layer (64 ->
    384) runs as one launch instead of the two score branches' (64 -> 128)."""
    from detzero_amd import centerpoint
    from detzero_amd.synth import VOXEL_SIZE_01
    from tests.util import make_model
    model, cfg, info = make_model(VOXEL_SIZE_01, seed=0)
    centerpoint.set_dense_engine(model, dense_engine)
    pipe = centerpoint.FramePipeline(model, info, math=mode)
    if full_head:
        pipe.head_at_candidates = False
    nb = {'single': 1, 'ref_batch': 8, 'dense_group': pipe.dense_group, 'sub_pass': 32}[frames]
    stride = int(model.dense_head.feature_map_stride)
    gx, gy = int(info.grid_size[0]), int(info.grid_size[1])
    h, w = gy // stride, gx // stride
    rows_c = model.backbone2d.input_channels // 2
    meta = torch.device('meta')
    rec = []

    def fake_conv2d(desc, math=0, out_f32=False, tiles=None, f32_engine=None):
        rec.append((dict(desc), int(math), bool(out_f32), tiles is not None, f32_engine))

    def fake_row_index(level, feat_rows, pad=1):
        return torch.empty((nb, h + 2 * pad, w + 2 * pad, 2), dtype=torch.int32, device=meta)

    def fake_to_bev(feats, level, c, pad=1, out=None, math=0):
        return torch.empty((nb, h + 2 * pad, w + 2 * pad, c * level.shape[0]), dtype=torch.float32, device=meta)

    def fake_tile_list(ridx, ho, wo, nlists=1):
        return torch.empty((nlists, 16), dtype=torch.int32, device=meta)

    saved = {k: getattr(ops, k) for k in ('conv2d', 'bev_row_index', 'sparse_to_bev', 'bev_tile_list', 'bev_fill_empty_tiles')}
    saved_cap = torch.cuda.is_current_stream_capturing
    try:
        ops.conv2d, ops.bev_row_index, ops.sparse_to_bev = fake_conv2d, fake_row_index, fake_to_bev
        ops.bev_tile_list, ops.bev_fill_empty_tiles = fake_tile_list, lambda *a, **k: None
        torch.cuda.is_current_stream_capturing = lambda: False
        x = torch.empty((300000, rows_c), dtype=torch.float32, device=meta)
        lvl = types.SimpleNamespace(shape=(2, h, w))
        pipe.dense_stage({'encoded': (x, lvl)}, nb)
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
        torch.cuda.is_current_stream_capturing = saved_cap
    assert rec, 'dense_stage launched no convolution'
    cases, seen = [], set()
    skip = ('inp', 'out', 'w', 'scale', 'shift', 'in_rowidx', 'in_tiles')
    for desc, math, out_f32, tiles, f32_engine in rec:
        geo = {k: v for k, v in desc.items() if k not in skip}
        key = (tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in geo.items())), out_f32, tiles,
               desc.get('scale') is not None, desc.get('shift') is not None, f32_engine)
        if key in seen:
            continue
        seen.add(key)
        sparse = bool(geo.get('in_row_channels'))
        in_rows = geo.pop('in_rows', 0)
        geo.pop('in_row_channels', None)
        geo.setdefault('phase_groups', 0)
        label = 'prod %df %dx%d %d->%s k%d s%d%s%s%s%s' % (
            geo['batch'], geo['ho'], geo['wo'], geo['cin'] * (1 if geo['phase_groups'] else geo['groups']),
            geo['g_cout'][0] if geo['phase_groups'] else sum(geo['g_cout'][:geo['groups']]),
            geo['kh'], geo['stride'], ' phases' if geo['phase_groups'] else '',
            ' phase (%d, %d)' % (geo['out_dy'] - 1, geo['out_dx'] - 1) if geo['out_sy'] > 1 and not geo['phase_groups'] else '', ' sparse-in' if sparse else '', ' tiles' if tiles else '') + (' ' + f32_engine if f32_engine else '')
        cases.append(types.SimpleNamespace(label=label, mode=mode, desc=geo, out_f32=out_f32, scale=desc.get('scale') is not None,
                                           shift=desc.get('shift') is not None, tiles=tiles, sparse=sparse, in_rows=in_rows, expect=None,
                                           f32_engine=f32_engine))
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize('frames', FRAMES)
@pytest.mark.parametrize('mode', MODES)
def test_production_layers_vs_float64(mode, frames, device):
    cases = production_cases(mode, frames)
    print('\n  %s pass [%s]: %d distinct dense launches' % (frames, mode, len(cases)))
    for c in cases:
        run_case(c, device)
    torch.cuda.empty_cache()


def test_production_layers_recorded_for_the_bf16x3_engine():
    """The f32 pass recorded with the dense engine 'bf16x3' (host only): the same layers as with 'mfma32', the 3 x 3 stride-1 ones handed
    to the bf16x3 engine.  With the head at candidates (the default) no layer has three channel tiles; with full head maps the head's
    64 -> 384 layer is among them - at dense_group frames above the two-launch threshold of launch_t3, at one frame below it."""
    for frames in ('single', 'dense_group'):
        plain, limb = production_cases('f32', frames), production_cases('f32', frames, 'bf16x3')
        assert all(c.f32_engine is None for c in plain)
        assert [c.desc for c in plain] == [c.desc for c in limb]
        assert not any(limb3_launches(c.desc)[0] == 2 for c in limb if c.f32_engine)
        limb = _bf16x3_production(frames)
        on = [c for c in limb if c.f32_engine == 'bf16x3']
        assert on and all(c.desc['kh'] == 3 and c.desc['stride'] == 1 and c.desc['groups'] == 1 for c in on)
        assert all(c.f32_engine == 'bf16x3' for c in limb if c.desc['kh'] == 3 and c.desc['stride'] == 1 and c.desc['groups'] == 1 and c.desc['cout_pad'] % 64 == 0)
        split = [c for c in on if limb3_launches(c.desc)[0] == 2]
        print('  %s: %d of %d launches on the bf16x3 engine, %d as two launches' % (frames, len(on), len(limb), len(split)))
        assert bool(split) == (frames == 'dense_group'), (frames, [(c.label, limb3_launches(c.desc)) for c in on])
        assert all(c.desc['cout_pad'] == 384 for c in split)


def _bf16x3_production(frames):
    """Distinct launches of the f32 pass with the dense engine 'bf16x3': the default pass (head at candidates) and the pass with full
    head maps."""
    cases, seen = [], set()
    for c in production_cases('f32', frames, 'bf16x3') + production_cases('f32', frames, 'bf16x3', True):
        if c.label not in seen:
            seen.add(c.label)
            cases.append(c)
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize('frames', ('single', 'dense_group'))
def test_production_layers_on_the_bf16x3_engine(frames, device):
    """test_production_layers_vs_float64 for the launches the f32 detector hands its bf16x3 dense engine (k_conv3x3_t), with the head at
    candidates and with full head maps: the same float64 reference and bound.  At dense_group frames the full-map head's 384-channel
    layer runs as launch_t3's two launches (asserted from the launcher's rule); the layers that stay on k_conv2d are the f32 row's of
    test_production_layers_vs_float64."""
    cases = [c for c in _bf16x3_production(frames) if c.f32_engine == 'bf16x3']
    nsplit = sum(limb3_launches(c.desc)[0] == 2 for c in cases)
    print('\n  %s pass [f32, bf16x3 dense engine]: %d distinct launches on k_conv3x3_t, %d of them as two launches' % (frames, len(cases), nsplit))
    assert cases and (nsplit >= 1 or frames != 'dense_group'), (frames, [(c.label, limb3_launches(c.desc)) for c in cases])
    for c in cases:
        run_case(c, device)
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------
# GPU: the 2 GiB buffer window
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('mode', ('f32', 'f16x2'))
def test_input_just_under_2gib_window(mode, device):
    """The head's shared 512 -> 64 convolution over 28 frames of 188 x 188: an input image 2.07e9 bytes, 3 % under the window the
    kernels address through 32-bit offsets.  The last frame - the one at the far end of the window - is compared in full."""
    math = ops.math_id(mode)
    nb, h, w, cin, cout = 28, 188, 188, 512, 64
    assert nb * (h + 2) * (w + 2) * cin * 4 < 2 ** 31 <= (nb + 2) * (h + 2) * (w + 2) * cin * 4
    gen = torch.Generator(device=device).manual_seed(5)
    img = torch.randn((nb, h + 2, w + 2, cin), generator=gen, device=device)
    if math:
        img = ops.pair16_from_f32(img, math=math)
    w32 = torch.randn((1, 9, cin, cout), generator=gen, device=device)
    wk = ops.pack_weight_split(w32, math) if math else w32
    sc = (torch.rand(cout, generator=gen, device=device) + 0.5) / (9 * cin) ** 0.5
    sh = torch.randn(cout, generator=gen, device=device) * 0.5
    out = torch.full((nb, h + 2, w + 2, cout), SENTINEL, dtype=torch.int32, device=device)
    case = conv_case('2 GiB window', mode, nb, h, w, cin, cout)
    name = selected_variant(case)
    rc, msg = _launch(case, dict(inp=img.data_ptr(), out=out.data_ptr(), w=wk.data_ptr(), scale=sc.data_ptr(), shift=sh.data_ptr()), math)
    assert rc == 0, (rc, msg)
    torch.cuda.synchronize(device)
    x = _decode(img[nb - 1:], mode)
    del img
    wd = (_decode(wk, mode).transpose(-1, -2) if math else w32.double()).reshape(3, 3, cin, cout)
    acc, aacc = conv_ref(x, wd, 1, h, w)
    ref = (acc * sc.double() + sh.double()).clamp_min(0.0)
    den = aacc * sc.double() + sh.double().abs()
    last = out[nb - 1:, 1:-1, 1:-1, :].contiguous().view(torch.float32)
    got = _decode(last, mode)
    err = (got - ref).abs() / den
    e = float(torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err).max())
    print('  2 GiB window, last of %d frames [%s] %s: worst normalised error %.3e' % (nb, mode, name, e))
    assert e <= BOUND[mode], e
    border = out[nb - 1].clone()
    border[1:-1, 1:-1, :] = SENTINEL
    assert bool((border == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize('mode,k,s,cout', [('f32', 3, 1, 64), ('f16x2', 3, 1, 64), ('f16x2', 1, 1, 64), ('bf16x2', 3, 2, 128)])
def test_input_at_2gib_window_refused(mode, k, s, cout, device):
    """An input image of exactly 2^31 bytes (and one beyond) is refused before launch, with a message - on every engine.  The
    buffers are real, so a missing check would read inside them rather than fault."""
    math = ops.math_id(mode)
    cin = 512
    big = torch.empty((2 ** 31 + 2 ** 26) // 4, dtype=torch.float32, device=device)
    out = torch.full((2 ** 27,), SENTINEL, dtype=torch.int32, device=device)
    wk = torch.zeros((k * k * cin * cout,), dtype=torch.float32, device=device)
    for hp in (1024, 1056):                                  # 1024 x 1024 x 512 x 4 bytes = 2^31; 1056 rows: 2^31 + 2^26
        ho = (hp - k) // s + 1
        wo = (1024 - k) // s + 1
        case = conv_case('window', mode, 1, ho, wo, cin, cout, k=k, s=s, in_off=0, out_pad=0)
        case.desc.update(in_hp=hp, in_wp=1024, out_hp=ho, out_wp=wo)
        assert case.desc['out_hp'] * case.desc['out_wp'] * case.desc['out_cstride'] <= out.numel()
        rc, msg = _launch(case, dict(inp=big.data_ptr(), out=out.data_ptr(), w=wk.data_ptr()), math)
        torch.cuda.synchronize(device)
        print('  %s %dx%d s%d, %d-byte image -> rc %d: %s' % (mode, k, k, s, hp * 1024 * cin * 4, rc, msg))
        assert rc in (-1, -4) and '2 GiB' in msg, (rc, msg)
        assert bool((out == SENTINEL).all())
