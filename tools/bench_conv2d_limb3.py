"""The four dense layer classes of the f32 mode that the 3 x 3 stride-1 bf16x3 engine does not take, each timed alone at 16 frames of
the 0.1 m grid (188 x 188 / 94 x 94): k_conv2d_t (csrc/conv2d_t.hip, three bf16 limbs per operand) against k_conv2d (the f32 engine) on
the same tensors, launches interleaved in one process, one event pair per launch, median of --iters (20) launches each.
Printed per layer: us, algorithmic TF/s, the fraction of the 419 TF/s six-MFMA peak (2516.6 / 6), algorithmic GB/s (input + output +
weights once: what counts for the memory-bound output layer), and the ratio to k_conv2d.  --plain adds a 3 x 3 stride-1 layer."""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from detzero_amd import lib as L        # noqa: E402
from detzero_amd import ops             # noqa: E402


def layers(batch, hw, plain):
    """(label, desc fields) of the production classes: BaseBEVBackbone's strided layer and deblocks, CenterHead's output layer."""
    h, h2 = hw, hw // 2
    out = [
        ('3x3 s2 128->256', dict(batch=batch, ho=h2, wo=h2, in_hp=h + 2, in_wp=h + 2, in_cstride=128, cin=128, kh=3, kw=3, stride=2, in_off=0,
                                 out_hp=h2 + 2, out_wp=h2 + 2, out_cstride=256, out_dy=1, out_dx=1, cout_pad=256, g_cout=[256], relu=1)),
        ('deblock1 1x1 128->256', dict(batch=batch, ho=h, wo=h, in_hp=h + 2, in_wp=h + 2, in_cstride=128, cin=128, kh=1, kw=1, stride=1, in_off=1,
                                       out_hp=h + 2, out_wp=h + 2, out_cstride=512, out_dy=1, out_dx=1, cout_pad=256, g_cout=[256], relu=1)),
        ('deblock2 phase 256->256', dict(batch=batch, ho=h2, wo=h2, in_hp=h2 + 2, in_wp=h2 + 2, in_cstride=256, cin=256, kh=1, kw=1, stride=1,
                                         in_off=1, out_hp=h + 2, out_wp=h + 2, out_cstride=512, out_coff=256, out_sy=2, out_sx=2, out_dy=2,
                                         out_dx=1, cout_pad=256, g_cout=[256], relu=1)),
        ('output 6x(64->1..3)', dict(batch=batch, ho=h, wo=h, in_hp=h + 2, in_wp=h + 2, in_cstride=384, cin=64, kh=3, kw=3, stride=1, in_off=0,
                                     out_hp=h, out_wp=h, out_cstride=12, out_dy=0, out_dx=0, groups=6, cout_pad=16, g_cout=[2, 1, 3, 2, 1, 3],
                                     g_ooff=[0, 2, 3, 6, 8, 9], relu=0, no_scale=True)),
    ]
    if plain:
        out.append(('3x3 s1 128->128', dict(batch=batch, ho=h, wo=h, in_hp=h + 2, in_wp=h + 2, in_cstride=128, cin=128, kh=3, kw=3, stride=1,
                                            in_off=0, out_hp=h + 2, out_wp=h + 2, out_cstride=128, out_dy=1, out_dx=1, cout_pad=128, g_cout=[128],
                                            relu=1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--hw', type=int, default=188)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--plain', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    lib = L.load()
    g = torch.Generator(device=dev).manual_seed(0)
    print('%d frames of %d x %d, median of %d interleaved launches; TF/s and GB/s are algorithmic' % (a.batch, a.hw, a.hw, a.iters))
    print('  %-26s %-24s %9s %8s %6s %8s   %-22s %9s %8s %8s   %s' % ('layer', 'bf16x3 kernel', 'us', 'TF/s', '/419', 'GB/s', 'f32 kernel', 'us', 'TF/s',
                                                                     'GB/s', 'k_conv2d / k_conv2d_t'))
    for label, f in layers(a.batch, a.hw, a.plain):
        f = dict(f)
        no_scale = f.pop('no_scale', False)
        f.setdefault('groups', 1)
        f.setdefault('in_coff', 0)
        f.setdefault('out_coff', 0)
        f.setdefault('out_sy', 1)
        f.setdefault('out_sx', 1)
        f.setdefault('g_ooff', [0])
        groups, taps, cin, cp = f['groups'], f['kh'] * f['kw'], f['cin'], f['cout_pad']
        x = torch.zeros(f['batch'], f['in_hp'], f['in_wp'], f['in_cstride'], device=dev)
        x[:, 1:-1, 1:-1] = torch.randn(f['batch'], f['in_hp'] - 2, f['in_wp'] - 2, f['in_cstride'], generator=g, device=dev).clamp_min(0)
        wr = torch.randn(groups, taps, cin, cp, generator=g, device=dev) * 0.05
        wts = {'bf16x3': ops.pack_weight_limb3_generic(wr), 'f32': wr.contiguous()}
        scale = None if no_scale else torch.rand(groups * cp, generator=g, device=dev) + 0.5
        shift = torch.randn(groups * cp, generator=g, device=dev)
        ys = {k: torch.zeros(f['batch'], f['out_hp'], f['out_wp'], f['out_cstride'], device=dev) for k in wts}

        def run(k):
            desc = dict(f, inp=x.data_ptr(), out=ys[k].data_ptr(), w=wts[k].data_ptr(), scale=None if scale is None else scale.data_ptr(),
                        shift=shift.data_ptr())
            ops.conv2d(desc, f32_generic='bf16x3' if k == 'bf16x3' else None)
            return desc
        d = ops._conv2d_desc(run('bf16x3'))
        names = {'bf16x3': lib.dz_conv2d_limb3_variant(ctypes.byref(d)).decode(), 'f32': lib.dz_conv2d_variant(ctypes.byref(d)).decode()}
        for _ in range(3):
            for k in wts:
                run(k)
        torch.cuda.synchronize()
        diff = float((ys['bf16x3'].double() - ys['f32'].double()).abs().max() / ys['f32'].double().abs().max())
        ev = {k: [] for k in wts}
        for _ in range(a.iters):
            for k in wts:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(k)
                e1.record()
                ev[k].append((e0, e1))
        torch.cuda.synchronize()
        med = {k: sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in v)[len(v) // 2] for k, v in ev.items()}
        m = f['batch'] * f['ho'] * f['wo']
        cout = sum(f['g_cout'])
        fl = 2.0 * m * taps * cin * cout
        nbytes = 4.0 * (m * cin * groups + m * cout + taps * cin * cp * groups)
        tf = {k: fl / med[k] * 1e-6 for k in med}
        gb = {k: nbytes / med[k] * 1e-3 for k in med}
        print('  %-26s %-24s %9.1f %8.1f %6.2f %8.0f   %-22s %9.1f %8.1f %8.0f   %.2f x   (max |diff| / max |ref| %.1e)' % (
            label, names['bf16x3'], med['bf16x3'], tf['bf16x3'], tf['bf16x3'] / 419.4, gb['bf16x3'], names['f32'], med['f32'], tf['f32'], gb['f32'],
            med['f32'] / med['bf16x3'], diff))


if __name__ == '__main__':
    main()
