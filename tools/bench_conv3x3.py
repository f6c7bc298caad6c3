"""One BEV 3x3 layer (16 x 188 x 188, 128 -> 128 channels, pair16) timed alone: us per launch and algorithmic TF/s.
--data picks the operands (time vs operand data: clock / power); DZ_CHECK=1 also checks the result against float64.
--engine bf16x3: the three-limb kernel of the f32 mode (k_conv3x3_t) against k_conv2d (the f32 engine) and k_conv3x3_h (f16x2) on
the same tensors, interleaved in one process, one event pair per launch: median us, TF/s, fraction of the 419 TF/s six-MFMA peak
(2516.6 / 6), ratio to k_conv2d."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from detzero_amd import ops                      # noqa: E402
from detzero_amd.det_modules import conv_layer   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--hw', type=int, default=188)
    ap.add_argument('--cin', type=int, default=128)
    ap.add_argument('--cout', type=int, default=128)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--math', type=int, default=1, help='1 = f16x2, 2 = bf16x2, 3 = f16 (single product)')
    ap.add_argument('--data', default='randn', choices=['randn', 'relu', 'zero', 'const'])
    ap.add_argument('--engine', default=None, choices=['bf16x3'], help='compare the bf16x3 engine of the f32 mode with k_conv2d and k_conv3x3_h')
    a = ap.parse_args()
    if a.engine == 'bf16x3':
        return compare_bf16x3(a)
    dev = torch.device('cuda:0')
    g = torch.Generator(device='cpu').manual_seed(0)
    h = w = a.hw
    x = torch.zeros(a.batch, h + 2, w + 2, a.cin)
    x[:, 1:-1, 1:-1] = torch.randn(a.batch, h, w, a.cin, generator=g)
    wr = torch.randn(9, a.cin, a.cout, generator=g) * 0.05
    if a.data == 'relu':
        x = x.clamp_min(0)
    elif a.data == 'zero':
        x, wr = x * 0, wr * 0
    elif a.data == 'const':
        x, wr = (x != 0).float(), wr * 0 + 0.5
    xp = ops.pair16_from_f32(x.to(dev), math=1)
    wt = ops.pack_weight_split(wr.to(dev), 1)
    scale = torch.ones(wt.shape[-2], device=dev)
    shift = torch.zeros(wt.shape[-2], device=dev)
    y = torch.zeros(a.batch, h + 2, w + 2, a.cout, device=dev)

    def run():
        conv_layer(xp, (h + 2, w + 2), wt, scale, shift, True, y, (h + 2, w + 2), cin=a.cin, in_cstride=a.cin, ksize=3,
                   stride=1, in_off=0, out_cstride=a.cout, out_d=(1, 1), ho=h, wo=w, batch=a.batch, math=a.math)
    for _ in range(5):
        run()
    torch.cuda.synchronize()
    if os.environ.get('DZ_CHECK'):
        ref = torch.nn.functional.conv2d(x[:, 1:-1, 1:-1].permute(0, 3, 1, 2).double(), wr.reshape(3, 3, a.cin, a.cout).permute(3, 2, 0, 1).double(),
                                         padding=1).permute(0, 2, 3, 1).clamp_min(0)
        got = ops.pair16_to_f32(y, 1).cpu()[:, 1:-1, 1:-1].double()
        print('max |err| / max |ref| = %.3e   mean %.3e' % (float((got - ref).abs().max() / ref.abs().max()), float((got - ref).abs().mean() / ref.abs().mean())))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / a.iters
    fl = 2.0 * a.batch * h * w * 9 * a.cin * a.cout
    print('conv3x3 %dx%dx%d %d->%d data=%s  %.1f us  %.1f TF/s algorithmic' % (a.batch, h, w, a.cin, a.cout, a.data, us, fl / us * 1e-6))


def compare_bf16x3(a):
    """k_conv3x3_t | k_conv2d | k_conv3x3_h on the same layer and data, launches interleaved (the clock state is shared), median of
    --iters launches each."""
    import ctypes
    from detzero_amd import lib as L
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    h = w = a.hw
    x = torch.zeros(a.batch, h + 2, w + 2, a.cin, device=dev)
    x[:, 1:-1, 1:-1] = torch.randn(a.batch, h, w, a.cin, generator=g, device=dev)
    if a.data == 'relu':
        x = x.clamp_min(0)
    wr = torch.randn(9, a.cin, a.cout, generator=g, device=dev) * 0.05
    ops_ = {'bf16x3': (x, ops.pack_weight_limb3(wr), 0, 'bf16x3'), 'f32': (x, wr.contiguous(), 0, None),
            'f16x2': (ops.pair16_from_f32(x, math=1), ops.pack_weight_split(wr, 1), 1, None)}
    cp = ops_['bf16x3'][1].shape[-2]
    scale, shift = torch.ones(cp, device=dev), torch.zeros(cp, device=dev)
    ys = {k: torch.zeros(a.batch, h + 2, w + 2, a.cout, device=dev) for k in ops_}

    def run(k):
        xin, wt, math, eng = ops_[k]
        desc = dict(inp=xin.data_ptr(), out=ys[k].data_ptr(), w=wt.data_ptr(), scale=scale.data_ptr(), shift=shift.data_ptr(), batch=a.batch, ho=h, wo=w,
                    in_hp=h + 2, in_wp=w + 2, in_cstride=a.cin, in_coff=0, cin=a.cin, kh=3, kw=3, stride=1, in_off=0, out_hp=h + 2, out_wp=w + 2,
                    out_cstride=a.cout, out_coff=0, out_sy=1, out_sx=1, out_dy=1, out_dx=1, groups=1, cout_pad=cp, g_cout=[a.cout], g_ooff=[0], relu=1)
        ops.conv2d(desc, math=math, f32_engine=eng)
        return desc
    names = {}
    for k in ops_:
        d = ops._conv2d_desc(run(k))
        lib = L.load()
        names[k] = (lib.dz_conv3x3_limb3_variant(ctypes.byref(d)) if k == 'bf16x3' else
                    lib.dz_conv2d_variant_split(ctypes.byref(d), 0) if k == 'f16x2' else lib.dz_conv2d_variant(ctypes.byref(d))).decode()
    for _ in range(3):
        for k in ops_:
            run(k)
    torch.cuda.synchronize()
    got = ys['bf16x3'][:, 1:-1, 1:-1].double()
    ref = ys['f32'][:, 1:-1, 1:-1].double()
    print('bf16x3 vs f32 engine: max |diff| / max |ref| = %.3e' % float((got - ref).abs().max() / ref.abs().max()))
    ev = {k: [] for k in ops_}
    for _ in range(a.iters):
        for k in ops_:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(k)
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    fl = 2.0 * a.batch * h * w * 9 * a.cin * a.cout
    med = {k: sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in v)[len(v) // 2] for k, v in ev.items()}
    print('conv3x3 %dx%dx%d %d->%d data=%s, median of %d interleaved launches' % (a.batch, h, w, a.cin, a.cout, a.data, a.iters))
    for k in ('bf16x3', 'f32', 'f16x2'):
        tf = fl / med[k] * 1e-6
        extra = '  %.2f of the 419 TF/s six-MFMA peak' % (tf / 419.4) if k == 'bf16x3' else ''
        print('  %-7s %-24s %9.1f us  %7.1f TF/s algorithmic  %5.2f x k_conv2d%s' % (k, names[k], med[k], tf, med['f32'] / med[k], extra))


if __name__ == '__main__':
    main()
