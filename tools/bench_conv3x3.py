"""One BEV 3x3 layer (16 x 188 x 188, 128 -> 128 channels, pair16) timed alone: us per launch and algorithmic TF/s.
--data picks the operands (time vs operand data: clock / power); DZ_CHECK=1 also checks the result against float64."""
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
    a = ap.parse_args()
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


if __name__ == '__main__':
    main()
