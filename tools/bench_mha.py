#!/usr/bin/env python
"""Per-shape timing of the refiner's attention core in the exact-fp32 mode (development tool).

    python tools/bench_mha.py [--reps 5] [--rounds 3]

dz_mha_core ('mfma32', csrc/mha.hip) and dz_mha_core_limb3 ('bf16x3', csrc/mha_t.hip) through ops.mha_core, alternating shape by
shape in one process: `--rounds` rounds of `--reps` calls each with event timing; prints the median, the spread (max - min) / median of
the rounds, the algorithmic TF/s (4 b lq lk E flop) and the ratio of the medians; dz_mha_core_split in f16x2 for orientation.
Shapes: PRM's cross-attention (96 tracks x 200 queries x 9600 keys x 8 heads, masked) and self-attention (200 x 200), GRM's
self-attention (128 objects x 3 queries), and lk 64 / 256 / 1024 at lq 200 - the key lengths LIMB3_ATTN_MIN_KEYS
(detzero_amd/refine_modules.py) is chosen from.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

#          name               b    lq   lk  heads masked
SHAPES = [('PRM cross', 96, 200, 9600, 8, True),
          ('PRM self', 96, 200, 200, 8, True),
          ('GRM self', 128, 3, 3, 8, False),
          ('lk 64', 96, 200, 64, 8, True),
          ('lk 256', 96, 200, 256, 8, True),
          ('lk 1024', 96, 200, 1024, 8, True)]
ENGINES = (('mfma32', dict()), ('bf16x3', dict(f32_engine='bf16x3')), ('f16x2', dict(math=1)))


def time_call(fn, reps):
    """Microseconds per call (warm)."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    from detzero_amd import ops
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(0)
    med = lambda v: sorted(v)[len(v) // 2]           # noqa: E731
    for name, b, lq, lk, heads, masked in SHAPES:
        e = heads * 32
        q = torch.randn((b, lq, e), generator=g).to(dev)
        k = torch.randn((b, lk, e), generator=g).to(dev)
        v = torch.randn((b, lk, e), generator=g).to(dev)
        mask = None
        if masked:
            mask = (torch.rand((b, lk), generator=g) < 0.2).to(dev)
            mask[:, 0] = False
        t = {n: [] for n, _ in ENGINES}
        for _ in range(args.rounds):
            for n, kw in ENGINES:
                t[n].append(time_call(lambda: ops.mha_core(q, k, v, mask, heads, 32 ** -0.5, **kw), args.reps))
        line = '%-10s %3d x %3d x %4d x %d' % (name, b, lq, lk, heads)
        for n, _ in ENGINES:
            us = med(t[n])
            line += '   %s %8.1f us  spread %4.1f %%  %6.1f TF/s' % (n, us, 100.0 * (max(t[n]) - min(t[n])) / us, 4.0 * b * lq * lk * e / us / 1e6)
        line += '   mfma32 / bf16x3 %.2f' % (med(t['mfma32']) / med(t['bf16x3']))
        print(line, flush=True)
        del q, k, v, mask


if __name__ == '__main__':
    main()
