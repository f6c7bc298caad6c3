#!/usr/bin/env python
"""bench.py with the exact-fp32 switches that have no environment variable set on the detector it builds: one arm of a whole-pass A/B
(DESIGN.md 2a-quater, 2h-quater).  Everything behind `--` goes to bench.py unchanged; the engines that do have a variable are set
in the environment as usual.

    DZ_TUNE_DENSE_F32_ENGINE=bf16x3 DZ_TUNE_SPCONV_F32_ENGINE=xrun_bf16x3 DZ_TUNE_SPCONV_F32_GATHER=bf16x3 \\
        python tools/bench_f32_switches.py --f32-generic bf16x3 [--f32-small wave_bf16x3] -- --gpus 1 --math f32 --batch 32 --steps 100 --warmup 10
"""
import argparse
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    own, rest = (sys.argv[1:sys.argv.index('--')], sys.argv[sys.argv.index('--') + 1:]) if '--' in sys.argv else (sys.argv[1:], [])
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--f32-generic', default=None, help='mfma32 | bf16x3: set_dense_engine(model, <its 3 x 3 engine>, f32_generic=...)')
    ap.add_argument('--f32-small', default=None, help='gather | wave_bf16x3: set_sparse_engine(model, <its engine>, f32_small=...)')
    args = ap.parse_args(own)
    from detzero_amd import centerpoint
    build = centerpoint.synth_detector

    def switched(*a, **kw):
        model, cfg, info = build(*a, **kw)
        if args.f32_generic is not None:
            centerpoint.set_dense_engine(model, model.backbone2d.f32_dense_engine, f32_generic=args.f32_generic)
        if args.f32_small is not None:
            centerpoint.set_sparse_engine(model, model.backbone3d.engine, f32_small=args.f32_small)
        return model, cfg, info
    centerpoint.synth_detector = switched
    sys.argv = [os.path.join(ROOT, 'bench.py')] + rest
    runpy.run_path(sys.argv[0], run_name='__main__')


if __name__ == '__main__':
    main()
