#!/usr/bin/env python
"""Per-layer timing of the sparse 3-D backbone on one MI355X (development tool, not the headline bench).

    python tools/bench_spconv.py [--batch 4] [--reps 20] [--points 160000]
    python tools/bench_spconv.py --math f32 --f32-engine gather,xrun,xrun_bf16x3 [--rounds 2]
    python tools/bench_spconv.py --math f32 --f32-gather mfma32,bf16x3 [--rounds 2]
    python tools/bench_spconv.py --math f32 --f32-small gather,wave_bf16x3 [--rounds 2]

With --f32-engine: the submanifold layers of the 32 / 64 / 128-channel levels in exact fp32 on each listed engine, on the same
tensors and tables of one level, launches interleaved in one process (blocks of 5 launches per engine, alternating).
With --f32-gather: every distinct layer of the backbone on its plain table (the strided layers and conv_out included) in exact fp32
on each listed gather arithmetic - k_spconv and k_spconv_gt - on the same tensors and tables, interleaved in the same way.
With --f32-small: the layers the wave-private bf16x3 kernel covers (16 -> 16 with and without residual, 16 -> 32) on k_spconv_gt (what
f32_gather='bf16x3' runs, the 'gather' arm) and on k_spconv_wt, on the same tensors and tables, interleaved in the same way.

Builds the sparse levels of a batch of synthetic frames once, then times every distinct sparse conv of
VoxelResBackBone8x separately (HIP events on the launch stream) and prints rows, rulebook pairs, mean valid
taps per row, taps with at least one pair per 16-/64-/128-row tile, algorithmic TF/s and the "dense-tap"
TF/s (what the matrix pipe really executes with tile-level tap skipping).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--points', type=int, default=160000)
    ap.add_argument('--math', default='f32')
    ap.add_argument('--zero', action='store_true', help='time the layers on all-zero activations and weights (matrix-pipe power test)')
    ap.add_argument('--only', default='', help='comma list of cin-cout pairs to time (default: every layer)')
    ap.add_argument('--f32-engine', default='', help='comma list of gather | xrun | xrun_bf16x3: A/B of the fp32 engines per submanifold layer')
    ap.add_argument('--f32-gather', default='', help='comma list of mfma32 | bf16x3: A/B of the fp32 gather arithmetics per layer, strided ones included')
    ap.add_argument('--f32-small', default='', help='comma list of gather | wave_bf16x3: A/B of k_spconv_gt and k_spconv_wt on the 16-input-channel layers')
    ap.add_argument('--rounds', type=int, default=2, help='with --f32-engine / --f32-gather / --f32-small: repetitions of the whole comparison')
    args = ap.parse_args()
    if args.f32_engine:
        return compare_f32_engines(args)
    if args.f32_gather:
        return compare_f32_gather(args)
    if args.f32_small:
        return compare_f32_small(args)
    dev = torch.device('cuda', 0)
    from detzero_amd import ops
    from detzero_amd.centerpoint import FramePipeline, synth_detector
    from detzero_amd.synth import VOXEL_SIZE_01, synth_waymo_frame
    model, cfg, info = synth_detector(VOXEL_SIZE_01, seed=0)
    model = model.to(dev)
    pipe = FramePipeline(model, info, math=args.math)
    mm = ops.math_id(args.math)
    frames = [torch.from_numpy(synth_waymo_frame(i, args.points)).to(dev) for i in range(args.batch)]
    pipe.calibrate(frames[:4])
    feats, coords, d_n = pipe._voxelize(frames)

    calls = []
    real = ops.spconv_forward

    def spy(f, nbr, out_level, w, scale, shift, residual=None, relu=True, out=None, in_level=None, math=0, cout=None, f32_engine=None):
        calls.append((f, nbr, out_level, w, scale, shift, residual, relu, in_level, f32_engine))
        return real(f, nbr, out_level, w, scale, shift, residual, relu, out, in_level, math, cout, f32_engine)
    ops.spconv_forward = spy
    import detzero_amd.det_modules as dm
    dm.ops.spconv_forward = spy
    model.backbone3d.run_pyramid(model.backbone3d.build_pyramid(feats, coords, args.batch, d_n, caps=[c * args.batch for c in pipe.level_caps]))
    ops.spconv_forward = real
    dm.ops.spconv_forward = real
    torch.cuda.synchronize()

    seen = {}
    total = 0.0
    for (f, nbr, lvl, w, scale, shift, residual, relu, in_level, f32e) in calls:
        kvol = w.shape[0]
        variant = 'x' if nbr.xwin is not None and (w.shape[1] == w.shape[2] or f32e == 'xrun_bf16x3') else 'g'
        cin, cout = (w.shape[2], scale.shape[0]) if mm else (w.shape[1], w.shape[1]) if f32e == 'xrun_bf16x3' else (w.shape[1], w.shape[2])
        kname = ''
        if variant == 'x':          # the x-run kernel instance that ran (pair16 or exact fp32)
            from detzero_amd import lib as L
            kname = '  ' + (L.load().dz_spconv_x_variant(cin, cout) if mm else L.load().dz_spconv_x_limb3_variant(cin, cout) if f32e == 'xrun_bf16x3'
                             else L.load().dz_spconv_x_f32_variant(cin, cout)).decode()
        key = (kvol, cin, cout, lvl.cap, residual is not None, id(nbr))
        if args.only and '%d-%d' % (cin, cout) not in args.only.split(','):
            continue
        m = lvl.num_active()
        if key not in seen:
            valid = ops.unpack_table(nbr)[:, :m] >= 0
            pairs = int(valid.sum().item())

            def tile_taps(bm):
                pad = (-m) % bm
                v = torch.cat([valid, valid.new_zeros((kvol, pad))], dim=1).view(kvol, -1, bm).any(dim=2)
                return float(v.sum().item()) / v.shape[1]
            stats = (pairs, tile_taps(16), tile_taps(32), tile_taps(64), tile_taps(128))
            out = torch.empty((lvl.cap, cout), dtype=torch.float32, device=dev)
            if args.zero:
                f, w = torch.zeros_like(f), torch.zeros_like(w)
                residual = torch.zeros_like(residual) if residual is not None else None
            for _ in range(3):
                real(f, nbr, lvl, w, scale, shift, residual, relu, out, in_level, mm, f32_engine=f32e)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                real(f, nbr, lvl, w, scale, shift, residual, relu, out, in_level, mm, f32_engine=f32e)
            e1.record()
            torch.cuda.synchronize()
            us = 1000.0 * e0.elapsed_time(e1) / args.reps
            seen[key] = (us, stats)
        us, (pairs, t16, t32, t64, t128) = seen[key]
        halo = ''
        if nbr.tiles is not None:
            nh = nbr.tiles[1][:(m + 511) // 512].float()
            halo = '  tiles: halo/rows %.2f max %d' % (float(nh.sum().item()) / max(m, 1), int(nh.max().item()))
        total += us
        flop = 2.0 * pairs * cin * cout
        print(variant + ' k%-2d %3d->%-3d rows %8d pairs/row %5.2f taps/tile[16|32|64|128] %5.2f %5.2f %5.2f %5.2f  %8.1f us  alg %6.2f TF/s  '
              'dense64 %6.2f TF/s%s' % (kvol, cin, cout, m, pairs / max(m, 1), t16, t32, t64, t128, us, flop / us / 1e6,
                                        2.0 * m * t64 * cin * cout / us / 1e6, ('  +res' if residual is not None else '') + halo + kname))
    print('sum over the %d sparse convs: %.1f us per step (%.1f us per frame)' % (len(calls), total, total / args.batch))


BF16X3_PEAK_TFS = 419.0        # fp32-equivalent peak of six bf16 MFMAs per product: 2516 TF/s dense bf16 / 6


def compare_f32_engines(args):
    dev = torch.device('cuda', 0)
    from detzero_amd import lib as L
    from detzero_amd import ops
    from detzero_amd.centerpoint import FramePipeline, set_sparse_engine, synth_detector
    from detzero_amd.det_modules import K3, P1, S1
    from detzero_amd.synth import VOXEL_SIZE_01, synth_waymo_frame
    engines = [e for e in args.f32_engine.split(',') if e]
    for e in engines:
        if e not in ops.SPARSE_F32_ENGINES:
            raise SystemExit('unknown fp32 sparse engine %r (%s)' % (e, ' | '.join(ops.SPARSE_F32_ENGINES)))
    if args.math != 'f32':
        raise SystemExit('--f32-engine compares the engines of --math f32')
    lib = L.load()
    model, cfg, info = synth_detector(VOXEL_SIZE_01, seed=0)
    model = model.to(dev)
    bb = model.backbone3d
    set_sparse_engine(model, bb.engine, f32_engine='xrun')          # tables with windows: every engine's index
    pipe = FramePipeline(model, info, math='f32')
    frames = [torch.from_numpy(synth_waymo_frame(i, args.points)).to(dev) for i in range(args.batch)]
    pipe.calibrate(frames[:4])
    feats, coords, d_n = pipe._voxelize(frames)
    calls = []
    real = ops.spconv_forward

    def spy(f, nbr, out_level, w, scale, shift, residual=None, relu=True, out=None, in_level=None, math=0, cout=None, f32_engine=None):
        calls.append((f, nbr, out_level, w, scale, shift, residual, relu))
        return real(f, nbr, out_level, w, scale, shift, residual, relu, out, in_level, math, cout, f32_engine)
    import detzero_amd.det_modules as dm
    ops.spconv_forward = dm.ops.spconv_forward = spy
    bb.run_pyramid(bb.build_pyramid(feats, coords, args.batch, d_n, caps=[c * args.batch for c in pipe.level_caps]))
    ops.spconv_forward = dm.ops.spconv_forward = real
    torch.cuda.synchronize()

    layers, seen = [], set()
    for (f, nbr, lvl, w, scale, shift, residual, relu) in calls:
        c = int(w.shape[1])
        if nbr.xwin is None or w.shape[1] != w.shape[2] or (c, residual is not None) in seen:
            continue
        if args.only and '%d-%d' % (c, c) not in args.only.split(','):
            continue
        seen.add((c, residual is not None))
        layers.append((f, nbr, lvl, w, scale, shift, residual, relu))
    plain = {}
    for rnd in range(args.rounds):
        for (f, nbr, lvl, w, scale, shift, residual, relu) in layers:
            c = int(w.shape[1])
            m = lvl.num_active()
            if id(lvl) not in plain:
                plain[id(lvl)] = (lvl.neighbors_to(lvl, K3, S1, P1), ops.table_pairs(nbr, m))
            tab_g, pairs = plain[id(lvl)]
            out = torch.empty((lvl.cap, c), dtype=torch.float32, device=dev)
            runs = {}
            for e in engines:
                if e == 'gather':
                    runs[e] = (lib.dz_spconv_variant(c, c).decode(), lambda: real(f, tab_g, lvl, w, scale, shift, residual, relu, out))
                elif e == 'xrun_bf16x3' and lib.dz_spconv_x_limb3_window_rows(c, c) > 0:
                    wl = ops.pack_weight_limb3(w, cout_mult=32)
                    runs[e] = (lib.dz_spconv_x_limb3_variant(c, c).decode(),
                               lambda wl=wl: real(f, nbr, lvl, wl, scale, shift, residual, relu, out, f32_engine='xrun_bf16x3'))
                else:               # 'xrun', and a width the bf16x3 kernel does not ship for: what the backbone launches then
                    runs[e] = (lib.dz_spconv_x_f32_variant(c, c).decode(), lambda: real(f, nbr, lvl, w, scale, shift, residual, relu, out))
            for e in engines:
                for _ in range(3):
                    runs[e][1]()
            ms = {e: 0.0 for e in engines}
            blocks, per = max(1, args.reps // 5), 5
            evs = []
            for _ in range(blocks):
                for e in engines:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(per):
                        runs[e][1]()
                    e1.record()
                    evs.append((e, e0, e1))
            torch.cuda.synchronize()
            for e, e0, e1 in evs:
                ms[e] += e0.elapsed_time(e1)
            flop = 2.0 * pairs * c * c
            for e in engines:
                us = 1000.0 * ms[e] / (blocks * per)
                tfs = flop / us / 1e6
                print('round %d  %3d->%-3d rows %8d pairs/row %5.2f %s  %-12s %-22s %9.1f us  alg %6.2f TF/s  %5.1f %% of the %.0f TF/s six-MFMA peak'
                      % (rnd, c, c, m, pairs / max(m, 1), '+res' if residual is not None else '    ', e, runs[e][0], us, tfs,
                         100.0 * tfs / BF16X3_PEAK_TFS, BF16X3_PEAK_TFS), flush=True)


def compare_f32_gather(args):
    dev = torch.device('cuda', 0)
    from detzero_amd import lib as L
    from detzero_amd import ops
    arith = [e for e in args.f32_gather.split(',') if e]
    for e in arith:
        if e not in ops.SPARSE_F32_GATHER_ENGINES:
            raise SystemExit('unknown fp32 gather arithmetic %r (%s)' % (e, ' | '.join(ops.SPARSE_F32_GATHER_ENGINES)))
    if args.math != 'f32':
        raise SystemExit('--f32-gather compares the gather arithmetics of --math f32')
    lib = L.load()
    real = ops.spconv_forward
    layers = _plain_layers(args, dev)
    for rnd in range(args.rounds):
        for (f, nbr, lvl, w, scale, shift, residual, relu) in layers:
            kvol, cin, cout = (int(v) for v in w.shape)
            out = torch.empty((lvl.cap, cout), dtype=torch.float32, device=dev)
            runs = {}
            for e in arith:
                if e == 'bf16x3' and lib.dz_spconv_limb3_tile_rows(cin, cout) > 0:
                    wl = ops.pack_weight_limb3(w, cout_mult=32)
                    runs[e] = (lib.dz_spconv_limb3_variant(cin, cout).decode(),
                               lambda wl=wl: real(f, nbr, lvl, wl, scale, shift, residual, relu, out, cout=cout, f32_gather='bf16x3'))
                else:               # 'mfma32', and a layer the bf16x3 kernel does not ship for: what the backbone launches then
                    runs[e] = (lib.dz_spconv_variant(cin, cout).decode(), lambda: real(f, nbr, lvl, w, scale, shift, residual, relu, out))
            _alternate_and_print(args, rnd, arith, runs, nbr, lvl, w, residual)


def compare_f32_small(args):
    dev = torch.device('cuda', 0)
    from detzero_amd import lib as L
    from detzero_amd import ops
    arms = [e for e in args.f32_small.split(',') if e]
    for e in arms:
        if e not in ops.SPARSE_F32_SMALL_ENGINES:
            raise SystemExit('unknown fp32 small-layer engine %r (%s)' % (e, ' | '.join(ops.SPARSE_F32_SMALL_ENGINES)))
    if args.math != 'f32':
        raise SystemExit('--f32-small compares the kernels of --math f32')
    lib = L.load()
    real = ops.spconv_forward
    layers = [l for l in _plain_layers(args, dev) if lib.dz_spconv_limb3_w_tile_rows(int(l[3].shape[1]), int(l[3].shape[2])) > 0]
    if not layers:
        raise SystemExit('--f32-small: the library ships k_spconv_wt for none of the selected layers')
    for rnd in range(args.rounds):
        for (f, nbr, lvl, w, scale, shift, residual, relu) in layers:
            kvol, cin, cout = (int(v) for v in w.shape)
            out = torch.empty((lvl.cap, cout), dtype=torch.float32, device=dev)
            wl = ops.pack_weight_limb3(w, cout_mult=32)
            runs = {'gather': (lib.dz_spconv_limb3_variant(cin, cout).decode(),
                               lambda: real(f, nbr, lvl, wl, scale, shift, residual, relu, out, cout=cout, f32_gather='bf16x3')),
                    'wave_bf16x3': (lib.dz_spconv_limb3_w_variant(cin, cout).decode(),
                                    lambda: real(f, nbr, lvl, wl, scale, shift, residual, relu, out, cout=cout, f32_small='wave_bf16x3'))}
            _alternate_and_print(args, rnd, arms, runs, nbr, lvl, w, residual)


def _plain_layers(args, dev):
    """Every distinct sparse convolution of one exact-fp32 backbone pass on plain tables: (feats, table, level, taps, scale, shift,
    residual, relu) per layer."""
    from detzero_amd import ops
    from detzero_amd.centerpoint import FramePipeline, set_sparse_engine, synth_detector
    from detzero_amd.synth import VOXEL_SIZE_01, synth_waymo_frame
    model, cfg, info = synth_detector(VOXEL_SIZE_01, seed=0)
    model = model.to(dev)
    bb = model.backbone3d
    set_sparse_engine(model, bb.engine, f32_engine='gather', f32_gather='mfma32')          # plain tables everywhere
    pipe = FramePipeline(model, info, math='f32')
    frames = [torch.from_numpy(synth_waymo_frame(i, args.points)).to(dev) for i in range(args.batch)]
    pipe.calibrate(frames[:4])
    feats, coords, d_n = pipe._voxelize(frames)
    calls = []
    real = ops.spconv_forward

    def spy(f, nbr, out_level, w, scale, shift, residual=None, relu=True, out=None, in_level=None, math=0, cout=None):
        calls.append((f, nbr, out_level, w, scale, shift, residual, relu))
        return real(f, nbr, out_level, w, scale, shift, residual, relu, out, in_level, math, cout)
    import detzero_amd.det_modules as dm
    ops.spconv_forward = dm.ops.spconv_forward = spy
    bb.run_pyramid(bb.build_pyramid(feats, coords, args.batch, d_n, caps=[c * args.batch for c in pipe.level_caps]))
    ops.spconv_forward = dm.ops.spconv_forward = real
    torch.cuda.synchronize()

    layers, seen = [], set()
    for call in calls:
        f, nbr, lvl, w, scale, shift, residual, relu = call
        key = (int(w.shape[0]), int(w.shape[1]), int(w.shape[2]), residual is not None, id(nbr))
        if key in seen or (args.only and '%d-%d' % key[1:3] not in args.only.split(',')):
            continue
        seen.add(key)
        layers.append(call)
    return layers


def _alternate_and_print(args, rnd, arms, runs, nbr, lvl, w, residual):
    """runs: arm -> (kernel name, launch).  Three warm-up launches per arm, then blocks of 5 launches per arm alternating in this process,
    each block between two events; one line per arm."""
    from detzero_amd import ops
    kvol, cin, cout = (int(v) for v in w.shape)
    m = lvl.num_active()
    pairs = ops.table_pairs(nbr, m)
    for e in arms:
        for _ in range(3):
            runs[e][1]()
    ms = {e: 0.0 for e in arms}
    blocks, per = max(1, args.reps // 5), 5
    evs = []
    for _ in range(blocks):
        for e in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per):
                runs[e][1]()
            e1.record()
            evs.append((e, e0, e1))
    torch.cuda.synchronize()
    for e, e0, e1 in evs:
        ms[e] += e0.elapsed_time(e1)
    flop = 2.0 * pairs * cin * cout
    for e in arms:
        us = 1000.0 * ms[e] / (blocks * per)
        tfs = flop / us / 1e6
        print('round %d  k%-2d %3d->%-3d rows %8d pairs/row %5.2f %s  %-11s %-24s %9.1f us  alg %6.2f TF/s  %5.1f %% of the %.0f TF/s six-MFMA peak'
              % (rnd, kvol, cin, cout, m, pairs / max(m, 1), '+res' if residual is not None else '    ', e, runs[e][0], us, tfs,
                 100.0 * tfs / BF16X3_PEAK_TFS, BF16X3_PEAK_TFS), flush=True)


if __name__ == '__main__':
    main()
