"""Time the detection metrics (detzero_amd/waymo_eval.py) on a seeded workload at validation scale per frame.

    python tools/bench_waymo_eval.py [--frames 2000] [--ref-frames 50] [--repeat 3]

About 150 predictions and 40 ground truths per frame over the four object types.  Prints one JSON line per measurement:
  - waymo_evaluation with ['object'] and with ['object', 'range'] (host wall time of the whole call, best of --repeat);
  - the split of one call: conversion to flat arrays, sort + descriptors + kernel (+ reduction) + status read, host AP - and the
    kernel's device time from ops.LaunchProfiler, for the two accumulation schemes side by side;
  - the float64 restatement of the tests (tests/waymo_eval_ref.py: one scipy solve per problem and per cutoff) on the first
    --ref-frames frames, and that time SCALED by the frame count (it is not run on all frames).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {1: (4.6, 2.0, 1.7), 2: (0.9, 0.8, 1.75), 3: (0.6, 0.2, 0.9), 4: (1.8, 0.8, 1.7)}
NAMES = {1: 'Vehicle', 2: 'Pedestrian', 3: 'Truck', 4: 'Cyclist'}
GT_PER_FRAME = {1: 22, 2: 12, 3: 2, 4: 4}
CLASS_NAMES = ['Vehicle', 'Pedestrian', 'Truck', 'Cyclist']


def workload(n_frames, seed=0):
    rng = np.random.RandomState(seed)
    pds, gts = [], []
    for _ in range(n_frames):
        gb, gt_t, pb, pt, ps = [], [], [], [], []
        for t, n in GT_PER_FRAME.items():
            r, a = rng.uniform(3, 75, n), rng.uniform(-np.pi, np.pi, n)
            box = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-0.5, 1, n)] + [SIZES[t][k] * rng.uniform(0.9, 1.1, n) for k in range(3)] +
                           [rng.uniform(-np.pi, np.pi, n)], axis=1)
            gb.append(box)
            gt_t += [t] * n
            for k in range(3):                                  # three predictions per ground truth, tight to loose
                noisy = box.copy()
                noisy[:, :3] += rng.uniform(-1, 1, (n, 3)) * (0.03, 0.1, 0.25)[k] * box[:, 3:6]
                noisy[:, 6] += rng.uniform(-1, 1, n) * (0.02, 0.06, 0.3)[k]
                pb.append(noisy)
                pt += [t] * n
                ps.append(rng.uniform(0.05, 1.0, n) * (1.0, 0.8, 0.5)[k])
            m = n // 2 + 1                                      # free false positives
            r, a = rng.uniform(3, 75, m), rng.uniform(-np.pi, np.pi, m)
            pb.append(np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-0.5, 1, m)] + [np.full(m, SIZES[t][k]) for k in range(3)] +
                               [rng.uniform(-np.pi, np.pi, m)], axis=1))
            pt += [t] * m
            ps.append(rng.uniform(0.0, 0.4, m))
        gb, pb = np.concatenate(gb).astype(np.float32), np.concatenate(pb).astype(np.float32)
        gts.append({'gt_boxes_lidar': gb, 'name': np.array([NAMES[t] for t in gt_t]), 'difficulty': rng.randint(1, 3, len(gb)).astype(np.int32),
                    'num_points_in_gt': np.full(len(gb), 20, dtype=np.int64)})
        pds.append({'boxes_lidar': pb, 'name': np.array([NAMES[t] for t in pt]), 'score': np.concatenate(ps).astype(np.float32)})
    return pds, gts


def wall(fn, repeat):
    import torch
    best = None
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2000)
    ap.add_argument('--ref-frames', type=int, default=50)
    ap.add_argument('--repeat', type=int, default=3)
    args = ap.parse_args()
    import contextlib
    import io
    from detzero_amd import ops, waymo_eval
    est = waymo_eval.WaymoDetectionMetricsEstimator()
    pds, gts = workload(args.frames)
    n_pd, n_gt = sum(len(p['score']) for p in pds), sum(len(g['name']) for g in gts)
    quiet = contextlib.redirect_stdout(io.StringIO())

    def evaluate(config_type):
        with quiet:
            return est.waymo_evaluation(pds, gts, CLASS_NAMES, config_type, distance_thresh=1000, fake_gt_infos=False)

    evaluate(['object'])                                        # first call: library load, allocator warm-up
    for config_type in (['object'], ['object', 'range']):
        dt, out = wall(lambda: evaluate(config_type), args.repeat)
        print(json.dumps({'what': 'waymo_evaluation', 'config': config_type, 'frames': args.frames, 'predictions': n_pd, 'ground_truths': n_gt,
                          'seconds': round(dt, 4), 'vehicle_l2_aph': round(out['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_2/APH'][0], 4)}), flush=True)
        with quiet:
            t_conv, (pd, gt) = wall(lambda: est.waymo_arrays(pds, gts, CLASS_NAMES, config_type, 1000, False), args.repeat)
        t_prob, arrays = wall(lambda: waymo_eval.problem_arrays(config_type, len(gts), *pd, *gt), args.repeat)
        for scheme in ('atomic', 'slots'):
            t_match, table = wall(lambda: waymo_eval.match_counts(config_type, len(gts), *arrays, scheme=scheme), args.repeat)
            ops.PROFILER = ops.LaunchProfiler()
            waymo_eval.match_counts(config_type, len(gts), *arrays, scheme=scheme)
            kernel_ms = sum(v['ms'] for v in ops.PROFILER.summary().values())
            ops.PROFILER = None
            t_ap, _ = wall(lambda: waymo_eval.metrics_from_counts(table, config_type), args.repeat)
            print(json.dumps({'what': 'split', 'config': config_type, 'scheme': scheme, 'convert_s': round(t_conv, 4),
                              'shard_keys_s': round(t_prob, 4), 'sort_desc_kernel_read_s': round(t_match, 4),
                              'kernel_device_ms': round(kernel_ms, 3), 'host_ap_s': round(t_ap, 4)}), flush=True)

    # the float64 restatement on a subset, scaled
    from tests import waymo_eval_ref as ref
    n = min(args.ref_frames, args.frames)
    with quiet:
        pd, gt = est.waymo_arrays(pds[:n], gts[:n], CLASS_NAMES, ['object'], 1000, False)
    t0 = time.perf_counter()
    counts, _, fixed = ref.counts(['object'], '3d', n, pd[0], pd[1], pd[2], pd[3], gt[0], gt[1], gt[2], gt[3])
    dt = time.perf_counter() - t0
    arrays = waymo_eval.problem_arrays(['object'], n, *pd, *gt)
    same = bool(np.array_equal(waymo_eval.match_counts(['object'], n, *arrays)[..., :3], counts))
    print(json.dumps({'what': 'float64 restatement (scipy per problem and cutoff), CPU', 'config': ['object'], 'frames_run': n,
                      'seconds_run': round(dt, 3), 'seconds_scaled_to_frames': round(dt * args.frames / n, 1), 'scaled': True,
                      'frames': args.frames, 'counts_equal_device_on_subset': same}), flush=True)


if __name__ == '__main__':
    main()
