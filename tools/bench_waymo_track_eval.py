"""Time the tracking metrics (detzero_amd/waymo_eval_tracking.py) on seeded sequences at the workload's shape.

    python tools/bench_waymo_track_eval.py [--sequences 20] [--frames 200] [--ref-sequences 1] [--ref-frames 40] [--repeat 3]

Each sequence has --frames frames and about 40 ground-truth tracks over the four object types (tens per type and frame for vehicles
and pedestrians); tracks drift, enter and leave.  Every track has a prediction track whose id persists, with a few id swaps between
neighbours, gaps of some frames and renamed returns, plus short-lived false-positive tracks; a prediction track's score jitters
around its own level.  Prints one JSON line per measurement:
  - waymo_evaluation with ['object'] and with ['object', 'range']: host wall time of the whole call (best of --repeat) and its
    split - conversion (info dicts -> sorted flat arrays and descriptors), the weights kernel, the chain kernel under each wave
    mapping (device time between events around the library call alone - ops.LaunchProfiler - the launches of all groups added), the
    host metrics;
  - the share of the 101 chains per (sequence, shard) that the distinct-cutoff merge removes;
  - the float64 restatement of the tests (tests/mot_eval_ref.py: one scipy solve per frame and chain) on the first --ref-frames
    frames of --ref-sequences sequences, and that time SCALED by the frame count (it is not run on the whole workload).
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {1: (4.6, 2.0, 1.7), 2: (0.9, 0.8, 1.75), 3: (0.6, 0.2, 0.9), 4: (1.8, 0.8, 1.7)}
NAMES = {1: 'Vehicle', 2: 'Pedestrian', 3: 'Sign', 4: 'Cyclist'}
TRACKS = {1: 22, 2: 12, 3: 2, 4: 4}
CLASS_NAMES = ['Vehicle', 'Pedestrian', 'Sign', 'Cyclist']


def sequence(name, n_frames, rng):
    """-> (prediction infos, whole ground-truth infos) of one sequence."""
    gt_rows, pd_rows = [[] for _ in range(n_frames)], [[] for _ in range(n_frames)]
    next_id = [0]

    def new_id():
        next_id[0] += 1
        return next_id[0]

    for t, n in TRACKS.items():
        for k in range(n):
            r, a = rng.uniform(3, 75), rng.uniform(-np.pi, np.pi)
            box = np.array([r * np.cos(a), r * np.sin(a), rng.uniform(-0.5, 1)] + [SIZES[t][q] * rng.uniform(0.9, 1.1) for q in range(3)] +
                           [rng.uniform(-np.pi, np.pi)])
            vel = rng.uniform(-0.4, 0.4, 2) * (t != 3)
            first, last = sorted(rng.randint(0, n_frames, 2)) if rng.rand() < 0.4 else (0, n_frames - 1)
            pid, level, gap = new_id(), rng.uniform(0.3, 0.95), 0
            for f in range(first, last + 1):
                cur = box.copy()
                cur[:2] += vel * f
                gt_rows[f].append((cur, t, 'g%d_%d' % (t, k), int(rng.randint(1, 3))))
                if gap == 0 and rng.rand() < 0.02:
                    gap = int(rng.randint(1, 5))                # the track is lost for some frames ...
                    if rng.rand() < 0.5:
                        pid = new_id()                          # ... and half the time comes back under a new id
                if gap > 0:
                    gap -= 1
                    continue
                noisy = cur.copy()
                noisy[:3] += rng.uniform(-1, 1, 3) * 0.05 * cur[3:6]
                noisy[6] += rng.uniform(-1, 1) * 0.03
                pd_rows[f].append((noisy, t, pid, float(np.clip(level + rng.uniform(-0.05, 0.05), 0.0, 1.0))))
        for _ in range(n // 2 + 1):                             # short-lived false-positive tracks
            r, a = rng.uniform(3, 75), rng.uniform(-np.pi, np.pi)
            box = np.array([r * np.cos(a), r * np.sin(a), 0.0, *SIZES[t], rng.uniform(-np.pi, np.pi)])
            first = int(rng.randint(0, n_frames))
            pid, level = new_id(), rng.uniform(0.0, 0.4)
            for f in range(first, min(n_frames, first + int(rng.randint(1, 12)))):
                pd_rows[f].append((box, t, pid, float(np.clip(level + rng.uniform(-0.05, 0.05), 0.0, 1.0))))
    for f in range(n_frames):                                   # a few id swaps between two predictions of one type
        if rng.rand() < 0.03 and len(pd_rows[f]) > 4:
            i, j = rng.choice(len(pd_rows[f]), 2, replace=False)
            a, b = pd_rows[f][i][2], pd_rows[f][j][2]
            if pd_rows[f][i][1] == pd_rows[f][j][1]:
                for g in range(f, n_frames):
                    pd_rows[g] = [(x, t, b if p == a else a if p == b else p, s) for x, t, p, s in pd_rows[g]]
    pds, gts = [], []
    for f in range(n_frames):
        pb = np.array([x for x, _, _, _ in pd_rows[f]], dtype=np.float32).reshape(-1, 7)
        gb = np.array([x for x, _, _, _ in gt_rows[f]], dtype=np.float32).reshape(-1, 7)
        pds.append({'boxes_lidar': pb, 'name': np.array([NAMES[t] for _, t, _, _ in pd_rows[f]], dtype='<U10'),
                    'score': np.array([s for _, _, _, s in pd_rows[f]], dtype=np.float32),
                    'obj_ids': np.array([p for _, _, p, _ in pd_rows[f]], dtype=np.int64), 'sequence_name': name, 'frame_id': f})
        gts.append({'sequence_name': name, 'frame_id': f, 'sample_idx': f, 'annos': {
            'gt_boxes_lidar': gb, 'name': np.array([NAMES[t] for _, t, _, _ in gt_rows[f]], dtype='<U10'),
            'difficulty': np.array([d for _, _, _, d in gt_rows[f]], dtype=np.int32),
            'num_points_in_gt': np.full(len(gb), 20, dtype=np.int64), 'obj_ids': np.array([g for _, _, g, _ in gt_rows[f]], dtype='<U16')}})
    return pds, gts


def workload(n_sequences, n_frames, seed=0):
    rng = np.random.RandomState(seed)
    pds, gts = [], []
    for q in range(n_sequences):
        p, g = sequence('seq_%03d' % q, n_frames, rng)
        pds += p
        gts += g
    return pds, gts


def scene_of(pds, gts, est):
    """The infos as the flat arrays of tests/mot_eval_ref.py."""
    pd, gt = est.waymo_arrays(pds, gts, CLASS_NAMES, fake_gt_infos=False)
    seq_p, seq_g = pd[1].astype(np.int64), gt[1].astype(np.int64)
    return {'pd_seq': seq_p, 'pd_frame': pd[0], 'pd_id': pd[2], 'pd_box': pd[3].astype(np.float32), 'pd_type': pd[4], 'pd_score': pd[5].astype(np.float32),
            'gt_seq': seq_g, 'gt_frame': gt[0], 'gt_id': gt[2], 'gt_box': gt[3].astype(np.float32), 'gt_type': gt[4], 'gt_diff': gt[5].astype(np.int32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sequences', type=int, default=20)
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--ref-sequences', type=int, default=1)
    ap.add_argument('--ref-frames', type=int, default=40)
    ap.add_argument('--repeat', type=int, default=3)
    args = ap.parse_args()
    import torch
    from detzero_amd import waymo_eval_tracking as wt
    est = wt.WaymoTrackingMetricsEstimator()
    pds, gts = workload(args.sequences, args.frames)
    n_pd, n_gt = sum(len(p['score']) for p in pds), sum(len(g['annos']['name']) for g in gts)
    quiet = contextlib.redirect_stdout(io.StringIO())

    def evaluate(config_type, mapping, timings=None):
        with quiet:
            return est.waymo_evaluation(pds, gts, CLASS_NAMES, config_type, fake_gt_infos=False, mapping=mapping, timings=timings)

    evaluate(['object'], 'wave')                                # first call: library load, allocator warm-up
    for config_type in (['object'], ['object', 'range']):
        best, split = None, {}
        for mapping in ('wave', 'workgroup'):
            for _ in range(args.repeat):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = evaluate(config_type, mapping)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if mapping == 'wave':
                    best = dt if best is None else min(best, dt)
                timings = {}
                evaluate(config_type, mapping, timings)
                for key, value in timings.items():
                    split[key] = min(split.get(key, value), value)
        with quiet:
            arrays = wt.chain_arrays(config_type, *est.waymo_arrays(pds, gts, CLASS_NAMES, fake_gt_infos=False))
        # distinct prediction sets per (sequence, shard): the distinct highest cutoffs of its predictions, and the last cutoff
        cut = ((arrays['pred_score'][:, None] >= np.array([k * 0.01 for k in range(100)] + [1.0], dtype=np.float32)[None, :]).sum(axis=1) - 1)
        run = 0
        for c in arrays['cdesc']:
            lo = arrays['pdesc'][c[0], 0]
            hi = arrays['pdesc'][c[0] + c[1] - 1, 0] + arrays['pdesc'][c[0] + c[1] - 1, 1]
            run += len(set(cut[lo:hi][cut[lo:hi] >= 0].tolist()) | {100})
        total = 101 * len(arrays['cdesc'])
        print(json.dumps({'what': 'waymo_evaluation (tracking)', 'config': config_type, 'sequences': args.sequences, 'frames': args.frames,
                          'predictions': n_pd, 'ground_truths': n_gt, 'problems': int(len(arrays['pdesc'])), 'largest_p_plus_g': int(arrays['cdesc'][:, 5].max()),
                          'groups': len(wt.sequence_groups(arrays)), 'seconds': round(best, 4), 'conversion_s': round(split['conversion'], 4),
                          'weights_kernel_ms': round(split['weights'] * 1e3, 3), 'chain_kernel_wave_ms': round(split['chain[wave]'] * 1e3, 3),
                          'chain_kernel_workgroup_ms': round(split['chain[workgroup]'] * 1e3, 3), 'host_metrics_s': round(split['metrics'], 5),
                          'chains': total, 'chains_run': run, 'share_removed_by_merge': round(1.0 - run / total, 4),
                          'vehicle_l2_mota': round(out['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_2/MOTA'][0], 4),
                          'vehicle_l2_mismatch': round(out['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_2/MISMATCH'][0], 5)}), flush=True)

    # the float64 restatement on a subset, scaled
    from tests import mot_eval_ref as ref
    nq, nf = min(args.ref_sequences, args.sequences), min(args.ref_frames, args.frames)
    sub_p = [p for p in pds if int(p['sequence_name'][4:]) < nq and p['frame_id'] < nf]
    sub_g = [g for g in gts if int(g['sequence_name'][4:]) < nq and g['frame_id'] < nf]
    with quiet:
        s = scene_of(sub_p, sub_g, est)
        arrays = wt.chain_arrays(['object'], *est.waymo_arrays(sub_p, sub_g, CLASS_NAMES, fake_gt_infos=False))
    t0 = time.perf_counter()
    table = ref.counts(['object'], '3d', s)
    dt = time.perf_counter() - t0
    same = bool(np.array_equal(wt.chain_counts(arrays)[..., :4], table[..., :4]))
    scale = args.sequences * args.frames / (nq * nf)
    print(json.dumps({'what': 'float64 restatement (scipy per frame and chain, distinct chains only), CPU', 'config': ['object'], 'sequences_run': nq,
                      'frames_run': nf, 'seconds_run': round(dt, 3), 'seconds_scaled_to_workload': round(dt * scale, 1), 'scaled': True,
                      'counts_equal_device_on_subset': same}), flush=True)


if __name__ == '__main__':
    main()
