#!/usr/bin/env python
"""Tracker throughput on one sequence, for the record: the device ops (csrc/track.hip) and the numpy restatement of the same seven
ops (tests/track_ref.py) under the same orchestration (detzero_amd.track_models.TrackManager, shipped waymo_detzero_track values:
two-stage IoUBEV association, TRACK_MERGE, REVERSE_TRACKING, DEATH_AGE -1) and the same input.

    python tools/bench_track.py [--frames 200] [--objects 150] [--steps 3] [--no-numpy]

Input: one seeded sequence (detzero_amd.synth.synth_track_sequence) of --frames frames with about --objects detections each.
Prints one JSON line: sequences/s and ms per frame-pass of both, the number of tracks, and whether the two results agree.

    python tools/bench_track.py --batch 1 16 64 [--repeats 5]

The batched path (TrackManager.forward_batch, csrc/track_seq.hip) beside the per-sequence path (TrackManager.forward): for every N
the seeded sequence under N seeds, once through forward() one sequence after another and once through one forward_batch call.
One JSON line per N: sequences/s of both (host time per call, median of --repeats after a warm-up call), whether tracks, hits
and boxes agree, and how many sequences ran batched and how many fell back to forward() inside forward_batch.

    python tools/bench_track.py --filter AB3DMOT [--batch 16]
    python tools/bench_track.py --filter AB3DMOT --reference-only

The same two measurements with the values of waymo_ab3dmot.yaml (FILTER.NAME AB3DMOT: float64 filter on the device, one-stage IoUBEV
association, BIRTH_AGE 3 / DEATH_AGE 2, no merge, no reverse pass); the numpy side is tests/track_ab3dmot_ref.py.
--reference-only opens no GPU: it prints the wall time of the reference's own AB3DMOT and TrackManager classes on the same sequence on
this CPU, the baseline (needs the reference tree and the fixture generator's stand-ins: tests/golden/gen_track_ab3dmot_golden.py).
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODEL = {
    'FILTER': {'NAME': 'KalmanFilter', 'X_DIM': 5, 'Z_DIM': 3, 'Q': [5, 15], 'P': [50, 1000], 'R': 0.1, 'DELTA_T': 0.1},
    'TRACK_AGE': {'BIRTH_AGE': 1, 'DEATH_AGE': -1},
    'DATA_ASSOCIATION': {'CLASS_NAME': ['Vehicle', 'Pedestrian', 'Cyclist'], 'DISTINGUISH_CLASS': True, 'DISTANCE_METHOD': 'IoUBEV',
                         'ASSIGNMENT_METHOD': 'GNN',
                         'STAGE': {'NAME': 'two_stage', 'FIRST_STAGE': {'DIST_THRESHOLD': [0.2, 0.1, 0.1]},
                                   'SECOND_STAGE': {'SCORE_THRESHOLD': [0.1, 0.1, 0.1], 'POINT_THRESHOLD': [0, 0, 0],
                                                    'DIST_THRESHOLD': [0.3, 0.15, 0.15]}}},
    'TRACK_MERGE': {'ENABLE': True, 'CLASS_NAME': ['Vehicle', 'Pedestrian', 'Cyclist'], 'CLASS_THRESHOLD': [0.5, 0.4, 0.4]},
    'REVERSE_TRACKING': {'ENABLE': True},
}


AB3DMOT_MODEL = {
    'FILTER': {'NAME': 'AB3DMOT', 'X_DIM': 5, 'Z_DIM': 3, 'Q': [5, 15], 'P': [50, 1000], 'R': 5, 'DELTA_T': 0.1},
    'TRACK_AGE': {'BIRTH_AGE': 3, 'DEATH_AGE': 2},
    'DATA_ASSOCIATION': {'CLASS_NAME': ['Vehicle', 'Pedestrian', 'Cyclist'], 'DISTINGUISH_CLASS': False, 'DISTANCE_METHOD': 'IoUBEV',
                         'ASSIGNMENT_METHOD': 'GNN', 'STAGE': {'NAME': 'one_stage', 'FIRST_STAGE': {'DIST_THRESHOLD': [0.1, 0.1, 0.1]}}},
    'TRACK_MERGE': {'ENABLE': False},
    'REVERSE_TRACKING': {'ENABLE': False},
}


def reference_seconds(seq):
    """Wall time of the reference's TrackManager.forward with its AB3DMOT class (over the generator's filterpy stand-in), CPU."""
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import gen_track_ab3dmot_golden as gen
    from easydict import EasyDict
    tk, _ = gen.import_reference()
    manager = tk.TrackManager(EasyDict(copy.deepcopy(AB3DMOT_MODEL)))
    work = copy.deepcopy(seq)
    t0 = time.perf_counter()
    result = manager.forward(work)
    return time.perf_counter() - t0, result


def bench_batch(cfg, n, args):
    """n sequences (the seeded sequence under seeds seed .. seed + n - 1) through TrackManager.forward one after another and through
    TrackManager.forward_batch in one call: host time per call, median of --repeats after a warm-up, results on the host when the
    clock stops (both return host arrays)."""
    import numpy as np
    import torch
    from detzero_amd.synth import TRACK_EVENTS, synth_track_sequence
    from detzero_amd.track_models import TrackManager

    seqs = [synth_track_sequence(args.seed + k, args.frames, args.objects, events=TRACK_EVENTS) for k in range(n)]

    def timed(fn):
        times, result = [], None
        for k in range(args.repeats + 1):           # the first call is the warm-up
            work = copy.deepcopy(seqs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = fn(work)
            torch.cuda.synchronize()
            if k:
                times.append(time.perf_counter() - t0)
        return float(np.median(times)), result

    one = TrackManager(cfg)
    seq_s, seq_res = timed(lambda work: [one.forward(s) for s in work])
    many = TrackManager(cfg)
    bat_s, bat_res = timed(many.forward_batch)
    same_tracks = all(list(a) == list(b) for a, b in zip(seq_res, bat_res))
    same_hits = same_tracks and all(np.array_equal(a[t]['hit'], b[t]['hit']) for a, b in zip(seq_res, bat_res) for t in a)
    same_boxes = same_hits and all(np.array_equal(a[t]['boxes_global'], b[t]['boxes_global']) for a, b in zip(seq_res, bat_res) for t in a)
    return {'filter': args.filter, 'batch': n, 'frames': args.frames, 'repeats': args.repeats, 'tracks': [len(r) for r in bat_res][:4],
            'per_sequence_path_sequences_per_s': round(n / seq_s, 3), 'per_sequence_path_s_per_call': round(seq_s, 4),
            'forward_batch_sequences_per_s': round(n / bat_s, 3), 'forward_batch_s_per_call': round(bat_s, 4),
            'speedup': round(seq_s / bat_s, 3), 'reruns': many.seq_ops.reruns,
            'batched': many.batched, 'fallbacks': many.fallbacks,       # sequences over all calls (warm-up included): batched path / forward
            'same_tracks': same_tracks, 'same_hits': same_hits, 'same_boxes_bitwise': same_boxes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, nargs='+', default=None,
                    help='compare the per-sequence path with forward_batch on N sequences at once, for every N given')
    ap.add_argument('--repeats', type=int, default=5, help='--batch: timed calls per path (median), after one warm-up call')
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--objects', type=int, default=150)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--no-numpy', action='store_true')
    ap.add_argument('--filter', choices=['KalmanFilter', 'AB3DMOT'], default='KalmanFilter',
                    help='KalmanFilter: the shipped waymo_detzero_track values; AB3DMOT: those of waymo_ab3dmot.yaml')
    ap.add_argument('--reference-only', action='store_true', help='AB3DMOT: time the reference\'s own classes on the CPU, no GPU')
    args = ap.parse_args()

    import numpy as np
    import torch
    from detzero_amd.config import AttrDict
    from detzero_amd.synth import TRACK_EVENTS, synth_track_sequence
    from detzero_amd.track_models import TrackManager

    ab3dmot = args.filter == 'AB3DMOT'
    cfg = AttrDict(AB3DMOT_MODEL if ab3dmot else MODEL)
    if args.batch:
        for n in args.batch:
            print(json.dumps(bench_batch(cfg, n, args)), flush=True)
        return

    seq = synth_track_sequence(args.seed, args.frames, args.objects, events=TRACK_EVENTS)
    dets = sum(len(f['score']) for f in seq.values())
    if args.reference_only:
        if not ab3dmot:
            ap.error('--reference-only goes with --filter AB3DMOT')
        ref_s, ref = reference_seconds(seq)
        print(json.dumps({'filter': args.filter, 'frames': args.frames, 'detections_per_frame': round(dets / args.frames, 1), 'tracks': len(ref),
                          'rows': int(sum(len(t['hit']) for t in ref.values())), 'reference_cpu_sequences_per_s': round(1.0 / ref_s, 4),
                          'reference_cpu_ms_per_frame': round(1e3 * ref_s / args.frames, 3)}))
        return

    manager = TrackManager(cfg)
    result = manager.forward(copy.deepcopy(seq))            # warm-up: library load, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        result = manager.forward(copy.deepcopy(seq))
    torch.cuda.synchronize()
    hip_s = (time.perf_counter() - t0) / args.steps
    passes = args.frames * (1 if ab3dmot else 2)
    out = {'filter': args.filter, 'frames': args.frames, 'detections_per_frame': round(dets / args.frames, 1), 'tracks': len(result),
           'rows': int(sum(len(t['hit']) for t in result.values())),
           'hip_sequences_per_s': round(1.0 / hip_s, 3), 'hip_ms_per_frame_pass': round(1e3 * hip_s / passes, 3)}
    if not args.no_numpy:
        from tests import track_ab3dmot_ref, track_ref
        t0 = time.perf_counter()
        ref = TrackManager(cfg, ops_factory=track_ab3dmot_ref.NumpyAb3dTrackOps if ab3dmot else track_ref.NumpyTrackOps).forward(copy.deepcopy(seq))
        np_s = time.perf_counter() - t0
        same = list(ref) == list(result) and all(np.array_equal(ref[k]['hit'], result[k]['hit']) for k in ref)
        worst = max((float(np.abs(ref[k]['boxes_global'] - result[k]['boxes_global']).max()) for k in ref), default=0.0) if same else None
        out.update({'numpy_sequences_per_s': round(1.0 / np_s, 4), 'numpy_ms_per_frame_pass': round(1e3 * np_s / passes, 3),
                    'same_tracks_and_hits': same, 'max_box_difference': worst})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
