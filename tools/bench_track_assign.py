#!/usr/bin/env python
"""Assign mode and tracklet recall on one sequence, for the record: host time of assign_track_target and of
TrackRecall.eval_single_seq on the trajectory-pair kernel (csrc/traj_pair.hip, one launch per sequence) against the composition a
user of the shim had before it - the reference's three Python loops (tests/traj_ref.py) on one device IoU matrix per frame
(dz_boxes_iou_bev / dz_boxes_pairwise_metric), each copied back - under the same orchestration and the same input.

    python tools/bench_track_assign.py [--frames 200] [--objects 150] [--repeats 5]

Input: one seeded sequence (detzero_amd.synth.synth_track_sequence, the size tools/bench_track.py uses), its noise-free ground
truth (synth_track_ground_truth) and the device tracker's tracks of it.  Timing: one warm-up call, then the median of --repeats
calls, each ending with its results on the host (the copy back is the synchronisation); the loop composition is timed once.
Prints one JSON line with both times and whether the two gave the same dicts.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASS_NAMES = ['Vehicle', 'Pedestrian', 'Cyclist']
ASSIGN_THR = {'Vehicle': 0.3, 'Pedestrian': 0.1, 'Cyclist': 0.1}
RECALL_THR = {'Vehicle': 0.7, 'Pedestrian': 0.5, 'Cyclist': 0.5}


def same(a, b):
    import numpy as np
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.shape(a) == np.shape(b) and bool(np.all(np.asarray(a) == np.asarray(b)))
    return a == b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--objects', type=int, default=150)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()

    import torch
    from bench_track import MODEL
    from detzero_amd import ops, track_assign
    from detzero_amd.config import AttrDict
    from detzero_amd.synth import TRACK_EVENTS, synth_track_ground_truth, synth_track_sequence
    from detzero_amd.track_models import TrackManager
    from detzero_amd.track_recall import TrackRecall
    from tests import traj_ref

    seq = synth_track_sequence(args.seed, args.frames, args.objects, events=TRACK_EVENTS)
    gt = synth_track_ground_truth(args.seed, args.frames, args.objects, events=TRACK_EVENTS)
    tracks = TrackManager(AttrDict(MODEL)).forward(copy.deepcopy(seq))
    dev = torch.device('cuda', torch.cuda.current_device())

    def per_frame(metric):
        def fn(a, b):
            ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
            out = ops.boxes_pairwise(ta, tb, True) if metric == ops.TRACK_AFF_IOU_BEV else ops.boxes_pairwise_metric(ta, tb, ops.BOXM_IOU3D)
            return out.cpu().numpy()
        return fn

    def fresh():            # both functions write into their inputs: every call gets its own copy, made outside the timed region
        return copy.deepcopy(seq), copy.deepcopy(tracks), copy.deepcopy(gt)

    def assign(o, data):
        return track_assign.assign_track_target(data, ASSIGN_THR, ops=o)

    def recall(o, data):
        return TrackRecall.eval_single_seq({'gt': data[2], 'pred': data[1]}, CLASS_NAMES, ['l1', 'l2'], RECALL_THR, '3d', ops=o)

    out = {'frames': args.frames, 'ground_truth_trajectories': args.objects, 'tracks': len(tracks)}
    for name, fn in (('assign', assign), ('recall_3d', recall)):
        hip = track_assign.HipTrajOps(dev)
        result = fn(hip, fresh())                            # warm-up
        times = []
        for _ in range(args.repeats):
            data = fresh()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = fn(hip, data)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        data = fresh()
        t0 = time.perf_counter()
        before = fn(traj_ref.NumpyTrajOps(iou_fn=per_frame), data)
        torch.cuda.synchronize()
        loops_s = time.perf_counter() - t0
        out[name] = {'kernel_ms': round(1e3 * statistics.median(times), 2), 'kernel_ms_min_max': [round(1e3 * min(times), 2), round(1e3 * max(times), 2)],
                     'per_frame_loops_ms': round(1e3 * loops_s, 1), 'same_dicts': same(before, result)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
