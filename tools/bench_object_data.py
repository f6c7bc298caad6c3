#!/usr/bin/env python
"""Host time per sequence of the object-data stage, for the record: the sequence crop (object_data.SequencePlan +
object_crop.crop_sequence: points prepared once per frame, one crop for the boxes of all three classes) against the same output made
with the one-frame crop (object_crop.crop_frame_objects looped over the frames once per class, as daemon/prepare_object_data.py runs).

    python tools/bench_object_data.py [--frames 200] [--objects 150] [--points 100000] [--steps 5]

Input: one seeded sequence (detzero_amd.synth.synth_track_sequence, the box counts of tools/bench_track.py; box i of every frame is
track i) and --points seeded lidar points per frame, a third of them around the boxes, an eighth NLZ-flagged.  Each path: one warm-up,
then the median of --steps runs, results on the host when the clock stops, split into point preparation (host float64) and crop
(uploads, kernels, downloads).  Prints one JSON line; `agree` says that both paths produced the same rows.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--objects', type=int, default=150)
    ap.add_argument('--points', type=int, default=100000)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch
    from detzero_amd import object_crop, object_data
    from detzero_amd.synth import synth_track_sequence

    seq = synth_track_sequence(args.seed, args.frames, args.objects, events={})
    frames = sorted(seq, key=int)
    n = min(len(seq[f]['score']) for f in frames)
    tracks = {}
    for i in range(n):
        tracks[i] = {'obj_ids': np.full(len(frames), i), 'name': np.array([seq[f]['name'][i] for f in frames]),
                     'boxes_global': np.stack([seq[f]['boxes_global'][i] for f in frames]), 'score': np.array([seq[f]['score'][i] for f in frames]),
                     'hit': np.ones(len(frames), dtype=np.int64), 'sample_idx': np.array(frames), 'state': 'dynamic',
                     'pose': np.stack([seq[f]['pose'] for f in frames])}
    rng = np.random.default_rng(args.seed)
    points = {}
    for f in frames:
        boxes, pose, m = seq[f]['boxes_global'].astype(np.float64), seq[f]['pose'], args.points
        glob = rng.uniform(boxes[:, :3].min(0) - 10, boxes[:, :3].max(0) + 10, (m, 3))
        k = m // 3
        owner = rng.integers(0, boxes.shape[0], k)
        glob[:k] = boxes[owner, :3] + rng.uniform(-0.6, 0.6, (k, 3)) * boxes[owner, 3:6].max(1, keepdims=True)
        raw = np.empty((m, 6), np.float32)
        raw[:, :3] = (glob - pose[:3, 3]) @ pose[:3, :3]
        raw[:, 3:5] = rng.uniform(0, 1, (m, 2))
        raw[:, 5] = np.where(np.arange(m) % 8 == 3, 1, -1)
        points[str(f).zfill(4)] = raw
    loader = lambda s, frm: points[frm]
    dev = torch.device('cuda', torch.cuda.current_device())
    classes = object_data.CLASS_NAMES

    def new_path():
        t0 = time.perf_counter()
        plan = object_data.SequencePlan('bench', tracks, classes, 'test', loader)
        t1 = time.perf_counter()
        crop = object_crop.crop_sequence(plan.crop_frames(), 1.1, False, device=dev)
        rows = crop.to_lists()
        t2 = time.perf_counter()
        out = {(cn, obj, plan.entries[e]['frm_id']): rows[plan.flat(i)] for i, (cn, obj, e, _) in enumerate(plan.boxes)}
        return t1 - t0, t2 - t1, out, crop.n_groups

    def frame_path():
        prep = crop = 0.0
        out = {}
        for cn in classes:
            for frm_id, rec in object_data.frame_level(tracks, cn, 'test').items():
                t0 = time.perf_counter()
                pts = object_crop.prepare_frame_points(loader('bench', frm_id), rec['pose'])
                t1 = time.perf_counter()
                objs = object_crop.crop_objects(pts, object_crop.enlarge_boxes(rec['boxes_global'], 1.1, False), dev)
                t2 = time.perf_counter()
                prep, crop = prep + t1 - t0, crop + t2 - t1
                for obj, o in zip(rec['obj_id'], objs):
                    out[(cn, obj, frm_id)] = o
        return prep, crop, out

    res = {}
    for name, fn in (('sequence_crop', new_path), ('frame_crop_per_class', frame_path)):
        fn()
        torch.cuda.synchronize()
        runs = [fn() for _ in range(args.steps)]
        res[name] = runs[-1][2]
        prep, crop = statistics.median(r[0] for r in runs), statistics.median(r[1] for r in runs)
        res[name + '_s'] = {'prepare': round(prep, 4), 'crop': round(crop, 4), 'total': round(statistics.median(r[0] + r[1] for r in runs), 4)}
        if name == 'sequence_crop':
            res['frame_groups'] = runs[-1][3]
    a, b = res.pop('sequence_crop'), res.pop('frame_crop_per_class')
    agree = a.keys() == b.keys() and all(a[k].tobytes() == b[k].tobytes() for k in a)
    print(json.dumps(dict(res, frames=len(frames), boxes_per_frame=n, points_per_frame=args.points, kept_rows=int(sum(len(v) for v in a.values())),
                          steps=args.steps, agree=bool(agree))))


if __name__ == '__main__':
    main()
