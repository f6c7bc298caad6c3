"""Golden vectors for the object-data stage and the refining stage's other end from the REFERENCE's own functions, CPU.

    python tests/golden/gen_object_data_golden.py      (needs the reference tree, where gen_track_model_golden.py looks for it)

Runs daemon/prepare_object_data.py (WaymoObjectDataPrepare.prepare_data_worker), daemon/combine_output.py (combine_final,
convert_frame_format, combine_det) and daemon/generate_iou_gt.py (generate_refine_boxes_iou), imported by path with the stand-ins of
gen_track_assign_golden.py (np.bool, .cuda() a no-op, the compiled ops backed by oracle/cref.py and tests/track_ref.iou3d, a stub
detzero_utils.common_utils) plus points_in_boxes_gpu_v2 backed by oracle.cref.points_in_boxes_v2.

Input: the reference tracker's output and assign output of tests/golden/track_assign_golden.npz (the first 12 frames of two seeded sequences, with
an unlabelled track, a ground-truth object that leaves, a track named Pedestrian on one frame), to which one more frame is added that only
the unlabelled track touches; per frame a few hundred seeded points in and around the frame's boxes, an eighth of them NLZ-flagged.
Covered: the 'val' and 'test' splits, all three classes, crop_on_bev off and on.

Stored: the inputs and the reference's outputs.  The point rows of the pickles are stored as the kept point INDICES per object and frame
(rows of the frame's prepared points); a test re-makes the rows with the host preparation, so that a BLAS difference between machines
cannot fail it.  The refining results that combine_final and generate_refine_boxes_iou read are seeded perturbations of the tracks.

The generator ASSERTS that no point lies within 1e-4 m of a face of an enlarged box (it walks the point seeds until none does and
stores the smallest gap) and that no paired IoU lies within 1e-3 of 0.
"""
import copy
import importlib.util
import logging
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


ga = _load('gen_track_assign_golden', os.path.join(HERE, 'gen_track_assign_golden.py'))
base = ga.base

import torch  # noqa: E402

CLASS_NAMES = ['Vehicle', 'Pedestrian', 'Cyclist']
POINTS_PER_FRAME = 200
KEEP_FRAMES = 12                                      # the first frames of the 24 (the fixture stays small)
FACE_GAP, IOU_GAP = 1e-4, 1e-3
VARIANTS = [('val', False), ('val', True), ('test', False), ('test', True)]
EXTRA_FRAME = 24                                      # the frame that only the unlabelled track touches


def import_daemon():
    from oracle import cref
    ga.import_reference()
    base._pkg('detzero_utils.ops.roiaware_pool3d')
    roi = types.ModuleType('detzero_utils.ops.roiaware_pool3d.roiaware_pool3d_utils')
    roi.points_in_boxes_gpu_v2 = lambda pts, boxes: torch.from_numpy(cref.points_in_boxes_v2(pts[0].numpy(), boxes[0].numpy()))[None]
    sys.modules[roi.__name__] = roi
    daemon = base.REF + '/daemon/'
    return (_load('ref_prepare_object_data', daemon + 'prepare_object_data.py'), _load('ref_combine_output', daemon + 'combine_output.py'),
            _load('ref_generate_iou_gt', daemon + 'generate_iou_gt.py'))


def _cut(rec):
    """The entries of a track or ground-truth record on the first KEEP_FRAMES frames; None when nothing is left."""
    n = len(rec['sample_idx'])
    keep = np.asarray([int(f) < KEEP_FRAMES for f in rec['sample_idx']])
    if not keep.any():
        return None
    return {k: (v[keep] if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v) for k, v in rec.items()}


def first_frames(entry):
    """entry with every track cut to the first KEEP_FRAMES frames (tracks that start later are dropped)"""
    entry['tracks'] = {k: c for k, c in ((k, _cut(v)) for k, v in entry['tracks'].items()) if c is not None}
    label = {}
    for k, v in entry['assign']['label'].items():
        tk, gt = _cut(v['track']), _cut(v['gt'])
        if tk is not None and gt is not None:
            label[k] = {'track': tk, 'gt': gt}
    unlabel = {k: {'track': c} for k, c in ((k, _cut(v['track'])) for k, v in entry['assign']['unlabel'].items()) if c is not None}
    entry['assign'] = {'label': label, 'unlabel': unlabel}
    return entry


def add_unlabelled_frame(entry):
    """One more frame on the sequence's first unlabelled track (assign output and plain tracks alike): moved on by its last step."""
    uid = next(iter(entry['assign']['unlabel']))
    for tk in (entry['assign']['unlabel'][uid]['track'], entry['tracks'][uid]):
        n = len(tk['sample_idx'])
        for key, val in list(tk.items()):
            if isinstance(val, np.ndarray) and val.shape[:1] == (n,):
                tk[key] = np.concatenate([val, val[-1:]], axis=0)
        tk['sample_idx'] = tk['sample_idx'].astype('<U4')
        tk['sample_idx'][-1] = str(EXTRA_FRAME)
        tk['boxes_global'][-1, :3] += tk['boxes_global'][-2, :3] - tk['boxes_global'][-3, :3]
        tk['pose'][-1, :3, 3] += tk['pose'][-2, :3, 3] - tk['pose'][-3, :3, 3]
    return uid


def frame_boxes(entry):
    """{4-digit frame id: (pose, (T,7) float64 global boxes of every track on the frame)}"""
    out = {}
    for tk in entry['tracks'].values():
        for i, f in enumerate(tk['sample_idx']):
            rec = out.setdefault(str(f).zfill(4), [tk['pose'][i], []])
            rec[1].append(np.asarray(tk['boxes_global'][i][:7], np.float64))
    return {f: (p, np.stack(b)) for f, (p, b) in out.items()}


def make_points(entry, seed):
    """{frame id: (N,6) float32 lidar-frame points}: half around the frame's boxes (inside and just outside the enlarged box), half
    scattered; every eighth NLZ-flagged."""
    rng = np.random.default_rng(seed)
    pts = {}
    for f, (pose, boxes) in frame_boxes(entry).items():
        n, t = POINTS_PER_FRAME, boxes.shape[0]
        lo, hi = boxes[:, :3].min(0) - 5, boxes[:, :3].max(0) + 5
        glob = rng.uniform(lo, hi, (n, 3))
        owner = rng.integers(0, t, n)
        local = rng.uniform(-0.62, 0.62, (n, 3)) * boxes[owner, 3:6]
        c, s = np.cos(boxes[owner, 6]), np.sin(boxes[owner, 6])
        seeded = np.stack([local[:, 0] * c - local[:, 1] * s, local[:, 0] * s + local[:, 1] * c, local[:, 2]], 1) + boxes[owner, :3]
        near = rng.random(n) < 0.7
        glob[near] = seeded[near]
        raw = np.empty((n, 6), np.float32)
        raw[:, :3] = (glob - pose[:3, 3]) @ pose[:3, :3]
        raw[:, 3] = rng.uniform(0, 3, n)
        raw[:, 4] = rng.uniform(0, 1, n)
        raw[:, 5] = np.where(np.arange(n) % 8 == 3, 1, -1)
        pts[f] = raw
    return pts


def face_gap(entry, points, scale=1.1):
    """Smallest distance of a kept point to the surface of an enlarged box (x / y / z faces, crop_on_bev off and on), in the float32
    coordinates the inside test sees."""
    from detzero_amd.object_crop import prepare_frame_points
    worst = np.inf
    for f, (pose, boxes) in frame_boxes(entry).items():
        p = prepare_frame_points(points[f], pose)[:, :3].astype(np.float32).astype(np.float64)
        for b32 in boxes.astype(np.float32):
            b = b32.astype(np.float64)
            d = p - b[:3]
            c, s = np.cos(-b[6]), np.sin(-b[6])
            lx, ly = d[:, 0] * c - d[:, 1] * s, d[:, 0] * s + d[:, 1] * c
            gx, gy, gz = np.abs(lx) - b[3] * scale / 2, np.abs(ly) - b[4] * scale / 2, np.abs(d[:, 2]) - b[5] * scale / 2
            for g in (np.maximum(np.maximum(gx, gy), gz), np.maximum(gx, gy)):       # the signed distance to the surface, 3-D and BEV
                worst = min(worst, float(np.abs(g).min()))
    return worst


def rows_to_index(data_info, prepared):
    """The reference's object records with every 'pts' row set replaced by the rows' indices into the frame's prepared points."""
    lookup = {}
    for f, p in prepared.items():
        keys = [r.tobytes() for r in p]
        assert len(set(keys)) == len(keys), 'two identical points in frame %s' % f
        lookup[f] = {k: i for i, k in enumerate(keys)}
    out = {}
    for obj_id, obj in data_info.items():
        rec = dict(obj)
        rec['pts'] = [np.asarray([lookup[f][r.tobytes()] for r in rows], np.int32) for f, rows in zip(obj['sample_idx'], obj['pts'])]
        for rows, idx in zip(obj['pts'], rec['pts']):
            assert rows.dtype == np.float64 and rows.shape == (len(idx), 4) and (np.diff(idx) > 0).all()
        out[obj_id] = rec
    return out


def refine_results(prepared_val, rng):
    """Seeded geometry / position / confidence results (refine_results.*_prediction_dicts layout) for the objects of the reference's
    'val' pickles, a drop file for combine_det, and ground-truth boxes for the IoU labels."""
    from detzero_amd.track_adapter import get_inverse_transform_mat
    res = {cn: {'geo': {}, 'pos': {}, 'conf': {}} for cn in CLASS_NAMES}
    for cn in CLASS_NAMES:
        for seq, data_info in prepared_val[cn].items():
            for obj_id, obj in data_info.items():
                n = len(obj['sample_idx'])
                world = np.asarray(obj['boxes_global'], np.float64) + rng.normal(0, 0.05, (n, 7))
                lidar = world.copy()
                for i in range(n):
                    inv = get_inverse_transform_mat(obj['pose'][i]).astype(np.float64)
                    lidar[i, :3] = inv[:3, :3] @ world[i, :3] + inv[:3, 3]
                    lidar[i, 6] = world[i, 6] + np.arctan2(inv[1, 0], inv[0, 0])
                frames = [int(f) for f in obj['sample_idx']]
                size = np.abs(world[:, 3:6].mean(0) + rng.normal(0, 0.05, 3))
                geo_boxes = [np.concatenate([lidar[i, :3], size, lidar[i, 6:7]])[None, :] for i in range(n)]
                key = int(obj_id)
                res[cn]['geo'].setdefault(seq, {})[key] = {'sequence_name': seq, 'frame_id': frames, 'boxes_lidar': geo_boxes,
                                                           'score': list(obj['score']), 'name': [cn] * n, 'pose': list(obj['pose'])}
                res[cn]['pos'].setdefault(seq, {})[key] = {
                    'sequence_name': seq, 'frame_id': list(frames), 'boxes_lidar': list(lidar), 'boxes_global': list(world),
                    'score': list(obj['score']), 'name': [cn] * n, 'state': str(obj['state']), 'pose': list(obj['pose']),
                    'boxes_gt_global': list(world + rng.normal(0, 0.08, (n, 7)) * [1, 1, 1, 1, 1, 1, 0.3])}
                res[cn]['conf'].setdefault(seq, {})[key] = {'sequence_name': seq, 'frame_id': np.asarray(frames), 'score': np.asarray(obj['score']),
                                                            'new_score': rng.uniform(0, 1, n).astype(np.float32)}
    return res


def run_combine(co, res, drop, with_conf, with_drop):
    """combine_final of the reference on a scratch directory -> {file name: content}"""
    log = logging.getLogger('gen')
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'result'))
        for cn in CLASS_NAMES:
            for kind, word in (('geo', 'geometry'), ('pos', 'position'), ('conf', 'confidence')):
                with open(os.path.join(tmp, 'result', '%s_%s_val.pkl' % (cn, word)), 'wb') as f:
                    pickle.dump(copy.deepcopy(res[cn][kind]), f)
        drop_path = os.path.join(tmp, 'drop.pkl')
        with open(drop_path, 'wb') as f:
            pickle.dump(drop, f)
        co.combine_final(tmp, CLASS_NAMES, log, split='val', combine_conf_res=with_conf, combine_drop_path=drop_path if with_drop else None)
        out = {}
        for cn in CLASS_NAMES:
            for name in ('%s_final.pkl' % cn, '%s_final_frame.pkl' % cn):
                with open(os.path.join(tmp, 'result', name), 'rb') as f:
                    out[name] = pickle.load(f)
        return out


def main():
    from detzero_amd.object_crop import prepare_frame_points
    po, co, gi = import_daemon()
    fixture = pickle.loads(np.load(os.path.join(HERE, 'track_assign_golden.npz'))['pickle'].tobytes())
    sequences = []
    for e in fixture['sequences']:
        entry = {'name': e['det']['0']['sequence_name'], 'tracks': copy.deepcopy(e['tracks']), 'assign': copy.deepcopy(e['assign']),
                 'class_change': e['class_change']}
        entry['unlabelled'] = add_unlabelled_frame(first_frames(entry))
        sequences.append(entry)
    out = {'class_names': CLASS_NAMES, 'enlarge_scale': 1.1, 'variants': VARIANTS, 'extra_frame': str(EXTRA_FRAME).zfill(4), 'sequences': sequences}

    gaps = []
    for si, entry in enumerate(sequences):
        for seed in range(7000 + 100 * si, 7100 + 100 * si):
            pts = make_points(entry, seed)
            gap = face_gap(entry, pts)
            print('%s points seed %d: face gap %.2e' % (entry['name'], seed, gap))
            if gap > FACE_GAP:
                entry['points'], entry['points_seed'] = pts, seed
                gaps.append(gap)
                break
        else:
            raise SystemExit('no point seed met the face gap')
    out['min_face_gap'] = min(gaps)

    # the reference's prepare stage, per variant and class
    out['prepare'] = {}
    real_load = np.load
    for split, bev in VARIANTS:
        per_class = {}
        for cn in CLASS_NAMES:
            per_class[cn] = {}
            for entry in sequences:
                boxes = frame_boxes(entry)
                with tempfile.TemporaryDirectory() as tmp:
                    prep = po.WaymoObjectDataPrepare(cn, root_path=tmp, split=split, track_data_path=None, enlarge_scale=1.1, crop_on_bev=bev,
                                                     workers=1, logger=logging.getLogger('gen'))
                    np.load = lambda path, _e=entry: _e['points'][os.path.basename(path)[:-4]]
                    try:
                        seq_info = copy.deepcopy(entry['assign'] if split == 'val' else entry['tracks'])
                        prep.prepare_data_worker({entry['name']: seq_info})
                    finally:
                        np.load = real_load
                    with open(os.path.join(tmp, 'refining', cn, '%s.pkl' % entry['name']), 'rb') as f:
                        data_info = pickle.load(f)
                # (sic) the frame's pose is the first track's OF THE CLASS; in these sequences every track carries the frame's one pose
                prepared = {f: prepare_frame_points(entry['points'][f], pose) for f, (pose, _) in boxes.items()}
                per_class[cn][entry['name']] = rows_to_index(data_info, prepared)
        out['prepare'][(split, bev)] = per_class
    kinds = {
        'two_classes': sum(1 for e in sequences if e['class_change'] in out['prepare'][('val', False)]['Vehicle'][e['name']]
                           and e['class_change'] in out['prepare'][('val', False)]['Pedestrian'][e['name']]),
        'unlabelled': sum(1 for cn in CLASS_NAMES for d in out['prepare'][('val', False)][cn].values() for o in d.values() if not o['matched_tracklet']),
        'unmatched_frames': sum(int((~np.asarray(o['matched'])).sum()) for cn in CLASS_NAMES for d in out['prepare'][('val', False)][cn].values() for o in d.values()),
        'extra_frame_objects': sum(1 for cn in CLASS_NAMES for d in out['prepare'][('val', False)][cn].values() for o in d.values()
                                   if out['extra_frame'] in list(o['sample_idx'])),
        'kept_points': sum(len(i) for cn in CLASS_NAMES for d in out['prepare'][('val', False)][cn].values() for o in d.values() for i in o['pts']),
        'empty_crops': sum(1 for cn in CLASS_NAMES for d in out['prepare'][('val', False)][cn].values() for o in d.values() for i in o['pts'] if len(i) == 0),
    }
    print(kinds)
    assert kinds['two_classes'] >= 1 and kinds['unlabelled'] >= 1 and kinds['unmatched_frames'] >= 1 and kinds['extra_frame_objects'] >= 1
    assert kinds['kept_points'] > 1000
    out['kinds'] = kinds

    # the refining stage's other end
    rng = np.random.default_rng(4242)
    res = refine_results(out['prepare'][('val', False)], rng)
    first = run_combine(co, res, None, True, False)
    drop = {}
    for cn in CLASS_NAMES:
        for rec in first['%s_final_frame.pkl' % cn]:
            frames = drop.setdefault(rec['sequence_name'], {})
            if str(rec['frame_id']) not in frames:
                k = int(rng.integers(0, 3))
                frames[str(rec['frame_id'])] = {'boxes_lidar': rng.normal(0, 20, (k, 7)).astype(np.float32),
                                                'name': np.array(['Vehicle'] * k, dtype=object), 'score': rng.uniform(0, 0.2, k).astype(np.float32)}
    out['refine'], out['drop'] = res, drop
    plain = run_combine(co, res, drop, False, False)
    # (sic) combine_final's dict collects class after class: the last class's track-level file holds every earlier one's objects
    out['combine'] = {'conf_drop': run_combine(co, res, drop, True, True),
                      'plain': {k: v for k, v in plain.items() if k.endswith('_frame.pkl') or k == '%s_final.pkl' % CLASS_NAMES[-1]}}

    out['iou'] = {}
    worst = 1.0
    with tempfile.TemporaryDirectory() as tmp:
        for cn in CLASS_NAMES:
            geo_path, pos_path = os.path.join(tmp, '%s_geometry_train.pkl' % cn), os.path.join(tmp, '%s_position_train.pkl' % cn)
            for path, kind in ((geo_path, 'geo'), (pos_path, 'pos')):
                with open(path, 'wb') as f:
                    pickle.dump(res[cn][kind], f)
            gi.generate_refine_boxes_iou(cn, geo_path, pos_path, tmp, logging.getLogger('gen'))
            with open(os.path.join(tmp, '%s_iou_train.pkl' % cn), 'rb') as f:
                out['iou'][cn] = pickle.load(f)
            for d in out['iou'][cn].values():
                for v in d.values():
                    worst = min(worst, float(np.min(v)))
    print('smallest paired IoU %.3f' % worst)
    assert worst > IOU_GAP
    out['min_iou'] = worst

    path = os.path.join(HERE, 'object_data_golden.npz')
    np.savez_compressed(path, pickle=np.frombuffer(pickle.dumps(out, protocol=4), dtype=np.uint8))
    size = os.path.getsize(path)
    print('saved %d KiB, face gap %.2e' % (size // 1024, out['min_face_gap']))
    assert size < (1 << 20)


if __name__ == '__main__':
    logging.basicConfig(level=logging.WARNING)
    main()
