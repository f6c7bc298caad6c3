"""Golden vectors for assign mode and tracklet recall from the REFERENCE's own functions, CPU.

    python tests/golden/gen_track_assign_golden.py      (needs the reference tree, where gen_track_model_golden.py looks for it)

Runs tracking/detzero_track/models/tracking_modules/target_assign.py (assign_track_target) and utils/track_recall.py
(TrackRecall.eval_single_seq, calculate_tracklet_recall), imported by path with the stand-ins of gen_track_model_golden.py (np.int /
np.bool, .cuda() a no-op, the iou3d imports backed by oracle/cref.py and tests/track_ref.iou3d, an empty filterpy) plus a stub
detzero_utils.common_utils for track_recall.py's import.  Input: the reference DetZeroTracker's output (shipped config) on two
seeded sequences of 24 frames (detzero_amd.synth.synth_track_sequence) and their ground truth (synth_track_ground_truth), with
the edge cases scripted per sequence (EDGES): a ground-truth object that is never detected and has few points (an unmatched
ground truth in 'l2'), a detected object removed from the ground truth (an unlabelled track), a ground-truth object that leaves
mid-sequence, a 'Sign' the class mask drops, a track whose class name changes on one frame; both ``state`` values occur.
Thresholds: the shipped REFINING.IOU_THRESHOLDS for assign, [0.7, 0.5, 0.5] with '3d' and with 'bev' for recall.

The generator ASSERTS that no per-frame IoU lies within 1e-3 of a threshold it is compared with (which also removes the
float32-versus-float64 ambiguity of numpy's scalar comparison) and that every Hungarian assignment is unchanged under a +-1e-4
perturbation of its finite costs; it walks the seeds until the reference meets the conditions and stores the inputs, both
functions' complete outputs and the measured gaps.  It also checks that the product's orchestration on the numpy ops
(tests/traj_ref.py) reproduces the reference's outputs, so a fixture is only ever written for inputs both sides agree on.
"""
import copy
import importlib
import importlib.util
import os
import pickle
import sys
import types
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location('gen_track_model_golden', os.path.join(HERE, 'gen_track_model_golden.py'))
base = importlib.util.module_from_spec(spec)
spec.loader.exec_module(base)          # sys.path, np.int / np.bool

import yaml  # noqa: E402

CLASS_NAMES = ['Vehicle', 'Pedestrian', 'Cyclist']
RECALL_THR = [0.7, 0.5, 0.5]
DIFFICULTYS = ['l1', 'l2']
GAP = 1e-3
# per sequence: never detected + few points / removed from the ground truth / (object, last ground-truth frame)
EDGES = [{'undetected': 12, 'removed': 9, 'leaves': (7, 10)}, {'undetected': 3, 'removed': 11, 'leaves': (7, 10)}]


def import_reference():
    _, dt = base.import_reference()
    cu = types.ModuleType('detzero_utils.common_utils')
    cu.create_logger = lambda *a, **k: None
    cu.get_log_info = lambda s, *a, **k: s
    cu.multi_processing = lambda function, data_dict, workers, bar=False: [function(x) for x in data_dict]
    sys.modules[cu.__name__] = cu
    sys.modules['detzero_utils'].common_utils = cu
    ta = importlib.import_module('detzero_track.models.tracking_modules.target_assign')
    tr = importlib.import_module('detzero_track.utils.track_recall')
    return dt, ta, tr


def plain(x):
    """defaultdicts -> dicts, recursively; arrays and scalars as they are"""
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, list):
        return [plain(v) for v in x]
    return x


def diff(a, b, path=''):
    """path of the first difference, or None"""
    if isinstance(a, dict):
        if not isinstance(b, dict) or list(a.keys()) != list(b.keys()):
            return path + ': keys'
        return next((d for d in (diff(a[k], b[k], '%s/%s' % (path, k)) for k in a) if d), None)
    if isinstance(a, (list, tuple)):
        if not isinstance(b, (list, tuple)) or len(a) != len(b):
            return path + ': length'
        return next((d for d in (diff(x, y, '%s[%d]' % (path, i)) for i, (x, y) in enumerate(zip(a, b))) if d), None)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        ok = a.shape == b.shape and a.dtype.kind == b.dtype.kind and bool(np.all(a == b))
        return None if ok else '%s: %s %s against %s %s' % (path, a.dtype, a.shape, b.dtype, b.shape)
    return None if type(a) == type(b) and a == b else '%s: %r against %r' % (path, a, b)


def same(a, b):
    d = diff(a, b)
    if d:
        print('   differs at', d)
    return d is None


def gt_lens(gt):
    from detzero_amd import track_assign
    return np.array([[len(v['sample_idx'])] for v in track_assign.get_gt_id_data(gt, ['name'], CLASS_NAMES).values()], np.float32)


def inputs(seed, si):
    """(detection frames, ground-truth frames) of sequence ``si`` with its scripted edge cases"""
    from detzero_amd.synth import TRACK_EVENTS, synth_track_ground_truth, synth_track_sequence
    edge = EDGES[si]
    n_frames, n_objects = 24, (20, 19)[si]
    origin = ((3000.0, -2000.0, 40.0), (-4100.0, 2600.0, -12.0))[si]
    events = TRACK_EVENTS if si == 0 else dict(TRACK_EVENTS, missing={6: [9, 10, 11]}, chain={9: 3}, dup={0: 12}, empty=[4], low={7: [3, 17, 18]})
    missing = dict(events['missing'])
    missing[edge['undetected']] = list(range(n_frames))
    events = dict(events, missing=missing)
    name = 'seq_%s' % 'ab'[si]
    det = synth_track_sequence(seed + si, n_frames, n_objects, origin=origin, events=events, sequence_name=name)
    gt = synth_track_ground_truth(seed + si, n_frames, n_objects, origin=origin, events=events, sequence_name=name)
    for f, info in gt.items():
        annos = info['annos']
        keep = np.ones(n_objects, dtype=bool)
        keep[edge['removed']] = False
        if int(f) > edge['leaves'][1]:
            keep[edge['leaves'][0]] = False
        annos['num_points_in_gt'][edge['undetected']] = 3
        for key in list(annos):
            annos[key] = annos[key][keep]
        sign = annos['gt_boxes_global'][:1].copy()
        sign[0, :2] -= 80.0
        sign[0, 3:6] = (0.6, 0.6, 2.4)
        sign_lidar = annos['gt_boxes_lidar'][:1].copy()
        sign_lidar[0, :2] -= 80.0
        sign_lidar[0, 3:6] = (0.6, 0.6, 2.4)
        annos['name'] = np.concatenate([annos['name'], np.array(['Sign'], dtype=annos['name'].dtype)])
        annos['obj_ids'] = np.concatenate([annos['obj_ids'], np.array(['sign_0'], dtype=annos['obj_ids'].dtype)])
        annos['gt_boxes_global'] = np.concatenate([annos['gt_boxes_global'], sign])
        annos['gt_boxes_lidar'] = np.concatenate([annos['gt_boxes_lidar'], sign_lidar])
        annos['difficulty'] = np.concatenate([annos['difficulty'], [0]])
        annos['num_points_in_gt'] = np.concatenate([annos['num_points_in_gt'], [40]])
    return det, gt


def change_one_class(tracks):
    """the first Vehicle track of ten frames or more is called a Pedestrian on its sixth frame; -> its id"""
    for tid, tk in tracks.items():
        if len(tk['name']) >= 10 and np.all(tk['name'] == 'Vehicle'):
            tk['name'] = tk['name'].astype('<U10')
            tk['name'][5] = 'Pedestrian'
            return tid
    return None


def threshold_gap(ops, metric, thr):
    worst = 1.0
    for _, _, mat, cls in ops._frames(metric, True):
        if mat.size:
            t = np.asarray(thr, np.float32)[cls][:, None]
            live = mat > 0
            if live.any():
                worst = min(worst, float(np.min(np.abs(mat - t)[live])))
    return worst


def try_seed(seed, dt, ta, tr, model, iou_thresholds):
    from easydict import EasyDict
    from tests import traj_ref
    from detzero_amd import track_assign, track_recall
    rng = np.random.default_rng(seed)
    recall_thr = dict(zip(CLASS_NAMES, RECALL_THR))
    out = {'seed': seed, 'class_names': CLASS_NAMES, 'iou_thresholds': dict(iou_thresholds), 'recall_thresholds': RECALL_THR,
           'difficultys': DIFFICULTYS, 'sequences': []}
    gaps = {'assign_bev': 1.0, 'recall_3d': 1.0, 'recall_bev': 1.0}
    kinds = defaultdict(int)
    for si in range(2):
        det, gt = inputs(seed, si)
        tracks = dt.DetZeroTracker(EasyDict(copy.deepcopy(model))).forward(copy.deepcopy(det))
        changed = change_one_class(tracks)
        if changed is None:
            return None, 'no track to rename'
        entry = {'det': det, 'gt': gt, 'tracks': plain(copy.deepcopy(tracks)), 'class_change': changed}

        ref = plain(ta.assign_track_target((copy.deepcopy(det), copy.deepcopy(tracks), copy.deepcopy(gt)), iou_thresholds))
        ops = traj_ref.NumpyTrajOps()
        mine = plain(track_assign.assign_track_target((copy.deepcopy(det), plain(copy.deepcopy(tracks)), copy.deepcopy(gt)), iou_thresholds, ops=ops))
        if not same(ref, mine):
            return None, 'assign: the restatement differs from the reference'
        gaps['assign_bev'] = min(gaps['assign_bev'], threshold_gap(ops, traj_ref.AFF_IOU_BEV, [iou_thresholds[n] for n in CLASS_NAMES]))
        costs = []
        _, sum_hit, n_hit, _ = ops.tables[-1]
        sim = sum_hit / gt_lens(gt)
        sim[n_hit <= 0] = -1.
        costs.append((1 - sim).astype(np.float32))
        entry['assign'] = ref
        states = [v['track']['state'] for v in ref['label'].values()]
        kinds['static'] += states.count('static')
        kinds['dynamic'] += states.count('dynamic')
        kinds['unlabel'] += len(ref['unlabel'])
        kinds['class_change_labelled'] += int(changed in ref['label'])
        kinds['leaves'] += sum(1 for v in ref['label'].values() if len(v['gt']['sample_idx']) == EDGES[si]['leaves'][1] + 1)
        kinds['sign'] += sum(int('Sign' in info['annos']['name']) for info in gt.values())

        entry['recall'] = {}
        for method, metric in (('3d', traj_ref.AFF_IOU3D), ('bev', traj_ref.AFF_IOU_BEV)):
            ref_r = plain(tr.TrackRecall.eval_single_seq({'gt': copy.deepcopy(gt), 'pred': copy.deepcopy(tracks)}, CLASS_NAMES, DIFFICULTYS,
                                                         recall_thr, method))
            ops = traj_ref.NumpyTrajOps()
            mine_r = plain(track_recall.TrackRecall.eval_single_seq({'gt': copy.deepcopy(gt), 'pred': plain(copy.deepcopy(tracks))}, CLASS_NAMES,
                                                                    DIFFICULTYS, recall_thr, method, ops=ops))
            if not same(ref_r, mine_r):
                return None, 'recall %s: the restatement differs from the reference' % method
            gaps['recall_' + method] = min(gaps['recall_' + method], threshold_gap(ops, metric, RECALL_THR))
            sum_all, _, n_hit, _ = ops.tables[-1]
            sim = sum_all / gt_lens(gt)
            sim[n_hit <= 0] = -1.
            costs.append((1 - sim).astype(np.float32))
            entry['recall'][method] = ref_r
            if method == '3d':
                # an unmatched ground truth appends to gt_box_nums_list only
                for diff in DIFFICULTYS:
                    for cn in CLASS_NAMES:
                        cur = ref_r[diff][cn]
                        kinds['unmatched_gt_' + diff] += len(cur.get('gt_box_nums_list', [])) - len(cur.get('match_rate', []))
        if not base.assignments_stable(costs, rng):
            return None, 'an assignment moves under a 1e-4 perturbation'
        out['sequences'].append(entry)
    for key, val in gaps.items():
        if val < GAP:
            return None, '%s gap %.2e' % (key, val)
    need = ('static', 'dynamic', 'unlabel', 'class_change_labelled', 'leaves', 'sign', 'unmatched_gt_l2')
    missing = [k for k in need if kinds[k] < 1]
    if missing:
        return None, 'no entry of kind %s' % ', '.join(missing)
    out['gaps'], out['kinds'] = gaps, dict(kinds)

    recall = object.__new__(tr.TrackRecall)
    recall.difficultys, recall.class_names, recall.match_rate_list = DIFFICULTYS, CLASS_NAMES, np.arange(0, 10) * 0.1
    out['recall_summary'] = {m: plain(recall.calculate_tracklet_recall({e['det']['0']['sequence_name']: copy.deepcopy(e['recall'][m])
                                                                        for e in out['sequences']})) for m in ('3d', 'bev')}
    return out, 'ok'


def main():
    dt, ta, tr = import_reference()
    with open(base.REF + '/tracking/tools/cfgs/tk_model_cfgs/waymo_detzero_track.yaml') as f:
        cfg = yaml.safe_load(f)
    for seed in range(100, 160):
        out, why = try_seed(seed, dt, ta, tr, cfg['MODEL'], cfg['REFINING']['IOU_THRESHOLDS'])
        print('seed %d: %s' % (seed, why))
        if out is not None:
            # the nesting (dicts of dicts of arrays, in order) is kept by pickle; the poses repeat and compress well, so the pickle
            # travels as one byte array of a compressed .npz: load with pickle.loads(np.load(path)['pickle'].tobytes())
            path = os.path.join(HERE, 'track_assign_golden.npz')
            np.savez_compressed(path, pickle=np.frombuffer(pickle.dumps(out, protocol=4), dtype=np.uint8))
            print('saved %d KiB' % (os.path.getsize(path) // 1024), out['gaps'], out['kinds'])
            return
    raise SystemExit('no seed met the conditions')


if __name__ == '__main__':
    main()
