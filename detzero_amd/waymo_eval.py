"""Waymo-style detection metrics (AP / APH per object type and range bin, difficulty levels 1 and 2) with the matching on the
device.

Mirrors detection/detzero_det/datasets/waymo/waymo_eval_detection.py (``WaymoDetectionMetricsEstimator``: the conversion of info
dicts to flat arrays, the distance mask, the configuration) and evaluator/detzero_eval.py (the command line).  The reference hands
the flat arrays to TensorFlow / waymo_open_dataset; here csrc/eval_match.hip counts TP / FP / FN / heading accuracy at the 101 score
cutoffs (``ops.eval_match_counts``) and ``metrics_from_counts`` turns the count table into AP / APH in float64.  The protocol is
this project's statement (include/detzero_hip.h), not pinned to the official tool.

What the tracking metrics (waymo_eval_tracking.py) define alike lives here once: cutoffs, thresholds, shards, the
ground-truth difficulty rule, the fake-lidar conversion, the count-table check, the table formatter and the command line.

    python -m detzero_amd.waymo_eval --det_result_path result.pkl --gt_info_path waymo_infos_val.pkl \\
        [--evaluate_metrics object range] [--iou_type 3d|bev] [--class_name Vehicle Pedestrian Cyclist] \\
        [--info_with_fakelidar] [--distance_thresh 1000] [--human_study]
"""
import argparse
import copy
import os
import pickle
from collections import defaultdict

import numpy as np

from .lib import DetZeroHipError
from .ops import EVAL_FIXED_ONE

TYPE_NAMES = ('VEHICLE', 'PEDESTRIAN', 'SIGN', 'CYCLIST')               # object types 1..4 as the metric names spell them
RANGE_NAMES = ('[0, 30)', '[30, 50)', '[50, +inf)')
RANGE_EDGES = (30.0, 50.0)
IOU_THRESHOLDS = (0.0, 0.7, 0.5, 0.5, 0.5)                              # waymo_eval_detection.py:111-115
N_CUTOFFS = 101
HUMAN_STUDY_LIST = [
    '17703234244970638241_220_000_240_000',
    '15611747084548773814_3740_000_3760_000',
    '11660186733224028707_420_000_440_000',
    '1024360143612057520_3580_000_3600_000',
    '6491418762940479413_6520_000_6540_000',
]


def limit_period(val, offset=0.5, period=np.pi):
    return val - np.floor(val / period + offset) * period


def score_cutoffs():
    """c_k = float32(k * 0.01), k = 0..99, and 1.0 (build_config, :129-131: doubles appended to a float field)."""
    return np.array([k * 0.01 for k in range(100)] + [1.0], dtype=np.float32)


def breakdown_names(config_type):
    """The shard names of a configuration, in table order: OBJECT_TYPE shards (one per type), then RANGE shards (type, bin)."""
    names = []
    if 'object' in config_type:
        names += ['OBJECT_TYPE_TYPE_%s' % t for t in TYPE_NAMES]
    if 'range' in config_type:
        names += ['RANGE_TYPE_%s_%s' % (t, r) for t in TYPE_NAMES for r in RANGE_NAMES]
    return names


def _envelope_area(precision, recall):
    """Sum over the distinct recalls rho_1 < rho_2 < ... (rho_0 = 0) of (rho_i - rho_{i-1}) * max{p_j: r_j >= rho_i}."""
    area, prev = 0.0, 0.0
    for rho in np.unique(recall):
        area += (rho - prev) * precision[recall >= rho].max()
        prev = rho
    return float(area)


def check_count_table(table, width, config_type, what):
    """A (n_shards, 2, 101, width) count table and its configuration (None: by the shard count, 4 = ['object'], 12 = ['range'],
    16 = both) -> (shard names, config_type)."""
    if table.ndim != 4 or table.shape[1:] != (2, N_CUTOFFS, width):
        raise DetZeroHipError('%s: a (n_shards, 2, 101, %d) table, got %s' % (what, width, table.shape))
    if config_type is None:
        config_type = {4: ['object'], 12: ['range'], 16: ['object', 'range']}.get(table.shape[0])
        if config_type is None:
            raise DetZeroHipError('%s: %d shards name no configuration' % (what, table.shape[0]))
    names = breakdown_names(config_type)
    if len(names) != table.shape[0]:
        raise DetZeroHipError('%s: %d shards for %s' % (what, table.shape[0], list(config_type)))
    return names, config_type


def metrics_from_counts(table, config_type=None):
    """table (n_shards, 2, 101, 4) integers [TP, FP, FN, HA * 2^32] -> {'<shard>_LEVEL_<L>/AP': [value], '.../APH': [value]} in
    float64.  config_type defaults by the shard count: 4 = ['object'], 12 = ['range'], 16 = both."""
    table = np.asarray(table)
    names, config_type = check_count_table(table, 4, config_type, 'metrics_from_counts')
    t = table.astype(np.float64)
    out = {}
    for s, name in enumerate(names):
        for lv in range(2):
            tp, fp, fn, ha = t[s, lv, :, 0], t[s, lv, :, 1], t[s, lv, :, 2], t[s, lv, :, 3] / EVAL_FIXED_ONE
            det, gt = tp + fp, tp + fn
            safe_det, safe_gt = np.where(det > 0, det, 1.0), np.where(gt > 0, gt, 1.0)
            p, r = np.where(det > 0, tp / safe_det, 0.0), np.where(gt > 0, tp / safe_gt, 0.0)
            ph, rh = np.where(det > 0, ha / safe_det, 0.0), np.where(gt > 0, ha / safe_gt, 0.0)
            out['%s_LEVEL_%d/AP' % (name, lv + 1)] = [_envelope_area(p, r)]
            out['%s_LEVEL_%d/APH' % (name, lv + 1)] = [_envelope_area(ph, rh)]
    return out


def shard_ids(config_type, obj_type, boxes):
    """Per breakdown of the configuration, the shard of every object (-1 = in none): [(first shard, ids)]."""
    obj_type = np.asarray(obj_type).astype(np.int64)
    known = (obj_type >= 1) & (obj_type <= 4)
    out, first = [], 0
    if 'object' in config_type:
        out.append(np.where(known, obj_type - 1, -1))
        first = 4
    if 'range' in config_type:
        centre = boxes[:, :3] if boxes.shape[1] == 7 else boxes[:, :2]           # a BEV box has no z
        dist = np.sqrt((centre.astype(np.float64) ** 2).sum(axis=1))
        rbin = (dist >= RANGE_EDGES[0]).astype(np.int64) + (dist >= RANGE_EDGES[1])
        out.append(np.where(known, first + (obj_type - 1) * 3 + rbin, -1))
    return out


def box7(b):
    """(n, 7) or BEV (n, 5) boxes -> (n, 7) float32; no box at all is (0, 7)."""
    b = np.asarray(b, dtype=np.float32)
    b = b.reshape(len(b), -1) if len(b) else np.zeros((0, 7), dtype=np.float32)
    if b.shape[1] == 7:
        return b
    out = np.zeros((len(b), 7), dtype=np.float32)             # [x, y, dx, dy, heading]: z = 0, dz = 1 (the BEV IoU reads neither)
    out[:, [0, 1, 3, 4, 6]] = b
    out[:, 5] = 1.0
    return out


def rows_by_shard(config_type, obj_type, boxes):
    """One row per breakdown an object falls in, breakdown by breakdown: (the objects' indices, their shards)."""
    ids = shard_ids(config_type, obj_type, boxes)
    rows = [np.flatnonzero(i >= 0) for i in ids]
    shards = [i[at] for i, at in zip(ids, rows)]
    cat = lambda parts: parts[0] if len(parts) == 1 else np.concatenate(parts + [np.zeros((0,), np.int64)])      # (one part: no copy)
    return cat(rows), cat(shards)


def problem_arrays(config_type, n_frames, pd_frameid, pd_boxes, pd_type, pd_score, gt_frameid, gt_boxes, gt_type, gt_difficulty):
    """The flat arrays of generate_waymo_type_results -> what ops.eval_match_counts takes, on the host and unsorted:
    (pred key, pred box7 f32, pred score f32, gt key, gt box7 f32, gt difficulty i32, gt type of each key's shard, n_shards).
    key = frame * n_shards + shard; an object appears once per breakdown."""
    n_shards = len(breakdown_names(config_type))

    def side(frameid, boxes, obj_type, col):
        rows, shards = rows_by_shard(config_type, obj_type, boxes)
        return np.asarray(frameid, dtype=np.int64)[rows] * n_shards + shards, box7(boxes)[rows], col[rows]

    pk, pb, ps = side(pd_frameid, pd_boxes, pd_type, np.asarray(pd_score, dtype=np.float32))
    gk, gb, gd = side(gt_frameid, gt_boxes, gt_type, np.asarray(gt_difficulty).astype(np.int32))
    if pk.size and pk.max() >= n_frames * n_shards or gk.size and gk.max() >= n_frames * n_shards:
        raise DetZeroHipError('waymo_evaluation: a frame id beyond the %d frames' % n_frames)
    if not np.isfinite(ps).all():
        raise DetZeroHipError('waymo_evaluation: a prediction score is not finite')
    return pk, pb, ps, gk, gb, gd, n_shards


def shard_type(config_type, shard):
    """Object type (1..4) of the shards of a configuration."""
    shard = np.asarray(shard, dtype=np.int64)
    n_obj = 4 if 'object' in config_type else 0
    return np.where(shard < n_obj, shard + 1, (shard - n_obj) // 3 + 1)


def match_counts(config_type, n_frames, pk, pb, ps, gk, gb, gd, n_shards, box_type='3d', scheme='atomic', device=None):
    """Sort by problem (torch, on the device), describe the problems, run the kernel: the host count table."""
    import torch
    from . import ops
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    n_keys = n_frames * n_shards
    d_ps, d_pk = torch.from_numpy(ps).to(dev), torch.from_numpy(pk).to(dev)
    by_score = torch.sort(d_ps, descending=True, stable=True)[1]                # ties: ascending input index
    order = by_score[torch.sort(d_pk[by_score], stable=True)[1]]                # then by problem, the score order kept inside
    d_pb = torch.from_numpy(pb).to(dev)[order].contiguous()
    d_ps = d_ps[order].contiguous()
    d_gk = torch.from_numpy(gk).to(dev)
    g_order = torch.sort(d_gk, stable=True)[1]
    d_gb = torch.from_numpy(gb).to(dev)[g_order].contiguous()
    d_gd = torch.from_numpy(gd).to(dev)[g_order].contiguous()
    p_cnt, g_cnt = np.bincount(pk, minlength=n_keys), np.bincount(gk, minlength=n_keys)
    p_at, g_at = np.cumsum(p_cnt) - p_cnt, np.cumsum(g_cnt) - g_cnt
    live = np.flatnonzero((p_cnt > 0) | (g_cnt > 0))
    shard = live % n_shards
    desc = np.stack([p_at[live], p_cnt[live], g_at[live], g_cnt[live], shard, shard_type(config_type, shard)], axis=1).astype(np.int64)
    return ops.eval_match_counts(d_pb.reshape(-1, 7), d_ps, d_gb.reshape(-1, 7), d_gd, desc, n_shards, box_type, IOU_THRESHOLDS, scheme)


def fakelidar_to_lidar(boxes3d_lidar):
    """boxes3d_kitti_fakelidar_to_lidar of both reference estimators, on a copy."""
    boxes3d_lidar = np.array(boxes3d_lidar, copy=True)
    w, l, h, r = boxes3d_lidar[:, 3:4], boxes3d_lidar[:, 4:5], boxes3d_lidar[:, 5:6], boxes3d_lidar[:, 6:7]
    boxes3d_lidar[:, 2] += h[:, 0] / 2
    return np.concatenate([boxes3d_lidar[:, 0:3], l, w, h, -(r + np.pi / 2)], axis=-1)


def gt_frame(annos, class_names, fake_gt_infos):
    """The ground-truth part of a frame in both estimators' generate_waymo_type_results, on copies: (the mask of the boxes of the
    named classes that hold a point, the difficulties with 0 rewritten by the point count, the boxes in true lidar coordinates)."""
    box_mask = np.array([n in class_names for n in annos['name']], dtype=np.bool_)
    if 'num_points_in_gt' not in annos:
        raise NotImplementedError('Please provide the num_points_in_gt for evaluating on Waymo Dataset (infos created '
                                  'before 20201126 lack it: re-create the validation infos)')
    diff = np.array(annos['difficulty'], copy=True)
    zero_difficulty_mask = diff == 0
    diff[(annos['num_points_in_gt'] > 5) & zero_difficulty_mask] = 1
    diff[(annos['num_points_in_gt'] <= 5) & zero_difficulty_mask] = 2
    box_mask = box_mask & (annos['num_points_in_gt'] > 0)
    gt_boxes = fakelidar_to_lidar(annos['gt_boxes_lidar']) if fake_gt_infos else np.asarray(annos['gt_boxes_lidar'])
    return box_mask, diff, gt_boxes


def build_config(config_type):
    """The configuration of both reference estimators as a plain dict.  A config_type with neither '3d' nor 'bev' means '3d'."""
    breakdowns = [b for b, key in (('OBJECT_TYPE', 'object'), ('RANGE', 'range')) if key in config_type]
    return {
        'breakdown_generator_ids': breakdowns,
        'difficulties': [[1, 2] for _ in breakdowns],
        'matcher_type': 'TYPE_HUNGARIAN',
        'iou_thresholds': list(IOU_THRESHOLDS),
        'box_type': 'TYPE_2D' if ('bev' in config_type and '3d' not in config_type) else 'TYPE_3D',
        'score_cutoffs': score_cutoffs().tolist(),
    }


def normalise_scores(pd_score):
    """The sigmoid of unnormalised prediction scores, with the reference's warning."""
    if len(pd_score) and pd_score.max() > 1:
        pd_score = 1 / (1 + np.exp(-pd_score))
        print('Warning: Waymo evaluation only supports normalized scores')
    return pd_score


class WaymoDetectionMetricsEstimator:
    WAYMO_CLASSES = ['unknown', 'Vehicle', 'Pedestrian', 'Truck', 'Cyclist']

    def generate_waymo_type_results(self, infos, class_names, is_gt=False, fake_gt_infos=True, bev=False):
        """waymo_eval_detection.py:21-85, on copies: the caller's dicts are not written (the reference rewrites ``difficulty`` and
        ``gt_boxes_lidar`` in place)."""
        frame_id, boxes3d, obj_type, score, overlap_nlz, difficulty = [], [], [], [], [], []
        for frame_index, info in enumerate(infos):
            if is_gt:
                box_mask, diff, gt_boxes = gt_frame(info, class_names, fake_gt_infos)
                num_boxes = box_mask.sum()
                box_name = info['name'][box_mask]
                difficulty.append(diff[box_mask])
                score.append(np.ones(num_boxes))
                boxes3d.append(gt_boxes[box_mask][:, [0, 1, 3, 4, 6]] if bev else gt_boxes[box_mask][:, :7])
            else:
                num_boxes = len(info['boxes_lidar'])
                difficulty.append([0] * num_boxes)
                score.append(info['score'])
                boxes3d.append(info['boxes_lidar'][:, [0, 1, 3, 4, 6]] if bev else info['boxes_lidar'][:, :7])
                box_name = info['name']
            obj_type += [self.WAYMO_CLASSES.index(name) for name in box_name]
            frame_id.append(np.array([frame_index] * num_boxes))
            overlap_nlz.append(np.zeros(num_boxes))

        frame_id = np.concatenate(frame_id).reshape(-1).astype(np.int64)
        boxes3d = np.concatenate(boxes3d, axis=0)              # (a new array: the heading below is not written into an info)
        obj_type = np.array(obj_type).reshape(-1)
        score = np.concatenate(score).reshape(-1)
        overlap_nlz = np.concatenate(overlap_nlz).reshape(-1)
        difficulty = np.concatenate(difficulty).reshape(-1).astype(np.int8)
        if len(infos) == 1:                                    # np.concatenate of one array may hand the array itself back
            boxes3d = np.array(boxes3d, copy=True)
        boxes3d[:, -1] = limit_period(boxes3d[:, -1], offset=0.5, period=np.pi * 2)
        return frame_id, boxes3d, obj_type, score, overlap_nlz, difficulty

    def build_config(self, config_type):
        """waymo_eval_detection.py:87-134 as a plain dict.  A config_type with neither '3d' nor 'bev' means '3d': the reference
        leaves such a configuration without thresholds."""
        return build_config(config_type)

    def mask_by_distance(self, distance_thresh, boxes_3d, *args):
        mask = np.linalg.norm(boxes_3d[:, 0:2], axis=1) < distance_thresh + 0.5
        return tuple([boxes_3d[mask]] + [arg[mask] for arg in args])

    def waymo_arrays(self, prediction_infos, gt_infos, class_name, config_type=('object',), distance_thresh=100, fake_gt_infos=True):
        """The masked flat arrays of waymo_evaluation (:209-229), the sigmoid of unnormalised scores included."""
        assert len(prediction_infos) == len(gt_infos), '%d vs %d' % (len(prediction_infos), len(gt_infos))
        bev = 'bev' in config_type
        pd_frameid, pd_boxes3d, pd_type, pd_score, pd_overlap_nlz, _ = self.generate_waymo_type_results(
            prediction_infos, class_name, is_gt=False, bev=bev)
        gt_frameid, gt_boxes3d, gt_type, gt_score, _, gt_difficulty = self.generate_waymo_type_results(
            gt_infos, class_name, is_gt=True, fake_gt_infos=fake_gt_infos, bev=bev)
        pd_boxes3d, pd_frameid, pd_type, pd_score, pd_overlap_nlz = self.mask_by_distance(
            distance_thresh, pd_boxes3d, pd_frameid, pd_type, pd_score, pd_overlap_nlz)
        gt_boxes3d, gt_frameid, gt_type, gt_score, gt_difficulty = self.mask_by_distance(
            distance_thresh, gt_boxes3d, gt_frameid, gt_type, gt_score, gt_difficulty)
        return (pd_frameid, pd_boxes3d, pd_type, normalise_scores(pd_score)), (gt_frameid, gt_boxes3d, gt_type, gt_difficulty)

    def waymo_evaluation(self, prediction_infos, gt_infos, class_name, config_type=['object'], distance_thresh=100, fake_gt_infos=True):
        print('Start the waymo evaluation...')
        config_type = list(config_type)
        if 'object' not in config_type and 'range' not in config_type:
            raise DetZeroHipError("waymo_evaluation: config_type %s names no breakdown ('object', 'range')" % config_type)
        pd, gt = self.waymo_arrays(prediction_infos, gt_infos, class_name, config_type, distance_thresh, fake_gt_infos)
        print('Number: (pd, %d) VS. (gt, %d)' % (len(pd[1]), len(gt[1])))
        print('Level 1: %d, Level2: %d)' % ((gt[3] == 1).sum(), (gt[3] == 2).sum()))
        arrays = problem_arrays(config_type, len(gt_infos), *pd, *gt)
        box_type = 'bev' if self.build_config(config_type)['box_type'] == 'TYPE_2D' else '3d'
        table = match_counts(config_type, len(gt_infos), *arrays, box_type=box_type)
        return metrics_from_counts(table, config_type)


def pair_by_frame(det_result, gt_infos, human_study=False, whole_info=False, ordered=False):
    """detzero_eval.py:56-105: ground truth looked up by (sequence_name, frame_id) for every prediction item; frames without a
    prediction get an empty one.  The ground truth of a pair is the annos, or with ``whole_info`` (--tracking, :84) the whole info.
    ``ordered`` puts the pairs in (sequence, frame) order, which the reference leaves to the order of the result file."""
    gt_table, missed = defaultdict(dict), defaultdict(dict)
    for item in gt_infos:
        if human_study and item['sequence_name'] not in HUMAN_STUDY_LIST:
            continue
        gt_table[item['sequence_name']][item['sample_idx']] = item
        missed[item['sequence_name']][item['sample_idx']] = item
    part = (lambda info: info) if whole_info else (lambda info: info['annos'])
    pairs = []
    for item in det_result:
        if human_study and item['sequence_name'] not in HUMAN_STUDY_LIST:
            continue
        pairs.append((copy.deepcopy(item), copy.deepcopy(part(gt_table[item['sequence_name']][item['frame_id']]))))
        del missed[item['sequence_name']][item['frame_id']]
    notes = []
    for seq in missed:
        for frame in missed[seq]:
            notes.append('sequence:{}, frame:{} is missed'.format(seq, frame))
            empty = {'sequence_name': seq, 'frame_id': frame, 'boxes_lidar': np.array([]).reshape(0, 7), 'score': np.array([]),
                     'name': np.array([])}
            if whole_info:
                empty['obj_ids'] = np.array([])
            pairs.append((empty, part(missed[seq][frame])))
    if ordered:
        pairs.sort(key=lambda pair: (pair[0]['sequence_name'], pair[0]['frame_id']))
    return [p for p, _ in pairs], [g for _, g in pairs], notes


CATEGORY_LABELS = ('Vehicle', 'Pedestrain', 'Cyclist', 'Sign')                  # detzero_eval.py:146-205 (its spelling)
CATEGORY_TYPES = ('VEHICLE', 'PEDESTRIAN', 'CYCLIST', 'SIGN')


def format_table(header, rows):
    """A label and float columns as text lines: tabulate's grid where the package is installed."""
    try:
        from tabulate import tabulate
        return tabulate(rows, headers=header, tablefmt='grid').splitlines()
    except ImportError:
        lines = ['%-24s' % header[0] + ''.join('%10s' % h for h in header[1:])]
        return lines + ['%-24s' % r[0] + ''.join('%10.4f' % v for v in r[1:]) for r in rows]


def result_table(ap_dict, evaluate_metrics):
    rows = []

    def row(label, name):
        return (label,) + tuple(ap_dict['%s_LEVEL_%d/%s' % (name, lv, m)][0] for lv in (1, 2) for m in ('AP', 'APH'))

    if 'object' in evaluate_metrics:
        rows += [row(lb, 'OBJECT_TYPE_TYPE_%s' % t) for lb, t in zip(CATEGORY_LABELS, CATEGORY_TYPES)]
    if 'range' in evaluate_metrics:
        rows += [row('%s_%s' % (t.capitalize(), r), 'RANGE_TYPE_%s_%s' % (t, r)) for t in CATEGORY_TYPES for r in RANGE_NAMES]
    return format_table(['Category', 'L1/AP', 'L1/APH', 'L2/AP', 'L2/APH'], rows)


def detzero_eval_main(argv, *, tracking):
    """The command line of evaluator/detzero_eval.py.  Detection refuses --tracking; ``tracking`` (waymo_eval_tracking's second
    command line) implies it and hands the pairs, whole infos in sequence order, to the tracking estimator."""
    if tracking:
        from . import waymo_eval_tracking as wt
        what, noun, estimator = 'tracking evaluation (MOTA / MOTP)', 'tracking', wt.WaymoTrackingMetricsEstimator()
        pair, table = wt.pair_by_frame, wt.result_table
    else:
        what, noun, estimator = 'detection evaluation (AP / APH)', 'prediction', WaymoDetectionMetricsEstimator()
        pair, table = pair_by_frame, result_table
    parser = argparse.ArgumentParser(description='Offline %s on the device.' % what)
    parser.add_argument('--det_result_path', type=str, default='', help='path to the %s result file' % noun)
    parser.add_argument('--gt_info_path', type=str, default='../data/waymo/waymo_infos_val.pkl', help='path to ground-truth info pkl file')
    parser.add_argument('--evaluate_metrics', nargs='+', default=['object'], help='object, range or both')
    parser.add_argument('--iou_type', type=str, default='3d', help='3d or bev')
    parser.add_argument('--class_name', nargs='+', default=['Vehicle', 'Pedestrian', 'Cyclist'])
    parser.add_argument('--info_with_fakelidar', action='store_true', default=False)
    parser.add_argument('--distance_thresh', type=int, default=1000)
    parser.add_argument('--tracking', action='store_true', default=tracking,
                        help='(implied)' if tracking else '(refused: tracking metrics are out of scope)')
    parser.add_argument('--human_study', action='store_true', default=False)
    args = parser.parse_args(argv)
    if args.tracking and not tracking:
        raise DetZeroHipError('--tracking: the tracking metrics (MOTA / MOTP) are another protocol and are not provided by the HIP backend')
    if any(item not in ['object', 'range'] for item in args.evaluate_metrics):
        raise ValueError('evaluate_metrics error')
    if args.iou_type not in ('3d', 'bev'):
        raise KeyError(args.iou_type)
    log_path = os.path.join(os.path.dirname(os.path.abspath(args.det_result_path)), 'mAP.txt')
    log_file = open(log_path, 'a')

    def log(line=''):
        print(line, flush=True)
        log_file.write(line + '\n')

    log(str(args))
    with open(args.gt_info_path, 'rb') as f:
        gt_infos = pickle.load(f)
    with open(args.det_result_path, 'rb') as f:
        det_result = pickle.load(f)
    log('Prediction Set Length: {}, Ground Truth Set Length: {}.'.format(len(det_result), len(gt_infos)))
    eval_det, eval_gt, notes = pair(det_result, gt_infos, args.human_study)
    for note in notes:
        log(note)
    log('\tEvaluation data pair: ' + str(len(eval_gt)))
    result = estimator.waymo_evaluation(
        eval_det, eval_gt, config_type=args.evaluate_metrics + [args.iou_type], class_name=args.class_name,
        distance_thresh=args.distance_thresh, fake_gt_infos=args.info_with_fakelidar)
    log('================= Evaluation Result =================')
    log(args.det_result_path)
    for key in result:
        log('%s: %.4f ' % (key, result[key][0]))
    for line in table(result, args.evaluate_metrics):
        log(line)
    log('The whole evaulation process is done.')
    log_file.close()
    return result


def main(argv=None):
    return detzero_eval_main(argv, tracking=False)


if __name__ == '__main__':
    main()


