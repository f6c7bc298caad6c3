"""Waymo-style tracking metrics (MOTA / MOTP / MISS / MISMATCH / FP per object type and range bin, difficulty levels 1 and 2) with
the chains on the device.

Mirrors evaluator/waymo_eval_tracking.py (``WaymoTrackingMetricsEstimator``: the conversion of info dicts to flat arrays with object
and sequence ids, the distance mask that passes everything, the configuration, its command line) and the ``--tracking`` branch of
evaluator/detzero_eval.py.  The reference hands the flat arrays to TensorFlow / waymo_open_dataset; here csrc/mot_chain.hip computes
the pair weights once (``ops.mot_weights``) and walks one chain per (sequence, shard, distinct cutoff) (``ops.mot_chain_counts``), and
``metrics_from_mot_counts`` turns the count table into the five figures in float64.  The protocol is this project's statement
(include/detzero_hip.h), not pinned to the official tool.

    python -m detzero_amd.waymo_eval_tracking --pred_infos pred.pkl --gt_infos waymo_infos_val.pkl \\
        [--class_names Vehicle Pedestrian Cyclist] [--sampled_interval 1]
    python -m detzero_amd.waymo_eval_tracking --det_result_path result.pkl --gt_info_path waymo_infos_val.pkl \\
        [--evaluate_metrics object range] [--iou_type 3d|bev] [--class_name ...] [--info_with_fakelidar] [--human_study]
"""
import argparse
import pickle
import sys

import numpy as np

from . import waymo_eval
from .lib import DetZeroHipError
from .ops import EVAL_FIXED_ONE
from .waymo_eval import (CATEGORY_LABELS, CATEGORY_TYPES, IOU_THRESHOLDS, N_CUTOFFS, RANGE_NAMES, box7, breakdown_names, build_config,
                         check_count_table, detzero_eval_main, format_table, gt_frame, limit_period, normalise_scores, rows_by_shard,
                         shard_type)

METRIC_KEYS = ('MOTA', 'MOTP', 'MISS', 'MISMATCH', 'FP')
# The `last` arrays of a group's chains (101 cutoffs each) and its weights stay under this many bytes.  A 200-frame sequence of
# tools/bench_waymo_track_eval.py needs about 2 MiB of both with ['object', 'range'] (1.7 MiB of it `last`), so a group holds on
# the order of a hundred sequences - some 1 500 (sequence, shard) descriptors, enough workgroups to fill the device many times
# over - while the workspace stays a thousandth of its memory.
WORKSPACE_CAP = 256 << 20


def metrics_from_mot_counts(table, config_type=None):
    """table (n_shards, 2, 101, 5) integers [TP, FP, MISS, MISMATCH, COST * 2^32] -> {'<shard>_LEVEL_<L>/<MOTA|MOTP|MISS|MISMATCH|FP>':
    [value]} in float64: the values of the cutoff with the highest MOTA (the lowest k among equals); N = TP + MISS = 0 gives zeros.
    config_type defaults by the shard count: 4 = ['object'], 12 = ['range'], 16 = both."""
    table = np.asarray(table)
    names, config_type = check_count_table(table, 5, config_type, 'metrics_from_mot_counts')
    t = table.astype(np.float64)
    out = {}
    for s, name in enumerate(names):
        for lv in range(2):
            tp, fp, miss, mm, cost = (t[s, lv, :, q] for q in range(5))
            n = tp + miss                                       # (the same at every cutoff: the ground truths of the level)
            values = [0.0] * 5
            if n[0] > 0:
                mota = 1.0 - (miss + mm + fp) / n
                k = int(np.argmax(mota))                        # the first of the maxima
                values = [mota[k], cost[k] / EVAL_FIXED_ONE / tp[k] if tp[k] > 0 else 0.0, miss[k] / n[k], mm[k] / n[k], fp[k] / n[k]]
            for key, v in zip(METRIC_KEYS, values):
                out['%s_LEVEL_%d/%s' % (name, lv + 1, key)] = [float(v)]
    return out


def _dense_per_sequence(seq, oid, n_seq):
    """-> (dense index of every (sequence, object id) within its sequence, ids per sequence (n_seq,): a sequence may have none)."""
    if not seq.size:
        return np.zeros((0,), np.int64), np.zeros((n_seq,), np.int64)
    span = int(oid.max()) + 1
    uniq, inv = np.unique(seq * span + oid, return_inverse=True)
    seq_of = uniq // span
    first = np.searchsorted(seq_of, np.arange(n_seq), side='left')
    return inv.reshape(-1) - first[seq], np.bincount(seq_of, minlength=n_seq)


def chain_arrays(config_type, pd, gt):
    """The flat arrays of generate_waymo_type_results, pd = (frame, sequence, object id, box, type, score) and gt = (frame, sequence,
    object id, box, type, difficulty) -> the host arrays of the device ops, sorted by (sequence, shard, frame): a dict of pred_box,
    pred_score, pred_id, gt_box, gt_id, gt_diff, pdesc (n, 5), cdesc (c, 6), chain_seq (c,), n_shards.  An object appears once per
    breakdown.  Raises on an object id that appears twice in a frame."""
    n_shards = len(breakdown_names(config_type))
    names = np.unique(np.concatenate([np.asarray(pd[1]).astype(str), np.asarray(gt[1]).astype(str)]))
    n_frames = int(max(np.max(pd[0], initial=-1), np.max(gt[0], initial=-1))) + 1

    def side(what, frame, seq, oid, boxes, obj_type, col, dtype):
        frame, oid = np.asarray(frame, dtype=np.int64), np.asarray(oid, dtype=np.int64)
        seq = np.searchsorted(names, np.asarray(seq).astype(str)).astype(np.int64)
        if oid.size and oid.min() < 0:
            raise DetZeroHipError('waymo_evaluation: a negative %s object id' % what)
        pairs = frame * (int(oid.max()) + 1 if oid.size else 1) + oid
        if np.unique(pairs).size != pairs.size:
            raise DetZeroHipError('waymo_evaluation: a %s object id appears twice in one frame' % what)
        dense, n_ids = _dense_per_sequence(seq, oid, len(names))           # (the other side may hold sequences this one lacks)
        boxes = box7(boxes)
        rows, shards = rows_by_shard(config_type, obj_type, boxes)
        keys = (seq[rows] * n_shards + shards) * n_frames + frame[rows]
        return keys, boxes[rows], dense[rows].astype(np.int32), np.asarray(col).astype(dtype)[rows], n_ids

    pk, pb, pi, ps, n_pid = side('prediction', pd[0], pd[1], pd[2], pd[3], pd[4], pd[5], np.float32)
    gk, gb, gi, gd, n_gid = side('ground-truth', gt[0], gt[1], gt[2], gt[3], gt[4], gt[5], np.int32)
    if not np.isfinite(ps).all():
        raise DetZeroHipError('waymo_evaluation: a prediction score is not finite')
    by_score = np.argsort(-ps, kind='stable')                   # ties: ascending input index
    order = by_score[np.argsort(pk[by_score], kind='stable')]   # then by problem, the score order kept inside
    g_order = np.argsort(gk, kind='stable')
    pk, pb, pi, ps = pk[order], pb[order], pi[order], ps[order]
    gk, gb, gi, gd = gk[g_order], gb[g_order], gi[g_order], gd[g_order]
    live = np.unique(np.concatenate([pk, gk]))
    p_cnt = np.bincount(np.searchsorted(live, pk), minlength=live.size)
    g_cnt = np.bincount(np.searchsorted(live, gk), minlength=live.size)
    chain_of = live // max(n_frames, 1)                          # sequence * n_shards + shard
    shard = chain_of % n_shards
    pdesc = np.stack([np.cumsum(p_cnt) - p_cnt, p_cnt, np.cumsum(g_cnt) - g_cnt, g_cnt, shard_type(config_type, shard)], axis=1).astype(np.int64)
    chains, first = np.unique(chain_of, return_index=True)
    count = np.diff(np.append(first, live.size))
    seq = chains // n_shards
    biggest = np.maximum.reduceat(p_cnt + g_cnt, first) if live.size else np.zeros((0,), np.int64)
    cdesc = np.stack([first, count, chains % n_shards, n_pid[seq], n_gid[seq], biggest], axis=1).astype(np.int64).reshape(-1, 6)
    return {'pred_box': pb, 'pred_score': ps, 'pred_id': pi, 'gt_box': gb, 'gt_id': gi, 'gt_diff': gd, 'pdesc': pdesc, 'cdesc': cdesc,
            'chain_seq': seq, 'n_shards': n_shards}


def sequence_groups(arrays, cap=WORKSPACE_CAP):
    """Runs of whole sequences whose weights and chain workspaces stay under ``cap`` bytes (a sequence alone may pass it):
    [(first chain, end chain)]."""
    from . import ops
    cdesc, pdesc, seq = arrays['cdesc'], arrays['pdesc'], arrays['chain_seq']
    size = pdesc[:, 1] * pdesc[:, 3] * 4
    need = np.array([ops.mot_chain_ws_bytes(c[3], c[4], c[5]) for c in cdesc], dtype=np.int64)     # (the library's own size)
    need = need + np.add.reduceat(size, cdesc[:, 0]) if len(cdesc) else need
    groups, lo, total = [], 0, 0
    for c in range(len(cdesc)):
        if c > lo and seq[c] != seq[c - 1]:
            nxt = int(need[c:][seq[c:] == seq[c]].sum())
            if total + nxt > cap:
                groups.append((lo, c))
                lo, total = c, 0
        total += int(need[c])
    if len(cdesc):
        groups.append((lo, len(cdesc)))
    return groups


def chain_counts(arrays, box_type='3d', mapping='wave', merge=True, cap=WORKSPACE_CAP, device=None, timings=None):
    """Group by group: the weights kernel, then the chain kernel, all adding to one device table -> the host count table.
    ``timings`` (a dict) gets the device time of the launches alone under 'weights' and 'chain[<mapping>]' (events around each
    library call, ops.LaunchProfiler), the groups added."""
    import torch
    from . import ops
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    table = torch.zeros((arrays['n_shards'], 2, N_CUTOFFS, ops.MOT_COUNTS), dtype=torch.int64, device=dev)
    pdesc, cdesc = arrays['pdesc'], arrays['cdesc']
    statuses = []

    saved = ops.PROFILER
    if timings is not None:
        ops.PROFILER = ops.LaunchProfiler()
    try:
        for lo, hi in sequence_groups(arrays, cap):
            f0, f1 = int(cdesc[lo, 0]), int(cdesc[hi - 1, 0] + cdesc[hi - 1, 1])
            pd5 = pdesc[f0:f1].copy()
            p0, p1, g0, g1 = int(pd5[0, 0]), int(pd5[-1, 0] + pd5[-1, 1]), int(pd5[0, 2]), int(pd5[-1, 2] + pd5[-1, 3])
            pd5[:, 0] -= p0
            pd5[:, 2] -= g0
            cd = cdesc[lo:hi].copy()
            cd[:, 0] -= f0
            pd6, w_len = ops.mot_problem_desc(pd5)
            t = lambda a, lo_, hi_: torch.from_numpy(np.ascontiguousarray(a[lo_:hi_])).to(dev)
            pb, ps, pi = t(arrays['pred_box'], p0, p1).reshape(-1, 7), t(arrays['pred_score'], p0, p1), t(arrays['pred_id'], p0, p1)
            gb, gi, gd = t(arrays['gt_box'], g0, g1).reshape(-1, 7), t(arrays['gt_id'], g0, g1), t(arrays['gt_diff'], g0, g1)
            weights, cut = ops.mot_weights(pb, ps, gb, pd6, w_len, box_type, IOU_THRESHOLDS)
            statuses.append(ops.mot_chain_counts_nosync(weights, cut, pi, gi, gd, pd6, cd, np.arange(f1 - f0, dtype=np.int64), arrays['n_shards'],
                                                        mapping, merge, table)[1])
        if timings is not None:
            for name, rec in ops.PROFILER.summary().items():
                key = 'weights' if name.startswith('mot_weights') else 'chain[%s]' % mapping
                timings[key] = timings.get(key, 0.0) + rec['ms'] * 1e-3
    finally:
        ops.PROFILER = saved
    for status in statuses:
        ops._eval_raise(status, 'mot_chain_counts')
    return table.cpu().numpy()


class WaymoTrackingMetricsEstimator:
    WAYMO_CLASSES = ['unknown', 'Vehicle', 'Pedestrian', 'Sign', 'Cyclist']

    def generate_waymo_type_results(self, infos, class_names, is_gt=False, fake_gt_infos=True):
        """waymo_eval_tracking.py:20-101, on copies: the caller's dicts are not written (the reference rewrites ``difficulty`` and
        ``gt_boxes_lidar`` in place).  A ground-truth info is the whole info (with 'annos') or the annos with 'sequence_name'."""
        frame_id, sequence_id, object_id, boxes3d, obj_type, score, overlap_nlz, difficulty, speed = [], [], [], [], [], [], [], [], []
        sequence_id_dict, object_id_dict = {}, {}
        for frame_index, info in enumerate(infos):
            sequence_name = info['sequence_name']
            if is_gt:
                annos = info['annos'] if 'annos' in info else info
                box_mask, diff, gt_boxes = gt_frame(annos, class_names, fake_gt_infos)
                num_boxes = box_mask.sum()
                box_name = annos['name'][box_mask]
                difficulty.append(diff[box_mask])
                score.append(np.ones(num_boxes))
                boxes3d.append(gt_boxes[box_mask][:, :7])
                speed.append(gt_boxes[box_mask][:, 7:])
                ids = np.asarray(annos['obj_ids'])[box_mask]
                keys = [obj_id for obj_id in ids.tolist()]
            else:
                num_boxes = len(info['boxes_lidar'])
                difficulty.append([0] * num_boxes)
                score.append(info['score'])
                boxes3d.append(np.array(info['boxes_lidar'][:, :7]))
                speed.append(np.array(info['boxes_lidar'][:, 7:]))
                box_name = info['name']
                keys = [sequence_name + '-' + str(obj_id) for obj_id in np.asarray(info['obj_ids']).tolist()] if num_boxes else []
            for key in keys:
                if key not in object_id_dict:
                    object_id_dict[key] = len(object_id_dict)
                object_id.append(object_id_dict[key])
            if sequence_name not in sequence_id_dict:
                sequence_id_dict[sequence_name] = len(sequence_id_dict)
            obj_type += [self.WAYMO_CLASSES.index(name) for name in box_name]
            frame_id.append(np.array([frame_index] * num_boxes))
            sequence_id.append(np.array([sequence_id_dict[sequence_name]] * num_boxes))
            overlap_nlz.append(np.zeros(num_boxes))

        frame_id = np.concatenate(frame_id).reshape(-1).astype(np.int64)
        sequence_id = np.concatenate(sequence_id).reshape(-1).astype(np.int64).astype(str)
        object_id = np.array(object_id).reshape(-1).astype(np.int64)
        boxes3d = np.array(np.concatenate(boxes3d, axis=0), dtype=np.float64)   # (a new array: the heading below is not written into an info)
        speed = np.concatenate(speed, axis=0)
        obj_type = np.array(obj_type).reshape(-1)
        score = np.concatenate(score).reshape(-1)
        overlap_nlz = np.concatenate(overlap_nlz).reshape(-1)
        difficulty = np.concatenate(difficulty).reshape(-1).astype(np.int8)
        boxes3d[:, -1] = limit_period(boxes3d[:, -1], offset=0.5, period=np.pi * 2)
        return frame_id, sequence_id, object_id, boxes3d, obj_type, score, overlap_nlz, difficulty, speed

    def build_config(self, config_type):
        """waymo_eval_tracking.py:103-137 as a plain dict; 'bev' alone selects the BEV IoU as in the detection mirror (the reference's
        tracking configuration is always TYPE_3D)."""
        return build_config(config_type)

    def mask_by_distance(self, distance_thresh, boxes_3d, *args):
        """waymo_eval_tracking.py:219-227: the mask passes every box (distance < inf)."""
        mask = np.linalg.norm(boxes_3d[:, 0:2], axis=1) < float('inf')
        return tuple([boxes_3d[mask]] + [arg[mask] for arg in args])

    def waymo_arrays(self, prediction_infos, gt_infos, class_name, distance_thresh=100, fake_gt_infos=True):
        """The masked flat arrays of waymo_evaluation (:234-254), the sigmoid of unnormalised scores included; the sequence ids of
        both sides are the sequence names' order of first appearance among the predictions."""
        assert len(prediction_infos) == len(gt_infos), '%d vs %d' % (len(prediction_infos), len(gt_infos))
        gt_infos = [g if 'sequence_name' in g else dict(g, sequence_name=p['sequence_name']) for p, g in zip(prediction_infos, gt_infos)]
        pd_frameid, pd_seq, pd_objid, pd_boxes3d, pd_type, pd_score, pd_nlz, _, pd_speed = self.generate_waymo_type_results(
            prediction_infos, class_name, is_gt=False, fake_gt_infos=fake_gt_infos)
        gt_frameid, gt_seq, gt_objid, gt_boxes3d, gt_type, gt_score, _, gt_difficulty, gt_speed = self.generate_waymo_type_results(
            gt_infos, class_name, is_gt=True, fake_gt_infos=fake_gt_infos)
        pd_boxes3d, pd_frameid, pd_seq, pd_objid, pd_type, pd_score, pd_nlz, pd_speed = self.mask_by_distance(
            distance_thresh, pd_boxes3d, pd_frameid, pd_seq, pd_objid, pd_type, pd_score, pd_nlz, pd_speed)
        gt_boxes3d, gt_frameid, gt_seq, gt_objid, gt_type, gt_score, gt_difficulty, gt_speed = self.mask_by_distance(
            distance_thresh, gt_boxes3d, gt_frameid, gt_seq, gt_objid, gt_type, gt_score, gt_difficulty, gt_speed)
        return ((pd_frameid, pd_seq, pd_objid, pd_boxes3d, pd_type, normalise_scores(pd_score)), (gt_frameid, gt_seq, gt_objid, gt_boxes3d, gt_type, gt_difficulty))

    def waymo_evaluation(self, prediction_infos, gt_infos, class_name, config_type=['object'], distance_thresh=100, fake_gt_infos=True,
                         mapping='wave', timings=None):
        print('Start the waymo evaluation...')
        config_type = list(config_type)
        if 'object' not in config_type and 'range' not in config_type:
            raise DetZeroHipError("waymo_evaluation: config_type %s names no breakdown ('object', 'range')" % config_type)
        import time
        start = time.perf_counter()
        pd, gt = self.waymo_arrays(prediction_infos, gt_infos, class_name, distance_thresh, fake_gt_infos)
        print('Number: (pd, %d) VS. (gt, %d)' % (len(pd[3]), len(gt[3])))
        print('Level 1: %d, Level2: %d' % ((gt[5] == 1).sum(), (gt[5] == 2).sum()))
        box_type = 'bev' if self.build_config(config_type)['box_type'] == 'TYPE_2D' else '3d'
        arrays = chain_arrays(config_type, pd, gt)
        if timings is not None:
            timings['conversion'] = time.perf_counter() - start
        table = chain_counts(arrays, box_type=box_type, mapping=mapping, timings=timings)
        start = time.perf_counter()
        out = metrics_from_mot_counts(table, config_type)
        if timings is not None:
            timings['metrics'] = time.perf_counter() - start
        return out


def pair_by_frame(det_result, gt_infos, human_study=False):
    """detzero_eval.py:56-105 with --tracking: the whole ground-truth info (:84) of every prediction item, the pairs in (sequence,
    frame) order - the estimator walks a sequence's frames in list order."""
    return waymo_eval.pair_by_frame(det_result, gt_infos, human_study, whole_info=True, ordered=True)


def result_table(mot_dict, evaluate_metrics):
    """detzero_eval.py:164-206: one row per category and level (the reference's range rows read detection keys; here they carry
    the tracking figures too)."""
    rows = []

    def two(label, name):
        return [(label,) + tuple(mot_dict['%s_LEVEL_%d/%s' % (name, lv, m)][0] for m in METRIC_KEYS) for lv in (1, 2)]

    if 'object' in evaluate_metrics:
        for lb, t in zip(CATEGORY_LABELS, CATEGORY_TYPES):
            rows += two(lb, 'OBJECT_TYPE_TYPE_%s' % t)
    if 'range' in evaluate_metrics:
        for t in CATEGORY_TYPES:
            for r in RANGE_NAMES:
                rows += two('%s_%s' % (t.capitalize(), r), 'RANGE_TYPE_%s_%s' % (t, r))
    return format_table(['Category'] + list(METRIC_KEYS), rows)


def main_detzero_eval(argv=None):
    """The command line of evaluator/detzero_eval.py with --tracking implied."""
    return detzero_eval_main(argv, tracking=True)


def main(argv=None):
    """evaluator/waymo_eval_tracking.py:271-295; with --det_result_path in the arguments, detzero_eval.py's command line instead."""
    argv = sys.argv[1:] if argv is None else list(argv)
    if any(a.split('=')[0] == '--det_result_path' for a in argv):
        return main_detzero_eval(argv)
    parser = argparse.ArgumentParser(description='Tracking evaluation (MOTA / MOTP) of waymo-format results on the device.')
    parser.add_argument('--pred_infos', type=str, default=None, help='pickle file')
    parser.add_argument('--gt_infos', type=str, default=None, help='pickle file')
    parser.add_argument('--class_names', type=str, nargs='+', default=['Vehicle', 'Pedestrian', 'Cyclist'], help='')
    parser.add_argument('--sampled_interval', type=int, default=1, help='sampled interval for GT sequences')
    args = parser.parse_args(argv)
    with open(args.pred_infos, 'rb') as f:
        pred_infos = pickle.load(f)
    with open(args.gt_infos, 'rb') as f:
        gt_infos = pickle.load(f)
    print('Start to evaluate the waymo format results...')
    gt_infos_dst = []
    for idx in range(0, len(gt_infos), args.sampled_interval):
        cur_info = dict(gt_infos[idx]['annos'])                 # (a copy: the reference writes frame_id into the caller's annos)
        cur_info['frame_id'] = gt_infos[idx]['frame_id']
        if 'sequence_name' in gt_infos[idx]:
            cur_info['sequence_name'] = gt_infos[idx]['sequence_name']
        gt_infos_dst.append(cur_info)
    # (the reference calls waymo_evaluation without its config_type argument, which fails; ['object'] is the estimator's usual one)
    waymo_mot = WaymoTrackingMetricsEstimator().waymo_evaluation(
        pred_infos, gt_infos_dst, class_name=args.class_names, config_type=['object'], distance_thresh=1000, fake_gt_infos=True)
    print(waymo_mot)
    return waymo_mot


if __name__ == '__main__':
    main()
