"""Tracklet recall of a tracking result against the ground truth (tracking/tools/eval_track.py) on one trajectory-pair kernel.

Mirror of the reference's ``tracking/detzero_track/utils/track_recall.py:19-262`` (TrackRecall) and
``utils/track_calculation.py:84-123`` (get_trajectory_similarity): same names, arguments, result dicts and log lines.

The reference calls get_trajectory_similarity - a Python merge walk over two frame lists - once per (ground-truth trajectory,
track) pair, on per-frame IoU matrices computed and copied back one by one.  Here ``eval_single_seq`` makes one
dz_traj_pair_table call per sequence (track_assign.trajectory_sides builds the tables): ``similarity`` = sum_all / the ground
truth's length where n_hit > 0, else -1; ``match_count`` = n_hit; ``same_frame_count`` = n_same.  Frame ordinals are the
ground-truth frames in ascending ``int(sample_idx)``, the order the merge walk assumes; a trajectory whose sample_idx does not
ascend is refused by name, where the reference would silently skip frames.  Sequences run one after another in this process.
"""
import os
import pickle
from collections import defaultdict

import numpy as np

from . import track_adapter, track_assign
from .lib import DetZeroHipError


def get_trajectory_similarity(track_a, track_b, iou_mat_dict, iou_thresholds, least_len=0.):
    """The reference's merge walk of one pair (track_calculation.py:84-123), host only: (similarity, match_count,
    same_frame_count).  Kept for users of the shim; TrackRecall takes the three numbers of every pair from the kernel."""
    frames_a = [int(x) for x in track_a['sample_idx']]
    frames_b = [int(x) for x in track_b['sample_idx']]
    if frames_a[0] > frames_b[-1] or frames_a[-1] < frames_b[0]:
        return -1, 0, 0
    similarity, match_count, same_frame_count = 0, 0, 0
    ia = ib = 0
    while ia < len(frames_a) and ib < len(frames_b):
        if frames_a[ia] == frames_b[ib]:
            iou = iou_mat_dict[str(frames_a[ia])][track_a['iou_idx'][ia], track_b['iou_idx'][ib]]
            similarity += iou
            if iou >= iou_thresholds[track_a['name'][ia]]:
                match_count += 1
            ia += 1
            ib += 1
            same_frame_count += 1
        elif frames_a[ia] < frames_b[ib]:
            ia += 1
        else:
            ib += 1
    if match_count / len(frames_a) >= least_len and match_count > 0:
        similarity = similarity / len(frames_a)
    else:
        similarity = -1.
    return similarity, match_count, same_frame_count


def _ascending(sample_idx, what):
    frames = [int(x) for x in sample_idx]
    if any(b <= a for a, b in zip(frames, frames[1:])):
        raise DetZeroHipError('tracklet recall: sample_idx of %s is not ascending' % what)


class TrackRecall():
    def __init__(self, root_path, data_path, split, workers, class_names, difficultys=['l2'], iou_threshold=[0.7, 0.5, 0.5], method='3d',
                 logger=None, ops=None):
        self.root_path = root_path
        self.data_path = data_path
        self.split = split
        self.workers = workers              # accepted for the reference's signature: no process pool opens the GPU
        self.class_names = class_names
        self.difficultys = difficultys
        self.method = method
        self.ops = ops
        assert len(class_names) == len(iou_threshold)
        self.iou_thresholds = dict(zip(self.class_names, iou_threshold))
        if logger is None:
            import logging
            logger = logging.getLogger(__name__)
        self.logger = logger
        self.logger.info('Begin Tracklet Recall Evaluation'.center(100, '-'))
        self.match_rate_list = np.arange(0, 10) * 0.1
        self.init_data()

    def init_data(self):
        self.gt_path = os.path.join(self.root_path, 'data/waymo', 'waymo_infos_%s.pkl' % self.split)
        with open(self.gt_path, 'rb') as f:
            self.gt_data = track_adapter.sequence_list_to_dict(pickle.load(f))
        with open(self.data_path, 'rb') as f:
            self.pred_data = pickle.load(f)
        self.seq_name_list = list(self.pred_data.keys())

    def get_tracklet_recall(self):
        eval_results = {}
        for seq in self.seq_name_list:
            eval_results[seq] = self.eval_single_seq({'gt': self.gt_data[seq], 'pred': self.pred_data[seq]}, class_names=self.class_names,
                                                     difficultys=self.difficultys, iou_thresholds=self.iou_thresholds, method=self.method,
                                                     ops=self.ops)
        result = self.calculate_tracklet_recall(eval_results)
        result['iou_thresholds'] = self.iou_thresholds
        result['method'] = self.method
        self.logger.info('Tracklet Recall Results'.center(100, '-'))
        self.show_traj_ap_infos(result)
        return result

    def show_traj_ap_infos(self, trk_recall_result):
        show_attributes = ['cutoffs', 'recalls', 'tp', 'fp', 'pred_nums', 'gt_nums']
        for class_n in self.class_names:
            for difficulty in self.difficultys:
                for i in range(len(trk_recall_result[difficulty][class_n]['tp'])):
                    if i != 8:
                        continue
                    log_str = '{:<3s} {:<10s}'.format(difficulty.upper(), class_n)
                    for attribute in show_attributes:
                        val = trk_recall_result[difficulty][class_n][attribute][i]
                        if attribute in ['tp', 'fp']:
                            log_str += '{}{} {:<4.1f}'.format(' ' * 2, attribute.upper() + ':', val / len(self.seq_name_list))
                        elif attribute in ['pred_nums', 'gt_nums']:
                            log_str += '{}{} {:<4.1f}'.format(' ' * 2, attribute.capitalize() + ':', val / len(self.seq_name_list))
                        else:
                            log_str += '{}{} {:<.4f}'.format(' ' * 2, attribute[:-1].capitalize() + ':', val)
                    self.logger.info(log_str)

    def calculate_tracklet_recall(self, eval_result):
        temp = defaultdict(dict)
        for difficulty in self.difficultys:
            for class_n in self.class_names:
                temp[difficulty][class_n] = defaultdict(list)
                for seq_n in eval_result.keys():
                    for key, val in eval_result[seq_n][difficulty][class_n].items():
                        temp[difficulty][class_n][key].extend(val)
        ap_result = defaultdict(dict)
        for difficulty in self.difficultys:
            for class_n in self.class_names:
                ap_result[difficulty][class_n] = defaultdict(list)
                cur = temp[difficulty][class_n]
                for key in cur.keys():
                    cur[key] = np.array(cur[key], dtype=object) if key == 'duplicate_preds' else np.array(cur[key])
        for difficulty in self.difficultys:
            for class_n in self.class_names:
                cur, ap = temp[difficulty][class_n], ap_result[difficulty][class_n]
                gt_nums = len(cur['gt_box_nums_list'])
                pred_nums = len(cur['match_pred_box_nums_list']) + len(cur['unmatch_pred_box_nums_list'])
                for match_rate_threshold in self.match_rate_list:
                    tp = np.count_nonzero(cur['match_rate'] >= match_rate_threshold) if gt_nums > 0 else 0
                    fp = pred_nums - tp
                    ap['precisions'].append(tp / (tp + fp + 1e-9))
                    ap['recalls'].append(tp / (gt_nums + 1e-9))
                    ap['tp'].append(tp)
                    ap['fp'].append(fp)
                    ap['pred_nums'].append(pred_nums)
                    ap['cutoffs'].append(float(match_rate_threshold))
                    ap['gt_nums'].append(gt_nums)
        return ap_result

    @staticmethod
    def eval_single_seq(data_dict, class_names, difficultys, iou_thresholds, method='3d', ops=None):
        """``data_dict`` = ``{'gt': {sample_idx: info}, 'pred': {track id: track}}`` of one sequence -> per difficulty and class the
        lists gt_box_nums_list, match_rate, match_pred_box_nums_list, match_len, same_len, duplicate_preds,
        unmatch_pred_box_nums_list (track_recall.py:153-262).  ``method``: '3d' or 'bev'."""
        from .track_models import GNN_assignment
        if method not in track_assign.METRIC_OF:
            raise DetZeroHipError('tracklet recall: method %r (3d or bev)' % (method,))
        gt_data, pred_data = data_dict['gt'], data_dict['pred']
        ops = ops if ops is not None else track_assign.HipTrajOps()

        track_frames = track_adapter.frame_list_to_dict(track_adapter.tracklets_to_frames({'reference': gt_data, 'source': pred_data}))
        gt_keys = ['gt_boxes_global', 'name', 'obj_ids', 'difficulty', 'num_points_in_gt']
        gt_id_data = track_assign.get_gt_id_data(gt_data, gt_keys, class_names)
        gt_ids, pred_ids = list(gt_id_data.keys()), list(pred_data.keys())
        for gt_id in gt_ids:
            gt_info = gt_id_data[gt_id]
            for key in gt_info.keys():
                gt_info[key] = np.array(gt_info[key])
            _ascending(gt_info['sample_idx'], 'ground-truth object %s' % gt_id)
        for pred_id in pred_ids:
            _ascending(pred_data[pred_id]['sample_idx'], 'track %s' % pred_id)

        frame_keys = sorted(gt_data.keys(), key=int)
        ops.set_sides(*track_assign.trajectory_sides(frame_keys, gt_data, track_frames, class_names, gt_ids, pred_ids, False, 'tracklet recall'))
        shape = (len(gt_ids), len(pred_ids))
        if shape[0] and shape[1]:
            sum_all, _, n_hit, n_same = ops.table(track_assign.METRIC_OF[method], True, [float(iou_thresholds[n]) for n in class_names])
        else:
            sum_all, n_hit, n_same = np.zeros(shape, np.float32), np.zeros(shape, np.int32), np.zeros(shape, np.int32)
        gt_len = np.array([len(gt_id_data[g]['sample_idx']) for g in gt_ids], dtype=np.float32).reshape(-1, 1)
        traj_similar_mat = (np.asarray(sum_all, dtype=np.float32) / gt_len).astype(np.float32)
        traj_similar_mat[np.asarray(n_hit) <= 0] = -1.
        traj_same_count_mat = np.asarray(n_same).astype(np.float32)
        traj_match_count_mat = np.asarray(n_hit).astype(np.float32)

        match, unmatch_gt, unmatch_pred = GNN_assignment(1 - traj_similar_mat)

        eval_result = defaultdict(dict)
        for difficulty in difficultys:
            for class_n in class_names:
                eval_result[difficulty][class_n] = defaultdict(list)
        for gt_id in gt_ids:
            difficulty = np.array(gt_id_data[gt_id]['difficulty'])
            num_points_in_gt = np.array(gt_id_data[gt_id]['num_points_in_gt'])
            l1_mask = (num_points_in_gt > 5) & (difficulty == 0)
            l2_mask = (num_points_in_gt <= 5) & (difficulty == 0)
            difficulty[l1_mask] = 1
            difficulty[l2_mask] = 2
            gt_id_data[gt_id]['difficulty'] = difficulty

        difficulty_dict = {1: 'l1', 2: 'l2'}
        for k in range(len(match)):
            gt_idx, pred_idx = match[k, 0], match[k, 1]
            gt_id = gt_ids[gt_idx]
            name = gt_id_data[gt_id]['name'][0]
            difficulty = gt_id_data[gt_id]['difficulty']
            cur = eval_result['l2' if np.count_nonzero(difficulty == 2) > 0 else 'l1'][name]
            cur['gt_box_nums_list'].append(len(difficulty))
            cur['match_rate'].append(traj_match_count_mat[gt_idx, pred_idx] / len(difficulty))
            cur['match_pred_box_nums_list'].append(len(pred_data[pred_ids[pred_idx]]['name']))
            cur['match_len'].append(traj_match_count_mat[gt_idx, pred_idx])
            cur['same_len'].append(traj_same_count_mat[gt_idx, pred_idx])
            cur['duplicate_preds'].append(traj_match_count_mat[gt_idx, :])
        for pred_idx in unmatch_pred:
            pred_id = pred_ids[pred_idx]
            name = pred_data[pred_id]['name'][0]
            for difficulty in difficultys:
                eval_result[difficulty][name]['unmatch_pred_box_nums_list'].append(len(pred_data[pred_id]['name']))
        for gt_idx in unmatch_gt:
            gt_id = gt_ids[gt_idx]
            name = gt_id_data[gt_id]['name'][0]
            difficulty = gt_id_data[gt_id]['difficulty']
            eval_result[difficulty_dict[difficulty[0]]][name]['gt_box_nums_list'].append(len(difficulty))
        return eval_result
