"""The refining stage's other end: mirrors of ``daemon/combine_output.py`` and ``daemon/generate_iou_gt.py``.

    python -m detzero_amd.refine_combine combine --split val [--combine_conf_res] [--combine_drop_path P] [--root_path data/waymo/refining]
    python -m detzero_amd.refine_combine iou --class_name Vehicle --geo_path G --pos_path P [--root_path data/waymo/refining]

``combine_final`` merges the three refiners' result pickles (refine_results.{grm,prm,crm}_prediction_dicts: sizes from the geometry
model, centres and headings from the position model, scores from the confidence model) into ``<Class>_final.pkl`` (track level) and
``<Class>_final_frame.pkl`` (frame level); ``convert_frame_format`` and ``combine_det`` are its two steps.  Host numpy as there, one box
at a time through the bit-exact track_adapter.transform_boxes3d, in this process (the reference starts a one-worker process pool).

``generate_refine_boxes_iou`` computes the IoU labels of the confidence model's training (``<Class>_iou_train.pkl``).  The reference
builds, per object, the N x N IoU matrix of its refined boxes against its ground-truth boxes and keeps the diagonal; here all objects
of a sequence go through ONE iou3d_nms_utils.boxes_iou3d_paired_gpu call over the concatenated boxes.
"""
import argparse
import logging
import os
import pickle
from collections import defaultdict

import numpy as np

from .track_adapter import dict_to_sequence_list, sequence_list_to_dict, transform_boxes3d


def load_pkl(path):
    with open(path, 'rb') as f:
        return pickle.load(f)


def save_pkl(data, path):
    with open(path, 'wb') as f:
        pickle.dump(data, f)


def combine_det(combine_data, drop_path):
    """combine_output.py:27-41: the boxes the tracker dropped (``drop_path``: {seq: {frame: record}}) appended to every frame."""
    drop_data = load_pkl(drop_path)
    combine_data = sequence_list_to_dict(combine_data)
    for seq, frames in combine_data.items():
        for frm, rec in frames.items():
            for key in ('boxes_lidar', 'name', 'score'):
                rec[key] = np.concatenate([rec[key], drop_data[seq][frm][key]], axis=0)
    return dict_to_sequence_list(combine_data)


def convert_frame_format(track_data):
    """combine_output.py:44-99: {track id: track} of one sequence -> list of frame records, frames and objects in first-seen order."""
    order_map = defaultdict(list)
    for tk_id, tk in track_data.items():
        for i, sa_idx in enumerate(tk['sample_idx']):
            order_map[sa_idx].append([tk_id, i])
    frames = []
    for frm_id, pairs in order_map.items():
        pairs = np.stack(pairs)
        obj_ids, orders = pairs[:, 0], pairs[:, 1]
        first = track_data[obj_ids[0]]
        seq, pose = first['sequence_name'], first['pose'][orders[0]]          # (sic) the frame's pose: that of its first object
        n = len(obj_ids)
        boxes_lidar = np.zeros((n, 7), dtype=np.float32)
        boxes_global = np.zeros((n, 9), dtype=np.float32)
        score = np.zeros((n), dtype=np.float32)
        name = np.full(n, 'none', dtype=object)
        for i, obj_id in enumerate(obj_ids):
            tk, idx = track_data[obj_id], orders[i]
            if 'boxes_lidar' in tk:
                boxes_lidar[i] = tk['boxes_lidar'][idx]
            elif 'boxes_global' in tk:
                boxes_global[i] = tk['boxes_global'][idx]
                # one box at a time (the reference hands transform_boxes3d the 1-D row here, which it cannot index: as a row of one)
                boxes_lidar[i] = transform_boxes3d(boxes_global[i][None, :], pose, inverse=True).reshape(-1)
            score[i] = tk['score'][idx]
            name[i] = tk['name'][idx]
        frames.append({'sequence_name': seq, 'frame_id': int(frm_id), 'obj_ids': obj_ids, 'name': name, 'score': score,
                       'boxes_lidar': boxes_lidar, 'boxes_global': boxes_global, 'pose': pose})
    return frames


def combine_final(root_path, class_names, logger, split='val', combine_conf_res=True, combine_drop_path=None, track_save=True,
                  frame_save=True):
    """combine_output.py:102-167.  (sic) one dict collects every class: the file of a later class holds the earlier classes' objects
    too, and its frame-level list covers the sequences of ITS position result."""
    combine_dict = defaultdict(dict)
    root_path = os.path.join(root_path, 'result')
    for name in class_names:
        geo_path = os.path.join(root_path, '%s_geometry_%s.pkl' % (name, split))
        pos_path = os.path.join(root_path, '%s_position_%s.pkl' % (name, split))
        if not os.path.exists(geo_path) or not os.path.exists(pos_path):
            raise FileNotFoundError('Cannot find the input files.')
        geo_res, pos_res = load_pkl(geo_path), load_pkl(pos_path)
        conf_res = load_pkl(os.path.join(root_path, '%s_confidence_%s.pkl' % (name, split))) if combine_conf_res else None
        seq_names = list(pos_res.keys())
        for seq in seq_names:
            for obj, rec in pos_res[seq].items():
                boxes_geo = np.concatenate(geo_res[seq][obj]['boxes_lidar'], axis=0)
                rec['boxes_lidar'] = np.array(rec['boxes_lidar'])
                rec['boxes_lidar'][:, 3:6] = boxes_geo[:, 3:6]
                if combine_conf_res:
                    rec['score'] = conf_res[seq][obj]['new_score']
                rec['sample_idx'] = np.array([str(x) for x in rec['frame_id']])
                combine_dict[seq][obj] = rec
        if track_save:
            save_path = os.path.join(root_path, '%s_final.pkl' % name)
            save_pkl(combine_dict, save_path)
            logger.info('Track level final result is saved at %s' % save_path)
        if frame_save:
            logger.info('Start to convert track level result into frame level')
            final_res = []
            for seq in seq_names:
                final_res.extend(convert_frame_format(combine_dict[seq]))
            if combine_drop_path is not None:                      # not combined when the result serves as auto labels
                logger.info('Start to combine the dropped objects from %s' % combine_drop_path)
                final_res = combine_det(final_res, combine_drop_path)
            save_path = os.path.join(root_path, '%s_final_frame.pkl' % name)
            save_pkl(final_res, save_path)
            logger.info('Frame level final result is saved at %s' % save_path)


def paired_iou3d_device(boxes_a, boxes_b, device=None):
    """(N,7),(N,7) float64 numpy -> (N,) float32 numpy on the device (boxes_iou3d_gpu(a, b).diag() bit for bit)."""
    import torch
    from . import iou3d_nms_utils
    dev = device if device is not None else torch.device('cuda', torch.cuda.current_device())
    a, b = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (boxes_a, boxes_b))
    return iou3d_nms_utils.boxes_iou3d_paired_gpu(a, b).cpu().numpy()


def generate_refine_boxes_iou(class_name, geo_path, pos_path, root_path, logger, paired_iou=None):
    """generate_iou_gt.py:14-59: per object the IoU of every refined box (position model's box, geometry model's size) with its
    ground-truth box -> ``<Class>_iou_train.pkl`` {seq: {object: (T,) float32}}.  One paired-IoU call per sequence."""
    if 'train' not in geo_path or 'train' not in pos_path:
        raise ValueError('Please provide the refining results for training split.')
    paired_iou = paired_iou if paired_iou is not None else paired_iou3d_device
    geo_res, pos_res = load_pkl(geo_path), load_pkl(pos_path)
    data_info = {}
    for seq in list(geo_res.keys()):
        data_info[seq] = {}
        refine, gt, lens = [], [], []
        for obj_id in geo_res[seq].keys():
            geo_pred = np.array(geo_res[seq][obj_id]['boxes_lidar']).reshape(-1, 7)
            boxes_refine = np.array(pos_res[seq][obj_id]['boxes_global']).copy()
            boxes_refine[:, 3:6] = geo_pred[:, 3:6]
            refine.append(boxes_refine[:, 0:7])
            gt.append(np.array(pos_res[seq][obj_id]['boxes_gt_global'])[:, 0:7])
            lens.append(boxes_refine.shape[0])
        if not lens:
            continue
        iou = np.asarray(paired_iou(np.concatenate(refine, axis=0), np.concatenate(gt, axis=0)))
        for obj_id, part in zip(geo_res[seq].keys(), np.split(iou, np.cumsum(lens)[:-1])):
            data_info[seq][obj_id] = part.copy()
    iou_path = os.path.join(root_path, '%s_iou_train.pkl' % class_name)
    save_pkl(data_info, iou_path)
    logger.info('The generated IoU label is saved at %s' % iou_path)


def main(argv=None):
    parser = argparse.ArgumentParser(description='arg parser')
    sub = parser.add_subparsers(dest='cmd', required=True)
    c = sub.add_parser('combine', help='daemon/combine_output.py')
    c.add_argument('--num', type=int, default=None)
    c.add_argument('--path', type=str, default=None)
    c.add_argument('--split', type=str, default='val', help='specify the target split for processing')
    c.add_argument('--combine_conf_res', action='store_true', default=False, help='combine the confidence refining results together')
    c.add_argument('--combine_drop_path', type=str, default=None, help='determine the dropped results at tracking module')
    c.add_argument('--track_save', action='store_true', default=True, help='save the combined result as original object track dict')
    c.add_argument('--frame_save', action='store_true', default=True, help='save the combined result as frame level list')
    i = sub.add_parser('iou', help='daemon/generate_iou_gt.py')
    i.add_argument('--class_name', type=str, default='Vehicle', help='class name')
    i.add_argument('--geo_path', type=str, help='file path of geometry refine result')
    i.add_argument('--pos_path', type=str, help='file path of position refine result')
    for p in (c, i):
        p.add_argument('--root_path', type=str, default=os.path.join('data', 'waymo', 'refining'), help='the refining directory')
    args = parser.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format='%(asctime)s %(levelname)5s %(message)s')
    logger = logging.getLogger('refine_combine')
    if args.cmd == 'combine':
        combine_final(root_path=args.root_path, class_names=['Vehicle', 'Pedestrian', 'Cyclist'], logger=logger, split=args.split,
                      combine_conf_res=args.combine_conf_res, combine_drop_path=args.combine_drop_path, track_save=args.track_save,
                      frame_save=args.frame_save)
    else:
        generate_refine_boxes_iou(args.class_name, args.geo_path, args.pos_path, args.root_path, logger=logger)


if __name__ == '__main__':
    main()
