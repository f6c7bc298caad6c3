"""Data layer of the refining stage in test mode: mirror of refining/detzero_refine/datasets/ on the HIP backend.

``DatasetTemplate`` (datasets/dataset.py:16-163, the test-mode half): reads ``ImageSets/<split>.txt`` and the per-class
``refining/<Class>/<seq>.pkl`` track files, applies the ``matched_tracklet`` / ``save_to_file`` filter of ``load_infos_worker``
and keeps ``track_infos``.  The files are read in this process (no process pool).  Where the reference's ``__getitem__`` +
``collate_batch`` build one object's features in numpy and stack them (waymo_*_dataset.py ``extract_track_feature``,
dataset.py:207-265), ``RefineLoader`` takes ``batch_size`` tracks at a time and calls ``object_features.{grm,prm,crm}_features``
on them ONCE, on the device (the fixed-size point selections are drawn from Python's `random` in the reference's order, so a
run seeded like the reference keeps the same points); the bookkeeping and ground-truth keys are added on the host exactly as the reference returns
and collates them.  ``generate_prediction_dicts`` forwards to ``refine_results``.
"""
import os
import pickle
import random

import numpy as np

from . import object_features, refine_results
from .lib import DetZeroHipError

CLASS_MAP = {'Vehicle': 1, 'Pedestrian': 2, 'Cyclist': 3, 1: 'Vehicle', 2: 'Pedestrian', 3: 'Cyclist'}


def rotate_yaw(yaw):
    """data_utils.py:6-9 (float32, as the reference builds it)."""
    return np.array([[np.cos(yaw), np.sin(yaw), 0], [-np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]], dtype=np.float32)


def limit_heading_range(angle):
    """data_utils.py:33-42: into [-pi, pi), in place."""
    while (angle >= np.pi).sum() > 0:
        angle[angle >= np.pi] -= 2 * np.pi
    while (angle < -np.pi).sum() > 0:
        angle[angle < -np.pi] += 2 * np.pi
    return angle


def gt_to_init_box_frame(traj_all, traj_gt_all):
    """The ground-truth half of init_coords_transform (data_utils.py:72-106) for a test-mode track: the frame is the track's
    middle box (waymo_position_dataset.py:75-76), heading limited first.  Returns a (T,7) float64 copy."""
    init_box = np.array(traj_all[len(traj_all) // 2, 0:7], dtype=np.float64, copy=True)
    init_box[6] = limit_heading_range(init_box[[6]])[0]
    gt = np.array(traj_gt_all[:, :7], dtype=np.float64, copy=True)
    gt[:, 6] = limit_heading_range(gt[:, 6])
    gt[:, :3] -= init_box[:3]
    gt[:, :3] = gt[:, :3] @ rotate_yaw(init_box[6]).T
    gt[:, 6] -= init_box[6]
    gt[:, 6] = limit_heading_range(gt[:, 6])
    return gt


class DatasetTemplate:
    """datasets/dataset.py:16-163 for training=False."""
    default_query_num = 200

    def __init__(self, dataset_cfg=None, class_names=None, training=True, root_path=None, logger=None):
        if training:
            raise DetZeroHipError('%s: the training path is out of scope of the HIP backend' % type(self).__name__)
        self.dataset_cfg = dataset_cfg
        self.class_names = class_names
        self.training = False
        self.root_path = root_path if root_path is not None else self.dataset_cfg.DATA_PATH
        self.logger = logger
        self.split = self.dataset_cfg.DATA_SPLIT[self.mode]
        with open(os.path.join(str(self.root_path), 'ImageSets', self.split + '.txt')) as f:
            self.sample_sequence_list = [x.strip() for x in f.readlines()]
        self.augment_single = self.augment_full = False
        self.tta = dataset_cfg.get('TTA', False)
        self.encoding = self.dataset_cfg.get('ENCODING', ['placeholder'])
        self.iou = None
        self.class_map = dict(CLASS_MAP)
        self.box_num = 0
        self.track_infos = []
        self.query_num = self.dataset_cfg.get('QUERY_NUM', self.default_query_num)
        self.query_pts_num = self.dataset_cfg.get('QUERY_POINTS_NUM', 256)
        self.init_infos()

    @property
    def mode(self):
        return 'train' if self.training else 'test'

    def _log(self, msg):
        if self.logger is not None:
            self.logger.info(msg)

    def init_infos(self):
        """dataset.py:47-143: the sequences of the split that have a file, class by class, then object by object."""
        seq_files = []
        for cls_name in self.class_names:
            data_path = os.path.join(str(self.root_path), 'refining', cls_name)
            file_names = os.listdir(data_path)
            for seq in self.sample_sequence_list:
                # (sic) str.strip with character sets, as the reference spells it (dataset.py:76)
                seq = seq.strip('segment-').strip('_with_camera_labels.tfrecord') + '.pkl'
                if seq in file_names:
                    seq_files.append(os.path.join(data_path, seq))
        self._log('Total Sequences: %d' % len(seq_files))
        data_infos = {}
        for path in seq_files:
            data_infos.update(self.load_infos_worker(path))
        for val in data_infos.values():
            self.box_num += len(val['boxes_global'])
            self.track_infos.append(val)
        self._log('Total Object Tracks for Waymo dataset: %d' % len(self.track_infos))
        self._log('Total Boxes for Waymo dataset: %d' % self.box_num)

    def load_infos_worker(self, seq_name):
        """dataset.py:97-124: false-positive tracks are kept only when results are written to file."""
        data_infos = {}
        with open(seq_name, 'rb') as f:
            seq_infos = pickle.load(f)
        for obj_id in list(seq_infos.keys()):
            obj_info = seq_infos[obj_id]
            if not obj_info.get('matched_tracklet', True) and not self.dataset_cfg.get('save_to_file', False):
                continue
            assert len(obj_info['boxes_global']) == len(obj_info['gt_boxes_global'])
            obj_info['refine_iou'] = np.zeros(len(obj_info['sample_idx']))
            data_infos[obj_info['sequence_name'] + '/' + str(obj_id)] = obj_info
        return data_infos

    def __len__(self):
        return len(self.track_infos)

    def _common(self, infos, frame_key='sample_idx'):
        return {'sequence_name': [d['sequence_name'] for d in infos], 'frame': [d[frame_key] for d in infos],
                'obj_id': [d['obj_id'] for d in infos]}

    def collate_tracks(self, infos):
        raise NotImplementedError


class WaymoGeometryDataset(DatasetTemplate):
    """waymo_geometry_dataset.py:16-155 (test mode) + generate_prediction_dicts."""
    default_query_num = 3

    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, logger=None):
        self.memory_pts_num = dataset_cfg.get('MEMORY_POINTS_NUM', 4096)
        super().__init__(dataset_cfg, class_names, training, root_path, logger)

    def collate_tracks(self, infos):
        """One device pass for the batch's model inputs; the keys extract_track_feature returns next to them (:135-152) as
        collate_batch keeps them: lists per object, `obj_cls` stacked, `gt_geo_query_boxes` padded to the batch's largest
        query count.  Every track gets QUERY_NUM queries or its length (the reference's dataset object lowers its own
        query_num for good at the first shorter track, :73-74 - not mirrored)."""
        batch = object_features.grm_features(infos, encoding=tuple(self.encoding), query_num=self.query_num,
                                             query_pts_num=self.query_pts_num, memory_pts_num=self.memory_pts_num, rng=random)
        q_max = max(batch['geo_query_num'])
        gt_q = np.zeros((len(infos), q_max, np.asarray(infos[0]['gt_boxes_global']).shape[1]))
        for i, d in enumerate(infos):
            query_idx = np.argsort(d['score'])[::-1][:self.query_num]
            gt_box = np.array([d['gt_boxes_global'][ind, :].copy() for ind in query_idx])
            gt_box[:, [0, 1, 2, 6]] = 0
            gt_q[i, :len(query_idx)] = gt_box
        batch.update(self._common(infos))
        batch.update({
            'obj_cls': np.stack([self.class_map[d['name']] for d in infos], axis=0),
            'geo_trajectory': [d['boxes_global'] for d in infos], 'geo_score': [d['score'] for d in infos],
            'gt_geo_query_boxes': gt_q, 'gt_geo_trajectory': [d['gt_boxes_global'] for d in infos],
            'pose': [d['pose'] for d in infos], 'state': [d['state'] for d in infos], 'matched': [d['matched'] for d in infos],
            'matched_tracklet': [d['matched_tracklet'] for d in infos],
        })
        return batch

    def generate_prediction_dicts(self, batch_dict, pred_dicts, single_pred_dict, output_path=None):
        return refine_results.grm_prediction_dicts(batch_dict, pred_dicts['pred_boxes'], single_pred_dict)


class WaymoPositionDataset(DatasetTemplate):
    """waymo_position_dataset.py:20-184 (test mode) + generate_prediction_dicts."""
    default_query_num = 200

    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, logger=None):
        self.memory_pts_num = dataset_cfg.get('MEMORY_POINTS_NUM', 48)
        super().__init__(dataset_cfg, class_names, training, root_path, logger)

    def collate_tracks(self, infos):
        batch = object_features.prm_features(infos, encoding=tuple(self.encoding), query_num=self.query_num,
                                             query_pts_num=self.query_pts_num, memory_pts_num=self.memory_pts_num, rng=random)
        # the ground-truth trajectory goes through the same init_coords_transform as the trajectory (:79-80), padded with
        # zero rows (:159-160) and stacked
        gt = np.zeros((len(infos), self.query_num, 7))
        for i, d in enumerate(infos):
            gt[i, :len(d['boxes_global'])] = gt_to_init_box_frame(np.asarray(d['boxes_global']), np.asarray(d['gt_boxes_global']))
        batch.update(self._common(infos))
        batch.update({
            'obj_cls': np.stack(batch['obj_cls'], axis=0), 'gt_pos_trajectory': gt, 'pos_scores': [d['score'] for d in infos],
            'pose': [d['pose'] for d in infos], 'state': [d['state'] for d in infos], 'matched': [d['matched'] for d in infos],
            'matched_tracklet': [d['matched_tracklet'] for d in infos],
        })
        return batch

    def generate_prediction_dicts(self, batch_dict, pred_dicts, single_pred_dict, output_path=None):
        return refine_results.prm_prediction_dicts(batch_dict, pred_dicts['pred_boxes'], single_pred_dict)


class WaymoConfidenceDataset(DatasetTemplate):
    """waymo_confidence_dataset.py:16-162 (test mode) + generate_prediction_dicts."""
    default_query_num = 200

    def collate_tracks(self, infos):
        batch = object_features.crm_features(infos, encoding=tuple(self.encoding), query_num=self.query_num,
                                             query_pts_num=self.query_pts_num, rng=random)
        iou = np.full((len(infos), self.query_num), -1.0)          # refine_iou (zeros outside training, dataset.py:122), padded with -1 (:147)
        for i, d in enumerate(infos):
            iou[i, :len(d['refine_iou'])] = d['refine_iou']
        batch.update(self._common(infos))
        batch.update({'state': [d['state'] for d in infos], 'matched_tracklet': [d['matched_tracklet'] for d in infos], 'iou': iou})
        return batch

    def generate_prediction_dicts(self, batch_dict, pred_dicts, single_pred_dict, output_path=None):
        return refine_results.crm_prediction_dicts(batch_dict, pred_dicts['pred_score'], single_pred_dict)


class RefineLoader:
    """What build_dataloader returns in place of a torch DataLoader: a plain iterable over batches of `batch_size` tracks in
    dataset order (shuffle is off in test mode, drop_last=False), with `.dataset` and `__len__`."""

    def __init__(self, dataset, batch_size, length=0):
        if batch_size < 1:
            raise DetZeroHipError('RefineLoader: batch_size %d' % batch_size)
        self.dataset, self.batch_size = dataset, int(batch_size)
        self.count = min(len(dataset), length) if length > 0 else len(dataset)

    def __len__(self):
        return (self.count + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for start in range(0, self.count, self.batch_size):
            yield self.dataset.collate_tracks(self.dataset.track_infos[start:min(start + self.batch_size, self.count)])


__all__ = {
    'DatasetTemplate': DatasetTemplate,
    'WaymoGeometryDataset': WaymoGeometryDataset,
    'WaymoPositionDataset': WaymoPositionDataset,
    'WaymoConfidenceDataset': WaymoConfidenceDataset,
}


def build_dataloader(dataset_cfg, class_names, batch_size, dist, root_path=None, workers=4, logger=None, training=True,
                     merge_all_iters_to_one_epoch=False, total_epochs=0, length=0):
    """datasets/__init__.py:43-79 for training=False, dist=False.  The features are built on the device, which forked
    DataLoader workers cannot own: the loader runs in-process (`workers` is accepted and ignored).  Returns
    (dataset, loader, None)."""
    if training:
        raise DetZeroHipError('build_dataloader: the training path is out of scope of the HIP backend')
    if dist:
        raise DetZeroHipError('build_dataloader: distributed refining is out of scope of the HIP backend')
    if merge_all_iters_to_one_epoch:
        raise DetZeroHipError('build_dataloader: merge_all_iters_to_one_epoch belongs to the training path')
    if dataset_cfg.DATASET not in __all__ or dataset_cfg.DATASET == 'DatasetTemplate':
        raise DetZeroHipError('build_dataloader: DATASET %r' % (dataset_cfg.DATASET,))
    dataset = __all__[dataset_cfg.DATASET](dataset_cfg=dataset_cfg, class_names=class_names, root_path=root_path,
                                          training=training, logger=logger)
    return dataset, RefineLoader(dataset, batch_size, length), None
