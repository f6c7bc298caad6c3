"""The object-data stage between tracking and refining: mirror of ``daemon/prepare_object_data.py`` on the HIP backend.

    python -m detzero_amd.object_data --split val --track_data_path <tracking pickle> [--root_path data/waymo]

``WaymoObjectDataPrepare`` reads the tracker's pickle (``train`` / ``val``: the ``{'label', 'unlabel'}`` assign output of
track_assign.assign_track_target; ``test``: the plain track dict), turns every sequence's tracks into the frame-level form, crops each
object's points and writes ``refining/<Class>/<seq>.pkl`` - the files ``refine_dataset.DatasetTemplate.init_infos`` reads - with the
reference's keys, key order, dtypes and shapes (prepare_object_data.py:56-329).

What differs is how the points are handled.  The reference is run once per class and loads, transforms and masks every frame's points
each time, one (T, M) mask and one device round trip per frame.  Here a sequence is ONE pass for all requested classes: a frame's points
are loaded and prepared once (object_crop.prepare_frame_points, host float64 as the reference computes them), the boxes of all classes
are cropped in one object_crop.crop_sequence (two launches and one sync per frame group), and the rows are dealt out to the classes'
objects.  ``pack_sequence`` is the same crop with an object-major rank, handed to object_features as a PackedTracks without leaving the
device.  All per-frame point work goes through one ops object (object_crop.HipCropOps, the only implementation in the product).

The frame-level conversion depends on the class filter (pose and state of a frame are those of the first track OF THAT CLASS that
touches it), so it runs per class, on the host, as there.  Its quirks are kept and marked (sic).
"""
import argparse
import logging
import os
import pickle

import numpy as np

from . import object_crop
from .object_crop import HipCropOps  # noqa: F401  (the stage's ops object)

CLASS_NAMES = ['Vehicle', 'Pedestrian', 'Cyclist']
_LIST_KEYS = ('sample_idx', 'matched', 'matched_tracklet')                                   # kept as they are at frame level (:247)
_OBJ_PLAIN = ('obj_id', 'name', 'state', 'matched_tracklet', 'pts', 'sequence_name', 'gt_obj_id', 'gt_name')   # (:320-321)


def default_points_loader(root_path):
    """(seq, frame_id) -> (N,6) points of ``waymo_processed_data/segment-<seq>/<frame>.npy`` (:258-260)."""
    return lambda seq, frm_id: np.load(os.path.join(root_path, 'waymo_processed_data/segment-%s/%s.npy' % (seq, frm_id)))


def _tracks_of(seq_info, split):
    """The sequence's tracks in the reference's order: (track, ground truth or None, kind)."""
    if split in ('train', 'val'):
        for tklet in seq_info['label'].values():
            yield tklet['track'], tklet['gt'], 'label'
        for tklet in seq_info['unlabel'].values():
            yield tklet['track'], None, 'unlabel'
    elif split == 'test':
        for tk in seq_info.values():
            yield tk, None, 'test'


def frame_level(seq_info, class_name, split):
    """Step 1 (:63-238) and the array conversion of step 2 (:246-248): {frame id: record}, frames and objects in first-seen order."""
    frames = {}
    for tk, gt, kind in _tracks_of(seq_info, split):
        # (sic) a track belongs to a class if the class name occurs ANYWHERE in its per-frame names: a track named differently on one
        # frame lands in two classes' files, with all its boxes
        if class_name not in tk['name']:
            continue
        boxes, pose = tk['boxes_global'], (np.array(tk['pose']) if kind == 'unlabel' else tk['pose'])
        for idx, frm in enumerate(tk['sample_idx']):
            frm_id = str(frm).zfill(4)
            rec = frames.get(frm_id)
            if rec is None:
                # (sic) pose and state of a frame: those of the first track of this class that touches it
                rec = {'obj_id': [], 'name': [], 'boxes_global': [], 'score': [], 'hit': [], 'sample_idx': frm_id, 'pose': pose[idx],
                       'state': tk['state'], 'matched': [], 'matched_tracklet': []}
                if kind != 'test':
                    rec['gt_obj_id'], rec['gt_name'] = [], []
                rec['gt_boxes_global'] = []
                frames[frm_id] = rec
            rec['obj_id'].append(tk['obj_ids'][idx])
            rec['name'].append(tk['name'][idx])
            rec['boxes_global'].append(boxes[idx][:7])
            rec['score'].append(tk['score'][idx])
            rec['hit'].append(tk['hit'][idx])
            zero_box = np.zeros_like(boxes[idx][:7])
            if kind == 'label':
                rec['matched_tracklet'].append(True)
                hit = np.where(gt['sample_idx'] == tk['sample_idx'][idx])[0]
                if len(hit) > 0:
                    rec['gt_obj_id'].append(gt['obj_ids'][hit[0]])
                    rec['gt_name'].append(gt['name'][hit[0]])
                    rec['gt_boxes_global'].append(gt['gt_boxes_global'][hit[0]][:7])
                    rec['matched'].append(True)
                else:
                    # (sic) unmatched frames of a labelled track: the dummy id and name (the first ground-truth frame's), a zero box
                    rec['gt_obj_id'].append(gt['obj_ids'][0])
                    rec['gt_name'].append(gt['name'][0])
                    rec['gt_boxes_global'].append(zero_box)
                    rec['matched'].append(False)
            else:
                # (sic) unlabelled and test tracks count as matched on every frame, with zero ground-truth boxes
                rec['matched'].append(True)
                rec['matched_tracklet'].append(False)
                if kind == 'unlabel':
                    rec['gt_obj_id'].append(None)
                    rec['gt_name'].append(None)
                rec['gt_boxes_global'].append(zero_box)
    for rec in frames.values():
        for key in rec:
            if key not in _LIST_KEYS:
                rec[key] = np.array(rec[key])             # 'state' becomes the 0-d string array np.array makes of it (sic)
    return frames


def object_level(seq, frames):
    """Step 2 without the points (:275-308): ({object id: record with empty 'pts'}, [(object id, frame id, box of the frame)] in the
    order the reference appends the points)."""
    data_info, order = {}, []
    for frm_id, rec in frames.items():
        for idx, obj_id in enumerate(rec['obj_id']):
            obj = data_info.get(obj_id)
            if obj is None:
                # (sic) name and state: the object's name at its first frame, the FRAME's state where the object first appears
                obj = {'sequence_name': seq, 'obj_id': obj_id, 'name': rec['name'][idx], 'boxes_global': [], 'score': [], 'sample_idx': [],
                       'hit': [], 'pose': [], 'state': rec['state'], 'matched': [], 'matched_tracklet': rec['matched_tracklet'][idx],
                       'pts': [], 'gt_boxes_global': []}
                labelled = rec['matched_tracklet'][idx]
                obj['gt_obj_id'] = rec['gt_obj_id'][idx] if labelled else None
                obj['gt_name'] = rec['gt_name'][idx] if labelled else None
                data_info[obj_id] = obj
            obj['boxes_global'].append(rec['boxes_global'][idx])
            obj['score'].append(rec['score'][idx])
            obj['sample_idx'].append(frm_id)
            obj['hit'].append(rec['hit'][idx])
            obj['pose'].append(rec['pose'])
            obj['matched'].append(rec['matched'][idx])
            obj['gt_boxes_global'].append(rec['gt_boxes_global'][idx])
            order.append((obj_id, frm_id, idx))
    return data_info, order


def finish_objects(data_info):
    """:316-323: the per-frame lists of every object as arrays."""
    for obj in data_info.values():
        for key in obj:
            if key not in _OBJ_PLAIN:
                obj[key] = np.array(obj[key])
    return data_info


class SequencePlan:
    """One sequence, all requested classes: per class the frame and object records, and ONE list of crop frames - a frame's points
    prepared once per (frame, pose) and the boxes of every class that touches it back to back."""

    def __init__(self, seq, seq_info, class_names, split, points_loader):
        self.seq, self.classes = seq, {}
        self.entries, self._entry_of = [], {}                      # crop frames: {'frm_id', 'pose', 'boxes': [...], 'pts'}
        self.boxes = []                                            # (class, object id, entry, box within the entry), in append order
        for cn in class_names:
            frames = frame_level(seq_info, cn, split)
            data_info, order = object_level(seq, frames)
            self.classes[cn] = (frames, data_info)
            at = {}
            for frm_id, rec in frames.items():
                key = (frm_id, np.ascontiguousarray(rec['pose']).tobytes())
                e = self._entry_of.get(key)
                if e is None:
                    e = self._entry_of[key] = len(self.entries)
                    self.entries.append({'frm_id': frm_id, 'pose': rec['pose'], 'boxes': [], 'pts': None})
                at[frm_id] = (e, sum(b.shape[0] for b in self.entries[e]['boxes']))
                self.entries[e]['boxes'].append(rec['boxes_global'])
            for obj_id, frm_id, idx in order:
                e, first = at[frm_id]
                self.boxes.append((cn, obj_id, e, first + idx))
        for ent in self.entries:
            ent['pts'] = object_crop.prepare_frame_points(points_loader(seq, ent['frm_id']), ent['pose'])
            ent['boxes'] = np.concatenate(ent['boxes'], axis=0)
        n_box = [e['boxes'].shape[0] for e in self.entries]
        self.box_start = np.concatenate([[0], np.cumsum(n_box)]).astype(np.int64)
        self.pt_start = np.concatenate([[0], np.cumsum([e['pts'].shape[0] for e in self.entries])]).astype(np.int64)

    def crop_frames(self):
        return [(e['pts'], e['boxes']) for e in self.entries]

    def flat(self, i):
        """Frame-major index of self.boxes[i]."""
        _, _, e, k = self.boxes[i]
        return int(self.box_start[e]) + k

    def object_major_rank(self):
        """rank for crop_sequence: segment of every frame-major box = its place in self.boxes sorted by (class, object, frame) -
        first-seen order throughout, the order of object_features.PackedTracks."""
        first = {}
        for i, (cn, obj_id, _, _) in enumerate(self.boxes):
            first.setdefault((cn, obj_id), len(first))
        order = sorted(range(len(self.boxes)), key=lambda i: (first[self.boxes[i][:2]], i))
        rank = np.empty(len(self.boxes), dtype=np.int64)
        for seg, i in enumerate(order):
            rank[self.flat(i)] = seg
        return rank, [self.boxes[i][:2] for i in order]


def pack_sequence(seq, seq_info, class_names, split='test', points_loader=None, root_path=None, enlarge_scale=1.1, crop_on_bev=False,
                  crop_ops=None, device=None, budget_bytes=256 << 20):
    """A sequence's objects as (object_features.PackedTracks, [object record without points]): the crop of the prepare stage with an
    object-major rank, handed to grm_features / prm_features / crm_features without the points leaving the device (only the per-box
    counts come to the host).  Objects: class by class, first-seen order."""
    from .object_features import PackedTracks
    class_names = [class_names] if isinstance(class_names, str) else list(class_names)
    loader = points_loader if points_loader is not None else default_points_loader(root_path)
    plan = SequencePlan(seq, seq_info, class_names, split, loader)
    rank, seg_owner = plan.object_major_rank()
    crop = object_crop.crop_sequence(plan.crop_frames(), enlarge_scale, crop_on_bev, order=rank, device=device, budget_bytes=budget_bytes,
                                     crop_ops=crop_ops)
    infos = [finish_objects(plan.classes[cn][1])[obj_id] for cn, obj_id in dict.fromkeys(seg_owner)]
    packed = PackedTracks.from_crop(crop, [o['boxes_global'] for o in infos], [o['score'] for o in infos], [o['name'] for o in infos])
    return packed, infos


class WaymoObjectDataPrepare:
    """prepare_object_data.py:15-329.  ``class_name``: one class as there, or a list - then a sequence's points are loaded, prepared and
    cropped once for all of them.  ``workers`` is accepted and ignored: sequences run one after another in this process."""

    def __init__(self, class_name, root_path=None, split='train', track_data_path=None, enlarge_scale=1.1, crop_on_bev=False, workers=1,
                 logger=None, points_loader=None, crop_ops=None, device=None, budget_bytes=256 << 20, keep_index=False):
        self.class_name = class_name
        self.class_names = [class_name] if isinstance(class_name, str) else list(class_name)
        self.root_path = root_path
        self.split = split
        self.tk_data_path = track_data_path
        self.enlarge_scale = enlarge_scale
        self.crop_on_bev = crop_on_bev
        self.workers = workers
        self.logger = logger if logger is not None else logging.getLogger(__name__)
        self.points_loader = points_loader if points_loader is not None else default_points_loader(root_path)
        self.crop_ops, self.device, self.budget_bytes = crop_ops, device, budget_bytes
        self.keep_index = keep_index
        self.pts_index = {}                         # keep_index: {(class, seq): {object id: [kept rows of the frame's prepared points]}}
        self.processed_infos = {}
        self.save_paths = {cn: os.path.join(root_path, 'refining', cn) for cn in self.class_names}
        self.save_path = self.save_paths[self.class_names[0]]
        for p in self.save_paths.values():
            os.makedirs(p, exist_ok=True)

    def init_infos_from_tracking(self):
        self.logger.info('Loading generated object tracks for %s set.' % self.split)
        with open(self.tk_data_path, 'rb') as f:
            waymo_infos = pickle.load(f)
        self.logger.info('Total object sequences for Waymo dataset: %d.' % len(waymo_infos))
        self.logger.info('Start to convert object tracks into frame-level format.')
        for seq in list(waymo_infos.keys()):
            self.prepare_data_worker({seq: waymo_infos[seq]})

    def prepare_data_worker(self, seq_dict):
        seq, seq_info = list(seq_dict.items())[0]
        todo = [cn for cn in self.class_names if not os.path.exists(os.path.join(self.save_paths[cn], '%s.pkl' % seq))]
        if not todo:
            return
        plan = SequencePlan(seq, seq_info, todo, self.split, self.points_loader)
        crop = object_crop.crop_sequence(plan.crop_frames(), self.enlarge_scale, self.crop_on_bev, order='frame', device=self.device,
                                         budget_bytes=self.budget_bytes, want_index=self.keep_index, crop_ops=self.crop_ops)
        rows = crop.to_lists()
        index = crop.index_lists() if self.keep_index else None
        for i, (cn, obj_id, e, _) in enumerate(plan.boxes):
            g = plan.flat(i)
            plan.classes[cn][1][obj_id]['pts'].append(rows[g])
            if index is not None:
                self.pts_index.setdefault((cn, seq), {}).setdefault(obj_id, []).append(index[g] - plan.pt_start[e])
        for cn in todo:
            data_info = finish_objects(plan.classes[cn][1])
            with open(os.path.join(self.save_paths[cn], '%s.pkl' % seq), 'wb') as f:
                pickle.dump(data_info, f)


def check_split(split, track_data_path):
    if split not in track_data_path:
        raise ValueError('The object tracks data does not match the dataset split.')


def main(argv=None):
    parser = argparse.ArgumentParser(description='arg parser')
    parser.add_argument('--enlarge_scale', type=float, default=1.1, help='scale-up raito of object proposals')
    parser.add_argument('--crop_on_bev', type=bool, default=False, help='whether to crop object points on bird-eye view')
    parser.add_argument('--split', type=str, default='val')
    parser.add_argument('--workers', type=int, default=1, help='accepted for compatibility; sequences run in this process')
    parser.add_argument('--track_data_path', type=str, default=None, help='the generated tracking results pickle file')
    parser.add_argument('--root_path', type=str, default=os.path.join('data', 'waymo'), help='the dataset root (data/waymo of the checkout)')
    args = parser.parse_args(argv)
    check_split(args.split, args.track_data_path)
    logging.basicConfig(level=logging.INFO, format='%(asctime)s %(levelname)5s %(message)s')
    logger = logging.getLogger('object_data')
    logger.info('Start to process %s data ...' % ', '.join(CLASS_NAMES))
    WaymoObjectDataPrepare(CLASS_NAMES, root_path=args.root_path, split=args.split, track_data_path=args.track_data_path,
                           enlarge_scale=args.enlarge_scale, crop_on_bev=args.crop_on_bev, workers=args.workers,
                           logger=logger).init_infos_from_tracking()


if __name__ == '__main__':
    main()
