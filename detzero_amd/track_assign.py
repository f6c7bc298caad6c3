"""Ground-truth assignment of a sequence's tracks (assign mode: every split but 'test') on one trajectory-pair kernel.

Mirror of the reference's
  * ``tracking/detzero_track/models/tracking_modules/target_assign.py:8-139``   assign_track_target
  * ``tracking/detzero_track/utils/track_calculation.py:9-81``                   get_iou_mat_dict, get_gt_id_data
same names, same arguments, same return value ``{'label': {track id: {'track', 'gt'}}, 'unlabel': {track id: {'track'}}}``, the same
mutation of the track dicts (``iou`` added, ``state`` overwritten) and the same quirks, marked "(sic)".

What is where.  The reference builds one IoU matrix per frame, copies each to the host and walks frame x ground-truth box x
track in Python.  Both it and TrackRecall.eval_single_seq (track_recall.py) want the same four numbers per (ground-truth
trajectory, track) pair over the frames the two share, so here a sequence is two row tables - the ground-truth boxes left after
the class mask and the tracks' boxes, each with a (frame ordinal, trajectory) slot table - and ONE launch of dz_traj_pair_table
gives ``n_hit`` (= traj_count_mat), ``sum_hit`` (= traj_similar_mat before the division), ``sum_all`` and ``n_same``; a second
launch, dz_traj_pair_rows, gives the per-frame IoUs of the matched pairs.  The sums are sequential fp32 sums in frame order as
the reference's ``+=`` on a float32 matrix.  The Hungarian assignment, ``pos_diff`` and ``state`` stay host numpy.

All device arithmetic goes through one ops object (``HipTrajOps`` is the only implementation in the product); the tests drive
the same orchestration with a numpy restatement of its three methods.
"""
from collections import defaultdict

import numpy as np

from . import ops, track_adapter
from .lib import DetZeroHipError

METRIC_OF = {'bev': ops.TRACK_AFF_IOU_BEV, '3d': ops.BOXM_IOU3D}
MAX_CLASSES = ops.TRACK_MAX_CLASSES


# ------------------------------------------------------------------------------------------------
# ops: the pair arithmetic of one sequence
# ------------------------------------------------------------------------------------------------
class HipTrajOps:
    """The three ops on csrc/traj_pair.hip.

    Interface (what a stand-in for tests implements):
      set_sides(a_box, a_cls, a_slot, b_box, b_cls, b_slot)    host arrays: *_box (rows,7) f32, *_cls (rows,) i32,
                                                               *_slot (n_frames, n) i32 frame-major, -1 = no box at that frame
      table(metric, distinguish_class, thr) -> (sum_all, sum_hit) f32, (n_hit, n_same) i32, each (n_a, n_b), host
      rows(metric, distinguish_class, pairs) -> (len(pairs), n_frames) f32 host; pairs (P,2) [a trajectory, b trajectory]
    """

    def __init__(self, device=None):
        import torch
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.sides = None

    def _dev(self, a, dtype):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.device)

    def set_sides(self, a_box, a_cls, a_slot, b_box, b_cls, b_slot):
        self.sides = (self._dev(a_box, np.float32), self._dev(a_cls, np.int32), self._dev(a_slot, np.int32),
                      self._dev(b_box, np.float32), self._dev(b_cls, np.int32), self._dev(b_slot, np.int32))

    def table(self, metric, distinguish_class, thr):
        out = ops.traj_pair_table(*self.sides, metric, distinguish_class, thr)
        return tuple(t.cpu().numpy() for t in out)

    def rows(self, metric, distinguish_class, pairs):
        pairs = self._dev(np.asarray(pairs).reshape(-1, 2), np.int32)
        return ops.traj_pair_rows(*self.sides, metric, distinguish_class, pairs).cpu().numpy()


# ------------------------------------------------------------------------------------------------
# track_calculation.py
# ------------------------------------------------------------------------------------------------
def class_mask(names, class_names):
    mask = np.zeros(len(names), dtype=bool)
    for class_n in class_names:
        mask = mask | (names == class_n)
    return mask


def pair_iou(boxes_a, boxes_b, iou='bev'):
    """(N,7), (M,7) host boxes -> (N,M) float32 host IoU matrix on the box ops ('bev': dz_boxes_iou_bev, '3d': DZ_BOXM_IOU3D)."""
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    a = torch.from_numpy(np.ascontiguousarray(boxes_a[:, :7], dtype=np.float32)).to(dev)
    b = torch.from_numpy(np.ascontiguousarray(boxes_b[:, :7], dtype=np.float32)).to(dev)
    out = ops.boxes_pairwise(a, b, True) if iou == 'bev' else ops.boxes_pairwise_metric(a, b, ops.BOXM_IOU3D)
    return out.cpu().numpy()


def get_iou_mat_dict(gt_data, pred_data, class_names, distinguish_class=True, iou='bev', iou_fn=None):
    """One IoU matrix per ground-truth frame, (ground-truth boxes left after the class mask, the frame's tracks)
    (track_calculation.py:9-52).  Kept for users of the shim; assign_track_target and TrackRecall do not call it."""
    if iou not in METRIC_OF:
        raise DetZeroHipError('get_iou_mat_dict: iou %r (bev or 3d)' % (iou,))
    iou_fn = iou_fn if iou_fn is not None else pair_iou
    out = {}
    for sample_idx in list(gt_data.keys()):
        track_len = len(pred_data[sample_idx]['boxes_lidar']) if sample_idx in pred_data.keys() else 0
        annos = gt_data[sample_idx]['annos']
        name_len = len(annos['name'])
        if name_len == 0 or track_len == 0:
            mat = np.zeros((name_len, track_len), dtype=np.float32)       # (sic) every row, not only the masked ones
        else:
            mask = class_mask(annos['name'], class_names)
            mat = iou_fn(annos['gt_boxes_lidar'][mask, :][:, :7], pred_data[sample_idx]['boxes_lidar'][:, :7], iou)
            if distinguish_class:
                track_name = pred_data[sample_idx]['name']
                for gt_idx, gt_n in enumerate(annos['name'][mask]):
                    mat[gt_idx, track_name != gt_n] = 0.
        out[sample_idx] = mat
    return out


def get_gt_id_data(gt_data, gt_keys, class_names):
    """Ground truth by frame -> by object id, in the order in which the ids first appear: lists per key of ``gt_keys`` plus
    ``sample_idx`` (str) and ``iou_idx`` = the object's row among the frame's rows left after the class mask (:55-81)."""
    out = {}
    for sample_idx, item in gt_data.items():
        annos = item['annos']
        if len(annos['name']) == 0:
            continue
        mask = class_mask(annos['name'], class_names)
        kept = {key: annos[key][mask] for key in gt_keys}
        for idx, obj_id in enumerate(annos['obj_ids'][mask]):
            if obj_id not in out:
                out[obj_id] = defaultdict(list)
            for key in gt_keys:
                out[obj_id][key].append(kept[key][idx])
            out[obj_id]['sample_idx'].append(str(sample_idx))
            out[obj_id]['iou_idx'].append(idx)
    return out


# ------------------------------------------------------------------------------------------------
# a sequence as two row tables
# ------------------------------------------------------------------------------------------------
def _codes(names, class_names, strict, what):
    """Class codes of ``names``: the index in ``class_names``.  Another name raises when ``strict``, else it gets a code past the
    table, which equals no ground-truth class (both consumers mask on class)."""
    table = {n: i for i, n in enumerate(class_names)}
    out = np.zeros(len(names), dtype=np.int32)
    for k, n in enumerate(names):
        if n not in table:
            if strict:
                raise DetZeroHipError('%s: class %s is not in %s' % (what, n, list(class_names)))
            table[n] = len(table)
        out[k] = table[n]
    return out


def trajectory_sides(frame_keys, gt_data, track_frames, class_names, gt_ids, tk_ids, strict_names, what):
    """-> (a_box, a_cls, a_slot, b_box, b_cls, b_slot) for ``ops.set_sides``: frame ordinal f = position in ``frame_keys``; side a =
    the ground-truth boxes left after the class mask (gt_boxes_lidar, fp32 as the reference's ``.float()``), side b = the tracks'
    boxes_lidar of ``track_frames`` (tracklets_to_frames by sample_idx).  An object id twice in one frame is refused: the
    reference would count its first box twice."""
    if len(class_names) > MAX_CLASSES:
        raise DetZeroHipError('%s: %d classes (at most %d)' % (what, len(class_names), MAX_CLASSES))
    gt_col = {g: i for i, g in enumerate(gt_ids)}
    tk_col = {t: i for i, t in enumerate(tk_ids)}
    n_frames = len(frame_keys)
    a_slot = np.full((n_frames, len(gt_ids)), -1, dtype=np.int32)
    b_slot = np.full((n_frames, len(tk_ids)), -1, dtype=np.int32)
    a_box, a_cls, b_box, b_cls = [], [], [], []
    a_rows = b_rows = 0
    for f, key in enumerate(frame_keys):
        annos = gt_data[key]['annos']
        if len(annos['name']):
            mask = class_mask(annos['name'], class_names)
            ids = annos['obj_ids'][mask]
            cols = np.array([gt_col[g] for g in ids], dtype=int)
            if len(set(cols.tolist())) != len(cols):
                raise DetZeroHipError('%s: frame %s holds a ground-truth object id twice' % (what, key))
            a_slot[f, cols] = a_rows + np.arange(len(cols))
            a_box.append(np.asarray(annos['gt_boxes_lidar'][mask, :][:, :7], dtype=np.float32))
            a_cls.append(_codes(annos['name'][mask], class_names, True, what))
            a_rows += len(cols)
        frame = track_frames.get(key)
        if frame is not None and len(frame['obj_ids']):
            cols = np.array([tk_col[t] for t in frame['obj_ids']], dtype=int)
            b_slot[f, cols] = b_rows + np.arange(len(cols))
            b_box.append(np.asarray(frame['boxes_lidar'][:, :7], dtype=np.float32))
            b_cls.append(_codes(frame['name'], class_names, strict_names, what))
            b_rows += len(cols)

    def cat(parts, width, dtype):
        return np.concatenate(parts, axis=0) if parts else np.zeros((0, width) if width else (0,), dtype=dtype)
    return cat(a_box, 7, np.float32), cat(a_cls, 0, np.int32), a_slot, cat(b_box, 7, np.float32), cat(b_cls, 0, np.int32), b_slot


# ------------------------------------------------------------------------------------------------
# target_assign.py
# ------------------------------------------------------------------------------------------------
def assign_track_target(input_data, iou_thresholds, ops=None):
    """``input_data`` = (processed detection frames, the tracker's ``{track id: track}``, ground-truth frames
    ``{sample_idx: info}``); ``iou_thresholds`` = ``{class name: BEV IoU a frame must reach to count}``, whose keys are the classes.
    Tracks are matched to ground-truth trajectories one to one (Hungarian, on 1 - the mean over the ground truth's frames of the
    counted IoUs); a matched track gets ``iou`` (per frame, 0 where the two share none) and ``state`` from the ground truth's motion,
    and goes to ``label`` with the ground-truth trajectory as arrays; an unmatched one goes to ``unlabel``.  Frame ordinals follow
    the key order of the ground-truth dict.  A track class outside ``iou_thresholds`` raises DetZeroHipError."""
    from .track_models import GNN_assignment
    det_data, tk_data, list_gt_data = input_data[0], input_data[1], input_data[2]
    class_names = list(iou_thresholds.keys())
    ops = ops if ops is not None else HipTrajOps()

    track_frames = track_adapter.frame_list_to_dict(track_adapter.tracklets_to_frames({'reference': det_data, 'source': tk_data}))
    gt_keys = ['gt_boxes_global', 'gt_boxes_lidar', 'name', 'obj_ids']
    gt_data = get_gt_id_data(list_gt_data, gt_keys, class_names)
    gt_ids, tk_ids = list(gt_data.keys()), list(tk_data.keys())
    frame_keys = list(list_gt_data.keys())

    ops.set_sides(*trajectory_sides(frame_keys, list_gt_data, track_frames, class_names, gt_ids, tk_ids, True, 'assign_track_target'))
    thr = [float(iou_thresholds[n]) for n in class_names]
    if gt_ids and tk_ids:
        _, sum_hit, n_hit, _ = ops.table(METRIC_OF['bev'], True, thr)
    else:
        sum_hit, n_hit = np.zeros((len(gt_ids), len(tk_ids)), np.float32), np.zeros((len(gt_ids), len(tk_ids)), np.int32)

    gt_len = np.array([len(gt_data[g]['sample_idx']) for g in gt_ids], dtype=np.float32).reshape(-1, 1)
    traj_similar_mat = (np.asarray(sum_hit, dtype=np.float32) / gt_len).astype(np.float32)
    traj_similar_mat[np.asarray(n_hit) <= 0] = -1.
    match, _, unmatch_track = GNN_assignment(1 - traj_similar_mat)

    ordinal = {str(k): f for f, k in enumerate(frame_keys)}
    iou_rows = ops.rows(METRIC_OF['bev'], True, match) if len(match) else np.zeros((0, len(frame_keys)), np.float32)
    label_data, unlabel_data = {}, {}
    for k in range(len(match)):
        gt_id, tk_id = gt_ids[match[k, 0]], tk_ids[match[k, 1]]
        tk, gt = tk_data[tk_id], gt_data[gt_id]
        tk['iou'] = np.zeros(len(tk['sample_idx']), np.float32)
        seen = set()
        for at, sample_idx in enumerate(tk['sample_idx']):
            f = ordinal.get(str(sample_idx))
            if f is not None and sample_idx not in seen:          # list.index: the first row of a repeated sample_idx
                tk['iou'][at] = iou_rows[k, f]
                seen.add(sample_idx)
        gt.pop('iou_idx')
        for key in gt.keys():
            gt[key] = np.array(gt[key])
        pos_diff = np.linalg.norm(gt['gt_boxes_global'][0, :2] - gt['gt_boxes_global'][-1, :2], ord=2, axis=0)
        speed = np.linalg.norm(gt['gt_boxes_global'][:, 7:9], ord=2, axis=1)
        # (sic) ``speed.any() > 1`` compares a bool with 1 and is never true: only the displacement makes a track dynamic
        tk['state'] = 'dynamic' if (speed.any() > 1 or pos_diff > 1) else 'static'
        label_data[tk_id] = {'track': tk, 'gt': gt}
    for j in unmatch_track:
        unlabel_data[tk_ids[j]] = {'track': tk_data[tk_ids[j]]}
    return {'label': label_data, 'unlabel': unlabel_data}
