"""Model layer of the refining stage on the HIP backend: mirror of refining/detzero_refine/models/ (inference only).

``RefineTemplate`` (refine_template.py:18-77), ``GeometryRefineModel`` / ``PositionRefineModel`` / ``ConfidenceRefineModel``
(geometry_refine_model.py, position_refine_model.py, confidence_refine_model.py) and ``build_network`` / ``load_data_to_gpu`` /
``model_fn_decorator`` (models/__init__.py:16-48): same class names, constructor arguments ``(model_cfg, dataset)``, ``data_dict``
keys, return values and ``state_dict()`` layout (the ``global_step`` buffer, the regression module under ``reg.``).

The recall records of GRM and PRM (box-level and track-level recall of the input and the refined boxes) are where the reference
spends its time: per track two T x T ``boxes_iou3d_gpu`` matrices cut to ``.diag()`` and five or more ``.item()``
(geometry_refine_model.py:98-141, position_refine_model.py:100-133).  Here one launch of ``dz_track_recall_iou3d`` counts every
matched box of every track of the batch against the thresholds, one small integer table comes back, and everything after it is
the reference's integer / float arithmetic on the host, in the reference's types - quirks included (marked "(sic)").
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from . import ops, refine_modules
from .lib import DetZeroHipError

RECALL_SIDES = ('input', 'output')
TRACK_LEVEL_BAR = 0.7       # the literal of geometry_refine_model.py:153-155 / position_refine_model.py:145-147


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _empty_recall_dict(thresh_list, extra=None):
    """The key set both box models start from (geometry_refine_model.py:59-83, position_refine_model.py:68-92)."""
    rec = {'Box num': 0, 'Track num': 0, 'static': 0, 'dynamic': 0}
    rec.update(extra or {})
    for cur_th in thresh_list:
        for level in ('Box', 'Track'):
            for scope in ('', ' (static)', ' (dynamic)'):
                for side in RECALL_SIDES:
                    rec['%s level %s%s %s' % (level, side, scope, str(cur_th))] = 0
    return rec


def recall_record_from_counts(counts, states, mth_tk, thresh_list, recall_dict, track_bar_inclusive, who):
    """Host half of the GRM / PRM recall record: `counts` (B, 2, n_thr + 1) integers of dz_track_recall_iou3d ([b][side][0] =
    matched boxes of track b, [b][side][1 + k] = those with IoU > thresh_list[k]) -> the reference's counters, added to
    `recall_dict`.  geometry_refine_model.py:98-176 / position_refine_model.py:100-167 from `obj_len` on."""
    counts = np.asarray(counts)
    states, mth_tk = np.array(states), np.array(mth_tk)
    if recall_dict.__len__() == 0:
        recall_dict = _empty_recall_dict(thresh_list)
    tk_frac = ([], [])
    box_hits = np.zeros((2, len(thresh_list)), dtype=np.int64)
    cur_gt_num = 0
    for idx in range(len(mth_tk)):
        if mth_tk[idx] == False:      # noqa: E712  false positive tracks are removed for statistics
            continue
        obj_len = int(counts[idx, 0, 0])
        if obj_len == 0:
            # the reference divides by zero here (tk_input_num / obj_len)
            raise DetZeroHipError('%s: matched track %d of the batch has no matched box' % (who, idx))
        cur_gt_num += obj_len
        for s in range(2):
            # (sic) the track's fraction is taken at thresh_list[0] whatever the list holds, as Python int / int
            tk_frac[s].append(int(counts[idx, s, 1]) / obj_len)
        recall_dict['%s' % states[idx]] += obj_len
        for k, cur_th in enumerate(thresh_list):
            for s, side in enumerate(RECALL_SIDES):
                recall_dict['Box level %s (%s) %s' % (side, states[idx], str(cur_th))] += int(counts[idx, s, 1 + k])
                box_hits[s, k] += int(counts[idx, s, 1 + k])
    # (sic) the fractions go through torch.Tensor(list): float32 from here on
    all_tk = [torch.Tensor(tk_frac[0]), torch.Tensor(tk_frac[1])]
    for i, state in enumerate(states[mth_tk.astype(bool)]):
        for cur_th in thresh_list:
            for s, side in enumerate(RECALL_SIDES):
                # (sic) per state the bar is the literal 0.7, counted once per entry of the list; `>` in GRM, `>=` in PRM
                hit = all_tk[s][i] >= TRACK_LEVEL_BAR if track_bar_inclusive else all_tk[s][i] > TRACK_LEVEL_BAR
                recall_dict['Track level %s (%s) %s' % (side, state, str(cur_th))] += int(hit)
    for k, cur_th in enumerate(thresh_list):
        for s, side in enumerate(RECALL_SIDES):
            recall_dict['Box level %s %s' % (side, str(cur_th))] += int(box_hits[s, k])
            # the overall track counters compare with the threshold itself
            recall_dict['Track level %s %s' % (side, str(cur_th))] += int((all_tk[s] > cur_th).sum().item())
    recall_dict['Box num'] += cur_gt_num
    recall_dict['Track num'] += int(np.where(mth_tk == True)[0].shape[0])      # noqa: E712
    return recall_dict


def _match_mask(matched, mth_tk, lengths, t_cap):
    """(B, t_cap) uint8: 1 = box of a matched track that is itself matched - the rows the reference's loops look at."""
    mask = np.zeros((len(lengths), t_cap), dtype=np.uint8)
    for idx, n in enumerate(lengths):
        if mth_tk[idx] == False:      # noqa: E712
            continue
        m = np.asarray(matched[idx]).astype(bool)
        if m.shape[0] != n:
            raise DetZeroHipError('recall record: track %d has %d boxes and %d `matched` flags' % (idx, n, m.shape[0]))
        mask[idx, :n] = m
    return mask


def _device_recall_counts(boxes_in, boxes_out, boxes_gt, mask, lengths, thresh_list):
    """One launch, one device-to-host copy: the (B, 2, n_thr + 1) table as numpy."""
    dev = boxes_in.device
    d_mask = torch.from_numpy(mask).to(dev)
    d_len = torch.from_numpy(np.asarray(lengths, dtype=np.int32)).to(dev)
    counts, _, _ = ops.track_recall_iou3d_nosync(boxes_in, boxes_out, boxes_gt, d_mask, d_len, list(thresh_list), want_iou=False)
    return counts.cpu().numpy()


class RefineTemplate(nn.Module):
    """refine_template.py:18-77."""

    def __init__(self, model_cfg, dataset):
        super().__init__()
        self.model_cfg = model_cfg
        self.dataset = dataset
        self.tta = self.dataset.tta
        self.register_buffer('global_step', torch.LongTensor(1).zero_())
        self.build_networks()

    @property
    def mode(self):
        return 'TRAIN' if self.training else 'TEST'

    def update_global_step(self):
        self.global_step += 1

    def build_networks(self):
        model_info_dict = {
            'module_list': [],
            'query_point_dims': self.model_cfg.get('QUERY_POINT_DIMS', 0),
            'memory_point_dims': self.model_cfg.get('MEMORY_POINT_DIMS', 0),
        }
        name = self.model_cfg.REGRESSION['NAME']
        if name not in refine_modules.__all__:
            raise DetZeroHipError('RefineTemplate: REGRESSION.NAME %r (have %s)' % (name, sorted(refine_modules.__all__)))
        reg = refine_modules.__all__[name](model_cfg=self.model_cfg.REGRESSION,
                                           query_point_dims=model_info_dict['query_point_dims'],
                                           memory_point_dims=model_info_dict['memory_point_dims'])
        self.add_module('reg', reg)
        return model_info_dict

    def forward(self, data_dict):
        if self.training:
            raise DetZeroHipError('%s: training is out of scope of the HIP backend; call .eval()' % type(self).__name__)
        data_dict = self.reg(data_dict)
        pred_dicts, recall_dict = self.post_processing(data_dict)
        return pred_dicts, recall_dict, {}

    def _refuse_tta(self):
        if self.tta:
            raise DetZeroHipError("%s: dataset.tta is set, but the reference's own test_time_augment is `raise NotImplementedError` "
                                  '(geometry_refine_model.py:41-43, position_refine_model.py:46-48)' % type(self).__name__)


class GeometryRefineModel(RefineTemplate):
    """geometry_refine_model.py:10-178."""

    def post_processing(self, data_dict):
        post_process_cfg = self.model_cfg.POST_PROCESSING
        recall_dict = {}
        batch_box_preds = data_dict['batch_box_preds']
        self._refuse_tta()
        if post_process_cfg.get('GENERATE_RECALL', True):
            recall_dict = self.generate_recall_record(box_preds=batch_box_preds, recall_dict=recall_dict, data_dict=data_dict,
                                                      thresh_list=post_process_cfg.RECALL_THRESH_LIST)
        pred_dicts = {
            'pred_boxes': batch_box_preds.detach().cpu().numpy(),
            'pose': data_dict['pose'],
            'geo_trajectory': data_dict['geo_trajectory'],
        }
        return pred_dicts, recall_dict

    def generate_recall_record(self, box_preds, recall_dict, data_dict=None, thresh_list=None):
        if 'gt_geo_trajectory' not in data_dict:
            return recall_dict
        if self.model_cfg.POST_PROCESSING.get('CENTER_ALIGN', False):
            # no config sets it, and the reference's branch indexes per_gt_traj[idx] with the BATCH index (:110-112)
            raise DetZeroHipError('GeometryRefineModel: POST_PROCESSING.CENTER_ALIGN is not supported')
        traj, gt_traj = data_dict['geo_trajectory'], data_dict['gt_geo_trajectory']
        mth_tk = np.array(data_dict['matched_tracklet'])
        if recall_dict.__len__() == 0:
            recall_dict = _empty_recall_dict(thresh_list)
        # (sic) trailing all-zero rows of gt_geo_query_boxes are trimmed (never the first), and an empty rest or an empty
        # prediction skips the batch (:85-92)
        cur_gt = data_dict['gt_geo_query_boxes']
        k = cur_gt.__len__() - 1
        while k > 0 and cur_gt[k].sum() == 0:
            k -= 1
        if cur_gt[:k + 1].shape[0] == 0 or box_preds.shape[0] == 0:
            return recall_dict
        return recall_record_from_counts(self._recall_counts(box_preds, traj, gt_traj, data_dict['matched'], mth_tk, thresh_list),
                                         data_dict['state'], mth_tk, thresh_list, recall_dict, False, 'GeometryRefineModel')

    @staticmethod
    def _recall_counts(box_preds, traj, gt_traj, matched, mth_tk, thresh_list):
        """The lists of (L,7) global-frame arrays, cast to float32 as the reference's `.float()` does (:115-116), padded into
        ONE (2, B, Tmax, 7) block and uploaded in one copy; the output boxes are the input boxes with the object's predicted
        size in columns 3:6 (:105-108)."""
        lengths = [len(t) for t in traj]
        b, t_cap = len(traj), max(max(lengths, default=0), 1)
        block = np.zeros((2, b, t_cap, 7), dtype=np.float32)
        for idx, n in enumerate(lengths):
            if len(gt_traj[idx]) != n:
                raise DetZeroHipError('GeometryRefineModel: track %d has %d boxes and %d ground-truth boxes' % (idx, n, len(gt_traj[idx])))
            block[0, idx, :n] = np.asarray(traj[idx])[:, 0:7]
            block[1, idx, :n] = np.asarray(gt_traj[idx])[:, 0:7]
        d_block = torch.from_numpy(block).to(box_preds.device)
        boxes_in, boxes_gt = d_block[0], d_block[1]
        boxes_out = boxes_in.clone()
        boxes_out[:, :, 3:6] = box_preds[:, None, 3:6].float()
        return _device_recall_counts(boxes_in, boxes_out, boxes_gt, _match_mask(matched, mth_tk, lengths, t_cap), lengths, thresh_list)


class PositionRefineModel(RefineTemplate):
    """position_refine_model.py:13-169."""

    def post_processing(self, data_dict):
        post_process_cfg = self.model_cfg.POST_PROCESSING
        recall_dict = {}
        batch_box_preds = data_dict['batch_box_preds'].clone()
        self._refuse_tta()
        if post_process_cfg.get('GENERATE_RECALL', True):
            recall_dict = self.generate_recall_record(box_preds=batch_box_preds, recall_dict=recall_dict, data_dict=data_dict,
                                                      thresh_list=post_process_cfg.RECALL_THRESH_LIST)
        pred_dicts = {
            'pred_boxes': batch_box_preds.detach().cpu().numpy(),
            'pose': data_dict['pose'],
            'pos_init_box': _np(data_dict['pos_init_box']),
        }
        if 'gt_pos_trajectory' in data_dict:      # (the reference needs the key, :41; inference on unlabelled tracks has none)
            pred_dicts['gt_pos_trajectory'] = _np(data_dict['gt_pos_trajectory'])
        return pred_dicts, recall_dict

    @staticmethod
    def generate_recall_record(box_preds, recall_dict, data_dict=None, thresh_list=None):
        if 'gt_pos_trajectory' not in data_dict:
            return recall_dict
        # pos_trajectory, gt_pos_trajectory and box_preds (B, query_num, 7) are taken as they are, on the device
        traj, gt_traj = data_dict['pos_trajectory'], data_dict['gt_pos_trajectory']
        if not (torch.is_tensor(traj) and torch.is_tensor(gt_traj) and traj.is_cuda and gt_traj.is_cuda):
            raise DetZeroHipError('PositionRefineModel: pos_trajectory / gt_pos_trajectory must be device tensors (load_data_to_gpu)')
        box_num = [int(n) for n in data_dict['box_num']]
        mth_tk = np.array(data_dict['matched_tracklet'])
        t_cap = traj.shape[1]
        if max(box_num, default=0) > t_cap:
            raise DetZeroHipError('PositionRefineModel: a track of %d boxes in trajectories of %d rows' % (max(box_num), t_cap))
        counts = _device_recall_counts(traj[..., 0:7].float().contiguous(), box_preds[..., 0:7].float().contiguous(),
                                       gt_traj[..., 0:7].float().contiguous(), _match_mask(data_dict['matched'], mth_tk, box_num, t_cap),
                                       box_num, thresh_list)
        return recall_record_from_counts(counts, data_dict['state'], mth_tk, thresh_list, recall_dict, True, 'PositionRefineModel')


class ConfidenceRefineModel(RefineTemplate):
    """confidence_refine_model.py:12-108."""

    def post_processing(self, data_dict):
        post_process_cfg = self.model_cfg.POST_PROCESSING
        recall_dict = {}
        self._refuse_tta()
        if post_process_cfg.get('GENERATE_RECALL', True):
            recall_dict = self.generate_recall_record(box_preds=None, recall_dict=recall_dict, data_dict=data_dict,
                                                      thresh_list=post_process_cfg.RECALL_THRESH_LIST)
        return {'pred_score': data_dict['pred_score'].cpu().numpy()}, recall_dict

    @staticmethod
    def generate_recall_record(box_preds, recall_dict, data_dict=None, thresh_list=None):
        """A few values per box: host numpy like the reference (:36-108), the three tensors fetched once per batch instead of
        once per track.  The counters are Python ints (the reference's turn into numpy integers on the first `+=`)."""
        if 'iou' not in data_dict:
            return recall_dict
        bs, box_num = data_dict['batch_size'], data_dict['box_num']
        mth_tk = np.array(data_dict['matched_tracklet'])
        if recall_dict.__len__() == 0:
            recall_dict = _empty_recall_dict(thresh_list, extra={'matched_up': 0, 'matched_down': 0, 'unmatched_up': 0, 'unmatched_down': 0,
                                                                 'gt_score': [], 'pred_score': [], 'ori_score': []})
        conf, pred, iou = _np(data_dict['conf_score']), _np(data_dict['pred_score']), _np(data_dict['iou'])
        for i in range(bs):
            num = int(box_num[i])
            ori_score, pred_score, gt_score = conf[i][:num], pred[i][:num], iou[i][:num]
            gt_label = gt_score >= 0.7
            recall_dict['ori_score'].extend(ori_score)
            recall_dict['pred_score'].extend(pred_score)
            recall_dict['gt_score'].extend(gt_label)
            matched_up = int((gt_label & (pred_score >= ori_score)).sum())
            matched_down = int((gt_label & (pred_score < ori_score)).sum())
            unmatched_up = int(((gt_score < 0.7) & (pred_score >= ori_score)).sum())
            recall_dict['matched_up'] += matched_up
            recall_dict['matched_down'] += matched_down
            recall_dict['unmatched_up'] += unmatched_up
            recall_dict['unmatched_down'] += num - matched_up - matched_down - unmatched_up
            recall_dict['Box num'] += num
        recall_dict['Track num'] += int(np.where(mth_tk == True)[0].shape[0])      # noqa: E712
        return recall_dict


__all__ = {
    'GeometryRefineModel': GeometryRefineModel,
    'PositionRefineModel': PositionRefineModel,
    'ConfidenceRefineModel': ConfidenceRefineModel,
}


def build_network(model_cfg, dataset):
    """models/__init__.py:16-20."""
    if model_cfg.NAME not in __all__:
        raise DetZeroHipError('build_network: MODEL.NAME %r (have %s)' % (model_cfg.NAME, sorted(__all__)))
    return __all__[model_cfg.NAME](model_cfg=model_cfg, dataset=dataset)


def load_data_to_gpu(batch_dict):
    """models/__init__.py:23-30: every ndarray but the bookkeeping ones -> float32 device tensor; device tensors (what the
    loader of this backend produces) pass through untouched."""
    for key, val in batch_dict.items():
        if not isinstance(val, np.ndarray):
            continue
        if key in ['frame_id', 'sequence_name', 'poses']:
            continue
        batch_dict[key] = torch.from_numpy(val).float().cuda()


def model_fn_decorator():
    """models/__init__.py:33-48 - the training step wrapper; training is out of scope of the HIP backend."""
    ModelReturn = namedtuple('ModelReturn', ['loss', 'tb_dict', 'disp_dict'])      # noqa: F841  (name kept)

    def model_func(model, batch_dict):
        raise DetZeroHipError('model_fn_decorator: training is out of scope of the HIP backend')
    return model_func
