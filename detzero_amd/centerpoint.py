"""CenterPoint detector (plugin surface of the reference) and the sync-free per-frame pipeline.

``CenterPoint`` mirrors /root/reference/detection/detzero_det/models/centerpoint.py:15-129,210-352 and
``build_network`` / ``load_data_to_gpu`` mirror detzero_det/models/__init__.py:13-29, so
detection/tools/test.py's ``eval_one_epoch`` drives it unchanged: ``model(batch_dict)`` returns
``(pred_dicts, recall_dict)`` in eval mode.

``FramePipeline`` is the same computation arranged for throughput: points already resident in HBM ->
voxelize -> VFE -> sparse backbone -> BEV -> head -> decode -> NMS, every size-dependent quantity kept
in device counters, so one frame is ~110 kernel launches with no host synchronisation; results are
padded (500, 9) boxes + a count, which is also the payload of the RCCL gather.
"""
import contextlib
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import det_modules as cp_modules
from . import iou3d_nms_utils, ops, range_audit as _range_audit
from .lib import DetZeroHipError
from .range_audit import RangeAudit


class CenterPoint(nn.Module):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.dataset = dataset
        self.tta = getattr(self.dataset, 'tta', False)       # TTA: True in the dataset config -> copies, restore, weighted box fusion
        self.class_names = dataset.class_names
        self.register_buffer('global_step', torch.LongTensor(1).zero_())
        self.second_stage = model_cfg.SECOND_STAGE
        self.module_list = self.build_networks()

    def build_networks(self):
        """centerpoint.py:59-129."""
        info = {
            'num_point_features': self.dataset.point_feature_encoder.num_point_features,
            'grid_size': self.dataset.grid_size,
            'point_cloud_range': self.dataset.point_cloud_range,
            'voxel_size': self.dataset.voxel_size,
        }
        vfe = cp_modules.__all__[self.model_cfg.VFE.NAME](
            model_cfg=self.model_cfg.VFE, num_point_features=info['num_point_features'],
            point_cloud_range=info['point_cloud_range'], voxel_size=info['voxel_size'], grid_size=info['grid_size'])
        info['num_point_features'] = vfe.get_output_feature_dim()
        backbone3d = cp_modules.__all__[self.model_cfg.BACKBONE_3D.NAME](
            model_cfg=self.model_cfg.BACKBONE_3D, input_channels=info['num_point_features'],
            grid_size=info['grid_size'], voxel_size=info['voxel_size'], point_cloud_range=info['point_cloud_range'])
        map_to_bev = cp_modules.__all__[self.model_cfg.MAP_TO_BEV.NAME](
            model_cfg=self.model_cfg.MAP_TO_BEV, grid_size=info['grid_size'])
        backbone2d = cp_modules.__all__[self.model_cfg.BACKBONE_2D.NAME](
            model_cfg=self.model_cfg.BACKBONE_2D, input_channels=map_to_bev.num_bev_features)
        dense_head = cp_modules.__all__[self.model_cfg.DENSE_HEAD.NAME](
            model_cfg=self.model_cfg.DENSE_HEAD, input_channels=backbone2d.num_bev_features,
            num_class=self.num_class if not self.model_cfg.DENSE_HEAD.CLASS_AGNOSTIC else 1,
            class_names=self.class_names, grid_size=info['grid_size'], voxel_size=info['voxel_size'],
            point_cloud_range=info['point_cloud_range'], tta=self.tta, predict_boxes_when_training=self.second_stage)
        self.add_module('vfe', vfe)
        self.add_module('backbone3d', backbone3d)
        self.add_module('map_to_bev', map_to_bev)
        self.add_module('backbone2d', backbone2d)
        self.add_module('dense_head', dense_head)
        module_list = [vfe, backbone3d, map_to_bev, backbone2d, dense_head]
        if self.second_stage:                                # centerpoint.py:115-127
            from .pdv_modules import PDVHead
            roi_heads = {'PDVHead': PDVHead}
            roi_head = roi_heads[self.model_cfg.ROI_HEAD.NAME](
                model_cfg=self.model_cfg.ROI_HEAD, input_channels=backbone2d.num_bev_features,
                num_class=self.num_class if not self.model_cfg.ROI_HEAD.CLASS_AGNOSTIC else 1,
                grid_size=info['grid_size'], voxel_size=info['voxel_size'], point_cloud_range=info['point_cloud_range'])
            self.add_module('roi_head', roi_head)
            module_list.append(roi_head)
        return module_list

    @property
    def mode(self):
        return 'TRAIN' if self.training else 'TEST'

    def update_global_step(self):
        self.global_step += 1

    def forward(self, batch_dict):
        if self.training:
            raise DetZeroHipError('CenterPoint: training is out of scope of the HIP backend; call .eval()')
        for cur_module in self.module_list:
            batch_dict = cur_module(batch_dict)
        return self.post_processing(batch_dict)

    def get_training_loss(self):
        """centerpoint.py:41-50, first stage: (loss, tb_dict, disp_dict) of the dense head after a forward on a batch with
        ``gt_boxes`` (inference mode: a validation loss, or the gradient at the head maps).  The PDV head's losses are not built."""
        if self.second_stage or self.model_cfg.get('ROI_HEAD', None) is not None:
            raise DetZeroHipError('CenterPoint.get_training_loss: the PDV head\'s losses (ROI_HEAD) are not built; only the '
                                  'first-stage CenterHead loss is provided')
        loss, tb_dict = self.dense_head.get_loss()
        return loss, tb_dict, {}

    def head_loss_backward(self, batch_dict):
        """Head fine-tuning with everything in front of the head frozen: the stages run as in ``forward`` up to the dense head, which then
        runs ``CenterHead.loss_backward`` on the batch's ``gt_boxes`` - the gradient of the first-stage loss accumulates in the
        ``.grad`` of ``dense_head``'s parameters.  -> (loss, tb_dict, disp_dict) as ``get_training_loss``.  The model stays in eval
        mode; after an optimiser step call ``dense_head.invalidate()``."""
        if self.training:
            raise DetZeroHipError('CenterPoint: training is out of scope of the HIP backend; call .eval()')
        if self.second_stage or self.model_cfg.get('ROI_HEAD', None) is not None:
            raise DetZeroHipError('CenterPoint.head_loss_backward: the PDV head\'s losses (ROI_HEAD) are not built; only the '
                                  'first-stage CenterHead loss is provided')
        for cur_module in self.module_list:
            if cur_module is self.dense_head:
                break
            batch_dict = cur_module(batch_dict)
        loss, tb_dict = self.dense_head.loss_backward(batch_dict)
        return loss, tb_dict, {}

    def post_processing(self, batch_dict):
        """centerpoint.py:283-307 (one-stage branch; with TTA the copies' boxes are restored and fused, :298-306)."""
        post_process_cfg = self.model_cfg.POST_PROCESSING
        recall_dict = {}
        if self.second_stage:                                # centerpoint.py:214-281 (the single-class-NMS branch of the PDV configs)
            if post_process_cfg.get('NMS_CONFIG', {}).get('MULTI_CLASSES_NMS', False):
                # the reference's own branch cannot run either: it reads `cls_preds` before assigning it (centerpoint.py:221-222,
                # UnboundLocalError on the first frame); no DetZero config sets the flag
                raise DetZeroHipError('post_processing: MULTI_CLASSES_NMS is not provided (the reference branch, centerpoint.py:221-245, '
                                      'fails on an unassigned `cls_preds`; no DetZero config sets the flag)')
            pred_dicts = []
            for index in range(batch_dict['batch_size']):
                box_preds = batch_dict['batch_box_preds'][index]
                cls_preds = batch_dict['batch_cls_preds'][index]                 # the predicted IoU
                label_preds = batch_dict['roi_labels'][index]
                scores = torch.sqrt(torch.sigmoid(cls_preds).reshape(-1) * batch_dict['roi_scores'][index].reshape(-1))
                mask = (label_preds != 0).reshape(-1)
                final_boxes, final_scores, final_labels = box_preds[mask, :], scores[mask], label_preds[mask]
                recall_dict = self.generate_recall_record(
                    box_preds=final_boxes if 'rois' not in batch_dict else box_preds, recall_dict=recall_dict,
                    batch_index=0 if self.tta else index, data_dict=batch_dict, thresh_list=post_process_cfg.RECALL_THRESH_LIST)
                pred_dicts.append({'pred_boxes': final_boxes, 'pred_scores': final_scores, 'pred_labels': final_labels})
        else:
            pred_dicts = batch_dict['final_box_dicts']
            for index in range(batch_dict['batch_size']):
                recall_dict = self.generate_recall_record(
                    box_preds=pred_dicts[index]['pred_boxes'], recall_dict=recall_dict, batch_index=0 if self.tta else index,
                    data_dict=batch_dict, thresh_list=post_process_cfg.RECALL_THRESH_LIST)
        if self.tta:
            boxes, scores, labels = self.test_time_augment(batch_dict, pred_dicts)
            pred_dicts = [{'pred_boxes': boxes, 'pred_scores': scores, 'pred_labels': labels}]
        return pred_dicts, recall_dict

    @staticmethod
    def test_time_augment(data_dict, pred_dicts):
        """centerpoint.py:131-208: the copies' boxes padded into one (frames, copies, rows, dim) tensor, restored to the original
        coordinates in place (dz_tta_restore_boxes) and fused (dz_wbf_fuse_3d).  Like the reference (its ``boxes.squeeze(0)``)
        this handles ONE frame per batch; ``data_dict['batch_size']`` becomes the number of frames."""
        from . import tta
        tta_ops = list(data_dict['tta_ops'])
        tta_num = len(tta_ops)
        bs = int(data_dict['batch_size'] // tta_num)
        if bs != 1:
            raise DetZeroHipError('TTA: one frame per batch (the reference squeezes the frame axis, centerpoint.py:205)')
        max_num = max(max(len(x['pred_boxes']) for x in pred_dicts), 1)
        ref = pred_dicts[0]['pred_boxes']
        dim = ref.shape[-1]
        boxes = torch.zeros((data_dict['batch_size'], max_num, dim), dtype=torch.float32, device=ref.device)
        scores = torch.zeros((data_dict['batch_size'], max_num, 1), dtype=torch.float32, device=ref.device)
        labels = torch.zeros((data_dict['batch_size'], max_num, 1), dtype=pred_dicts[0]['pred_labels'].dtype, device=ref.device)
        for i, pred in enumerate(pred_dicts):
            n = len(pred['pred_boxes'])
            boxes[i, :n] = pred['pred_boxes']
            scores[i, :n, 0] = pred['pred_scores']
            labels[i, :n, 0] = pred['pred_labels']
        boxes = tta.restore_boxes(boxes.reshape(bs, tta_num, max_num, dim), tta_ops)
        data_dict['batch_size'] = bs
        return tta.wbf_online(boxes[0], scores, labels)

    @staticmethod
    def generate_recall_record(box_preds, recall_dict, batch_index, data_dict=None, thresh_list=None):
        """centerpoint.py:310-352."""
        if 'gt_boxes' not in data_dict:
            return recall_dict
        rois = data_dict['rois'][batch_index] if 'rois' in data_dict else None          # second-stage runs: recall of the proposals too
        gt_boxes = data_dict['gt_boxes'][batch_index]
        if len(recall_dict) == 0:
            recall_dict = {'gt': 0}
            for t in thresh_list:
                recall_dict['roi_%s' % str(t)] = 0
                recall_dict['rcnn_%s' % str(t)] = 0
        cur_gt = gt_boxes
        k = len(cur_gt) - 1
        while k > 0 and cur_gt[k].sum() == 0:
            k -= 1
        cur_gt = cur_gt[:k + 1]
        if cur_gt.shape[0] > 0:
            if box_preds.shape[0] > 0:
                iou3d = iou3d_nms_utils.boxes_iou3d_gpu(box_preds[:, 0:7].contiguous(), cur_gt[:, 0:7].contiguous())
            else:
                iou3d = torch.zeros((0, cur_gt.shape[0]))
            iou3d_roi = None
            if rois is not None and rois.shape[0] > 0:
                iou3d_roi = iou3d_nms_utils.boxes_iou3d_gpu(rois[:, 0:7].contiguous(), cur_gt[:, 0:7].contiguous())
            for t in thresh_list:
                if iou3d.shape[0] > 0:
                    recall_dict['rcnn_%s' % str(t)] += (iou3d.max(dim=0)[0] > t).sum().item()
                if iou3d_roi is not None:
                    recall_dict['roi_%s' % str(t)] += (iou3d_roi.max(dim=0)[0] > t).sum().item()
            recall_dict['gt'] += cur_gt.shape[0]
        return recall_dict


__all__ = {'CenterPoint': CenterPoint}


def build_network(model_cfg, num_class, dataset):
    return __all__[model_cfg.NAME](model_cfg=model_cfg, num_class=num_class, dataset=dataset)


def load_data_to_gpu(batch_dict):
    """models/__init__.py:21-29 (every ndarray -> float32 device tensor)."""
    for key, val in batch_dict.items():
        if key in ['frame_id', 'metadata', 'sequence_name', 'pose', 'tta_ops', 'aug_matrix_inv']:
            continue
        elif isinstance(val, np.ndarray):
            batch_dict[key] = torch.from_numpy(val).float().cuda()


class SyntheticDatasetInfo:
    """The attributes build_networks reads from a DatasetTemplate (dataset.py:22-53)."""

    class _PFE:
        def __init__(self, n):
            self.num_point_features = n

    def __init__(self, cfg, num_point_features=5):
        dcfg = cfg.DATA_CONFIG
        self.class_names = list(cfg.CLASS_NAMES)
        self.point_cloud_range = np.array(dcfg.POINT_CLOUD_RANGE, dtype=np.float32)
        vox = [p for p in dcfg.DATA_PROCESSOR if p.NAME.startswith('transform_points_to_voxels')][0]
        self.voxel_size = list(vox.VOXEL_SIZE)
        self.max_points_per_voxel = vox.get('MAX_POINTS_PER_VOXEL', 5)
        self.max_voxels = vox.get('MAX_NUMBER_OF_VOXELS', {'test': 200000})
        self.grid_size = ops.grid_size_of(self.point_cloud_range, self.voxel_size)
        self.point_feature_encoder = self._PFE(num_point_features)
        self.tta = False


def set_math(model, mode):
    """Select the arithmetic of every convolution of the detector: 'f32' (fp32 MFMA, bit-for-bit an fmaf chain),
    'f16x2' / 'bf16x2' (split-precision pairs on the 16-bit matrix cores, csrc/hgemm.h).  All conv modules of a
    model run in the same mode (activations stay in the mode's storage format between layers)."""
    mid = ops.math_id(mode)
    for mod in model.modules():
        if hasattr(mod, 'set_math') and mod is not model:
            mod.set_math(mid)
    return model


def set_sparse_engine(model, engine, f32_engine=None, f32_gather=None, f32_small=None):
    """Convolution engine of the sparse backbone in the split math modes: 'xrun' (default: the gather kernels plus sparse_conv_x.hip
    for the submanifold convolutions of the 32 / 64 / 128-channel levels), 'gather' (sparse_conv_h.hip / sparse_conv_w.h only; both
    on rows in the canonical linear-key order) or 'tiles' (sparse_conv_t.hip: tile-resident inputs on rows in the brick order).
    f32_engine: the engine of the exact-fp32 mode, 'gather' (default: sparse_conv.hip) or 'xrun' (plus sparse_conv_xf.hip for the same
    submanifold convolutions, from the same index) or 'xrun_bf16x3' (the index of 'xrun'; those convolutions on the bf16 matrix pipe with
    three exact limbs per operand, sparse_conv_xt.hip, at the widths it covers and on sparse_conv_xf.hip at the others); None leaves it
    as it is.
    f32_gather: the arithmetic of the exact-fp32 convolutions that stay on the gather path whatever f32_engine says (conv_input, conv1,
    the strided layers, submanifold layers without x-run windows): 'mfma32' (default: sparse_conv.hip) or 'bf16x3' (three exact bf16
    limbs per operand, sparse_conv_gt.hip, for the layers it covers); None leaves it as it is.
    f32_small: the kernel of the exact-fp32 mode's 16-input-channel layers (conv_input, conv1, conv2's stride-2 layer): 'gather' (default:
    what f32_gather gives them) or 'wave_bf16x3' (wave-private tiles with resident limb weights, sparse_conv_wt.hip, for the layers it
    covers, whatever f32_gather says); None leaves it as it is.  A refused call changes nothing."""
    model.backbone3d.set_engine(engine, f32_engine, f32_gather, f32_small)
    return model


def set_dense_engine(model, f32_engine, f32_generic=None):
    """Engine of the 3 x 3 stride-1 dense layers (BEV backbone, the head's shared and hidden convolutions) in the exact-fp32 mode:
    'mfma32' (default: k_conv2d on the fp32 matrix cores) or 'bf16x3' (csrc/conv3x3_t.hip: every operand as three exact bf16 limbs,
    six bf16 MFMAs per product - fp32-class results in another accumulation order).
    f32_generic (None = unchanged): the engine of the dense layers that kernel does not run - the strided 3 x 3 layer, the deblocks, the
    head's grouped output layer, and with f32_engine 'mfma32' every other dense layer too: 'mfma32' (default) or 'bf16x3'
    (csrc/conv2d_t.hip, the generic implicit GEMM in the same three-limb arithmetic).  The head-at-candidates kernel stays where it is;
    the split math modes ignore both switches.  A refused value changes nothing."""
    if f32_engine not in ops.DENSE_F32_ENGINES:
        raise DetZeroHipError('unknown fp32 dense engine %r (%s)' % (f32_engine, ' | '.join(ops.DENSE_F32_ENGINES)))
    if f32_generic is not None and f32_generic not in ops.DENSE_F32_GENERIC_ENGINES:
        raise DetZeroHipError('unknown generic fp32 dense engine %r (%s)' % (f32_generic, ' | '.join(ops.DENSE_F32_GENERIC_ENGINES)))
    for name in ('backbone2d', 'dense_head'):
        mod = getattr(model, name, None)
        if mod is not None and hasattr(mod, 'set_dense_engine'):
            mod.set_dense_engine(f32_engine, f32_generic)
    return model


def set_linear_engine(model, f32_engine):
    """Engine of the linear layers of a detector's second stage (the PDV head's MLP / FC stacks, attention projections and feed-forward
    block) in the exact-fp32 mode: 'mfma32' (default: dz_linear_forward on the fp32 matrix cores) or 'bf16x3' (csrc/linear_t.hip, the
    three-limb arithmetic of set_dense_engine) for the layers that engine covers.  Set on every module of the model that runs linears;
    the split math modes ignore it.  A refused value changes nothing."""
    if f32_engine not in ops.LINEAR_F32_ENGINES:
        raise DetZeroHipError('unknown fp32 linear engine %r (%s)' % (f32_engine, ' | '.join(ops.LINEAR_F32_ENGINES)))
    for mod in model.modules():
        if hasattr(mod, 'set_linear_engine') and hasattr(mod, 'stack_math'):
            mod.set_linear_engine(f32_engine)
    return model


# development switch: DZ_TUNE_EAGER_PYRAMID=1 builds the whole index pyramid before the first convolution (the r01c-r03f schedule)
STAGGERED_PYRAMID = not os.environ.get('DZ_TUNE_EAGER_PYRAMID')

F16_PAIR_TARGET_PEAK = 2.0 ** 11    # where select_math places a stage's largest |activation|: 32x of headroom under fp16's 65504 for frames
# that run hotter than the calibration samples, and 14 binades (down to 2^-3) in which the lo half of the pair is a NORMAL fp16, i.e.
# the pair carries its full 22 bits; below that the absolute quantum 2^-25 applies (1.5e-11 of the peak)
PRESCALE_STAGES = ('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4', 'encoded', 'spatial_features_2d')


def set_prescale(model, exps):
    """Install (or clear, exps=None) the per-stage power-of-two pre-scale of the fp16-pair tensors on the detector's three convolution
    modules: exps = {stage: e} for PRESCALE_STAGES - a stage's tensors are stored as value * 2^e, the factors folded exactly into the
    layers' folded-BN scale / shift (det_modules._Cached._p).  Has no effect in 'f32' and 'bf16x2' math (their exponent range is fp32's)."""
    for name in ('backbone3d', 'backbone2d', 'dense_head'):
        mod = getattr(model, name, None)
        if mod is not None and hasattr(mod, 'set_prescale'):
            mod.set_prescale(exps)
    return model


def prescale_exponents(peaks, target=F16_PAIR_TARGET_PEAK):
    """{stage: floor(log2(target / peak))} from per-stage activation peaks; a stage without active rows (peak 0) gets 0."""
    out = {}
    for k in PRESCALE_STAGES:
        v = float(peaks.get(k, 0.0))
        out[k] = int(max(-100, min(100, math.floor(math.log2(target / v))))) if v > 0.0 and math.isfinite(v) else 0
    return out


@torch.no_grad()
def range_audit(model, dataset_info, frames, math=None, dynamic=False):
    """One FramePipeline pass over `frames` (sparse backbone, BEV backbone, the head's dense stage, decode) under a RangeAudit ->
    its report: one dict per STORED tensor (range_audit.RangeAudit.report).  math: the mode to run in (None = the model's current
    one); with 'f32' the peaks are the calibration measurement of every tensor.  One host sync."""
    audit = RangeAudit()
    pipe = FramePipeline(model, dataset_info, math=math, dynamic=dynamic, audit=audit)
    pipe(list(frames))
    return audit.report()


def group_peaks(report):
    """{stage: largest peak over the tensors of the stage's exponent group} of a range_audit report (fp32 outputs have no group)."""
    out = {k: 0.0 for k in PRESCALE_STAGES}
    for r in report:
        if r['stage'] in out:
            out[r['stage']] = max(out[r['stage']], float(r['peak']))
    return out


@torch.no_grad()
def activation_range(model, dataset_info, frames, dynamic=False, probe='stages'):
    """Largest |activation| per stage of the detector on sample frames, measured on the exact-fp32 engine.  probe='stages': the outputs
    of the five sparse stages and the concatenated 2-D feature map.  probe='all': per stage the maximum over EVERY stored tensor that
    shares the stage's exponent (hidden tensors of the residual blocks, every layer of the BEV blocks, the head's shared and hidden
    maps - a `range_audit` pass).  Leaves the model in 'f32' math."""
    if probe == 'all':
        return group_peaks(range_audit(model, dataset_info, frames, math='f32', dynamic=dynamic))
    if probe != 'stages':
        raise DetZeroHipError("activation_range: probe is 'stages' or 'all' (got %r)" % (probe,))
    pipe = FramePipeline(model, dataset_info, math='f32', dynamic=dynamic)
    frames = list(frames)
    out = {}
    res = pipe.backbone_stage(pipe.prepare(frames))
    for name, (feats, lvl) in res.items():
        out[name] = float(feats[:max(lvl.num_active(), 1)].abs().max().item())
    x, lvl = res['encoded']
    bev = ops.sparse_to_bev(x, lvl, x.shape[1], pad=1, math=0)
    out['spatial_features_2d'] = float(model.backbone2d.run(bev, len(frames)).abs().max().item())
    return out


def select_math(model, dataset_info, frames, prefer='f16x2', dynamic=False, target=F16_PAIR_TARGET_PEAK, probe='stages', verify=False):
    """Fit the split-precision arithmetic to a checkpoint from a calibration pass on the exact-fp32 engine: the per-stage activation
    peaks give per-stage power-of-two exponents (`prescale_exponents`) that put every stage's tensors where fp16 pairs carry 22 bits,
    whatever the checkpoint's own scale is - activations of 1e6 (fp16 saturates at 65504) as well as of 1e-4 (the lo half of an
    unscaled pair would be subnormal).  The factors are exact (powers of two folded into scale / shift), so the result is that of
    the same network at O(1000) activations.  Rounds 2-5 fell back to bf16 pairs (16 bits) outside [2^-6, 3e4]; round 6 measured
    bf16 pairs at up to 5e-3 on data-dependent boxes - outside the north star's 1e-3 - so they are an opt-in mode only.
    probe='all' takes each stage's peak over every stored tensor of its exponent group instead of over the stage outputs alone
    (`activation_range`): a checkpoint whose hidden activations run hotter than its stage outputs then gets smaller exponents.
    verify=True runs one audited pass in the chosen mode on the calibration frames afterwards and raises DetZeroHipError naming the
    first tensor that saturated or went non-finite.
    Returns (mode, per-stage maxima); sets the mode and the pre-scale (model.prescale = the exponents)."""
    frames = list(frames)
    rng = activation_range(model, dataset_info, frames, dynamic, probe=probe)
    exps = prescale_exponents(rng, target)
    set_prescale(model, exps if ops.storage_math(ops.math_id(prefer)) == 1 else None)
    model.prescale = exps
    set_math(model, prefer)
    if verify:
        bad = _range_audit.first_violation(range_audit(model, dataset_info, frames, math=prefer, dynamic=dynamic))
        if bad is not None:
            raise DetZeroHipError("select_math: %r math with the %r exponents %s does not hold this checkpoint's activations - %s"
                                  % (prefer, probe, exps, _range_audit.describe(bad)))
    return prefer, rng


PAD_RAGGED = os.environ.get('DZ_TUNE_PAD_RAGGED', '1') != '0'      # development switch: 0 = ragged lists through one fused voxelizer chain per frame (r01-r05)
GROUPED_DEEP_BLOCKS = os.environ.get('DZ_TUNE_GROUPED_DEEP', '1') != '0'       # development switch: 0 = every dense layer per frame group (r04)


class _StackedFrames(list):
    """List view of a (B,N,C) tensor of equally long frames that remembers the backing tensor (no re-concatenation)."""

    def __init__(self, tensor):
        super().__init__(tensor.unbind(0))
        self.tensor = tensor


class FramePipeline:
    """Sync-free detector step on one GPU over a batch of frames (reference eval batches frames the same way:
    tools/test.py builds the loader with OPTIMIZATION.BATCH_SIZE_PER_GPU, collate_batch stacks the voxels with
    a batch-index column).

    ``__call__(points)``: points = one (N,C) float32 device tensor or a list of B such tensors (already
    range-masked or not - the xy mask of data_processor.py:24-37 is applied on the device).
    Returns (boxes9, count): for a single tensor (K,9) and (1,) i32; for a list (B,K,9) and (B,) i32.  Rows
    [0,count) are ``[x,y,z,dx,dy,dz,heading,score,label(1-based)]`` after NMS.
    """

    def __init__(self, model, dataset_info, mode='test', dynamic=False, math=None, ways=None, audit=None):
        self.model = model.eval()
        # audit: a RangeAudit - every pass of this pipeline then probes the tensors it stores into it (`check_range`); None = no probe
        self.audit = audit
        if math is not None:
            set_math(model, math)
        # ways: a batch is split into this many sub-passes that run CONCURRENTLY on their own streams (`_call_split`): every launch of
        # the persistent kernels leaves CUs idle while it ramps up and while its last tiles finish (busy CUs 0.84-0.96,
        # profiles/r06a_clock_table.txt) - an independent second pass fills them: +1.0 % frames/s at 32 frames per batch, +3.0 % at 16,
        # +-0 at 8 (batches under `split_min` frames are not split); three or four ways, or two ways of 32 frames, give nothing
        # (profiles/r06_ab_notes.txt).  None = DZ_TUNE_WAYS or 2
        self.ways = int(os.environ.get('DZ_TUNE_WAYS', '2')) if ways is None else int(ways)
        self.split_min = int(os.environ.get('DZ_TUNE_SPLIT_MIN', '12'))     # smallest batch that is split (8 frames: +-0, sometimes a loss)
        self._subs = None
        self._way_streams = None
        self.side_key = 0
        self.fork_ok = True           # False while this pipeline is a branch of somebody's graph capture: no forks of its own
        self.info = dataset_info
        self.mode = mode
        self.dynamic = dynamic
        self.head = model.dense_head
        if len(self.head.class_names_each_head) != 1:
            raise DetZeroHipError('FramePipeline: the batched route packs ONE head\'s detections (the layout of every DetZero config); a '
                                  'multi-head CenterHead runs through the module API (CenterPoint.forward)')
        post = self.head.model_cfg.POST_PROCESSING
        self.k = post.MAX_OBJ_PER_SAMPLE
        self.post_max = post.NMS_CONFIG.NMS_POST_MAXSIZE
        self._streams = {}
        self.level_caps = None        # per-frame row capacities of the strided stages (None = worst case)
        self._ws = {}                 # zero-bordered activation images of the dense stage, reused across steps
        self.dense_group = int(os.environ.get('DZ_TUNE_DENSE_GROUP', '16'))     # frames per pass of the dense layers (2 GiB image window)
        self.last_overflow = None
        self._overflow_acc = None
        # True: the head's regression branches (center, center_z, dim, rot) are evaluated at the top-K cells only (post_stage), the
        # dense stage runs the iou / hm branches alone; False: the full-map route (all six branches at every cell)
        self.head_at_candidates = True
        self._partial_head = None     # (address, shape, shared map) of the partial head map the last dense_stage returned

    def _voxelize(self, frames, cid=0):
        """-> (features (M,C), coords (M,4) [b,z,y,x], d_n or None).  Rows of a frame beyond its device-side
        voxel count carry b = -1 and are ignored by the index build (no host sync, capacity-sized)."""
        info = self.info
        rng = info.point_cloud_range
        nb = len(frames)
        if self.dynamic:
            pb = torch.cat([torch.cat([p.new_full((p.shape[0], 1), float(i)), p], dim=1) for i, p in enumerate(frames)], dim=0)
            return ops.voxelize_dynamic_nosync(pb.contiguous(), rng, info.voxel_size, nb, xy_range_mask=True)
        dev = frames[0].device
        main = torch.cuda.current_stream(dev)
        cap = int(min(info.max_voxels[self.mode], max(max(p.shape[0] for p in frames), 1)))
        c = frames[0].shape[1]
        if nb > 1 and all(p.shape[0] == frames[0].shape[0] for p in frames):
            # equally long frames: ONE launch chain voxelizes the whole batch (the frame index extends the voxel key)
            if isinstance(frames, _StackedFrames):
                pts = frames.tensor.reshape(-1, c)
            else:
                pts = torch.cat(list(frames), dim=0)
            feats, coords, _ = ops.voxelize_hard_mean_batched(pts, nb, rng, info.voxel_size, info.max_points_per_voxel,
                                                              info.max_voxels[self.mode], cap, xy_range_mask=True)
            return feats, coords, None
        feats = torch.empty((nb * cap, c), dtype=torch.float32, device=dev)
        coords = torch.full((nb * cap, 4), -1, dtype=torch.int32, device=dev)
        d_ns = torch.zeros((nb,), dtype=torch.int32, device=dev)
        streams = [main] * nb
        fork = nb > 1 and self.fork_ok
        if fork:
            streams = self._streams.setdefault(cid, [])
            if len(streams) < nb:
                streams += [torch.cuda.Stream(device=dev) for _ in range(nb - len(streams))]
            for st in streams[:nb]:                # fork: frames are independent, so they are voxelized on parallel
                st.wait_stream(main)               # streams (parallel branches of a captured graph) - each is a chain
        for i, p in enumerate(frames):             # of ~17 launches too small to fill the chip on its own
            with torch.cuda.stream(streams[i]):
                # fused voxelizer + MeanVFE writing row block i of the batch buffers; the xy range mask of
                # data_processor.py:24-37 is applied inside the kernel
                ops.voxelize_hard_mean_into(p, rng, info.voxel_size, info.max_points_per_voxel, info.max_voxels[self.mode], i,
                                            feats[i * cap:(i + 1) * cap], coords[i * cap:(i + 1) * cap], d_ns[i:i + 1],
                                            xy_range_mask=True)
        if fork:
            for st in streams[:nb]:                # join
                main.wait_stream(st)
        return feats, coords, None

    @torch.no_grad()
    def voxelize_stage(self, frames):
        """Points -> voxels.  Equally long frames that cannot overflow max_voxels are voxelized straight into the level-1
        sparse index (one launch chain for the whole batch; no voxel list, no first-appearance ordering, no separate index
        build / scatter): returns ('level', SparseLevel, rows).  Otherwise ('voxels', features, coords, d_n)."""
        nb = len(frames)
        bb = self.model.backbone3d
        n0 = frames[0].shape[0]
        if (PAD_RAGGED and not self.dynamic and nb > 1 and not isinstance(frames, _StackedFrames) and any(p.shape[0] != n0 for p in frames)):
            # frames of different lengths (what real sweeps are): padded on the device to the longest with rows OUTSIDE the point-cloud
            # range - the xy mask of data_processor.py:24-37 inside the kernels drops them - and voxelized as ONE stacked batch straight
            # into the level-1 index, instead of one fused-voxelizer chain per frame: nb small copies buy the batched route (round 6:
            # the `ragged/list` leg of bench.py)
            nmax = max(p.shape[0] for p in frames)
            if nmax <= self.info.max_voxels[self.mode]:
                c = frames[0].shape[1]
                buf = frames[0].new_zeros((nb, nmax, c))
                buf[:, :, 0] = 1.0e6
                for i, p in enumerate(frames):
                    buf[i, :p.shape[0]].copy_(p)
                frames = _StackedFrames(buf)
                n0 = nmax
        if (not self.dynamic and nb > 1 and n0 <= self.info.max_voxels[self.mode] and all(p.shape[0] == n0 for p in frames)):
            c = frames[0].shape[1]
            pts = frames.tensor.reshape(-1, c) if isinstance(frames, _StackedFrames) else torch.cat(list(frames), dim=0)
            lvl1, x = ops.voxelize_to_level(pts, nb, self.info.point_cloud_range, self.info.voxel_size,
                                            self.info.max_points_per_voxel, self.info.max_voxels[self.mode], bb.sparse_shape,
                                            bb.CIN_PAD, math=bb.math, xy_range_mask=True, layout=bb.layout)
            return ('level', lvl1, x)
        return ('voxels',) + tuple(self._voxelize(frames))

    @torch.no_grad()
    def pyramid_stage(self, vox, nb, overlap=True, staggered=False):
        """Voxels -> the sparse index pyramid of the backbone (output sets, bitmaps, neighbour tables of every stage).
        staggered (with overlap): the deeper stages are indexed from inside `backbone_stage`, each under the convolutions of the
        stage before it (VoxelResBackBone8x.build_pyramid)."""
        caps = None if self.level_caps is None else [c * nb for c in self.level_caps]
        bb = self.model.backbone3d
        # (side_key: the index pyramid's side stream - a concurrent sub-pass (`_call_split`) has its own)
        if vox[0] == 'level':
            pyr = bb.build_pyramid(vox[2], None, nb, None, overlap=overlap, side_key=self.side_key, caps=caps, level1=vox[1], staggered=staggered)
        else:
            pyr = bb.build_pyramid(vox[1], vox[2], nb, vox[3], overlap=overlap, side_key=self.side_key, caps=caps, staggered=staggered)
        pyr['nb'] = nb
        return pyr

    def prepare(self, frames, overlap=True, staggered=False):
        """Stage A: everything that depends only on the points - voxelization, voxel features, the sparse index
        pyramid of the backbone.  Returns an opaque dict for ``infer``."""
        return self.pyramid_stage(self.voxelize_stage(frames), len(frames), overlap, staggered)

    @torch.no_grad()
    def calibrate(self, frames, margin=1.5):
        """Measure the active-site counts of the strided backbone stages on sample frames (one host sync) and size
        the per-frame row capacities to `margin` x the largest count seen; afterwards buffers grow with B x that
        instead of the worst case.  Frames that later exceed a capacity lose rows; `self.last_overflow` (device bool, set by
        `backbone_stage` - with a staggered pyramid the flag exists only once the convolutions have requested the last stage's index)
        and the sticky counter behind `overflow_seen()` / `check_overflow()` tell.  Call before graph capture: the counter is
        allocated here, so a capture that follows immediately records no allocation / memset node for it."""
        self.level_caps = None
        best = [0, 0, 0, 0]
        for f in frames:
            pyr = self.prepare([f], overlap=False)
            for i, st in enumerate(pyr['steps'][1:]):
                best[i] = max(best[i], st[2].num_active())
        self.level_caps = [int(margin * b) + 4096 for b in best]
        if self._overflow_acc is None and frames:
            self._overflow_acc = torch.zeros((), dtype=torch.int32, device=frames[0].device)
        if self.ways > 1 and frames:                 # (the sub-passes' counters too: nothing is allocated inside a capture)
            for sub in self._make_subs(frames[0].device):
                if sub._overflow_acc is None:
                    sub._overflow_acc = torch.zeros((), dtype=torch.int32, device=frames[0].device)
        return self.level_caps

    def _make_subs(self, dev):
        if self._subs is None:
            self._subs = [FramePipeline(self.model, self.info, self.mode, self.dynamic, ways=1) for _ in range(self.ways)]
            for k, sub in enumerate(self._subs):
                sub.side_key = 1 + k
            self._way_streams = [torch.cuda.Stream(device=dev) for _ in range(self.ways)]
        return self._subs

    def overflow_seen(self, clear=True):
        """Host-side read (one sync) of the STICKY overflow counter: True when any pass since the last read (eager or replayed from
        a graph - the OR into the counter is a kernel of the pass) lost sparse sites to a calibrated capacity."""
        accs = [a for a in [self._overflow_acc] + [sub._overflow_acc for sub in (self._subs or [])] if a is not None]
        if not accs:
            return False
        seen = bool(torch.stack([a.reshape(()) for a in accs]).sum().item())
        if clear:
            for a in accs:
                a.zero_()
        return seen

    def check_overflow(self):
        """Raises when a pass since the last check overflowed a calibrated level capacity (`calibrate`): a frame much denser than
        the samples silently loses the sites past a capacity, so the outputs since the last check are the ones to discard - re-run
        calibrate() on denser samples / with a larger margin, or use worst-case capacities (no `calibrate`).  One host sync: call it
        after a pass or once per chunk of passes (frame_parallel.run_frame_parallel does)."""
        if self.overflow_seen():
            raise DetZeroHipError('FramePipeline: a sparse level overflowed its calibrated row capacity (%s per frame): '
                                  're-run calibrate() on denser samples / with a larger margin, or drop the calibration'
                                  % (self.level_caps,))

    def _recording(self):
        return self.audit.recording() if self.audit is not None else contextlib.nullcontext()

    def check_range(self):
        """Raises when a tensor stored by a pass since the last check saturated its fp16 pairs or went non-finite (needs `audit=`):
        the pre-scale in force does not hold these frames - re-run select_math(probe='all') on hotter samples; stale exponents after
        new weights show here too.  One host sync; the records are cleared for the next check."""
        if self.audit is None:
            raise DetZeroHipError('FramePipeline.check_range: construct the pipeline with audit=RangeAudit()')
        bad = _range_audit.first_violation(self.audit.report())
        self.audit.reset()
        if bad is not None:
            raise DetZeroHipError('FramePipeline: range check failed - ' + _range_audit.describe(bad))

    @torch.no_grad()
    def backbone_stage(self, prep):
        """The 21 sparse convolutions -> {name: (rows, SparseLevel)}."""
        with self._recording():
            res = self.model.backbone3d.run_pyramid(prep)        # (a staggered pyramid finishes its index, and the flag, in here)
        self.last_overflow = prep.get('overflow', None)          # flag of THIS pass (device bool); the counter below is sticky
        if self.last_overflow is not None:
            # (after run_pyramid: the flag is written on the index-pyramid side stream, and the main stream has by now waited for
            # the last stage's event, which covers it)
            if self._overflow_acc is None:                       # (capacities set by hand instead of calibrate())
                if torch.cuda.is_current_stream_capturing():
                    raise DetZeroHipError('FramePipeline: the overflow counter must exist before graph capture - run calibrate() or '
                                          'one eager pass first (a counter allocated inside a capture is re-zeroed by every replay)')
                self._overflow_acc = torch.zeros((), dtype=torch.int32, device=self.last_overflow.device)
            self._overflow_acc |= self.last_overflow.to(torch.int32)
        return res

    @torch.no_grad()
    def dense_stage(self, res, nb):
        """`_dense_stage`, its stored tensors probed into the pipeline's audit when it has one."""
        with self._recording():
            return self._dense_stage(res, nb)

    def _dense_stage(self, res, nb):
        """HeightCompression + BaseBEVBackbone + the CenterHead convolutions -> (head map (B,H*W,12), H, W).
        With `head_at_candidates` (and a head csrc/head_cand.hip serves) only the branches the selection reads at every cell run here:
        columns 8:12 of the map (9:12 when IOU_WEIGHT is 0) are written, columns 0:8 are NOT - post_stage fills them at the selected
        cells from the shared map.  The pipeline keeps that hand-over itself (`_partial_head`: the map's address and shape, and the shared
        map, an image of this pipeline's workspace valid until the next dense_stage): post_stage must get THIS map, not a copy or a slice.
        More than `dense_group` frames go through the dense layers in groups: the kernels address an image through 32-bit buffer
        offsets, and the 512-channel concatenation of the Waymo config passes 2 GiB at ~20 frames.  The BEV image (1.2 GB at 32
        frames) is built once; a group is a contiguous slice of it."""
        m = self.model
        x, lvl = res['encoded']
        sparse = m.backbone3d.math != 0 and m.backbone2d.math == m.backbone3d.math and m.backbone2d.sparse_input_ok(x.shape[1], lvl.shape[0])
        if sparse:
            # HeightCompression without the image: 8 bytes of row indices per pixel; the first BEV convolution reads the rows
            bev = ops.bev_row_index(lvl, x.shape[0], pad=1)
            run2d = lambda g0, ng: m.backbone2d.run(None, ng, sparse_in=(x, bev[g0:g0 + ng]))          # noqa: E731
        else:
            bev = ops.sparse_to_bev(x, lvl, x.shape[1], pad=1, math=m.backbone3d.math)
            run2d = lambda g0, ng: m.backbone2d.run(bev[g0:g0 + ng], ng)                               # noqa: E731
        # frames per group: the configured number, but never more than the largest activation image (the concatenation of the
        # upsampled maps, channel-last fp32-sized words, zero border included) allows inside the 2 GiB buffer window
        per_frame = bev.shape[1] * bev.shape[2] * max(int(m.backbone2d.num_bev_features), 2 * int(x.shape[1])) * 4
        group = max(1, min(self.dense_group if self.dense_group > 0 else nb, (2 ** 31 - 1) // per_frame))
        at_cand = self.head_at_candidates and self.head.at_candidates_ok()
        self._partial_head = None
        if at_cand:
            self.head.candidate_params()             # (packed once, here: never inside post_stage's first captured call)
        if nb <= group:
            with cp_modules.workspace(self._ws):
                concat = run2d(0, nb)
                if not at_cand:
                    return self.head.run_convs(concat, nb)
                shared = self.head.run_shared(concat, nb)
                hd, hh, hw_ = self.head.run_score_head(shared, nb)
                self._partial_head = (hd.data_ptr(), tuple(hd.shape), shared)
                return hd, hh, hw_
        st = {'out': None, 'h': 0, 'w': 0, 'shared': None}

        def head_of_group(concat, g0, ng):
            if at_cand:
                # the shared maps outlive their group: every group writes its slice of one all-frames image
                if st['shared'] is None:
                    st['shared'] = cp_modules.bordered_zeros('head.shared_all', (nb,) + tuple(concat.shape[1:3]) + (self.head.plan()['c'],), concat.device)
                hd, st['h'], st['w'] = self.head.run_score_head(self.head.run_shared(concat, ng, out=st['shared'][g0:g0 + ng]), ng)
            else:
                hd, st['h'], st['w'] = self.head.run_convs(concat, ng)
            if st['out'] is None:
                st['out'] = hd.new_empty((nb,) + tuple(hd.shape[1:]))
            st['out'][g0:g0 + ng].copy_(hd)          # (the activation images, the head map among them, are reused by the next group)
        with cp_modules.workspace(self._ws):
            if GROUPED_DEEP_BLOCKS and m.backbone2d.grouped_fits(nb, bev.shape[1] - 2, bev.shape[2] - 2):
                # first block, deblocks and head in frame groups; the deeper (quarter-size) blocks over all frames at once (while the
                # all-frame images of those blocks fit the 2 GiB window: 116 frames at the Waymo size - beyond that every layer per group)
                m.backbone2d.run_grouped(nb, group, head_of_group, bev=None if sparse else bev, sparse_in=(x, bev) if sparse else None)
            else:
                for g0 in range(0, nb, group):
                    ng = min(group, nb - g0)
                    head_of_group(run2d(g0, ng), g0, ng)
        if at_cand:
            self._partial_head = (st['out'].data_ptr(), tuple(st['out'].shape), st['shared'])
        return st['out'], st['h'], st['w']

    @torch.no_grad()
    def post_stage(self, head, h, w):
        """Top-K decode, rotated NMS, packing -> (boxes9 (B,K,9), counts (B,)).  The map of a dense_stage with `head_at_candidates`
        goes select -> regression at the candidates -> decode of the selected; a full map as before.  While this pipeline's last
        dense_stage left a partial map, any other tensor is refused: a copy or slice of that map has no columns 0:8 to decode."""
        shared = None
        if self._partial_head is not None:
            ptr, shape, shared = self._partial_head
            if head.data_ptr() != ptr or tuple(head.shape) != shape:
                raise DetZeroHipError('FramePipeline.post_stage: the last dense_stage wrote only the selection columns of its head map '
                                      '(head_at_candidates) and this is not that tensor - pass dense_stage\'s result as it is, or set '
                                      'head_at_candidates = False for full maps')
        boxes, scores, labels, keep, d_nk = self.head.decode_batched_nosync(head, h, w, shared=shared)
        return ops.pack_detections(boxes, scores, labels, keep, d_nk, self.post_max), d_nk

    def infer(self, prep):
        """Stage B: the 21 sparse convolutions, BEV backbone, head, top-K decode, NMS -> (boxes9 (B,K,9), counts (B,))."""
        try:
            return self.post_stage(*self.dense_stage(self.backbone_stage(prep), prep['nb']))
        except DetZeroHipError as e:
            if '2 GiB' in str(e) and self.level_caps is None:
                raise DetZeroHipError('%s\n(FramePipeline: %d frames per pass with WORST-CASE row capacities for the strided sparse levels - call '
                                      'pipe.calibrate(sample_frames) first: it sizes them to 1.5 x the measured counts, a device-side flag and '
                                      'check_overflow() guard denser frames)' % (e, prep['nb'])) from None
            raise

    @torch.no_grad()
    def two_stage(self, points, before_second=None):
        """A model with SECOND_STAGE (the PDV configs): first stage as `__call__` (batched, sync-free, its own streams), then the model's
        roi_head ONCE over the whole batch - the RoIs of all frames pooled by one launch per branch (pdv_modules.PDVHead).  points: list of
        (N_i, C) tensors or a (B, N, C) tensor.  Returns the batch_dict the plugin path's roi_head returns (rois, roi_scores, roi_labels,
        batch_box_preds, batch_cls_preds; CenterPoint.post_processing reads exactly these).  The second stage sizes its work by the
        largest RoI count of the batch (one host sync), as the plugin path's reorder_rois does (center_head.py:388-406)."""
        from .det_modules import SparseConvTensor
        m = self.model
        if getattr(m, 'roi_head', None) is None:
            raise DetZeroHipError('FramePipeline.two_stage: the model has no roi_head (MODEL.SECOND_STAGE)')
        frames = _StackedFrames(points.contiguous()) if torch.is_tensor(points) else (points if isinstance(points, _StackedFrames) else list(points))
        nb = len(frames)
        prep = self.prepare(frames, staggered=STAGGERED_PYRAMID)
        res = self.backbone_stage(prep)
        out, d_nk = self.post_stage(*self.dense_stage(res, nb))
        bb = m.backbone3d

        k = max(int(d_nk.max().item()), 1)
        # a calibrated level that overflowed holds ranks beyond its row capacity in its bitmap / prefix: the second stage looks voxels
        # up by rank (PDVHead.get_point_voxel_features), so it must not run on such a pass - the flag of THIS pass is read here (the
        # host is synchronised by the line above anyway) and the pass is refused; the sticky counter still reports it to check_overflow
        if self.last_overflow is not None and bool(self.last_overflow.item()):
            raise DetZeroHipError('FramePipeline.two_stage: a sparse level overflowed its calibrated row capacity (%s per frame) - the second '
                                  'stage would read rows past the feature tensors; re-run calibrate() on denser samples / with a larger '
                                  'margin, or drop the calibration' % (self.level_caps,))

        def as_tensor(item):
            feats, level = item
            m_act = min(level.num_active(), level.cap, feats.shape[0])          # (never more rows than the tensors hold)
            return SparseConvTensor(None, level.coords[:m_act], level.shape, nb, level=level, padded=(feats, level), math=bb.math)
        pts = [frames[i] for i in range(nb)]
        points_b = torch.cat([torch.cat([p.new_full((p.shape[0], 1), float(i)), p], dim=1) for i, p in enumerate(pts)], dim=0)
        bd = {'batch_size': nb, 'points': points_b, 'rois': out[:, :k, :7].contiguous(), 'roi_scores': out[:, :k, 7].contiguous(),
              'roi_labels': out[:, :k, 8].long(), 'has_class_labels': True,
              'multi_scale_3d_features': {n: as_tensor(res[n]) for n in ('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4')},
              'multi_scale_3d_strides': {'x_conv1': 1, 'x_conv2': 2, 'x_conv3': 4, 'x_conv4': 8}}
        if before_second is not None:
            before_second()                 # (timing hook: called between the stages)
        return m.roi_head(bd)

    @torch.no_grad()
    def __call__(self, points):
        """points: (N,C) tensor = one frame; list of (N_i,C) tensors or a (B,N,C) tensor = a batch."""
        single = torch.is_tensor(points) and points.dim() == 2
        if single:
            frames = [points]
        elif torch.is_tensor(points):
            frames = _StackedFrames(points.contiguous())
        else:
            frames = points if isinstance(points, _StackedFrames) else list(points)
        nb = len(frames)
        if nb > self.max_pass_frames():
            # more frames than one pass can key: the voxel keys are 32 bits wide (batch x grid cells: 46 frames of the 1504 x 1504 x 41
            # Waymo grid) - the batch runs as consecutive chunks, each of them a pass (or two concurrent sub-passes) of its own
            step = self.max_pass_frames()
            outs = []
            for a in range(0, nb, step):
                part = _StackedFrames(frames.tensor[a:a + step]) if isinstance(frames, _StackedFrames) else list(frames[a:a + step])
                outs.append(self(part))
            return torch.cat([o for o, _ in outs], dim=0), torch.cat([n.view(-1) for _, n in outs], dim=0)
        if self.splits(nb):
            return self._call_split(frames)
        out, d_nk = self.infer(self.prepare(frames, staggered=STAGGERED_PYRAMID))
        return (out[0], d_nk) if single else (out, d_nk)

    def max_pass_frames(self):
        """Largest batch ONE call runs as one pass or one set of concurrent sub-passes: every (sub-)pass must key its frames' voxels in
        32 bits (csrc/voxelize.hip: batch x D x H x W < 2^32 - 1); 32 frames per (sub-)pass is also where the dense stage's images and the
        x-run tiles are sized best (bench.py's sweep), so that is the chunk."""
        g = self.info.grid_size
        cells = (int(g[2]) + 1) * int(g[1]) * int(g[0])
        per_pass = max(1, min(32, (2 ** 32 - 2) // cells))
        if self.dynamic:
            # DynamicMeanVFE merges on int32 keys, as the reference does (vfe.py:128-131: "overflows for b >= 24" on the Waymo grid)
            lim = (2 ** 31 - 1) // cells
            per_pass = max(1, min(per_pass, lim if lim < 8 else lim // 8 * 8))
        return per_pass * (self.ways if self.ways > 1 else 1)

    def splits(self, nb):
        """Whether a batch of nb frames runs as concurrent sub-passes."""
        return self.ways > 1 and nb >= max(2 * self.ways, self.split_min)

    def _split_parts(self, frames):
        nb, w = len(frames), self.ways
        bounds = [(k * nb) // w for k in range(w + 1)]
        return [(_StackedFrames(frames.tensor[a:b]) if isinstance(frames, _StackedFrames) else list(frames[a:b]), a, b)
                for a, b in zip(bounds[:-1], bounds[1:])]

    def _call_split(self, frames):
        """The batch as `ways` concurrent sub-passes: frames [k * nb / ways, (k + 1) * nb / ways) through their own FramePipeline (own
        activation images, same model / capacities, own overflow counter) on their own stream, forked from and joined to the caller's
        stream.  Frames are independent, so the results are those of the single pass bit for bit (tests/test_gpu_e2e.py).
        Inside a graph capture the sub-passes are parallel branches of the graph and must not fork again (hipStreamEndCapture of
        ROCm 7.2 crashes on a fork nested inside a forked branch, tools/dbg_nested_capture.py): they then build their index pyramids and voxelize
        ragged frames on their own stream."""
        dev = frames[0].device
        self._make_subs(dev)
        main = torch.cuda.current_stream(dev)
        nested_ok = not torch.cuda.is_current_stream_capturing()
        parts = self._split_parts(frames)
        # first pass of a cache generation (new weights / math mode / pre-scale / sub-pass shapes): the modules build their kernel-layout
        # weights, packed pairs and zero-response images lazily ON THE STREAM THAT ASKS FIRST - the sub-passes then run one after the
        # other, so that whatever the first one builds is complete before the second one reads it from another stream
        sig = (cp_modules.CACHE_GEN[0], tuple((len(p), tuple(p[0].shape)) for p, _, _ in parts), str(dev))
        serial = sig != getattr(self, '_split_sig', None)
        self._split_sig = sig
        if serial and not nested_ok:
            import warnings
            warnings.warn('FramePipeline: graph capture of a split pass without an eager pass of the same shapes before it - the sub-passes '
                          'are recorded ONE AFTER THE OTHER (correct, but without their overlap); run one eager pass first')
        outs = []
        prev = None
        for (part, _, _), sub, st in zip(parts, self._subs, self._way_streams):
            sub.head_at_candidates = self.head_at_candidates
            sub.audit = self.audit                   # (one record per tensor for both sub-passes: the probes add with device-scope atomics)
            sub.level_caps, sub.dense_group = self.level_caps, self.dense_group       # (every sub-pass keeps its OWN sticky overflow counter:
            sub.fork_ok = nested_ok                                                    # two streams OR-ing into one word would race)
            st.wait_stream(main)
            if serial and prev is not None:
                st.wait_stream(prev)
            prev = st
            with torch.cuda.stream(st):
                outs.append(sub.infer(sub.prepare(part, overlap=nested_ok, staggered=nested_ok and STAGGERED_PYRAMID)))
        for st in self._way_streams:
            main.wait_stream(st)
        for o, n in outs:
            o.record_stream(main)
            n.record_stream(main)
        flags = [sub.last_overflow for sub in self._subs if sub.last_overflow is not None]
        self.last_overflow = None if not flags else (flags[0] if len(flags) == 1 else torch.stack([f.reshape(()) for f in flags]).any())
        return torch.cat([o for o, _ in outs], dim=0), torch.cat([n for _, n in outs], dim=0)

    def capture(self, static_points):
        """hipGraph(s) of this pipeline over a STATIC input -> CapturedPass (replay(); results in .boxes (B, K, 9) / .counts (B,)).  Run
        calibrate() and one eager pass before (allocations, kernel-layout weights, zero-response images)."""
        return CapturedPass(self, static_points)


class CapturedPass:
    """FramePipeline over a static input as ONE captured graph; with ways > 1 the concurrent sub-passes are parallel branches of it
    (each on its own stream, without forks of its own: see `_call_split`).  Measured on one box against ways = 1 (profiles/
    r06_ab_notes.txt): +1.0 % frames/s at 32 frames per pass, +3.0 % at 16, +-0 at 8.  One graph PER sub-pass, replayed side by side
    (which keeps the sub-passes' inner forks) was built first and is slower than no split at all in bench.py: -2.7 % / -4.5 % / -13 %.

    The graph holds raw pointers into the plans of the model's modules (kernel-layout and packed weights, scale / shift vectors, the
    zero-response images).  The pass keeps the plan objects of capture time (`plans`), so those tensors stay alive, and `replay()`
    refuses with DetZeroHipError once a module has dropped its plan (load_state_dict, invalidate(), a device move): the weights
    changed, capture again.  `stale()` tells without raising.  Math, pre-scale and engine switches after the capture do not drop a
    plan: a replay then reproduces the configuration of CAPTURE time, not the model's current one."""

    def __init__(self, pipe, static_points):
        self.pipe = pipe
        nb = static_points.shape[0] if torch.is_tensor(static_points) else len(static_points)
        dev = static_points.device if torch.is_tensor(static_points) else static_points[0].device
        self.boxes = torch.zeros((nb, pipe.post_max, 9), dtype=torch.float32, device=dev)
        self.counts = torch.zeros((nb,), dtype=torch.int32, device=dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            o, n = pipe(static_points)
            self.boxes.copy_(o.view(self.boxes.shape))
            self.counts.copy_(n.view(-1))
        self.branches = pipe.ways if pipe.splits(nb) else 1
        self.plans = cp_modules.plan_snapshot(pipe.model)       # (strong references: what the graph points at lives as long as this pass)

    def stale(self):
        """True once a module of the model has dropped the plan this graph was captured on (identity of the plan objects: another
        model's reload does not count)."""
        return cp_modules.plans_changed(self.plans)

    def replay(self):
        if self.stale():
            raise DetZeroHipError('CapturedPass: weights changed since capture; capture again')
        self.graph.replay()


class StreamingDetector:
    """Two-stage software pipeline over a stream of equally shaped batches on one GPU.

    Stage A (``FramePipeline.prepare``: input copy, voxelization, index pyramid - dozens of small launches that
    cannot fill 256 CUs) of batch i+1 runs on its own stream WHILE stage B (``infer``: the convolutions, head, NMS)
    of batch i runs; each stage is a captured hipGraph with static buffers, double buffered so that the two
    batches in flight never share memory.  ``feed(frames)`` enqueues A(frames) and B(previous batch) and returns
    the previous batch's (boxes9 (B,K,9), counts (B,)) - device tensors that stay valid until the call after
    next - or None on the first call; ``flush()`` returns the last batch's.  Nothing here synchronises the host.

    Each slot's graphs are bound to the plans of the model's modules as `CapturedPass` is: the slot keeps the plan objects of capture
    time, and ``feed()`` / ``flush()`` raise DetZeroHipError before launching anything once a module has dropped its plan (``stale()``);
    math, pre-scale and engine switches after construction leave the graphs at the configuration they were captured in.
    """

    def __init__(self, pipe, example_frames, use_graph=True, warmup=3):
        self.pipe = pipe
        dev = example_frames[0].device
        self.dev = dev
        # stage A is a long chain of small launches: give its queue priority, otherwise its workgroups only get CU
        # slots at the pace the convolution kernels of stage B retire theirs and the chain never catches up
        self.s_a = torch.cuda.Stream(device=dev, priority=-1)
        self.s_b = torch.cuda.Stream(device=dev)
        self.slots = []
        self.graph_note = 'hipGraph replay (stage A / stage B graphs, double buffered)' if use_graph else 'eager launches (two streams)'
        cur = torch.cuda.current_stream(dev)
        for k in range(2):
            slot = {'in': [f.clone() for f in example_frames], 'ga': None, 'gb': None, 'prep': None, 'out': None, 'plans': [],
                    'a_done': torch.cuda.Event(), 'b_done': torch.cuda.Event()}
            self.s_a.wait_stream(cur)
            with torch.cuda.stream(self.s_a):
                for _ in range(max(1, warmup)):          # primes allocator pools and kernel-layout weights
                    prep = pipe.prepare(slot['in'], overlap=False)
                    out = pipe.infer(prep)
            cur.wait_stream(self.s_a)
            torch.cuda.synchronize(dev)
            if use_graph:
                try:
                    ga = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(ga):
                        prep = pipe.prepare(slot['in'], overlap=False)
                    gb = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gb):
                        out = pipe.infer(prep)
                    ga.replay(); gb.replay()
                    torch.cuda.synchronize(dev)
                    slot['ga'], slot['gb'] = ga, gb
                    slot['plans'] = cp_modules.plan_snapshot(pipe.model)
                except Exception as e:  # capture is an optimisation, not a requirement
                    self.graph_note = 'eager launches, two streams (graph capture failed: %s)' % str(e).split('\n')[0][:100]
                    slot['ga'] = slot['gb'] = None
                    torch.cuda.synchronize(dev)
            slot['prep'], slot['out'] = prep, out
            self.slots.append(slot)
        self.n_fed = 0

    def _stage_a(self, k, frames):
        slot = self.slots[k]
        with torch.cuda.stream(self.s_a):
            self.s_a.wait_event(slot['b_done'])            # the previous user of this slot has consumed its buffers
            for dst, src in zip(slot['in'], frames):
                dst.copy_(src, non_blocking=True)
            if slot['ga'] is not None:
                slot['ga'].replay()
            else:
                self.s_b.synchronize()                     # eager fallback only: the old buffers of this slot go back to the allocator
                slot['prep'] = self.pipe.prepare(slot['in'], overlap=False)
            slot['a_done'].record(self.s_a)

    def _stage_b(self, k):
        slot = self.slots[k]
        with torch.cuda.stream(self.s_b):
            self.s_b.wait_event(slot['a_done'])
            if slot['gb'] is not None:
                slot['gb'].replay()
            else:
                slot['out'] = self.pipe.infer(slot['prep'])
            slot['b_done'].record(self.s_b)
        return slot['out']

    def stale(self):
        """True once a module of the model has dropped the plan a slot's graphs were captured on (eager slots hold no pointers)."""
        return any(slot['gb'] is not None and cp_modules.plans_changed(slot['plans']) for slot in self.slots)

    def _check_fresh(self):
        if self.stale():
            raise DetZeroHipError('StreamingDetector: weights changed since capture; capture again (build a new StreamingDetector)')

    def feed(self, frames):
        self._check_fresh()
        cur = torch.cuda.current_stream(self.dev)
        self.s_a.wait_stream(cur)                          # the caller's frames are ready
        self.s_b.wait_stream(cur)                          # ... and it has finished reading the results handed out before
        k = self.n_fed & 1
        prev = self._stage_b(k ^ 1) if self.n_fed > 0 else None
        self._stage_a(k, frames)
        self.n_fed += 1
        if prev is not None:
            cur.wait_stream(self.s_b)                      # results are consumed on the caller's stream
        return prev

    def flush(self):
        if self.n_fed == 0:
            return None
        self._check_fresh()
        cur = torch.cuda.current_stream(self.dev)
        out = self._stage_b((self.n_fed - 1) & 1)
        cur.wait_stream(self.s_b)
        return out


def __getattr__(name):
    """The synthetic weight sets live in detzero_amd/synth_weights.py (they are test / bench fixtures, not part of the detection path);
    `from detzero_amd.centerpoint import synth_detector` keeps working."""
    if name in ('synth_detector', 'variance_preserving_init', 'uniform_field_response'):
        from . import synth_weights
        return getattr(synth_weights, name)
    raise AttributeError('module %r has no attribute %r' % (__name__, name))
