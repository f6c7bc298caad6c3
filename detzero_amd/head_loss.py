"""CenterHead's loss layer on the device (center_head.py:107-313, utils/loss_utils.py:143-243): the per-head driver behind
``CenterHead.get_loss`` and the two parameter-free loss modules ``build_losses`` registers.  Everything here is backed by
csrc/head_loss.hip (``ops.centerhead_targets`` / ``ops.centerhead_loss``); DESIGN.md 7p states the semantics.

The modules keep the reference's call signatures but take NCHW *views of the head map* - what ``forward_ret_dict['pred_dicts']``
holds: the heat-map branch as logits (the sigmoid and its clamp are part of the kernel) - because the kernels read the
channel-last (B, H*W, 12) map those views alias.  They return values only (inference-mode functionality); the gradient comes
from ``ops.centerhead_loss`` on the head map itself.
"""
import torch
import torch.nn as nn

from . import ops
from .lib import DetZeroHipError

COLS = 12


def head_map_of(view):
    """(head (B, H*W, 12), first column, H, W) of an NCHW view (B, C, H, W) of a channel-last head map."""
    if view.dim() != 4 or view.dtype != torch.float32 or not view.is_cuda:
        raise DetZeroHipError('head_loss: expected an NCHW float32 device view of a head map, got %s %s' % (tuple(view.shape), view.dtype))
    b, c, h, w = view.shape
    col = view.storage_offset() % COLS
    if tuple(view.stride()) != (h * w * COLS, 1, w * COLS, COLS) or col + c > COLS:
        raise DetZeroHipError('head_loss: not a view of a channel-last (B, H*W, 12) head map (strides %s)' % (tuple(view.stride()),))
    head = torch.as_strided(view.detach(), (b, h * w, COLS), (h * w * COLS, COLS, 1), view.storage_offset() - col)
    return head, col, h, w


class FocalLossCenterNet(nn.Module):
    """loss_utils.py:181-190 (neg_loss_cornernet) on the heat-map view of a head map: ``out`` (B, ncls, H, W) logits in columns
    9:9+ncls, ``target`` (B, ncls, H, W), optional ``mask`` (B, H, W).  The clamped sigmoid of center_head.py:262-264 is applied
    inside the kernel, so ``out`` is NOT passed through ``sigmoid`` first."""

    def forward(self, out, target, mask=None):
        head, col, h, w = head_map_of(out)
        if col != 9 or target.shape != out.shape:
            raise DetZeroHipError('FocalLossCenterNet: out is the hm view (columns 9:9+ncls) and target has its shape')
        b = head.shape[0]
        dev = head.device
        none = torch.zeros((b, 1), dtype=torch.int64, device=dev)
        rec = ops.centerhead_loss_nosync(head, target.float().contiguous(), torch.zeros((b, 1, 8), dtype=torch.float32, device=dev), none, none,
                                         None, h, w, (1.0, 0.0) + (0.0,) * 9, 1.0, (0.0, 0.0), (1.0, 1.0),
                                         hm_mask=None if mask is None else mask.float().contiguous())[0]
        return rec[0].to(torch.float32)


class RegLossCenterNet(nn.Module):
    """loss_utils.py:220-242 (_reg_loss) on a regression view of a head map: ``output`` (B, dim, H, W) inside columns 0:8,
    ``mask`` / ``ind`` (B, NMAX), ``target`` (B, NMAX, dim) -> (dim,) losses.  The IoU branch (column 8) has its targets formed
    inside ``ops.centerhead_loss`` and is not served here, nor is the reference's ``ind=None`` form."""

    def forward(self, output, mask, ind=None, target=None):
        if ind is None or target is None:
            raise DetZeroHipError('RegLossCenterNet: ind and target are required (the gather is part of the kernel)')
        head, col, h, w = head_map_of(output)
        dim = output.shape[1]
        if col + dim > 8 or target.dim() != 3 or target.shape[2] != dim:
            raise DetZeroHipError('RegLossCenterNet: output is a view inside columns 0:8 and target (B, NMAX, %d); the IoU term is '
                                  'part of ops.centerhead_loss' % dim)
        b, nmax = ind.shape
        dev = head.device
        tb = torch.zeros((b, nmax, 8), dtype=torch.float32, device=dev)
        tb[:, :, col:col + dim] = target.float()
        code = [1.0 if col <= q < col + dim else 0.0 for q in range(8)]
        heat = torch.zeros((b, 1, h, w), dtype=torch.float32, device=dev)
        rec = ops.centerhead_loss_nosync(head, heat, tb, ind.long().contiguous(), mask.long().contiguous(), None, h, w,
                                         (0.0, 1.0, *code, 0.0), 1.0, (0.0, 0.0), (1.0, 1.0))[0]
        return rec[1 + col:1 + col + dim].to(torch.float32)


def loss_weights(model_cfg):
    """(cls_weight, loc_weight, code_weights[8], iou_weight) of a DENSE_HEAD config (center_head.py:63,277,288,297)."""
    lc = model_cfg.get('LOSS_CONFIG', None)
    if lc is None:
        raise DetZeroHipError('CenterHead.get_loss: DENSE_HEAD has no LOSS_CONFIG')
    lw = lc['LOSS_WEIGHTS']
    code = [float(v) for v in lw['code_weights']]
    if len(code) != 8:
        raise DetZeroHipError('CenterHead.get_loss: %d code_weights (8: the `vel` head is not supported)' % len(code))
    return (float(lw['cls_weight']), float(lw['loc_weight']), *code, float(model_cfg.get('IOU_WEIGHT', 0)))


def class_table(class_names, head_class_names):
    """cls_table of ops.centerhead_targets: the head's 1-based class of every global class, 0 = not this head."""
    return [head_class_names.index(n) + 1 if n in head_class_names else 0 for n in class_names]


def device_targets(head_module, gt_boxes, feature_map_size):
    """center_head.py:202-260 with the per-frame, per-box loops on the device: the dictionary ``assign_targets`` returns, plus
    'records' (one (2,) i32 [num_pos, num] per head) for the loss."""
    cfg = head_module.model_cfg.TARGET_ASSIGNER_CONFIG
    if 'vel' in head_module.separate_head_cfg.HEAD_DICT.keys():
        raise DetZeroHipError('CenterHead: device targets for a `vel` head are not supported')
    if not gt_boxes.is_cuda:
        raise DetZeroHipError('CenterHead: device targets need gt_boxes on the device')
    h, w = int(feature_map_size[0]), int(feature_map_size[1])
    gt = torch.cat((gt_boxes[:, :, :7], gt_boxes[:, :, -1:]), dim=2).float().contiguous()      # :211-212
    ret = {'heatmaps': [], 'target_boxes': [], 'inds': [], 'masks': [], 'heatmap_masks': [], 'records': []}
    for names in head_module.class_names_each_head:
        heat, tb, inds, masks, rec = ops.centerhead_targets(
            gt, class_table(head_module.class_names, names), len(names), h, w, cfg.FEATURE_MAP_STRIDE, head_module.point_cloud_range,
            head_module.voxel_size, cfg.NUM_MAX_OBJS, cfg.GAUSSIAN_OVERLAP, cfg.MIN_RADIUS)
        for key, t in zip(('heatmaps', 'target_boxes', 'inds', 'masks', 'records'), (heat, tb, inds, masks, rec)):
            ret[key].append(t)
    return ret


def head_losses(head_module, heads, target_dicts, h, w):
    """One ops.centerhead_loss per head: heads = the (B, H*W, 12) head maps.  -> (totals, records): lists of 0-dim f32 tensors
    (differentiable with respect to a head map that requires grad) and (12,) f64 device records."""
    weights = loss_weights(head_module.model_cfg)
    records = target_dicts.get('records', None)
    totals, recs = [], []
    for i, head in enumerate(heads):
        dev = head.device
        tgt = [target_dicts[k][i].to(dev).contiguous() for k in ('heatmaps', 'target_boxes', 'inds', 'masks')]
        total, rec = ops.centerhead_loss(head, tgt[0].float(), tgt[1].float(), tgt[2].long(), tgt[3].long(),
                                         None if records is None else records[i], h, w, weights, head_module.feature_map_stride,
                                         head_module.point_cloud_range, head_module.voxel_size)
        totals.append(total)
        recs.append(rec)
    return totals, recs


def tb_dict_of(host, iou_weight, tb_dict):
    """The reference's tb_dict keys (center_head.py:266-313) from the heads' (n_heads, 12) records on the host."""
    for idx in range(host.shape[0]):
        r = host[idx]
        tb_dict['center_loss_head_%d' % idx] = float(r[1] + r[2])
        tb_dict['center_z_loss_head_%d' % idx] = float(r[3])
        tb_dict['dim_loss_head_%d' % idx] = float(r[4] + r[5] + r[6])
        tb_dict['rot_loss_head_%d' % idx] = float(r[7] + r[8])
        if iou_weight > 0:
            tb_dict['iou_loss_head_%d' % idx] = float(r[10])
        tb_dict['hm_loss_head_%d' % idx] = float(r[0])
        tb_dict['loc_loss_head_%d' % idx] = float(r[9])
    tb_dict['rpn_loss'] = float(host[:, 11].sum())
    return tb_dict
