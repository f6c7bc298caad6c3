"""Golden vectors of the CenterHead loss layer from the REFERENCE's own classes, CPU: CenterHead.assign_targets / get_loss
(center_head.py:107-313) with the real FocalLossCenterNet / RegLossCenterNet (utils/loss_utils.py:143-243), the prediction
tensors as autograd leaves and loss.backward() for the gradients.

    python tests/golden/gen_head_loss_golden.py      (build container only; needs /root/reference)

Stand-ins: `Tensor.cuda` is the identity, `torch.cuda.FloatTensor` the CPU constructor, and the CUDA extension call
`iou3d_nms_cuda.boxes_overlap_bev_gpu` under the reference's own iou3d_nms_utils.boxes_iou3d_gpu is the oracle's overlap routine
(oracle.cref.boxes_overlap_bev), as in the other generators.  Nothing of the reference's text is copied.

Geometry: a 23 x 19 map (stride 8, 0.1 m voxels), NUM_MAX_OBJS 16, three frames.  Cases (see `gt_case` / `head_map`):
  c1  one head, three classes: a box clamped into the last cell, a box whose radius exceeds the map, dx = 0, padding rows, a
      frame with more boxes than NUM_MAX_OBJS, two same-class boxes on one cell, two boxes of different classes on one cell,
      overlapping Gaussians, logits beyond +/- 9.3, one prediction equal to its target;
  c2  two heads [['Vehicle'], ['Pedestrian', 'Cyclist']] on the same batch: columns 9 + ncls .. 11 of the head maps hold NaN;
  c3  no valid box at all (num_pos == 0, num == 0);
  c4  c1 with IOU_WEIGHT 0.
Stored per case: gt_boxes, the head maps, the targets, every tb_dict value, the gradients with respect to the head maps, and
`dist_*`: |reference float32 - float64| / |float64| of every scalar against tests/head_loss_ref.py's float64 evaluation (absolute where
the float64 value is 0), likewise per gradient column relative to the column's largest float64 gradient.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg          # noqa: E402

sys.path.insert(0, os.path.join(gg.ROOT, 'tests'))
import head_loss_ref as hr       # noqa: E402

W, H, NMAX, B, M = 23, 19, 16, 3, 24
STRIDE, VOXEL = 8, [0.1, 0.1, 0.15]
RANGE = [-9.2, -7.6, -2.0, 9.2, 7.6, 4.0]
NAMES = ['Vehicle', 'Pedestrian', 'Cyclist']
COLS = {'center': (0, 2), 'center_z': (2, 1), 'dim': (3, 3), 'rot': (6, 2), 'iou': (8, 1), 'hm': (9, 3)}


def gt_case(empty=False):
    rng = np.random.default_rng(20240607)
    gt = np.zeros((B, M, 8), np.float32)

    def box(x, y, cls, dx=None, dy=None):
        size = {1: (4.6, 2.0, 1.7), 2: (0.9, 0.8, 1.75), 3: (1.8, 0.8, 1.6)}[cls]
        d = np.array(size) * rng.uniform(0.85, 1.15, 3)
        return [x, y, rng.uniform(-0.5, 1.5), d[0] if dx is None else dx, d[1] if dy is None else dy, d[2], rng.uniform(-3.14, 3.14), cls]
    f0 = [box(9.35, 7.69, 1),                   # clamped into the last cell
          box(0.3, -0.2, 1, dx=60.0, dy=50.0),  # radius beyond the map: clipped on all sides
          box(-3.0, 2.0, 2, dx=0.0),            # dx = 0: skipped, its slot stays empty
          [0] * 8,                              # padding row
          box(-5.0, -4.0, 1), box(-4.9, -3.9, 1),     # two boxes of one class on one cell
          box(4.1, -5.0, 2), box(4.3, -4.9, 3),       # two classes on one cell
          [0] * 8,
          box(-6.0, 4.0, 3), box(-4.9, 4.5, 3),       # overlapping Gaussians
          box(6.5, 3.1, 1)]
    gt[0, :len(f0)] = f0
    f1 = [box(rng.uniform(-9, 9), rng.uniform(-7.4, 7.4), int(rng.integers(1, 4))) for _ in range(20)]      # more than NMAX
    gt[1, :20] = f1
    gt[2, 3:8] = [box(rng.uniform(-9, 9), rng.uniform(-7.4, 7.4), c) for c in (2, 1, 3, 3, 1)]
    if empty:
        gt[:, :, 7] = np.where(gt[:, :, 3] > 50, gt[:, :, 7], 0)      # only the huge box keeps a class ...
        gt[0, 1, 3] = 0.0                                             # ... and has dx = 0: nothing valid
    return gt


def head_map(seed, ncls, tb, inds, masks):
    """(B, H*W, 12): random regression columns, the valid slots' cells near their targets (the IoUs are not all zero), one
    prediction equal to its target, logits beyond the clamp; NaN in the columns a narrow head leaves unwritten."""
    rng = np.random.default_rng(seed)
    head = (rng.standard_normal((B, H * W, 12)) * 0.5).astype(np.float32)
    head[:, :, 9:] = (rng.standard_normal((B, H * W, 3)) * 3.0).astype(np.float32)
    exact = None
    for b in range(B):
        for k in range(NMAX):
            if masks[b, k]:
                head[b, inds[b, k], 0:8] = tb[b, k] + (rng.standard_normal(8) * 0.08).astype(np.float32)
                head[b, inds[b, k], 8] = rng.uniform(-0.2, 1.0)
    for b in range(B):                       # the last slot whose cell no other slot shares
        for k in range(NMAX):
            if masks[b, k] and (inds[b][masks[b] > 0] == inds[b, k]).sum() == 1:
                exact = (b, k)
    if exact is not None:
        head[exact[0], inds[exact], 0:8] = tb[exact]
    for b in range(B):                       # the clamp region: at positives and at negatives, both signs
        cells = rng.choice(H * W, 12, replace=False)
        head[b, cells[:6], 9:9 + ncls] = 12.0
        head[b, cells[6:], 9:9 + ncls] = -12.0
        for k in range(min(NMAX, 4)):
            if masks[b, k]:
                head[b, inds[b, k], 9:9 + ncls] = 11.0 if k % 2 else -11.0
    head[:, :, 9 + ncls:] = np.nan
    return head


def reference_iou3d():
    from oracle import cref
    torch.cuda.FloatTensor = torch.FloatTensor

    def overlap_stub(a, b, out):
        out.copy_(torch.from_numpy(cref.boxes_overlap_bev(a.numpy().astype(np.float32), b.numpy().astype(np.float32))))
        return 1
    ext = types.ModuleType('detzero_utils.ops.iou3d_nms.iou3d_nms_cuda')
    ext.boxes_overlap_bev_gpu = overlap_stub
    sys.modules[ext.__name__] = ext
    sys.modules['detzero_utils.ops.iou3d_nms'].iou3d_nms_cuda = ext
    sys.modules['detzero_utils.common_utils'].check_numpy_to_torch = None
    return gg._load('ref_iou3d_nms_utils', gg.REF + '/utils/detzero_utils/ops/iou3d_nms/iou3d_nms_utils.py')


def run_case(mods, tag, each_head, iou_weight, empty, out):
    from detzero_amd.config import centerpoint_1sweep_cfg
    cfg = centerpoint_1sweep_cfg()
    hcfg = cfg.MODEL.DENSE_HEAD
    hcfg.CLASS_NAMES_EACH_HEAD = each_head
    hcfg.IOU_WEIGHT = iou_weight
    hcfg.SHARED_CONV_CHANNEL = 8
    hcfg.TARGET_ASSIGNER_CONFIG.NUM_MAX_OBJS = NMAX
    if iou_weight <= 0:
        hcfg.SEPARATE_HEAD_CFG.HEAD_ORDER = ['center', 'center_z', 'dim', 'rot']      # center_head.py:280-283 needs eight columns
    rng32 = np.array(RANGE, np.float32)
    head = mods['center_head'].CenterHead(hcfg, 8, 3, NAMES, np.array([W * STRIDE, H * STRIDE, 40]), rng32, VOXEL)
    gt = gt_case(empty)
    tgt = head.assign_targets(torch.from_numpy(gt).clone(), feature_map_size=torch.Size([H, W]))
    lw = hcfg.LOSS_CONFIG.LOSS_WEIGHTS
    weights = (lw['cls_weight'], lw['loc_weight'], *lw['code_weights'], iou_weight)
    out[tag + '_gt_boxes'] = gt
    out[tag + '_iou_weight'] = np.float64(iou_weight)
    preds, leaves, recs64, grads64 = [], [], [], []
    for i, names in enumerate(head.class_names_each_head):
        t = {k: tgt[k][i].numpy() for k in ('heatmaps', 'target_boxes', 'inds', 'masks')}
        hm = head_map(100 + 7 * i + len(tag), len(names), t['target_boxes'], t['inds'], t['masks'])
        img = torch.from_numpy(np.nan_to_num(hm)).view(B, H, W, 12).permute(0, 3, 1, 2)
        leaf = {n: img[:, o:o + (len(names) if n == 'hm' else c)].clone().contiguous().requires_grad_(True) for n, (o, c) in COLS.items()}
        leaves.append(leaf)
        preds.append(dict(leaf))
        for k, v in t.items():
            out['%s_h%d_%s' % (tag, i, k)] = v
        out['%s_h%d_head' % (tag, i)] = hm
        rec, g64 = hr.losses(np.nan_to_num(hm), t['heatmaps'], t['target_boxes'], t['inds'], t['masks'], weights, H, W, STRIDE, RANGE, VOXEL)
        recs64.append(rec)
        grads64.append(g64)
    head.forward_ret_dict = {'pred_dicts': preds, 'target_dicts': tgt}
    loss, tb = head.get_loss()
    loss.backward()
    tb64 = hr.tb_dict_of(recs64, iou_weight)
    assert sorted(tb) == sorted(tb64), (sorted(tb), sorted(tb64))
    assert abs(float(loss) - tb['rpn_loss']) == 0
    for k, v in tb.items():
        out['%s_tb_%s' % (tag, k)] = np.float64(v)
        out['%s_dist_%s' % (tag, k)] = np.float64(abs(v - tb64[k]) / abs(tb64[k]) if tb64[k] != 0 else abs(v))
    for i, leaf in enumerate(leaves):
        ncls = leaf['hm'].shape[1]
        g = np.zeros((B, H * W, 12), np.float32)
        for n, (o, c) in COLS.items():
            if leaf[n].grad is not None:
                c = ncls if n == 'hm' else c
                g[:, :, o:o + c] = leaf[n].grad.permute(0, 2, 3, 1).reshape(B, H * W, c).numpy()
        out['%s_h%d_grad' % (tag, i)] = g
        peak = np.abs(grads64[i]).max(axis=(0, 1))
        out['%s_h%d_dist_grad' % (tag, i)] = np.abs(g - grads64[i]).max(axis=(0, 1)) / np.where(peak > 0, peak, 1.0)
    print(tag, {k: '%.6g (%.1e)' % (v, out['%s_dist_%s' % (tag, k)]) for k, v in tb.items()})
    print(tag, 'masks', [int(m.sum()) for m in tgt['masks']], 'grad dist', [out['%s_h%d_dist_grad' % (tag, i)].max() for i in range(len(leaves))])


def main():
    mods = gg.install_stubs()
    ch = mods['center_head']
    ch.loss_utils = gg._load('detzero_det.utils.loss_utils', gg.REF + '/detection/detzero_det/utils/loss_utils.py')
    ch.iou3d_nms_utils = types.SimpleNamespace(boxes_iou3d_gpu=reference_iou3d().boxes_iou3d_gpu)
    out = {'geometry': np.array([W, H, NMAX, B, STRIDE], np.int64), 'range': np.array(RANGE, np.float64), 'voxel': np.array(VOXEL, np.float64)}
    run_case(mods, 'c1', [NAMES], 1, False, out)
    run_case(mods, 'c2', [['Vehicle'], ['Pedestrian', 'Cyclist']], 1, False, out)
    run_case(mods, 'c3', [NAMES], 1, True, out)
    run_case(mods, 'c4', [NAMES], 0, False, out)
    path = os.path.join(HERE, 'head_loss_golden.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
