"""Time CenterHead's device targets + losses (csrc/head_loss.hip) against the host target assignment they replace.

    python tools/bench_head_loss.py [--frames 32] [--boxes 100] [--repeat 20] [--host-repeat 3]

Workload: --frames frames of the 188 x 188 map of the shipped configuration, one head with three classes, about --boxes seeded
boxes per frame (plus padding rows), NUM_MAX_OBJS 500.  Prints one JSON line:
  - host_targets_ms: `target_assign.assign_targets` (the host route, unchanged by the device route) on the same batch, gt_boxes on
    the device as the dense head receives them, wall time ending in a device synchronise, best of --host-repeat;
  - device_targets_ms / device_loss_ms / device_all_ms: `ops.centerhead_targets`, `ops.centerhead_loss_nosync` with the gradient
    buffer, and both together: device events around --repeat back-to-back calls after a warm-up, per call;
  - ratio: host_targets_ms / device_all_ms;
  - the records of both target routes fed to the same loss call (they agree to the last bits of float32 or the line says so).
Needs a GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch(frames, boxes, seed=11):
    rng = np.random.default_rng(seed)
    m = boxes + boxes // 8
    gt = np.zeros((frames, m, 8), np.float32)
    size = np.array([[4.6, 2.0, 1.7], [0.9, 0.8, 1.75], [1.8, 0.8, 1.6]])
    for f in range(frames):
        n = int(rng.integers(boxes - boxes // 10, boxes + boxes // 10 + 1))
        cls = rng.choice([1, 2, 3], n, p=[0.6, 0.3, 0.1])
        gt[f, :n, 0:2] = rng.uniform(-75, 75, (n, 2))
        gt[f, :n, 2] = rng.uniform(-1, 2, n)
        gt[f, :n, 3:6] = size[cls - 1] * rng.uniform(0.8, 1.25, (n, 3))
        gt[f, :n, 6] = rng.uniform(-np.pi, np.pi, n)
        gt[f, :n, 7] = cls
    return gt


def device_ms(fn, repeat):
    fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(repeat):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / repeat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--boxes', type=int, default=100)
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--host-repeat', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_head_loss: needs a GPU')
    from detzero_amd import ops
    from detzero_amd.config import centerpoint_1sweep_cfg
    from detzero_amd.det_modules import CenterHead
    from detzero_amd.head_loss import loss_weights
    from detzero_amd.target_assign import assign_targets
    dev = torch.device('cuda', 0)
    cfg = centerpoint_1sweep_cfg()
    hcfg = cfg.MODEL.DENSE_HEAD
    pc_range, voxel = cfg.DATA_CONFIG.POINT_CLOUD_RANGE, [0.1, 0.1, 0.15]
    head = CenterHead(hcfg, 512, 3, cfg.CLASS_NAMES, np.array([1504, 1504, 40]), pc_range, voxel)
    h = w = 188
    gt = torch.from_numpy(batch(args.frames, args.boxes)).to(dev)
    torch.manual_seed(0)
    head_map = torch.randn((args.frames, h * w, 12), device=dev)
    head_map[:, :, 9:] = head_map[:, :, 9:] * 2 - 3
    weights = loss_weights(hcfg)
    tcfg = hcfg.TARGET_ASSIGNER_CONFIG

    def dev_targets():
        return ops.centerhead_targets(gt, [1, 2, 3], 3, h, w, tcfg.FEATURE_MAP_STRIDE, pc_range, voxel, tcfg.NUM_MAX_OBJS, tcfg.GAUSSIAN_OVERLAP,
                                      tcfg.MIN_RADIUS)

    def dev_loss(t):
        return ops.centerhead_loss_nosync(head_map, *t, h, w, weights, tcfg.FEATURE_MAP_STRIDE, pc_range, voxel, want_grad=True)

    host_ms = []
    for _ in range(args.host_repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = assign_targets(head, gt, (h, w))
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    tgt = dev_targets()
    res = {
        'workload': {'frames': args.frames, 'map': [h, w], 'classes': 3, 'boxes_per_frame': args.boxes, 'valid_slots': int(tgt[4][1].item()),
                     'num_max_objs': tcfg.NUM_MAX_OBJS},
        'host_targets_ms': round(min(host_ms), 3), 'host_targets_ms_all': [round(v, 3) for v in host_ms],
        'device_targets_ms': round(device_ms(dev_targets, args.repeat), 4),
        'device_loss_ms': round(device_ms(lambda: dev_loss(tgt), args.repeat), 4),
        'device_all_ms': round(device_ms(lambda: dev_loss(dev_targets()), args.repeat), 4),
    }
    res['ratio'] = round(res['host_targets_ms'] / res['device_all_ms'], 1)
    rec_dev = dev_loss(tgt)[0].cpu().numpy()
    rec_host = dev_loss((host['heatmaps'][0], host['target_boxes'][0], host['inds'][0], host['masks'][0], None))[0].cpu().numpy()
    res['total_device_targets'], res['total_host_targets'] = float(rec_dev[11]), float(rec_host[11])
    res['records_rel_diff'] = float(np.abs(rec_dev - rec_host).max() / np.abs(rec_host).max())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
