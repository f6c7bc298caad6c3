"""Time the backward through CenterHead's convolutions (csrc/head_backward.hip, detzero_amd/head_backward.py) on one MI355X.

    python tools/bench_head_backward.py [--frames 1] [--boxes 100] [--repeat 10]

Workload: --frames frames of the 188 x 188 map of the shipped configuration, 512 -> 64 -> 384 -> 12, one head with three classes;
the gradient at the head map is that of a real `ops.centerhead_loss` call on the head's own fp32 forward.  Device events around
--repeat back-to-back calls after a warm-up, per call.  Prints one JSON line:
  - per kernel call: milliseconds, the call's GFLOP (2 * pixels * 9 * cin * cout) and the share of the 157.3 TFLOP/s fp32 matrix
    peak it reaches (the streaming passes have no such figure).  A `wgrad` figure covers the MFMA kernel and the pass that adds
    its chunks' partials; a `dgrad` figure the weight packing (three small tensor ops) and dz_conv2d_forward: the launches
    inside a call are not timed apart here;
  - head_gradients_ms (with and without input_grad) and loss_backward_ms (forward, targets, loss, backward, .grad) end to end;
  - torch_autograd_ms, for orientation only: torch.autograd through torch.nn.functional.conv2d on the same device and shapes
    (float32, the module's own branches), or the reason it did not run.
Nothing here is a pass criterion.  Needs a GPU; there is no CPU fallback.
"""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_head_loss import batch, device_ms  # noqa: E402

PEAK_TFLOPS = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1)
    ap.add_argument('--boxes', type=int, default=100)
    ap.add_argument('--repeat', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_head_backward: needs a GPU')
    from detzero_amd import head_backward as hb
    from detzero_amd import ops
    from detzero_amd.config import centerpoint_1sweep_cfg
    from detzero_amd.det_modules import CenterHead, nchw_to_padded_nhwc
    from detzero_amd.head_loss import device_targets, loss_weights
    dev = torch.device('cuda', 0)
    cfg = centerpoint_1sweep_cfg()
    hcfg = cfg.MODEL.DENSE_HEAD
    pc_range, voxel = cfg.DATA_CONFIG.POINT_CLOUD_RANGE, [0.1, 0.1, 0.15]
    torch.manual_seed(0)
    head = CenterHead(hcfg, 512, 3, cfg.CLASS_NAMES, np.array([1504, 1504, 40]), pc_range, voxel).to(dev).eval()
    head.predict_boxes_when_training = False
    b, h, w, c = args.frames, 188, 188, 64
    x = torch.randn((b, 512, h, w), device=dev) * 0.1
    gt = torch.from_numpy(batch(b, args.boxes)).to(dev)
    concat = nchw_to_padded_nhwc(x)
    p = head.plan()
    hid, fin, shr = p['heads'][0]['hidden'], p['heads'][0]['final'], p['shared']
    shared, hidden, heads = hb.head_forward_f32(head, concat)
    targets = device_targets(head, gt, (h, w))
    _, grad_head = ops.centerhead_loss_nosync(heads[0], targets['heatmaps'][0], targets['target_boxes'][0], targets['inds'][0], targets['masks'][0],
                                              targets['records'][0], h, w, loss_weights(hcfg), head.feature_map_stride, pc_range, voxel, want_grad=True)
    g_hidden, _, _, _ = ops.head_final_backward(grad_head, fin['w'], hidden[0], fin['g_cout'], fin['g_ooff'])
    g_shared_y = ops.conv3x3_dgrad(g_hidden, hid['w'], hid['scale'])
    g_shared, _ = ops.relu_grad(g_shared_y, shared)
    pix = b * h * w
    calls = [
        ('head_final_backward (dgrad + mask + sums, grouped wgrad, bias)', lambda: ops.head_final_backward(grad_head, fin['w'], hidden[0], fin['g_cout'], fin['g_ooff']), None),
        ('wgrad 64 -> 384 (hidden layer)', lambda: ops.conv3x3_wgrad(shared, g_hidden, c, 6 * c), 2.0 * pix * 9 * c * 6 * c),
        ('dgrad 384 -> 64 (hidden layer, dz_conv2d_forward)', lambda: ops.conv3x3_dgrad(g_hidden, hid['w'], hid['scale']), 2.0 * pix * 9 * c * 6 * c),
        ('relu_grad 64 (shared map)', lambda: ops.relu_grad(g_shared_y, shared), None),
        ('wgrad 512 -> 64 (shared layer)', lambda: ops.conv3x3_wgrad(concat, g_shared, 512, c), 2.0 * pix * 9 * 512 * c),
        ('dgrad 64 -> 512 (input_grad, dz_conv2d_forward)', lambda: ops.conv3x3_dgrad(g_shared, shr['w'], shr['scale']), 2.0 * pix * 9 * 512 * c),
    ]
    res = {'workload': {'frames': b, 'map': [h, w], 'channels': [512, c, 6 * c, 12], 'classes': 3, 'boxes_per_frame': args.boxes}, 'kernels': []}
    for name, fn, flop in calls:
        ms = device_ms(fn, args.repeat)
        row = {'call': name, 'ms': round(ms, 4)}
        if flop is not None:
            row['gflop'] = round(flop / 1e9, 2)
            row['share_of_fp32_matrix_peak'] = round(flop / (ms * 1e-3) / (PEAK_TFLOPS * 1e12), 3)
        res['kernels'].append(row)
    state = (shared, hidden, heads)
    res['head_gradients_ms'] = round(device_ms(lambda: hb.head_gradients(head, concat, [grad_head], state=state), args.repeat), 4)
    res['head_gradients_input_grad_ms'] = round(device_ms(lambda: hb.head_gradients(head, concat, [grad_head], input_grad=True, state=state), args.repeat), 4)
    res['head_forward_f32_ms'] = round(device_ms(lambda: hb.head_forward_f32(head, concat), args.repeat), 4)
    data = {'spatial_features_2d': x, 'gt_boxes': gt, 'batch_size': b}
    res['loss_backward_ms'] = round(device_ms(lambda: head.loss_backward(dict(data)), max(args.repeat // 2, 1)), 4)
    head.zero_grad(set_to_none=True)

    # orientation only: torch autograd through torch.nn.functional.conv2d on the same device
    try:
        ref = copy.deepcopy(head)
        gh = grad_head.view(b, h, w, 12).permute(0, 3, 1, 2)

        def autograd_pass():
            ref.zero_grad(set_to_none=True)
            s = ref.shared_conv(x)
            total = 0.0
            for name, (o, n) in head.COLS.items():
                total = total + (getattr(ref.heads_list[0], name)(s) * gh[:, o:o + n]).sum()
            total.backward()

        res['torch_autograd_ms'] = round(device_ms(autograd_pass, max(args.repeat // 2, 1)), 4)
        want = dict(ref.named_parameters())
        got, _ = hb.head_gradients(head, concat, [grad_head], state=state)
        res['torch_autograd_max_rel_diff'] = max(float((got[k] - v.grad).abs().max() / v.grad.abs().max().clamp_min(1e-30)) for k, v in want.items())
    except Exception as e:      # noqa: BLE001  (the orientation figure is optional: say why it is missing)
        res['torch_autograd_ms'] = None
        res['torch_autograd_error'] = '%s: %s' % (type(e).__name__, str(e)[:200])
    print(json.dumps(res))


if __name__ == '__main__':
    main()
