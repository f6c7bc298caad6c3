"""Timing of the refiner's recall record on one GPU (development / DESIGN.md 7i numbers): PositionRefineModel.generate_recall_record
on 1024 tracks of up to 200 boxes, against the composition a user of this library had before dz_track_recall_iou3d - the
reference's per-track loop (position_refine_model.py:100-133: two `boxes_iou3d_gpu(a, b).diag()` and the `.item()` calls around
them) through iou3d_nms_utils.boxes_iou3d_gpu.  Median of 20 calls after warm-up, host time including the final
synchronisation; both paths must give the same recall dict."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from detzero_amd import iou3d_nms_utils                                                          # noqa: E402
from detzero_amd.refine_models import PositionRefineModel, _empty_recall_dict                    # noqa: E402
from detzero_amd.synth import synth_boxes                                                        # noqa: E402

TRACKS, T_CAP, THRESH = 1024, 200, [0.7]


def batch(dev):
    rng = np.random.default_rng(5)
    lens = rng.integers(1, T_CAP + 1, TRACKS)
    lens[:64] = T_CAP
    traj = np.zeros((TRACKS, T_CAP, 7), np.float32)
    for i, n in enumerate(lens):
        traj[i, :n] = synth_boxes(1000 + i, int(n), near_duplicates=0.0)
    gt = traj.copy()
    gt[..., :3] += rng.normal(0, 1, gt[..., :3].shape).astype(np.float32) * np.where(rng.random((TRACKS, T_CAP, 1)) < 0.5, 0.05, 0.5).astype(np.float32)
    pred = gt.copy()
    pred[..., :3] += rng.normal(0, 0.1, pred[..., :3].shape).astype(np.float32)
    matched = [rng.random(n) < 0.8 for n in lens]
    for m in matched:
        m[0] = True
    data = {'pos_trajectory': torch.from_numpy(traj).to(dev), 'gt_pos_trajectory': torch.from_numpy(gt).to(dev), 'box_num': lens.tolist(),
            'state': ['dynamic' if i % 2 else 'static' for i in range(TRACKS)], 'matched': matched,
            'matched_tracklet': [bool(i % 16) for i in range(TRACKS)]}
    return data, torch.from_numpy(pred).to(dev)


def per_track_loop(box_preds, data, thresh_list):
    """The reference's loop on the existing wrapper; returns (recall dict, host synchronisations)."""
    rec, syncs = _empty_recall_dict(thresh_list), 0
    traj, gt_traj, box_num, states = data['pos_trajectory'], data['gt_pos_trajectory'], data['box_num'], data['state']
    ious, frac, gt_num = ([], []), ([], []), 0
    for idx in range(len(box_num)):
        if not data['matched_tracklet'][idx]:
            continue
        m = torch.from_numpy(data['matched'][idx])
        n = box_num[idx]
        obj_len = m.sum().item()
        gt_num += obj_len
        per = (iou3d_nms_utils.boxes_iou3d_gpu(traj[idx][:n, 0:7][m], gt_traj[idx][:n, 0:7][m]).diag(),
               iou3d_nms_utils.boxes_iou3d_gpu(box_preds[idx, :n, 0:7][m], gt_traj[idx][:n, 0:7][m]).diag())
        rec[states[idx]] += obj_len
        for s, side in enumerate(('input', 'output')):
            ious[s].append(per[s])
            frac[s].append((per[s] > thresh_list[0]).sum().item() / obj_len)
            syncs += 1
            for th in thresh_list:
                rec['Box level %s (%s) %s' % (side, states[idx], th)] += (per[s] > th).sum().item()
                syncs += 1
    mth = np.array(data['matched_tracklet'])
    for s, side in enumerate(('input', 'output')):
        tk, box = torch.Tensor(frac[s]), torch.cat(ious[s])
        for i, state in enumerate(np.array(states)[mth]):
            for th in thresh_list:
                rec['Track level %s (%s) %s' % (side, state, th)] += int(tk[i] >= 0.7)
        for th in thresh_list:
            rec['Box level %s %s' % (side, th)] += (box > th).sum().item()
            rec['Track level %s %s' % (side, th)] += (tk > th).sum().item()
            syncs += 1
    rec['Box num'] += gt_num
    rec['Track num'] += int(mth.sum())
    return rec, syncs


def median_ms(fn, calls=20, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    dev = torch.device('cuda', 0)
    data, pred = batch(dev)
    new = PositionRefineModel.generate_recall_record(pred, {}, data, THRESH)
    old, syncs = per_track_loop(pred, data, THRESH)
    assert new == old, sorted((k, new[k], old[k]) for k in new if new[k] != old[k])
    boxes = int(new['Box num'])
    ms_new = median_ms(lambda: PositionRefineModel.generate_recall_record(pred, {}, data, THRESH))
    ms_old = median_ms(lambda: per_track_loop(pred, data, THRESH), calls=20, warmup=1)
    print('PRM recall record, %d tracks x up to %d boxes (%d matched boxes in %d tracks), thresholds %s' % (TRACKS, T_CAP, boxes, new['Track num'], THRESH))
    print('  dz_track_recall_iou3d path : %8.2f ms per call, 1 launch + 1 table fill, 1 device-to-host copy (the only synchronisation)' % ms_new)
    print('  per-track .diag() loop     : %8.2f ms per call, %d matrix launches, %d host synchronisations (.item())' % (
        ms_old, 2 * int(new['Track num']), syncs))
    print('  ratio %.1fx; recall dicts identical' % (ms_old / ms_new))


if __name__ == '__main__':
    main()
