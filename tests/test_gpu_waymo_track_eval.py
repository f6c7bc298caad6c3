"""GPU, end to end: dz_mot_weights against the restatement's weights, WaymoTrackingMetricsEstimator.waymo_evaluation and the command
line on the synthetic sequences of tests/mot_eval_cases.py against the float64 restatement (tests/mot_eval_ref.py), and one short
sequence through DetZeroTracker.forward and the evaluation.

Tolerances.  The weights are the values of dz_boxes_pairwise_metric's DZ_BOXM_IOU3D / the rotated BEV IoU (the same pair body,
csrc/box_geom.h); the restatement's IoU is tests/track_ref.iou3d / oracle.cref.boxes_iou_bev.  tests/test_gpu_box_ops.py holds
DZ_BOXM_IOU3D to the device's own composition bit for bit and grants nothing against this restatement; the tolerance the suite
grants these very kernels against this very restatement is tests/test_gpu_traj_pair.py:33-34 (BEV_TOL = 2e-5, IOU3D_TOL = 2e-5 + 8
* 2^-24, applied per pair at :302-322), and that is what is used here, per pair for the weights and - MOTP being a mean over pairs
of 1 - w - for MOTP.  The scenes keep every IoU 1e-4 from its threshold and every matching stable under +-1e-5 (checked on the CPU
for every seed), so the integer counts are asked to be equal.
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import mot_eval_cases as cases
from tests import mot_eval_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASS_NAMES = ['Vehicle', 'Pedestrian', 'Sign', 'Cyclist']
TOL = {'3d': 2e-5 + 8 * 2.0 ** -24, 'bev': 2e-5}                 # tests/test_gpu_traj_pair.py:33-34 (IOU3D_TOL, BEV_TOL)


@pytest.fixture(scope='module')
def dataset():
    s = cases.scene(cases.SEEDS[0])
    pds, gts = cases.infos_of(s)
    return s, pds, gts


@pytest.fixture(scope='module')
def expected(dataset):
    """{(config, box type)}: (the restatement's table, its metrics) - computed once per key, read-only.  With the BEV box type the
    conversion is the same (the tracking mirror keeps 7-dof boxes; only the IoU changes)."""
    from detzero_amd.waymo_eval import breakdown_names
    s = dataset[0]
    out = {}

    def get(config_type, box_type='3d'):
        key = (tuple(config_type), box_type)
        if key not in out:
            table = ref.counts(config_type, box_type, s)
            table.setflags(write=False)
            out[key] = (table, ref.metrics(table, breakdown_names(config_type)))
        return out[key]
    return get


@pytest.mark.parametrize('box_type', ['3d', 'bev'])
def test_weights_against_the_restatement(device, dataset, box_type):
    import torch
    from detzero_amd import ops
    probs = ref.problems(['object', 'range'], box_type, dataset[0])
    w, cut, pid, gid, gd, pdesc, cdesc, frames = cases.device_inputs(probs)
    pdesc6, w_len = ops.mot_problem_desc(pdesc)
    pb = torch.from_numpy(np.concatenate([p['pb'] for p in probs])).to(device)
    gb = torch.from_numpy(np.concatenate([p['gb'] for p in probs])).to(device)
    ps = torch.from_numpy(np.concatenate([p['score'] for p in probs])).to(device)
    got_w, got_cut = ops.mot_weights(pb, ps, gb, pdesc6, w_len, box_type)
    got_w, got_cut = got_w.cpu().numpy(), got_cut.cpu().numpy()
    assert got_w.dtype == np.float32 and got_w.shape == w.shape and np.array_equal(got_cut, cut)
    assert {0, 50, 100} <= set(got_cut.tolist())                                # the scores exactly on c_0, c_50, c_100
    want = np.concatenate([p['w'].reshape(-1) for p in probs])
    assert np.array_equal(got_w > 0, want > 0) and (want > 0).sum() > 200
    worst = float(np.abs(got_w.astype(np.float64) - want).max())
    print('\n[mot] weights %s: %d pairs, %d non-zero, worst |device - restatement| %.2e (tolerance %.2e)' % (
        box_type, want.size, int((want > 0).sum()), worst, TOL[box_type]))
    assert worst <= TOL[box_type]


def _check(got, table_metrics, tol):
    want = table_metrics[1]
    assert list(got) == list(want)
    for key in want:
        assert isinstance(got[key], list) and len(got[key]) == 1
        if key.endswith('/MOTP'):
            assert abs(got[key][0] - want[key][0]) <= tol, (key, got[key], want[key])
        else:                                                                   # ratios of equal integers, computed alike
            assert abs(got[key][0] - want[key][0]) <= 1e-12, (key, got[key], want[key])
    assert max(v[0] for k, v in want.items() if k.endswith('MISMATCH')) > 0 and max(v[0] for k, v in want.items() if k.endswith('MOTA')) > 0.3


@pytest.mark.parametrize('box_type', ['3d', 'bev'])
def test_waymo_evaluation_matches_the_restatement(device, dataset, expected, box_type):
    from detzero_amd import waymo_eval_tracking as wt
    s, pds, gts = dataset
    est = wt.WaymoTrackingMetricsEstimator()
    config = ['object', 'range']
    # the integer counts, on the estimator's own arrays
    arrays = wt.chain_arrays(config, *est.waymo_arrays(pds, gts, CLASS_NAMES, fake_gt_infos=False))
    table = wt.chain_counts(arrays, box_type=box_type)
    want = expected(config, box_type)[0]
    assert np.array_equal(table[..., :4], want[..., :4])
    pairs = np.maximum(want[..., 0], 1)
    assert (np.abs(table[..., 4] - want[..., 4]) / 4294967296.0 <= TOL[box_type] * pairs).all()
    for mapping in ('workgroup',):
        assert np.array_equal(wt.chain_counts(arrays, box_type=box_type, mapping=mapping), table)
    assert np.array_equal(wt.chain_counts(arrays, box_type=box_type, cap=1), table)               # one sequence per group
    # the result dict
    got = est.waymo_evaluation(pds, gts, CLASS_NAMES, config + [box_type], fake_gt_infos=False)
    _check(got, expected(config, box_type), TOL[box_type])
    assert len(got) == 16 * 2 * 5 and list(got)[:5] == ['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_1/' + m for m in ('MOTA', 'MOTP', 'MISS', 'MISMATCH', 'FP')]
    if box_type == '3d':
        _check(est.waymo_evaluation(pds, gts, CLASS_NAMES, ['object'], fake_gt_infos=False), expected(['object']), TOL['3d'])


def test_command_lines_in_a_child_process(device, dataset, expected, tmp_path):
    """detzero_eval.py's arguments: the tracks in shuffled frame order, ground truth in info form (the file's own
    arguments are checked without a device in tests/test_waymo_track_eval_cpu.py)."""
    _, pds, gts = dataset
    order = np.random.RandomState(3).permutation(len(pds))
    det_path, gt_path = str(tmp_path / 'result.pkl'), str(tmp_path / 'infos.pkl')
    with open(det_path, 'wb') as f:
        pickle.dump([pds[i] for i in order], f)
    with open(gt_path, 'wb') as f:
        pickle.dump(gts, f)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    res = subprocess.run([sys.executable, '-m', 'detzero_amd.waymo_eval_tracking', '--det_result_path', det_path, '--gt_info_path', gt_path,
                          '--evaluate_metrics', 'object', 'range', '--class_name'] + CLASS_NAMES,
                         cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stdout
    for word in ('Category', 'MOTA', 'MOTP', 'MISS', 'MISMATCH', 'FP', 'Pedestrain', 'Vehicle_[30, 50)'):
        assert word in res.stdout, word
    want = expected(['object', 'range'])[1]
    log = open(str(tmp_path / 'mAP.txt')).read()
    for key, value in want.items():
        if not key.endswith('/MOTP'):
            assert '%s: %.4f ' % (key, value[0]) in res.stdout and '%s: %.4f ' % (key, value[0]) in log, key


def test_a_tracked_sequence_end_to_end(device):
    """Five objects on straight lines, detected where they are: DetZeroTracker.forward, its tracks as prediction infos, the
    generating boxes as ground truth.  Where the tracker kept one id per object (asserted on its output) no mismatch is counted."""
    import copy
    from detzero_amd import waymo_eval_tracking as wt
    from detzero_amd.track_models import DetZeroTracker
    from tests.track_seq_ref import load_sequence
    model = load_sequence(0)[1]
    rng = np.random.RandomState(5)
    n_frames, names = 12, ['Vehicle', 'Vehicle', 'Vehicle', 'Pedestrian', 'Pedestrian']
    size = {'Vehicle': (4.6, 2.0, 1.7), 'Pedestrian': (0.9, 0.8, 1.75)}
    start = np.array([[10.0, 0.0], [-15.0, 12.0], [25.0, -20.0], [5.0, 18.0], [-8.0, -14.0]])
    vel = np.array([[0.8, 0.0], [0.0, 0.6], [-0.7, 0.0], [0.1, 0.05], [0.0, -0.1]])
    truth = np.zeros((n_frames, 5, 7), dtype=np.float32)
    for f in range(n_frames):
        for i, name in enumerate(names):
            truth[f, i] = [start[i, 0] + vel[i, 0] * f, start[i, 1] + vel[i, 1] * f, 0.5, *size[name], np.arctan2(vel[i, 1], vel[i, 0])]
    seq = {str(f): {'boxes_global': truth[f] + rng.uniform(-0.02, 0.02, (5, 7)).astype(np.float32) * np.array([1, 1, 1, 0, 0, 0, 0], np.float32),
                    'name': np.array(names, dtype='<U10'), 'score': np.full((5,), 0.9, np.float32), 'num_points': np.full((5,), 50, np.int32),
                    'pose': np.eye(4)} for f in range(n_frames)}
    tracks = DetZeroTracker(model).forward(copy.deepcopy(seq))
    pds = [{'boxes_lidar': [], 'score': [], 'name': [], 'obj_ids': [], 'sequence_name': 'walk', 'frame_id': f} for f in range(n_frames)]
    for tid, tk in tracks.items():
        for row, f in enumerate(tk['sample_idx']):
            p = pds[int(f)]
            p['boxes_lidar'].append(tk['boxes_global'][row, :7]); p['score'].append(tk['score'][row]); p['name'].append(tk['name'][row])
            p['obj_ids'].append(int(tk['obj_ids'][row]))
    for p in pds:
        p['boxes_lidar'] = np.array(p['boxes_lidar'], dtype=np.float32).reshape(-1, 7)
        p['score'], p['name'], p['obj_ids'] = np.array(p['score'], dtype=np.float32), np.array(p['name'], dtype='<U10'), np.array(p['obj_ids'], dtype=np.int64)
    gts = [{'sequence_name': 'walk', 'frame_id': f, 'annos': {'gt_boxes_lidar': truth[f], 'name': np.array(names, dtype='<U10'),
            'difficulty': np.ones((5,), np.int32), 'num_points_in_gt': np.full((5,), 50, np.int64), 'obj_ids': np.array(['a', 'b', 'c', 'd', 'e'])}}
           for f in range(n_frames)]
    # the tracker's own ids: the nearest track box to every object in every frame, and one id per object over the whole walk
    kept = True
    for i in range(5):
        ids = set()
        for f in range(n_frames):
            d = np.linalg.norm(pds[f]['boxes_lidar'][:, :2] - truth[f, i, :2], axis=1) if len(pds[f]['boxes_lidar']) else np.array([9.0])
            if d.min() < 0.5:
                ids.add(int(pds[f]['obj_ids'][int(np.argmin(d))]))
        kept = kept and len(ids) == 1
    assert kept, 'the tracker changed an id on straight, isolated walks'
    got = wt.WaymoTrackingMetricsEstimator().waymo_evaluation(pds, gts, ['Vehicle', 'Pedestrian'], ['object'], fake_gt_infos=False)
    for t in ('VEHICLE', 'PEDESTRIAN'):
        assert got['OBJECT_TYPE_TYPE_%s_LEVEL_1/MISMATCH' % t] == [0.0] and got['OBJECT_TYPE_TYPE_%s_LEVEL_2/MISMATCH' % t] == [0.0]
        print('\n[mot] tracked walk %s: MOTA %.4f MOTP %.4f' % (t, got['OBJECT_TYPE_TYPE_%s_LEVEL_1/MOTA' % t][0], got['OBJECT_TYPE_TYPE_%s_LEVEL_1/MOTP' % t][0]))
        assert 0.5 < got['OBJECT_TYPE_TYPE_%s_LEVEL_1/MOTA' % t][0] <= 1.0      # every object is detected where it is, in every frame
    assert got['OBJECT_TYPE_TYPE_CYCLIST_LEVEL_1/MOTA'] == [0.0]


@pytest.mark.parametrize('side,seq', [('pd', 2), ('gt', 2), ('pd', None), ('gt', None)],
                         ids=['last-sequence-without-predictions', 'last-sequence-without-ground-truth', 'no-predictions', 'no-ground-truth'])
def test_an_empty_side_through_waymo_evaluation(device, dataset, side, seq):
    """A sequence one side has nothing of, and a side with nothing at all, through the public call.  Dropping every prediction
    gives MOTA = 0 and MISS = 1 wherever there is ground truth; dropping every ground truth gives zeros (N = 0)."""
    from detzero_amd import waymo_eval_tracking as wt
    from detzero_amd.waymo_eval import breakdown_names
    s = cases.without(dataset[0], side, seq)
    pds, gts = cases.infos_of(s)
    config = ['object', 'range']
    got = wt.WaymoTrackingMetricsEstimator().waymo_evaluation(pds, gts, CLASS_NAMES, config, fake_gt_infos=False)
    table = ref.counts(config, '3d', s)
    want = ref.metrics(table, breakdown_names(config))
    assert list(got) == list(want)
    for key in want:
        assert abs(got[key][0] - want[key][0]) <= (TOL['3d'] if key.endswith('/MOTP') else 1e-12), (key, got[key], want[key])
    if seq is None:
        for name in breakdown_names(config):
            for lv in (1, 2):
                values = [got['%s_LEVEL_%d/%s' % (name, lv, m)][0] for m in ('MOTA', 'MOTP', 'MISS', 'MISMATCH', 'FP')]
                n = int(table[breakdown_names(config).index(name), lv - 1, 0, [0, 2]].sum())
                assert values == ([0.0, 0.0, 1.0, 0.0, 0.0] if side == 'pd' and n > 0 else [0.0] * 5), (name, lv, values)
        assert side == 'gt' or got['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_2/MISS'] == [1.0]
    else:
        assert got['OBJECT_TYPE_TYPE_PEDESTRIAN_LEVEL_2/MISMATCH'][0] > 0


@pytest.mark.parametrize('box_type', ['3d', 'bev'])
def test_one_frame_sequences_count_as_detection(device, box_type):
    """Where every sequence is one frame, no pair is carried and no mismatch can occur: the tracking table's [TP, FP, MISS] is the
    detection table's [TP, FP, FN] at every shard, level and cutoff, both from the device (tests/test_waymo_track_eval_cpu.py holds
    the two restatements to the same identity on this scene)."""
    import torch
    from detzero_amd import ops, waymo_eval
    from tests import waymo_eval_cases as det_cases
    det = det_cases.scene(*det_cases.SCENES[0])
    config = ['object', 'range']
    arrays = waymo_eval.problem_arrays(config, *det_cases.flat(det))
    want = waymo_eval.match_counts(config, det['n_frames'], *arrays, box_type=box_type, device=device)      # ops.eval_match_counts
    probs = ref.problems(config, box_type, cases.one_frame_sequences(det))
    _, _, pid, gid, gd, pdesc, cdesc, frames = cases.device_inputs(probs)
    pdesc6, w_len = ops.mot_problem_desc(pdesc)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    w, cut = ops.mot_weights(t(np.concatenate([p['pb'] for p in probs])), t(np.concatenate([p['score'] for p in probs])),
                             t(np.concatenate([p['gb'] for p in probs])), pdesc6, w_len, box_type)
    got = ops.mot_chain_counts(w, cut, t(pid), t(gid), t(gd), pdesc6, cdesc, frames, 16)
    assert got.shape[:3] == want.shape[:3] == (16, 2, 101) and want[..., 0].max() > 0 and want[..., 1].max() > 0
    assert np.array_equal(got[..., :3], want[..., :3]) and not got[..., 3].any()
