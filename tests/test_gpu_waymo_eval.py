"""GPU, end to end: WaymoDetectionMetricsEstimator.waymo_evaluation, the command line and WaymoDetectionDataset.evaluation on a
12-frame synthetic set (tests/waymo_eval_cases.py, with one ground truth and one prediction per frame beyond the distance mask),
against metrics_from_counts of the float64 restatement's counts (tests/waymo_eval_ref.py).

The AP / APH values are compared to 1e-12.  The restatement's table holds the heading sums as the protocol defines them (every
term times 2^32 rounded to nearest, then added as integers), and the integer counts are equal (tests/test_gpu_eval_match.py), so
the two tables can differ only where the device's double evaluation of a term falls on the other side of a rounding boundary.
With the BEV box type a box has no z (the conversion drops it), so the restatement gets z = 0 for the range bins.
First measured with the restatement on the scene's own (unwrapped) headings: APH differed by up to 4.8e-10, the float32 rounding of
limit_period's wrap in the conversion step; the restatement now reads the converted arrays, as the device does.
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import waymo_eval_cases as cases
from tests import waymo_eval_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASS_NAMES = ['Vehicle', 'Pedestrian', 'Cyclist']              # the Truck / SIGN ground truths are masked out, as by the reference
FAR, DIST = 300.0, 200                                          # every scene object is within 200.5 m, the extra pair is not


@pytest.fixture(scope='module')
def dataset():
    s = cases.scene(*cases.SCENES[0])
    pds, gts = cases.infos_of(s, beyond=FAR)
    return s, pds, gts


@pytest.fixture(scope='module')
def expected(dataset):
    """{config: result dict} from the restatement, on the flat arrays of the conversion step (tests/test_waymo_eval_cpu.py holds
    that step against the reference's own code).  They are the scene's arrays without the type-3 ground truths (not in CLASS_NAMES)
    and the far pair, with the headings wrapped in float32 by limit_period - which is why the scene's own arrays are not used:
    a wrapped float32 heading differs from the unwrapped one by a rounding the heading sums would show."""
    from detzero_amd import waymo_eval
    s, pds, gts = dataset
    out = {}

    def get(config_type, box_type='3d'):
        key = (tuple(config_type), box_type)
        if key not in out:
            with_box = list(config_type) + [box_type]
            pd, gt = waymo_eval.WaymoDetectionMetricsEstimator().waymo_arrays(pds, gts, CLASS_NAMES, with_box, DIST, False)
            keep = s['gt_type'] != 3
            assert np.array_equal(pd[0], s['pd_frame']) and np.array_equal(pd[2], s['pd_type']) and np.array_equal(pd[3], s['pd_score'])
            assert np.array_equal(gt[0], s['gt_frame'][keep]) and np.array_equal(gt[2], s['gt_type'][keep]) and np.array_equal(gt[3], s['gt_diff'][keep])
            cols = [0, 1, 3, 4] if box_type == 'bev' else [0, 1, 2, 3, 4, 5]
            assert np.array_equal(pd[1][:, :-1], s['pd_box'][:, cols]) and np.array_equal(gt[1][:, :-1], s['gt_box'][keep][:, cols])
            assert np.abs(np.angle(np.exp(1j * (pd[1][:, -1].astype(np.float64) - s['pd_box'][:, 6])))).max() < 1e-5

            def box7(b):
                if b.shape[1] == 7:
                    return b
                full = np.zeros((len(b), 7), dtype=np.float32)         # a BEV box has no z: 0, and height 1
                full[:, [0, 1, 3, 4, 6]], full[:, 5] = b, 1.0
                return full
            counts, _, fixed = ref.counts(config_type, box_type, s['n_frames'], pd[0], box7(pd[1]), pd[2], pd[3], gt[0], box7(gt[1]), gt[2], gt[3])
            out[key] = waymo_eval.metrics_from_counts(ref.table_of(counts, fixed), config_type)
        return out[key]
    return get


def _close(got, want):
    assert list(got) == list(want)
    for k in want:
        assert abs(got[k][0] - want[k][0]) <= 1e-12, (k, got[k], want[k])
    assert max(v[0] for v in want.values()) > 0.05


def test_waymo_evaluation_matches_the_restatement(device, dataset, expected):
    from detzero_amd.waymo_eval import WaymoDetectionMetricsEstimator
    _, pds, gts = dataset
    est = WaymoDetectionMetricsEstimator()
    got = est.waymo_evaluation(pds, gts, CLASS_NAMES, ['object', 'range', '3d'], distance_thresh=DIST, fake_gt_infos=False)
    _close(got, expected(['object', 'range']))
    assert got['OBJECT_TYPE_TYPE_SIGN_LEVEL_2/AP'] == [0.0]            # predictions of the type, no ground truth of it
    _close(est.waymo_evaluation(pds, gts, CLASS_NAMES, ['object'], distance_thresh=DIST, fake_gt_infos=False), expected(['object']))
    # without the mask the far pair is one more true positive per frame
    unmasked = est.waymo_evaluation(pds, gts, CLASS_NAMES, ['object'], distance_thresh=1000, fake_gt_infos=False)
    assert unmasked['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_1/AP'][0] > got['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_1/AP'][0]


def test_command_line_in_a_child_process(device, dataset, expected, tmp_path):
    """Predictions in shuffled order with one frame missing; ground truth in info form, keyed by (sequence_name, sample_idx)."""
    _, pds, gts = dataset
    infos = [{'sequence_name': p['sequence_name'], 'sample_idx': p['frame_id'], 'annos': g} for p, g in zip(pds, gts)]
    order = np.random.RandomState(3).permutation(len(pds))
    dets = [pds[i] for i in order if i != 0]                    # frame 0 has no prediction anyway: dropping it changes nothing
    det_path, gt_path = str(tmp_path / 'result.pkl'), str(tmp_path / 'infos.pkl')
    with open(det_path, 'wb') as f:
        pickle.dump(dets, f)
    with open(gt_path, 'wb') as f:
        pickle.dump(infos, f)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    res = subprocess.run([sys.executable, '-m', 'detzero_amd.waymo_eval', '--det_result_path', det_path, '--gt_info_path', gt_path,
                          '--evaluate_metrics', 'object', 'range', '--iou_type', 'bev', '--distance_thresh', str(DIST)],
                         cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stdout
    assert 'seq_0, frame:0 is missed' in res.stdout and 'Vehicle_[30, 50)' in res.stdout
    want = expected(['object', 'range'], 'bev')
    log = open(str(tmp_path / 'mAP.txt')).read()
    for key, value in want.items():
        assert '%s: %.4f ' % (key, value[0]) in res.stdout and '%s: %.4f ' % (key, value[0]) in log, key


def test_dataset_evaluation_with_and_without_the_key(device, dataset, expected):
    from detzero_amd.config import AttrDict
    from detzero_amd.waymo_dataset import WaymoDetectionDataset
    _, pds, gts = dataset
    near = lambda b: np.linalg.norm(b[:, :2], axis=1) < FAR - 1         # evaluation() masks at 1000 m: leave the far pair out here
    pds = [dict(p, boxes_lidar=p['boxes_lidar'][near(p['boxes_lidar'])], score=p['score'][near(p['boxes_lidar'])],
                name=p['name'][near(p['boxes_lidar'])]) for p in pds]
    gts = [{k: v[near(g['gt_boxes_lidar'])] for k, v in g.items()} for g in gts]
    ds = WaymoDetectionDataset.__new__(WaymoDetectionDataset)
    ds.infos = [{'annos': g} for g in gts]
    ds.dataset_cfg = AttrDict({'EVAL_ON_DEVICE': True})
    text, ap = ds.evaluation(pds, CLASS_NAMES)
    want = expected(['object'])
    assert list(ap) == list(want) and all(abs(ap[k] - want[k][0]) <= 1e-12 for k in want)
    assert text.startswith('\n') and 'OBJECT_TYPE_TYPE_VEHICLE_LEVEL_1/AP: %.4f \n' % want['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_1/AP'][0] in text
    ds.dataset_cfg = AttrDict({})
    assert ds.evaluation(pds, CLASS_NAMES) == ('Official Waymo metrics (waymo_open_dataset / TensorFlow) are not provided by the HIP backend', {})


def test_import_through_the_shim_path(device):
    import detzero_amd
    shim = os.path.join(os.path.dirname(os.path.abspath(detzero_amd.__file__)), 'shim')
    sys.path.insert(0, shim)
    try:
        from detzero_det.datasets.waymo.waymo_eval_detection import WaymoDetectionMetricsEstimator
    finally:
        sys.path.remove(shim)
    from detzero_amd import waymo_eval
    assert WaymoDetectionMetricsEstimator is waymo_eval.WaymoDetectionMetricsEstimator
