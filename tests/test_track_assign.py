"""CPU: assign mode and tracklet recall - the product's orchestration (detzero_amd.track_assign / track_recall / run_model) on the
numpy restatement of the trajectory-pair ops (tests/traj_ref.py) against the outputs of the reference's own assign_track_target and
TrackRecall.eval_single_seq (tests/golden/track_assign_golden.npz, recorded by gen_track_assign_golden.py).  The kernels' side of
the same orchestration is tests/test_gpu_traj_pair.py."""
import copy
import os
import pickle
import random

import numpy as np
import pytest

from oracle import cref
from tests import traj_ref
from tests.test_track_models import REF_TOOLS, fresh_cfg  # noqa: F401  (fresh_cfg: the shim's global cfg as a tool finds it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = pickle.loads(np.load(os.path.join(ROOT, 'tests', 'golden', 'track_assign_golden.npz'))['pickle'].tobytes())
    return _GOLDEN


def plain(x):
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, list):
        return [plain(v) for v in x]
    return x


def diff(a, b, path='', close=None):
    """Path of the first difference between two nested results, or None: keys in order, lengths, types, every value.  ``close`` =
    {key: tolerance} compares the float arrays stored under those keys within a tolerance instead of exactly."""
    if isinstance(a, dict):
        if not isinstance(b, dict) or list(a.keys()) != list(b.keys()):
            return path + ': keys %s against %s' % (list(a.keys()), list(b.keys()) if isinstance(b, dict) else type(b))
        return next((d for d in (diff(a[k], b[k], '%s/%s' % (path, k), close) for k in a) if d), None)
    if isinstance(a, (list, tuple)):
        if not isinstance(b, (list, tuple)) or len(a) != len(b):
            return path + ': length'
        return next((d for d in (diff(x, y, '%s[%d]' % (path, i), close) for i, (x, y) in enumerate(zip(a, b))) if d), None)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape or a.dtype.kind != b.dtype.kind:
            return '%s: %s %s against %s %s' % (path, a.dtype, a.shape, b.dtype, b.shape)
        key = path.rsplit('/', 1)[-1]
        if close and key in close:
            worst = float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if a.size else 0.0
            return None if worst <= close[key] else '%s: off by %.3g (> %.3g)' % (path, worst, close[key])
        return None if bool(np.all(a == b)) else path + ': values'
    return None if type(a) == type(b) and a == b else '%s: %r against %r' % (path, a, b)


def recall_thr():
    g = golden()
    return dict(zip(g['class_names'], g['recall_thresholds']))


# ------------------------------------------------------------------------------------------------
# the fixture
# ------------------------------------------------------------------------------------------------
def test_fixture_covers_the_scripted_cases_away_from_the_thresholds():
    g = golden()
    assert all(v >= 1e-3 for v in g['gaps'].values()), g['gaps']
    for kind in ('static', 'dynamic', 'unlabel', 'class_change_labelled', 'leaves', 'sign', 'unmatched_gt_l2'):
        assert g['kinds'][kind] >= 1, kind
    assert g['iou_thresholds'] == {'Vehicle': 0.3, 'Pedestrian': 0.1, 'Cyclist': 0.1} and g['recall_thresholds'] == [0.7, 0.5, 0.5]
    assert len(g['sequences']) == 2
    for e in g['sequences']:
        names = e['tracks'][e['class_change']]['name']
        assert len(set(names.tolist())) == 2
        assert all('iou_idx' not in v['track'] and 'iou_idx' not in v['gt'] for v in e['assign']['label'].values())


# ------------------------------------------------------------------------------------------------
# orchestration on the numpy ops against the reference's outputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('si', [0, 1])
def test_assign_on_numpy_ops_reproduces_the_reference(si):
    from detzero_amd.track_assign import assign_track_target
    g = golden()
    e = g['sequences'][si]
    tracks = copy.deepcopy(e['tracks'])
    out = assign_track_target((copy.deepcopy(e['det']), tracks, copy.deepcopy(e['gt'])), g['iou_thresholds'], ops=traj_ref.NumpyTrajOps())
    assert diff(e['assign'], plain(out)) is None
    # the track dicts are reused, not copied (target_assign.py:126-137)
    assert all(v['track'] is tracks[k] for part in ('label', 'unlabel') for k, v in out[part].items())
    assert any(v['track']['iou'].dtype == np.float32 and v['track']['iou'].max() > 0.3 for v in out['label'].values())


@pytest.mark.parametrize('method', ['3d', 'bev'])
@pytest.mark.parametrize('si', [0, 1])
def test_recall_on_numpy_ops_reproduces_the_reference(si, method):
    from detzero_amd.track_recall import TrackRecall
    g = golden()
    e = g['sequences'][si]
    out = TrackRecall.eval_single_seq({'gt': copy.deepcopy(e['gt']), 'pred': copy.deepcopy(e['tracks'])}, g['class_names'], g['difficultys'],
                                      recall_thr(), method, ops=traj_ref.NumpyTrajOps())
    assert diff(e['recall'][method], plain(out)) is None


def _recall_object(tmp_path, seqs):
    """A TrackRecall over files laid out as the reference expects: <root>/data/waymo/waymo_infos_<split>.pkl and a tracking pickle."""
    from detzero_amd.track_recall import TrackRecall
    g = golden()
    (tmp_path / 'data' / 'waymo').mkdir(parents=True)
    infos = [info for e in seqs for info in e['gt'].values()]
    (tmp_path / 'data' / 'waymo' / 'waymo_infos_val.pkl').write_bytes(pickle.dumps(infos))
    pred = tmp_path / 'tracking.pkl'
    pred.write_bytes(pickle.dumps({e['det']['0']['sequence_name']: e['tracks'] for e in seqs}))
    return TrackRecall(str(tmp_path), str(pred), 'val', 4, g['class_names'], difficultys=g['difficultys'], iou_threshold=g['recall_thresholds'],
                       method='3d', ops=traj_ref.NumpyTrajOps())


def test_calculate_tracklet_recall_reproduces_the_reference(tmp_path):
    g = golden()
    recall = _recall_object(tmp_path, g['sequences'])
    assert recall.seq_name_list == ['seq_a', 'seq_b'] and sorted(recall.gt_data) == ['seq_a', 'seq_b']
    for method in ('3d', 'bev'):
        results = {e['det']['0']['sequence_name']: copy.deepcopy(e['recall'][method]) for e in g['sequences']}
        assert diff(g['recall_summary'][method], plain(recall.calculate_tracklet_recall(results))) is None
    # the whole evaluation from the two files, sequences one after another, the table lines logged
    whole = recall.get_tracklet_recall()
    assert whole['method'] == '3d' and whole['iou_thresholds'] == recall_thr()
    assert diff(g['recall_summary']['3d'], {k: plain(v) for k, v in whole.items() if k in g['difficultys']}) is None


# ------------------------------------------------------------------------------------------------
# run_model and the dataset in assign mode
# ------------------------------------------------------------------------------------------------
def _val_dataset(tmp_path, seqs, gt_seqs=None):
    from detzero_amd.config import AttrDict
    from detzero_amd.track_models import build_dataloader
    cfg = AttrDict({'DATASET': 'WaymoTrackDataset', 'DATA_PATH': 'unused', 'PROCESSED_DATA_TAG': 'waymo_processed_data',
                    'CLASS_NAME': ['Vehicle', 'Pedestrian', 'Cyclist'], 'DATA_PROCESSOR': []})
    det = tmp_path / 'result.pkl'
    det.write_bytes(pickle.dumps({e['det']['0']['sequence_name']: copy.deepcopy(e['det']) for e in seqs}))
    if gt_seqs is not None:
        (tmp_path / 'waymo_infos_val.pkl').write_bytes(pickle.dumps([info for e in gt_seqs for info in e['gt'].values()]))
    return build_dataloader(cfg, log_time='20240101-000000', data_path=str(det), batch_size=2, workers=4, split='val', logger=None,
                            root_path=str(tmp_path))


class _FixtureModel:
    """stands in for the tracker: the reference tracker's recorded output of the sequence"""

    def forward(self, seq):
        name = seq['0']['sequence_name']
        return copy.deepcopy(next(e['tracks'] for e in golden()['sequences'] if e['det']['0']['sequence_name'] == name))


def test_run_model_in_assign_mode_writes_the_label_unlabel_pickle(tmp_path):
    from detzero_amd.config import AttrDict
    from detzero_amd.track_models import run_model
    g = golden()
    dataset, loader = _val_dataset(tmp_path, g['sequences'], g['sequences'])
    assert dataset.assign_mode
    cfgs = AttrDict({'REFINING': {'IOU_THRESHOLDS': dict(g['iou_thresholds'])}})
    run_model(_FixtureModel(), loader, dataset, workers=4, cfgs=cfgs, assign_ops=traj_ref.NumpyTrajOps())
    assert dataset.get_track_path() == str(tmp_path / 'tracking' / 'tracking-val-20240101-000000.pkl')
    assert dataset.get_drop_path() == str(tmp_path / 'tracking' / 'drop-val-20240101-000000.pkl')
    written = pickle.load(open(dataset.get_track_path(), 'rb'))
    assert list(written) == ['seq_a', 'seq_b']
    for e in g['sequences']:
        assert diff(e['assign'], plain(written[e['det']['0']['sequence_name']])) is None
    assert sorted(pickle.load(open(dataset.get_drop_path(), 'rb'))) == ['seq_a', 'seq_b']


def test_assign_mode_without_thresholds_is_still_refused():
    from detzero_amd.config import AttrDict
    from detzero_amd.lib import DetZeroHipError
    from detzero_amd.track_models import run_model

    class Dataset:
        assign_mode, split = True, 'train'
    for cfgs in (None, AttrDict({'MODEL': {}}), AttrDict({'REFINING': {}})):
        with pytest.raises(DetZeroHipError, match=r"split 'train'.*assign_track_target.*IOU_THRESHOLDS.*--split test"):
            run_model(None, [], Dataset(), workers=4, cfgs=cfgs)


def test_ground_truth_is_loaded_at_the_first_item_and_checked(tmp_path):
    g = golden()
    dataset, _ = _val_dataset(tmp_path, g['sequences'], None)             # no waymo_infos_val.pkl: the constructor does not open it
    assert dataset.assign_mode and dataset.gt_infos is None
    with pytest.raises(FileNotFoundError):
        dataset[0]
    (tmp_path / 'waymo_infos_val.pkl').write_bytes(pickle.dumps([info for info in g['sequences'][0]['gt'].values()]))
    with pytest.raises(ValueError, match='Ground-truth infomation loading falied.'):      # one sequence of ground truth for two of detections
        dataset[0]
    dataset, _ = _val_dataset(tmp_path, g['sequences'], g['sequences'])
    name, item = dataset[1]
    assert name == 'seq_b' and sorted(item) == ['det_drop', 'detection', 'gt'] and list(item['gt']) == list(g['sequences'][1]['gt'])


@pytest.mark.skipif(not os.path.isdir(REF_TOOLS), reason='the reference tree is not on this machine')
def test_reference_run_track_main_runs_with_split_val_on_the_shim(monkeypatch, tmp_path, fresh_cfg):
    """run_track.py's own main() with --split val: its parser, the shipped yaml (REFINING.IOU_THRESHOLDS included), build_dataloader,
    build_model, run_model's assign branch.  No GPU here: the tracker's and the assignment's ops objects and the overlap function are
    the numpy stand-ins; the kernels' side is tests/test_gpu_traj_pair.py::test_run_model_over_a_result_pickle_in_assign_mode."""
    import glob
    import runpy
    import sys
    from detzero_amd import shim, track_adapter, track_assign, track_models
    from tests import track_ref
    shim.install()
    e = golden()['sequences'][0]
    annos = []
    for f, fr in e['det'].items():
        lidar = track_adapter.transform_boxes3d(fr['boxes_global'], fr['pose'], inverse=True).astype(np.float32)
        annos.append({'sequence_name': fr['sequence_name'], 'frame_id': int(f), 'pose': fr['pose'], 'name': fr['name'], 'score': fr['score'],
                      'boxes_lidar': lidar})
    tools = tmp_path / 'tracking' / 'tools'
    tools.mkdir(parents=True)
    os.symlink(os.path.join(REF_TOOLS, 'cfgs'), tools / 'cfgs')
    det = tmp_path / 'result.pkl'
    det.write_bytes(pickle.dumps(annos))
    (tmp_path / 'data' / 'waymo').mkdir(parents=True)
    (tmp_path / 'data' / 'waymo' / 'waymo_infos_val.pkl').write_bytes(pickle.dumps(list(copy.deepcopy(e['gt']).values())))
    monkeypatch.chdir(tools)                                     # DATA_PATH '../../data/waymo' then lies under tmp_path
    monkeypatch.setattr(track_models, 'HipTrackOps', track_ref.NumpyTrackOps)
    monkeypatch.setattr(track_assign, 'HipTrajOps', traj_ref.NumpyTrajOps)
    monkeypatch.setattr(track_adapter, 'bev_overlap_gpu', cref.boxes_overlap_bev)
    monkeypatch.setattr(sys, 'argv', ['run_track.py', '--cfg_file', 'cfgs/tk_model_cfgs/waymo_detzero_track.yaml', '--data_path', str(det),
                                      '--split', 'val', '--workers', '4'])
    runpy.run_path(os.path.join(REF_TOOLS, 'run_track.py'), run_name='__main__')
    out = glob.glob(str(tmp_path / 'data' / 'waymo' / 'tracking' / 'tracking-val-*.pkl'))
    assert len(out) == 1 and len(glob.glob(str(tmp_path / 'data' / 'waymo' / 'tracking' / 'drop-val-*.pkl'))) == 1
    assigned = pickle.load(open(out[0], 'rb'))
    assert list(assigned) == ['seq_a'] and sorted(assigned['seq_a']) == ['label', 'unlabel']
    label, unlabel = assigned['seq_a']['label'], assigned['seq_a']['unlabel']
    assert len(label) >= 15 and len(unlabel) >= 1               # the object removed from the ground truth cannot be labelled
    for v in label.values():
        tk, gt = v['track'], v['gt']
        assert tk['state'] in ('static', 'dynamic') and tk['iou'].dtype == np.float32 and len(tk['iou']) == len(tk['sample_idx'])
        assert 'iou_idx' not in tk and 'iou_idx' not in gt and gt['gt_boxes_global'].shape[1] == 9
        assert tk['iou'].max() > 0.5 and len(set(gt['obj_ids'].tolist())) == 1


# ------------------------------------------------------------------------------------------------
# shim, refusals, frame order
# ------------------------------------------------------------------------------------------------
def test_shim_exposes_the_assign_and_recall_modules():
    """models/__init__.py:27, tools/eval_track.py:7, target_assign.py:3-5, track_recall.py:10-16."""
    from detzero_amd import shim, track_assign, track_recall
    shim.install()
    from detzero_track.models.tracking_modules import target_assign
    from detzero_track.models.tracking_modules import __all__ as modules
    from detzero_track.utils import track_calculation
    from detzero_track.utils.data_utils import frame_list_to_dict, tracklets_to_frames      # noqa: F401
    from detzero_track.utils.track_recall import TrackRecall
    assert target_assign.assign_track_target is track_assign.assign_track_target and TrackRecall is track_recall.TrackRecall
    assert track_calculation.get_iou_mat_dict is track_assign.get_iou_mat_dict
    assert track_calculation.get_gt_id_data is track_assign.get_gt_id_data
    assert track_calculation.get_trajectory_similarity is track_recall.get_trajectory_similarity
    assert sorted(modules) == ['PostProcessor', 'TrackManager']
    assert 'eval_track.py' in open(os.path.join(os.path.dirname(shim.__file__), '__main__.py')).read()


def test_non_ascending_trajectory_is_refused_by_name():
    from detzero_amd.lib import DetZeroHipError
    from detzero_amd.track_recall import TrackRecall
    g = golden()
    e = g['sequences'][0]
    tracks = copy.deepcopy(e['tracks'])
    tid = next(iter(tracks))
    for key, val in tracks[tid].items():
        if isinstance(val, np.ndarray):
            tracks[tid][key] = val[::-1].copy()
    with pytest.raises(DetZeroHipError, match='track %s is not ascending' % tid):
        TrackRecall.eval_single_seq({'gt': copy.deepcopy(e['gt']), 'pred': tracks}, g['class_names'], g['difficultys'], recall_thr(), '3d',
                                    ops=traj_ref.NumpyTrajOps())
    keys = list(e['gt'])
    gt = {k: copy.deepcopy(e['gt'][k]) for k in keys[1:] + keys[:1]}
    with pytest.raises(DetZeroHipError, match='ground-truth object .* is not ascending'):
        TrackRecall.eval_single_seq({'gt': gt, 'pred': copy.deepcopy(e['tracks'])}, g['class_names'], g['difficultys'], recall_thr(), '3d',
                                    ops=traj_ref.NumpyTrajOps())


def test_unknown_track_class_raises_in_assign():
    from detzero_amd.lib import DetZeroHipError
    from detzero_amd.track_assign import assign_track_target
    g = golden()
    e = g['sequences'][0]
    tracks = copy.deepcopy(e['tracks'])
    tid = next(iter(tracks))
    tracks[tid]['name'] = tracks[tid]['name'].astype('<U10')
    tracks[tid]['name'][0] = 'Sign'
    with pytest.raises(DetZeroHipError, match='Sign'):
        assign_track_target((copy.deepcopy(e['det']), tracks, copy.deepcopy(e['gt'])), g['iou_thresholds'], ops=traj_ref.NumpyTrajOps())


def test_entry_points_refuse_on_the_host_before_any_pointer_is_used():
    """Metric, thresholds, sizes: host code, answers without a GPU; an empty side launches nothing and needs no pointers."""
    from detzero_amd import lib as L
    lib = L.load()
    thr = (L.c_float * 3)(0.3, 0.1, 0.1)
    zero = (L.c_float * 3)(0.3, 0.0, 0.1)

    def table(n_a=4, a_rows=8, n_b=5, b_rows=8, n_frames=3, metric=16, t=thr, n_cls=3):
        return lib.dz_traj_pair_table(None, None, None, n_a, a_rows, None, None, None, n_b, b_rows, n_frames, metric, 1, t, n_cls,
                                      None, None, None, None, None)

    def rows(n_a=4, n_b=5, n_frames=3, metric=16, n_pairs=2):
        return lib.dz_traj_pair_rows(None, None, None, n_a, 8, None, None, None, n_b, 8, n_frames, metric, 1, None, n_pairs, None, None)
    for metric in (0, 2, 3, 17):                              # UNION_BEV, GIOU3D, GIOU3D_EXACT, unknown
        assert table(metric=metric) == L.ERR_INVALID and b'metric' in lib.dz_last_error()
        assert rows(metric=metric) == L.ERR_INVALID
    assert table(t=zero) == L.ERR_INVALID and b'> 0' in lib.dz_last_error()
    assert table(n_cls=9) == L.ERR_INVALID and table(n_cls=0) == L.ERR_INVALID
    assert table(n_a=-1) == L.ERR_INVALID
    assert table(n_a=1 << 20, n_frames=1 << 12) == L.ERR_INVALID and b'32-bit' in lib.dz_last_error()      # n_frames * n_a
    assert table(n_a=1 << 16, n_b=1 << 16, n_frames=1) == L.ERR_INVALID                                     # n_a * n_b
    assert table(a_rows=1 << 29) == L.ERR_INVALID                                                           # rows * 7
    assert rows(n_pairs=1 << 20, n_frames=1 << 12) == L.ERR_INVALID
    assert table() == L.ERR_INVALID and b'null' in lib.dz_last_error()                                      # sizes fine, no pointers
    assert table(n_a=0) == 0 and table(n_b=0) == 0 and rows(n_pairs=0) == 0 and rows(n_a=0, n_pairs=0) == 0
    assert rows(n_a=0) == L.ERR_INVALID                                                                     # pairs of an empty table


def _literal_assign_matrices(det, tracks, gt, iou_thresholds):
    """target_assign.py:23-75 as written, on the shim-level functions with the oracle's IoU: (traj_count_mat, traj_similar_mat)."""
    from detzero_amd.track_adapter import frame_list_to_dict, tracklets_to_frames
    from detzero_amd.track_assign import get_gt_id_data, get_iou_mat_dict
    class_names = list(iou_thresholds.keys())
    list_track_data = frame_list_to_dict(tracklets_to_frames({'reference': det, 'source': tracks}))
    iou_mat_dict = get_iou_mat_dict(gt, list_track_data, class_names, True, 'bev', iou_fn=lambda a, b, iou: cref.boxes_iou_bev(
        np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)))
    gt_data = get_gt_id_data(gt, ['gt_boxes_global', 'gt_boxes_lidar', 'name', 'obj_ids'], class_names)
    gt_ids, tk_ids = list(gt_data.keys()), list(tracks.keys())
    similar = np.zeros((len(gt_ids), len(tk_ids)), dtype=np.float32)
    count = np.zeros((len(gt_ids), len(tk_ids)), dtype=int)
    for sample_idx in list(gt.keys()):
        frame_gt, frame_tk, iou_mat = gt[sample_idx], list_track_data[sample_idx], iou_mat_dict[sample_idx]
        for f_idx, gt_id in enumerate(frame_gt['annos']['obj_ids']):
            gt_name = frame_gt['annos']['name'][f_idx]
            if gt_name not in class_names:
                continue
            gt_id_idx = gt_ids.index(gt_id)
            gt_idx = gt_data[gt_id]['iou_idx'][gt_data[gt_id]['sample_idx'].index(sample_idx)]
            for i, tk_id in enumerate(frame_tk['obj_ids']):
                tk_id_idx = tk_ids.index(tk_id)
                v = iou_mat[gt_idx, i]
                if gt_name == frame_tk['name'][i] and v >= np.float32(iou_thresholds[gt_name]):
                    count[gt_id_idx, tk_id_idx] += 1
                    similar[gt_id_idx, tk_id_idx] += v
    return count, similar


def test_shuffled_ground_truth_keys_give_the_literal_ports_matrices():
    """Frame ordinals follow the key order of the ground-truth dict - the order the reference's loop walks, and so the order of
    its float32 sums and of its ground-truth ids."""
    from detzero_amd.track_assign import assign_track_target
    g = golden()
    e = g['sequences'][1]
    keys = list(e['gt'])
    random.Random(7).shuffle(keys)
    assert keys != list(e['gt'])
    gt = {k: e['gt'][k] for k in keys}
    count, similar = _literal_assign_matrices(copy.deepcopy(e['det']), copy.deepcopy(e['tracks']), copy.deepcopy(gt), g['iou_thresholds'])
    ops = traj_ref.NumpyTrajOps()
    assign_track_target((copy.deepcopy(e['det']), copy.deepcopy(e['tracks']), copy.deepcopy(gt)), g['iou_thresholds'], ops=ops)
    _, sum_hit, n_hit, _ = ops.tables[-1]
    assert count.sum() > 300 and np.array_equal(n_hit, count)
    assert sum_hit.dtype == np.float32 and np.array_equal(sum_hit, similar)
