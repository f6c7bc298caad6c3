"""CPU: the tracker's host side (detzero_amd.track_models) against the reference's own TrackManager / PostProcessor output.

tests/golden/track_model_golden.npz (gen_track_model_golden.py) holds three seeded sequences and what the reference's classes made
of them.  Here the product's orchestration runs on the numpy restatement of the seven ops (tests/track_ref.py): every discrete
field must be exact, boxes within the fixture's own fp32 - fp64 difference.  Also: PostProcessor on hand-made tracks, the refusals,
the detzero_track shim's surface."""
import copy
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

from oracle import cref
from tests import track_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'track_model_golden.npz')
REF_TOOLS = '/root/reference/tracking/tools'
KEYS = ('boxes_global', 'name', 'score', 'sample_idx', 'hit', 'num_points', 'obj_ids', 'pose')
EXACT = ('sample_idx', 'hit', 'obj_ids', 'name', 'num_points', 'score', 'pose')

_cache = {}


def golden():
    if 'z' not in _cache:
        _cache['z'] = np.load(GOLDEN)
    return _cache['z']


def load_sequence(si):
    """(frames dict, model config, expected raw tracks, expected final tracks, final states, fp32 - fp64 difference)."""
    from detzero_amd.config import AttrDict
    z, p = golden(), 's%d_' % si
    seq = {}
    for f in range(int(z[p + 'n_frames'])):
        seq[str(f)] = {key: z['%sf%d_%s' % (p, f, key)] for key in ('boxes_global', 'name', 'score', 'num_points', 'pose')}
    tracks = {}
    for tag in ('raw', 'final'):
        ids, lens = z[p + tag + '_ids'], z[p + tag + '_len']
        off = np.concatenate([[0], np.cumsum(lens)])
        tracks[tag] = {int(t): {key: z['%s%s_%s' % (p, tag, key)][off[k]:off[k + 1]] for key in KEYS} for k, t in enumerate(ids)}
    model = AttrDict(json.loads(str(z[p + 'model'])))
    return seq, model, tracks['raw'], tracks['final'], z[p + 'final_state'], float(z[p + 'f64_diff'])


def assert_tracks(mine, ref, box_tol, what):
    assert list(mine.keys()) == list(ref.keys()), what          # the id set AND its order
    worst = 0.0
    for tid, exp in ref.items():
        got = mine[tid]
        for key in EXACT:
            assert np.array_equal(np.asarray(got[key]), exp[key]), (what, tid, key, got[key], exp[key])
        assert got['boxes_global'].shape == exp['boxes_global'].shape and got['boxes_global'].dtype == np.float32
        worst = max(worst, float(np.max(np.abs(got['boxes_global'].astype(np.float64) - exp['boxes_global']))))
    print('%s: max |boxes_global - reference| = %.3e (bound %.3e)' % (what, worst, box_tol))
    assert worst <= box_tol, (what, worst, box_tol)


def numpy_manager(model):
    from detzero_amd.track_models import TrackManager
    return TrackManager(model.TRACKING, ops_factory=track_ref.NumpyTrackOps)


@pytest.mark.parametrize('si', [0, 1, 2])
def test_orchestration_on_numpy_ops_matches_the_reference(si):
    from detzero_amd.track_models import PostProcessor
    seq, model, raw, final, states, diff = load_sequence(si)
    mine = numpy_manager(model).forward(copy.deepcopy(seq))
    assert_tracks(mine, raw, diff, 'sequence %d raw' % si)
    done = PostProcessor(model.POST_PROCESS, overlap_fn=cref.boxes_overlap_bev).forward(mine)
    assert [t['state'] for t in done.values()] == states.tolist()
    assert_tracks(done, final, diff, 'sequence %d post-processed' % si)


def test_fixture_covers_the_scripted_events():
    for si in (0, 1):
        seq, model, raw, final, states, diff = load_sequence(si)
        assert any(len(f['score']) == 0 for f in seq.values())                              # an empty frame
        assert sorted(set(range(max(raw) + 1)) - set(raw)), 'no merged track'               # ids spawned and merged away
        assert any((t['hit'] == 2).any() for t in raw.values())                             # second-stage matches
        assert any(t['hit'][0] != 1 for t in raw.values())                                  # rows the reverse pass put in front
        assert any(1 <= int((t['hit'] > 0).sum()) <= 4 for t in raw.values())               # short-lived false positives
        assert set(states.tolist()) == {'static', 'dynamic'} and len(final) < len(raw)
        assert 1000.0 < float(np.abs(seq['0']['boxes_global'][:, :2]).min())                # global coordinates
    seq, model, raw, _, _, _ = load_sequence(2)
    assert model.TRACKING.TRACK_AGE.DEATH_AGE == 2 and model.TRACKING.DATA_ASSOCIATION.DISTANCE_METHOD == 'IoU3D'
    assert any(len(t['hit']) < len(seq) for t in raw.values())                              # tracks that died


def test_fixture_gaps_keep_discrete_decisions_off_their_thresholds():
    z = golden()
    for key in ('affinity', 'merge', 'gate', 'score'):
        assert float(z['gap_' + key]) >= 1e-3, key
    assert float(z['gap_motion']) >= 1e-5
    for si in range(3):
        assert 0.0 < float(z['s%d_f64_diff' % si]) < 0.05


def test_second_instance_and_rerun_are_independent():
    seq, model, raw, _, _, diff = load_sequence(2)
    a = numpy_manager(model)
    first = a.forward(copy.deepcopy(seq))
    again = a.forward(copy.deepcopy(seq))
    other = numpy_manager(model).forward(copy.deepcopy(seq))
    for res in (again, other):
        assert list(res) == list(first)
        for tid in first:
            for key in KEYS:
                assert np.array_equal(res[tid][key], first[tid][key])


# ------------------------------------------------------------------------------------------------
# pieces
# ------------------------------------------------------------------------------------------------
def test_gnn_assignment_masks_and_lists():
    from detzero_amd.track_models import GNN_assignment
    cost = np.array([[0.2, 5000., 1.0], [0.3, 0.1, 5000.], [5000., 5000., 5000.]], dtype=np.float32)
    matched, rows, cols = GNN_assignment(cost)
    assert matched.tolist() == [[0, 0], [1, 1]] and rows.tolist() == [2] and cols.tolist() == [2]
    assert cost[0, 2] == 5000.
    for shape in ((0, 3), (3, 0)):
        matched, rows, cols = GNN_assignment(np.zeros(shape, np.float32))
        assert matched.shape == (0, 2) and len(rows) == shape[0] and len(cols) == shape[1]


def test_merge_sweep_chain_and_deprecated_lowest_id():
    # A-B-C chain: A ~ B, B ~ C, A !~ C -> B goes, A and C stay
    area = np.full(3, 9.0, np.float32)
    ov = np.array([[9, 5.4, 1.8], [5.4, 9, 5.4], [1.8, 5.4, 9]], np.float32)
    assert track_ref.merge_sweep(ov.copy(), area, [0, 0, 0], [0, 1, 2], [0.5]).tolist() == [False, True, False]
    # the lowest id (1, at index 1) of row 2's set was deprecated by row 0: its column is cleared, row 2 keeps itself
    assert track_ref.merge_sweep(ov.copy(), area, [0, 0, 0], [0, 1, 2], [0.5])[2] == False            # noqa: E712
    # the same geometry in different classes: nothing merges
    assert not track_ref.merge_sweep(ov.copy(), area, [0, 1, 2], [0, 1, 2], [0.5, 0.5, 0.5]).any()
    # the younger id listed first
    assert track_ref.merge_sweep(ov[:2, :2].copy(), area[:2], [0, 0], [7, 3], [0.5]).tolist() == [True, False]


def _track(hit, box=None, score=None, name='Vehicle'):
    n = len(hit)
    boxes = np.zeros((n, 9), np.float32)
    boxes[:, 0] = np.arange(n) * (1.0 if box is None else box)
    boxes[:, 3:6] = (4.0, 2.0, 1.5)
    return {'boxes_global': boxes, 'name': np.array([name] * n), 'score': np.asarray(score if score is not None else np.linspace(0.5, 0.9, n), np.float32),
            'sample_idx': np.array([str(i) for i in range(n)]), 'hit': np.asarray(hit, np.int64), 'num_points': np.zeros(n, np.int32),
            'obj_ids': np.zeros(n, np.int64), 'pose': np.zeros((n, 4, 4))}


def _post(*entries):
    from detzero_amd.config import AttrDict
    from detzero_amd.track_models import PostProcessor
    return PostProcessor(AttrDict({'CONFIG_LIST': [dict(e) for e in entries]}), overlap_fn=cref.boxes_overlap_bev)


def test_empty_track_delete_trims_leading_and_trailing_misses():
    tracks = {1: _track([0, 0, 1, 2, 0, 1, 1, 1, 0, 0]), 2: _track([1, 0, 0, 1, 0]), 3: _track([1, 1, 1, 1, 1])}
    out = _post({'NAME': 'empty_track_delete', 'LEAST_AGE': 5, 'END_REMOVE': True}).forward(tracks)
    assert list(out) == [1, 3]
    assert out[1]['hit'].tolist() == [1, 2, 0, 1, 1, 1] and out[1]['sample_idx'].tolist() == ['2', '3', '4', '5', '6', '7']
    assert all(len(v) == 6 for v in out[1].values())
    kept = _post({'NAME': 'empty_track_delete', 'LEAST_AGE': 1, 'END_REMOVE': False}).forward({2: _track([0, 1, 0])})
    assert kept[2]['hit'].tolist() == [0, 1, 0]


def test_velocity_optimize_header_and_short_tracks():
    proc = _post({'NAME': 'velocity_optimize', 'HEADER_LENGTH': 3})
    out = proc.forward({1: _track([1] * 6, box=0.5), 2: _track([1] * 3, box=0.2), 3: _track([1]), 4: _track([1] * 4, box=1.0)})
    assert np.allclose(out[1]['boxes_global'][:, 7], [5, 5, 5, 0, 0, 0])
    assert np.allclose(out[2]['boxes_global'][:, 7], [2, 2, 0])          # track_len <= HEADER_LENGTH: all but the last
    assert np.all(out[3]['boxes_global'][:, 7:9] == 0)                  # a single row is left alone
    assert np.allclose(out[4]['boxes_global'][:, 7], [10, 10, 10, 0])


def test_motion_classify_and_static_drift():
    proc = _post({'NAME': 'motion_classify'}, {'NAME': 'static_drift_eliminate'})
    parked = _track([1, 1, 1, 0, 0], box=0.01, score=[0.5, 0.9, 0.6, 0.6, 0.6])
    parked['boxes_global'][3:, 0] = 5.0                                 # the predicted rows drifted
    out = proc.forward({1: parked, 2: _track([1, 1, 1, 0], box=8.0), 3: _track([1, 0, 2]), 4: _track([1, 1, 0], box=0.01, name='Pedestrian')})
    assert [t['state'] for t in out.values()] == ['static', 'dynamic', 'static', 'static']
    assert np.array_equal(out[1]['boxes_global'][3], out[1]['boxes_global'][1]) and np.array_equal(out[1]['boxes_global'][4], out[1]['boxes_global'][1])
    assert out[2]['boxes_global'][3, 0] == 24.0                         # dynamic: untouched
    assert out[3]['state'] == 'static'                                  # a single hit == 1 row
    assert out[4]['boxes_global'][2, 0] == np.float32(0.02)             # not a Vehicle: untouched


def test_box_size_update_methods():
    for method, expect in (('max_score_box', 6.0), ('largest_box', 6.0), ('score_weigthed_box', (0.5 * 4 + 1.0 * 6) / 1.5)):
        tk = _track([1, 1], score=[0.5, 1.0])
        tk['boxes_global'][1, 3] = 6.0
        out = _post({'NAME': 'box_size_update', 'METHOD': method}).forward({1: tk})
        assert np.allclose(out[1]['boxes_global'][:, 3], expect), method


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def _shipped_model():
    return copy.deepcopy(load_sequence(0)[1])


def test_ab3dmot_is_refused_by_name():
    from detzero_amd.lib import DetZeroHipError
    from detzero_amd.track_models import build_model
    model = _shipped_model()
    model.TRACKING.FILTER.NAME = 'AB3DMOT'
    with pytest.raises(DetZeroHipError, match='AB3DMOT'):
        build_model(model)


def test_iou2d_is_refused_by_name():
    from detzero_amd.lib import DetZeroHipError
    from detzero_amd.track_models import build_model
    model = _shipped_model()
    model.TRACKING.DATA_ASSOCIATION.DISTANCE_METHOD = 'IoU2D'
    with pytest.raises(DetZeroHipError, match='IoU2D'):
        build_model(model)


def test_assign_mode_is_refused_and_points_to_split_test():
    from detzero_amd.lib import DetZeroHipError
    from detzero_amd.track_models import run_model

    class Dataset:
        assign_mode, split = True, 'val'
    with pytest.raises(DetZeroHipError, match=r'assign_track_target.*--split test'):
        run_model(None, [], Dataset(), workers=4)


def test_unknown_class_name_raises():
    from detzero_amd.lib import DetZeroHipError
    seq, model, _, _, _, _ = load_sequence(2)
    seq = copy.deepcopy(seq)
    seq['0']['name'] = seq['0']['name'].copy()
    seq['0']['name'][0] = 'Sign'
    with pytest.raises(DetZeroHipError, match='Sign'):
        numpy_manager(model).forward(seq)


def test_hip_ops_is_the_default_and_the_product_never_imports_the_numpy_ops():
    from detzero_amd import track_models
    model = _shipped_model()
    assert track_models.TrackManager(model.TRACKING).ops_factory is track_models.HipTrackOps
    src = open(track_models.__file__).read()
    assert 'track_ref' not in src and 'NumpyTrackOps' not in src


# ------------------------------------------------------------------------------------------------
# dataset and shim
# ------------------------------------------------------------------------------------------------
def _dataset_cfg():
    from detzero_amd.config import AttrDict
    return AttrDict({'DATASET': 'WaymoTrackDataset', 'DATA_PATH': 'unused', 'PROCESSED_DATA_TAG': 'waymo_processed_data',
                     'CLASS_NAME': ['Vehicle', 'Pedestrian', 'Cyclist'],
                     'DATA_PROCESSOR': [{'NAME': 'heading_process'}, {'NAME': 'transform_to_global'}]})


def test_dataset_loader_and_run_model_write_both_pickles(tmp_path):
    """The loader is a plain in-process iterable with the reference's collate; run_model (a stand-in model: no GPU here) names the
    two pickles as the reference does."""
    import pickle
    from detzero_amd.track_models import build_dataloader, run_model
    annos = []
    for s in ('seq_a', 'seq_b', 'seq_c'):
        for f in range(2):
            annos.append({'sequence_name': s, 'frame_id': f, 'pose': np.eye(4), 'name': np.array(['Vehicle']), 'score': np.array([0.5], np.float32),
                          'boxes_lidar': np.array([[1, 2, 0, 4, 2, 1.5, 0.1]], np.float32)})
    det = tmp_path / 'result.pkl'
    det.write_bytes(pickle.dumps(annos))
    dataset, loader = build_dataloader(_dataset_cfg(), log_time='20240101-000000', data_path=str(det), batch_size=2, workers=4, split='test',
                                       logger=None, root_path=str(tmp_path))
    assert len(dataset) == 3 and len(loader) == 2 and not dataset.assign_mode
    batches = list(loader)
    assert [b[0] for b in batches] == [['seq_a', 'seq_b'], ['seq_c']]
    assert sorted(batches[0][1]) == ['det_drop', 'detection'] and 'boxes_global' in batches[0][1]['detection'][0]['0']

    class Model:
        def forward(self, seq):
            return {'frames': sorted(seq)}
    run_model(Model(), loader, dataset, workers=4)
    assert dataset.get_track_path() == str(tmp_path / 'tracking' / 'tracking-test-20240101-000000.pkl')
    assert dataset.get_drop_path() == str(tmp_path / 'tracking' / 'drop-test-20240101-000000.pkl')
    assert pickle.load(open(dataset.get_track_path(), 'rb')) == {s: {'frames': ['0', '1']} for s in ('seq_a', 'seq_b', 'seq_c')}
    assert sorted(pickle.load(open(dataset.get_drop_path(), 'rb'))) == ['seq_a', 'seq_b', 'seq_c']
    other = build_dataloader(_dataset_cfg(), log_time='t', data_path=str(det), batch_size=2, workers=0, split='val', logger=None,
                             root_path=str(tmp_path))[0]
    assert other.assign_mode


def test_shim_exposes_every_name_the_tracking_tools_import():
    """run_track.py:8-12, models/__init__.py:6, daemon/combine_output.py:12-15."""
    from detzero_amd import shim
    shim.install()
    from detzero_utils.config_utils import cfg, cfg_from_yaml_file, log_cfg_info                 # noqa: F401
    from detzero_utils.common_utils import create_logger, get_log_info, multi_processing        # noqa: F401
    from detzero_track.models import build_model, run_model                                     # noqa: F401
    from detzero_track.datasets import build_dataloader                                         # noqa: F401
    from detzero_track.utils.transform_utils import transform_boxes3d                           # noqa: F401
    from detzero_track.utils.data_utils import dict_to_sequence_list, sequence_list_to_dict     # noqa: F401
    from detzero_track.models.tracking_modules.data_association import GNN_assignment, bev_overlap_gpu   # noqa: F401
    from detzero_track.models.tracking_modules import __all__ as modules
    assert sorted(modules) == ['PostProcessor', 'TrackManager']
    line = get_log_info('DetZero Tracking Module')
    assert 'DetZero Tracking Module' in line and line.startswith('-') and line.endswith('-') and 98 <= len(line) <= 100
    assert multi_processing(lambda x: x + 1, [1, 2], workers=8) == [2, 3]
    lines = []

    class Log:
        def info(self, msg):
            pass
    from detzero_amd.config import AttrDict
    log_cfg_info(AttrDict({'A': 1, 'B': {'C': 2}}), lines, Log())
    assert [ln.split()[0].rstrip(':') for ln in lines] == ['A', 'B', 'C']
    assert 'detzero_track' in shim.install.__doc__ and 'detzero_track' in shim.__doc__


@pytest.fixture
def fresh_cfg():
    """The shim's global ``cfg`` as a tool finds it at start-up (other tests load their own yaml into it), put back afterwards."""
    from detzero_amd import shim
    shim.install()
    import detzero_utils.config_utils as cu
    saved = dict(cu.cfg)
    cu.cfg.clear()
    cu.cfg.LOCAL_RANK = 0
    yield cu.cfg
    cu.cfg.clear()
    cu.cfg.update(saved)


@pytest.mark.skipif(not os.path.isdir(REF_TOOLS), reason='the reference tree is not on this machine')
def test_reference_run_track_reads_its_config_through_the_shim(monkeypatch, fresh_cfg):
    monkeypatch.chdir(REF_TOOLS)
    monkeypatch.setattr(sys, 'argv', ['run_track.py', '--cfg_file', 'cfgs/tk_model_cfgs/waymo_detzero_track.yaml', '--data_path', 'result.pkl', '--split', 'test'])
    spec = importlib.util.spec_from_file_location('ref_run_track', os.path.join(REF_TOOLS, 'run_track.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args, cfg = mod.parse_config()
    assert args.split == 'test' and cfg.MODEL.NAME == 'DetZeroTracker' and cfg.DATA_CONFIG.DATASET == 'WaymoTrackDataset'
    assert cfg.MODEL.TRACKING.TRACK_AGE.DEATH_AGE == -1 and cfg.DATA_CONFIG.DATA_PROCESSOR[1].NAME == 'overlap_box_filter'
    from detzero_track.models import build_model
    shipped = json.loads(str(golden()['s0_model']))
    assert json.loads(json.dumps(cfg.MODEL)) == shipped          # the fixture carries the shipped values
    assert build_model(cfg.MODEL).module_list[0].merge_thr == [0.5, 0.4, 0.4]


def test_entry_points_refuse_on_the_host_before_any_pointer_is_used():
    """32-bit offsets, class count, metric, merge limits: host code, answers without a GPU."""
    import ctypes
    from detzero_amd import lib as L
    lib = L.load()
    table = L.TrackTable()                       # all pointers NULL, cap 0
    t = ctypes.byref(table)
    thr = (L.c_float * 3)(0.5, 0.4, 0.4)
    big = 1 << 27                                # * 25 floats >= 2^31
    assert lib.dz_track_predict(t, big, 0, None) == L.ERR_UNSUPPORTED and b'32-bit' in lib.dz_last_error()
    assert lib.dz_track_compact(t, big, None, -1, t, None, None) == L.ERR_UNSUPPORTED
    assert lib.dz_track_log(t, 4, 0, None, (1 << 27), None) == L.ERR_UNSUPPORTED
    assert lib.dz_track_update(t, 1, None, 1 << 27, None, 1, 0.1, None) == L.ERR_UNSUPPORTED
    assert lib.dz_track_spawn(t, 1 << 26, None, 1, None, None, 1 << 26, 1, 1, 1, 1, 0.1, None) == L.ERR_UNSUPPORTED
    assert lib.dz_track_affinity(t, 0, None, 0, None, 1, None, 1, None, 1, 3, 1, thr, 3, None, None) == L.ERR_UNSUPPORTED      # UNION_BEV / unknown
    assert b'metric' in lib.dz_last_error()
    assert lib.dz_track_affinity(t, 0, None, 0, None, 1, None, 1, None, 1, 16, 1, thr, 9, None, None) == L.ERR_UNSUPPORTED
    assert lib.dz_track_affinity(t, 0, None, 0, None, 1, None, 1 << 27, None, 1, 16, 1, thr, 3, None, None) == L.ERR_UNSUPPORTED
    assert lib.dz_track_merge(t, 40000, thr, 3, None, None, 0, None) == L.ERR_UNSUPPORTED
    zero = (L.c_float * 3)(0.5, 0.0, 0.4)
    assert lib.dz_track_merge(t, 4, zero, 3, None, None, 0, None) == L.ERR_UNSUPPORTED and b'> 0' in lib.dz_last_error()
    # n == 0 launches nothing and needs no pointers
    assert lib.dz_track_predict(t, 0, 0, None) == 0 and lib.dz_track_update(t, 0, None, 0, None, 0, 0.1, None) == 0
    assert lib.dz_track_spawn(t, 0, None, 0, None, None, 0, 1, 1, 1, 1, 0.1, None) == 0 and lib.dz_track_merge(t, 0, thr, 3, None, None, 0, None) == 0
    assert lib.dz_track_affinity(t, 0, None, 0, None, 0, None, 5, None, 5, 16, 1, thr, 3, None, None) == 0
    assert lib.dz_track_log(t, 0, 0, None, 0, None) == 0
    # a live count beyond the table's capacity is an invalid argument, not a launch
    assert lib.dz_track_predict(t, 1, 0, None) == L.ERR_INVALID
    assert lib.dz_track_merge_workspace_bytes(130) >= 130 * 3 * 8 + 130 * 4


@pytest.mark.skipif(not os.path.isdir(REF_TOOLS), reason='the reference tree is not on this machine')
def test_reference_run_track_main_runs_unchanged_on_the_shim(monkeypatch, tmp_path, fresh_cfg):
    """run_track.py's own main() from start to finish: its argument parser, yaml, logger, build_dataloader, build_model, run_model.
    No GPU here, so the ops object and motion_classify's overlap are the numpy stand-ins; the kernels' side of the same path is
    tests/test_gpu_track.py::test_run_model_over_a_result_pickle."""
    import glob
    import pickle
    import runpy
    from detzero_amd import shim, track_adapter, track_models
    shim.install()
    seq = load_sequence(2)[0]
    annos = [{'sequence_name': 'seq_one', 'frame_id': int(f), 'pose': np.eye(4), 'name': fr['name'], 'score': fr['score'],
              'boxes_lidar': fr['boxes_global'].copy()} for f, fr in seq.items()]
    tools = tmp_path / 'tracking' / 'tools'
    tools.mkdir(parents=True)
    os.symlink(os.path.join(REF_TOOLS, 'cfgs'), tools / 'cfgs')
    det = tmp_path / 'result.pkl'
    det.write_bytes(pickle.dumps(annos))
    monkeypatch.chdir(tools)                                     # DATA_PATH '../../data/waymo' then lies under tmp_path
    monkeypatch.setattr(track_models, 'HipTrackOps', track_ref.NumpyTrackOps)
    monkeypatch.setattr(track_adapter, 'bev_overlap_gpu', cref.boxes_overlap_bev)
    monkeypatch.setattr(sys, 'argv', ['run_track.py', '--cfg_file', 'cfgs/tk_model_cfgs/waymo_detzero_track.yaml', '--data_path', str(det),
                                      '--split', 'test', '--workers', '4'])
    runpy.run_path(os.path.join(REF_TOOLS, 'run_track.py'), run_name='__main__')
    out = glob.glob(str(tmp_path / 'data' / 'waymo' / 'tracking' / 'tracking-test-*.pkl'))
    drop = glob.glob(str(tmp_path / 'data' / 'waymo' / 'tracking' / 'drop-test-*.pkl'))
    assert len(out) == 1 and len(drop) == 1
    tracks = pickle.load(open(out[0], 'rb'))
    assert list(tracks) == ['seq_one'] and len(tracks['seq_one']) >= 5
    assert all(t['state'] in ('static', 'dynamic') and t['boxes_global'].shape[1] == 9 for t in tracks['seq_one'].values())
