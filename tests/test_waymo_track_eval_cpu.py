"""CPU: the tracking-metric protocol on its restatement, the host side of detzero_amd.waymo_eval_tracking, and the
scenes the GPU tests use.

Hand-counted chains pin the restatement (tests/mot_eval_ref.py) itself; ``metrics_from_mot_counts`` is checked on hand-made
tables; the conversion of info dicts (ids per sequence, fake-lidar boxes, the sampled interval of the command line), the duplicate-id
error and the margin conditions of every seed need no device.
"""
import copy
import ctypes
import os
import pickle

import numpy as np
import pytest

from detzero_amd import waymo_eval_tracking as wt
from detzero_amd.lib import DetZeroHipError
from tests import mot_eval_cases as cases
from tests import mot_eval_ref as ref

OBJECT_NAMES = ['OBJECT_TYPE_TYPE_%s' % t for t in ('VEHICLE', 'PEDESTRIAN', 'SIGN', 'CYCLIST')]


@pytest.fixture(scope='module')
def scenes():
    return {seed: cases.scene(seed) for seed in cases.SEEDS}


def test_perfect_tracking_by_hand():
    table = ref.table_from_problems(cases.hand_cases()['perfect'], 4)
    # cutoffs 0..30 hold all three predictions, 31..60 two, 61..90 one, above none; 4 frames; difficulty 1, 2, 1
    assert table[0, 1, 0].tolist() == [12, 0, 0, 0, 0] and table[0, 0, 0].tolist() == [8, 0, 0, 0, 0]
    assert table[0, 1, 31].tolist() == [8, 0, 4, 0, 0] and table[0, 0, 31].tolist() == [4, 0, 4, 0, 0]       # the pair on a level-2 truth is no level-1 TP
    assert table[0, 1, 61].tolist() == [4, 0, 8, 0, 0] and table[0, 1, 91].tolist() == [0, 0, 12, 0, 0]
    m = ref.metrics(table, OBJECT_NAMES)
    for lv in (1, 2):
        assert m['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_%d/MOTA' % lv] == [1.0] and m['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_%d/MOTP' % lv] == [0.0]
        assert m['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_%d/MISMATCH' % lv] == [0.0]
    assert wt.metrics_from_mot_counts(table, ['object']) == m


def test_one_id_swap_is_two_mismatches_by_hand():
    table = ref.table_from_problems(cases.hand_cases()['swap'], 4)
    cost = int(np.round((1.0 - float(np.float32(0.8))) * 4294967296.0))
    for k in range(0, 81):                                      # both predictions present
        assert table[0, 0, k].tolist() == [12, 0, 0, 2, 12 * cost], k
    for k in range(81, 91):                                     # one prediction, on the first truth: its id changes once
        assert table[0, 0, k].tolist() == [6, 0, 6, 1, 6 * cost], k
    assert table[0, 0, 91].tolist() == [0, 0, 12, 0, 0]


def test_dropping_every_prediction_by_hand():
    table = ref.table_from_problems(cases.hand_cases()['dropped'], 4)
    assert (table[0, 1, :, :] == np.array([0, 0, 12, 0, 0])).all()
    m = wt.metrics_from_mot_counts(table, ['object'])
    assert m['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_2/MOTA'] == [0.0] and m['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_2/MISS'] == [1.0]
    assert m == ref.metrics(table, OBJECT_NAMES)


def test_unpairing_through_the_prediction_is_no_mismatch():
    # id 5 follows truth 10, then moves to truth 11 while 10 gets nothing: 11 had no partner, so nothing is a mismatch; when 10 is
    # found again by id 6 its last partner (5) differs: one mismatch
    w = [[1.0, 0.0]]
    probs = [cases._hand_problem(0, w, [.9], [5], [10, 11], [1, 1]), cases._hand_problem(1, [[0.0, 1.0]], [.9], [5], [10, 11], [1, 1]),
             cases._hand_problem(2, [[0.0, 1.0], [1.0, 0.0]], [.9, .8], [5, 6], [10, 11], [1, 1])]
    table = ref.table_from_problems(probs, 4)
    assert table[0, 0, 0].tolist() == [4, 0, 2, 0, 0]          # last[10] was dropped when 5 left it: 6 on 10 is no mismatch
    probs[2] = cases._hand_problem(2, [[1.0, 0.0], [0.0, 1.0]], [.9, .8], [6, 5], [10, 11], [1, 1])
    assert ref.table_from_problems(probs, 4)[0, 0, 0].tolist() == [4, 0, 2, 0, 0]


def test_metrics_best_cutoff_tie_and_empty():
    table = np.zeros((4, 2, 101, 5), dtype=np.int64)
    table[0, :, :, 0], table[0, :, :, 2] = 6, 4                 # N = 10 everywhere
    table[0, 0, :, 1] = 5                                       # MOTA 0.1 ...
    table[0, 0, 40:43, 1] = 1                                   # ... but 0.5 at k = 40, 41, 42: 40 is reported
    table[0, 0, 40, 4], table[0, 0, 41, 4] = 3 << 32, 6 << 32
    table[0, 0, 40, 3] = 0
    table[0, 1, :, 3] = 1                                       # level 2: the same value everywhere, k = 0 is reported
    table[0, 1, 0, 4] = 3 << 31
    m = wt.metrics_from_mot_counts(table)
    assert m['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_1/MOTA'] == [0.5] and m['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_1/MOTP'] == [0.5]
    assert m['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_1/FP'] == [0.1] and m['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_1/MISS'] == [0.4]
    assert m['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_2/MOTA'] == [1.0 - 5 / 10] and m['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_2/MOTP'] == [0.25]
    assert m['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_2/MISMATCH'] == [0.1]
    for key in wt.METRIC_KEYS:                                  # N = 0: five zeros
        assert m['OBJECT_TYPE_TYPE_CYCLIST_LEVEL_1/%s' % key] == [0.0]
    assert list(m)[:5] == ['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_1/%s' % k for k in ('MOTA', 'MOTP', 'MISS', 'MISMATCH', 'FP')]
    assert len(m) == 4 * 2 * 5 and m == ref.metrics(table, OBJECT_NAMES)
    with pytest.raises(DetZeroHipError):
        wt.metrics_from_mot_counts(np.zeros((4, 2, 101, 4), dtype=np.int64))


def test_config_and_mask():
    est = wt.WaymoTrackingMetricsEstimator()
    cfg = est.build_config(['object', 'range'])
    assert cfg['breakdown_generator_ids'] == ['OBJECT_TYPE', 'RANGE'] and cfg['box_type'] == 'TYPE_3D' and cfg['matcher_type'] == 'TYPE_HUNGARIAN'
    assert cfg['iou_thresholds'] == [0.0, 0.7, 0.5, 0.5, 0.5] and len(cfg['score_cutoffs']) == 101
    boxes = np.array([[1e6, 0, 0, 1, 1, 1, 0], [1, 1, 0, 1, 1, 1, 0]], dtype=np.float64)
    kept, ids = est.mask_by_distance(10, boxes, np.array([7, 8]))
    assert len(kept) == 2 and ids.tolist() == [7, 8]           # the reference's mask passes everything


def test_conversion_ids_fakelidar_and_copies(scenes):
    s = scenes[cases.SEEDS[0]]
    pds, gts = cases.infos_of(s)
    before = copy.deepcopy((pds, gts))
    est = wt.WaymoTrackingMetricsEstimator()
    names = ['Vehicle', 'Pedestrian', 'Sign', 'Cyclist']
    frame, seq, oid, boxes, typ, score, nlz, diff, speed = est.generate_waymo_type_results(pds, names, is_gt=False)
    assert len(frame) == len(s['pd_id']) and speed.shape == (len(frame), 0) and (diff == 0).all()
    walk = cases.frames_of(s)
    assert [walk[f] for f in frame.tolist()] == list(zip(s['pd_seq'][np.lexsort((np.arange(len(frame)), s['pd_frame'], s['pd_seq']))].tolist(),
                                                         s['pd_frame'][np.lexsort((np.arange(len(frame)), s['pd_frame'], s['pd_seq']))].tolist()))
    assert sorted(set(seq.tolist())) == ['0', '1', '2']
    # one dense id per (sequence name, object id), the same number wherever the pair returns
    order = np.lexsort((np.arange(len(frame)), s['pd_frame'], s['pd_seq']))
    pairs = list(zip(s['pd_seq'][order].tolist(), s['pd_id'][order].tolist()))
    assert len(set(zip(pairs, oid.tolist()))) == len(set(pairs)) == len(set(oid.tolist()))
    assert typ.tolist() == s['pd_type'][order].tolist()        # 'Sign' is type 3 here
    g = est.generate_waymo_type_results(gts, names, is_gt=True, fake_gt_infos=False)
    assert np.array_equal(g[3][:, :6].astype(np.float32), s['gt_box'][np.lexsort((np.arange(len(g[0])), s['gt_frame'], s['gt_seq']))][:, :6])
    fake = est.generate_waymo_type_results(gts, names, is_gt=True, fake_gt_infos=True)
    raw = s['gt_box'][np.lexsort((np.arange(len(g[0])), s['gt_frame'], s['gt_seq']))].astype(np.float64)
    assert np.allclose(fake[3][:, 2], raw[:, 2] + raw[:, 5] / 2) and np.array_equal(fake[3][:, 3], raw[:, 4]) and np.array_equal(fake[3][:, 4], raw[:, 3])
    few = est.generate_waymo_type_results(gts, ['Vehicle'], is_gt=True, fake_gt_infos=False)
    assert (few[4] == 1).all() and len(few[0]) == int((s['gt_type'] == 1).sum())
    # nothing of the caller's was written
    for a, b in zip(before[1], gts):
        assert np.array_equal(a['annos']['gt_boxes_lidar'], b['annos']['gt_boxes_lidar']) and np.array_equal(a['annos']['difficulty'], b['annos']['difficulty'])
    # zero difficulty is filled from the point count; boxes without points leave
    one = copy.deepcopy(gts[:1])
    n = len(one[0]['annos']['name'])
    one[0]['annos']['difficulty'][:] = 0
    one[0]['annos']['num_points_in_gt'] = np.array([0] + [3] * (n - 2) + [9])
    out = est.generate_waymo_type_results(one, names, is_gt=True, fake_gt_infos=False)
    assert out[7].tolist() == [2] * (n - 2) + [1]
    del one[0]['annos']['num_points_in_gt']
    with pytest.raises(NotImplementedError):
        est.generate_waymo_type_results(one, names, is_gt=True)


def test_chain_arrays_match_the_restatement(scenes):
    s = scenes[cases.SEEDS[0]]
    pds, gts = cases.infos_of(s)
    est = wt.WaymoTrackingMetricsEstimator()
    for config_type in (['object'], ['object', 'range']):
        pd, gt = est.waymo_arrays(pds, gts, ['Vehicle', 'Pedestrian', 'Sign', 'Cyclist'], fake_gt_infos=False)
        a = wt.chain_arrays(config_type, pd, gt)
        probs = ref.problems(config_type, '3d', s)
        assert a['pdesc'][:, [1, 3, 4]].tolist() == [[len(p['pid']), len(p['gid']), p['type']] for p in probs]
        assert np.array_equal(a['pred_score'], np.concatenate([p['score'] for p in probs]))
        want = np.concatenate([p['pb'] for p in probs])
        turn = (a['pred_box'][:, 6].astype(np.float64) - want[:, 6]) / (2 * np.pi)             # the estimator wraps headings to [-pi, pi)
        assert np.array_equal(a['pred_box'][:, :6], want[:, :6]) and np.abs(turn - np.round(turn)).max() < 1e-6
        assert np.array_equal(a['gt_diff'], np.concatenate([p['gd'] for p in probs]))
        ws, cut, pid, gid, gd, pdesc, cdesc, frames = cases.device_inputs(probs)
        assert np.array_equal(a['cdesc'][:, [0, 1, 2, 5]], cdesc[:, [0, 1, 2, 5]])
        # dense ids: the same partition of the objects of a sequence, and within the id counts
        for c in a['cdesc']:
            lo, hi = a['pdesc'][c[0], 0], a['pdesc'][c[0] + c[1] - 1, 0] + a['pdesc'][c[0] + c[1] - 1, 1]
            assert (a['pred_id'][lo:hi] < c[3]).all() and len(set(zip(a['pred_id'][lo:hi].tolist(), pid[lo:hi].tolist()))) == len(set(pid[lo:hi].tolist()))
        assert wt.sequence_groups(a, cap=1) == [(int(np.flatnonzero(a['chain_seq'] == q)[0]), int(np.flatnonzero(a['chain_seq'] == q)[-1]) + 1)
                                                 for q in range(3)]
        assert wt.sequence_groups(a) == [(0, len(a['cdesc']))]


def test_duplicate_ids_raise(scenes):
    s = scenes[cases.SEEDS[0]]
    pds, gts = cases.infos_of(s)
    est = wt.WaymoTrackingMetricsEstimator()
    names = ['Vehicle', 'Pedestrian', 'Sign', 'Cyclist']
    bad = copy.deepcopy(pds)
    bad[3]['obj_ids'][1] = bad[3]['obj_ids'][0]
    with pytest.raises(DetZeroHipError, match='twice'):
        wt.chain_arrays(['object'], *est.waymo_arrays(bad, gts, names, fake_gt_infos=False))
    bad = copy.deepcopy(gts)
    bad[2]['annos']['obj_ids'][1] = bad[2]['annos']['obj_ids'][0]
    with pytest.raises(DetZeroHipError, match='twice'):
        wt.chain_arrays(['object'], *est.waymo_arrays(pds, bad, names, fake_gt_infos=False))
    dup = dict(s)
    dup['pd_id'] = s['pd_id'].copy()
    same = np.flatnonzero((s['pd_seq'] == 0) & (s['pd_frame'] == 2))
    dup['pd_id'][same[1]] = dup['pd_id'][same[0]]
    with pytest.raises(ValueError):
        ref.check_ids(dup)


def test_pairing_and_sampled_interval(tmp_path, monkeypatch, scenes):
    s = scenes[cases.SEEDS[0]]
    pds, gts = cases.infos_of(s)
    shuffled = [pds[i] for i in np.random.RandomState(0).permutation(len(pds)) if i != 4]      # one frame has no result item
    det, gt, notes = wt.pair_by_frame(shuffled, gts)
    assert [(d['sequence_name'], d['frame_id']) for d in det] == [(g['sequence_name'], g['frame_id']) for g in gts]
    assert all('annos' in g for g in gt) and len(notes) == 1 and len(det[4]['boxes_lidar']) == 0
    seen = {}
    monkeypatch.setattr(wt.WaymoTrackingMetricsEstimator, 'waymo_evaluation',
                        lambda self, pred, gt_, **kw: seen.update(pred=pred, gt=gt_, kw=kw) or {})
    with open(tmp_path / 'pred.pkl', 'wb') as f:
        pickle.dump(pds[::2], f)
    with open(tmp_path / 'gt.pkl', 'wb') as f:
        pickle.dump(gts, f)
    wt.main(['--pred_infos', str(tmp_path / 'pred.pkl'), '--gt_infos', str(tmp_path / 'gt.pkl'), '--sampled_interval', '2', '--class_names', 'Vehicle'])
    assert len(seen['gt']) == len(gts[::2]) and [g['frame_id'] for g in seen['gt']] == [g['frame_id'] for g in gts[::2]]
    assert all('name' in g and 'sequence_name' in g for g in seen['gt']) and seen['kw']['class_name'] == ['Vehicle']


def test_every_seed_passes_the_margin_conditions(scenes):
    for seed, s in scenes.items():
        ref.check_ids(s)
        for box_type in ('3d', 'bev'):
            assert ref.margins_hold(['object', 'range'], box_type, s), (seed, box_type)


def test_scenes_are_what_they_claim(scenes):
    for seed, s in scenes.items():
        assert set(s['gt_type'].tolist()) == {1, 2, 3, 4} and set(s['gt_diff'].tolist()) == {1, 2}
        frames = cases.frames_of(s)
        assert [q for q, _ in frames].count(2) == 1 and [q for q, _ in frames].count(0) == cases.N_FRAMES
        assert not ((s['pd_seq'] == 1) & (s['pd_frame'] == 7)).any() and ((s['gt_seq'] == 1) & (s['gt_frame'] == 7)).any()
        assert not ((s['gt_seq'] == 1) & (s['gt_frame'] == 8)).any() and ((s['pd_seq'] == 1) & (s['pd_frame'] == 8)).any()
        for exact in (0.0, 0.5, 1.0):
            assert (s['pd_score'] == np.float32(exact)).any()
        table = ref.counts(['object'], '3d', s)
        ped = table[1, 1]                                       # pedestrians carry the constructed tracks
        assert ped[0, 3] >= 2 * (2 + 1)                         # per sequence: the swap (2) and the renamed return (1)
        assert ped[45, 3] > ped[30, 3] or ped[45, 3] > ped[55, 3]          # the score that crosses 0.39..0.50 costs those chains a mismatch
        # the carried pair wins over the closer newcomer: every frame matched afresh has the same pairs but for those, at a lower cost
        probs = [p for p in ref.problems(['object'], '3d', s) if p['shard'] == 1]
        afresh = [(p, ref.det_ref.matching(p['w'])) for p in probs]
        assert ped[0, 0] == sum(len(m) for _, m in afresh)
        assert ped[0, 4] > sum(int(np.round((1.0 - p['w'][r, c]) * ref.ONE)) for p, m in afresh for r, c in m)


@pytest.mark.parametrize('box_type', ['3d', 'bev'])
def test_one_frame_sequences_count_as_detection(box_type):
    """Where every sequence is one frame, no pair is carried and no mismatch can occur: the tracking table's [TP, FP, MISS] is the
    detection table's [TP, FP, FN] at every shard, level and cutoff.  (The scene passes the detection margin conditions, so the
    optimum's pair set is unique.)"""
    from tests import waymo_eval_cases as det_cases
    det = det_cases.scene(*det_cases.SCENES[0])
    config = ['object', 'range']
    want = ref.det_ref.counts(config, box_type, *det_cases.flat(det))[0]
    got = ref.counts(config, box_type, cases.one_frame_sequences(det))
    assert got.shape[:3] == want.shape[:3] == (16, 2, 101) and want[..., 0].max() > 0 and want[..., 1].max() > 0
    assert np.array_equal(got[..., :3], want) and not got[..., 3].any()


def test_header_symbols_are_in_the_library():
    from detzero_amd import lib as L
    from detzero_amd.build import build
    build(verbose=False)
    cdll = ctypes.CDLL(L.LIB_PATH)
    names = ('dz_mot_weights', 'dz_mot_chain_counts', 'dz_mot_chain_ws_bytes')
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'detzero_hip.h')).read()
    for name in names:
        assert name + '(' in header and name in L.exported_symbols()
        if cdll is not None:
            assert hasattr(cdll, name)
    for const in ('DZ_MOT_PDESC_WORDS 6', 'DZ_MOT_CDESC_WORDS 7', 'DZ_MOT_COUNTS 5', 'DZ_MOT_LDS_DIM 192'):
        assert '#define ' + const in header


@pytest.mark.parametrize('side,seq', [('pd', 2), ('gt', 2), ('pd', 0), ('pd', None), ('gt', None)],
                         ids=['last-sequence-without-predictions', 'last-sequence-without-ground-truth', 'first-sequence-without-predictions',
                              'no-predictions', 'no-ground-truth'])
def test_chain_arrays_with_an_empty_side(scenes, side, seq):
    """A sequence one side knows nothing of (the id counts are per sequence of BOTH sides' names), and a side with no row at all."""
    s = cases.without(scenes[cases.SEEDS[0]], side, seq)
    pds, gts = cases.infos_of(s)
    est = wt.WaymoTrackingMetricsEstimator()
    config_type = ['object', 'range']
    a = wt.chain_arrays(config_type, *est.waymo_arrays(pds, gts, ['Vehicle', 'Pedestrian', 'Sign', 'Cyclist'], fake_gt_infos=False))
    probs = ref.problems(config_type, '3d', s)
    assert len(probs) > 50 and a['pdesc'][:, [1, 3, 4]].tolist() == [[len(p['pid']), len(p['gid']), p['type']] for p in probs]
    assert a['pred_box'].shape == (sum(len(p['pid']) for p in probs), 7) and a['gt_box'].shape == (sum(len(p['gid']) for p in probs), 7)
    cdesc = cases.device_inputs(probs)[6]
    assert np.array_equal(a['cdesc'], cdesc)                    # the id counts too: 0 for a sequence the side lacks
    if seq is not None:
        gone = a['cdesc'][a['chain_seq'] == seq]
        assert len(gone) and (gone[:, 3 if side == 'pd' else 4] == 0).all() and (gone[:, 4 if side == 'pd' else 3] > 0).all()
    else:
        assert (a['cdesc'][:, 3 if side == 'pd' else 4] == 0).all() and len(a['pred_box' if side == 'pd' else 'gt_box']) == 0
    groups = wt.sequence_groups(a, cap=1)
    assert [lo for lo, _ in groups] == [int(np.flatnonzero(a['chain_seq'] == q)[0]) for q in sorted(set(a['chain_seq'].tolist()))]


def test_chain_arrays_of_nothing():
    est = wt.WaymoTrackingMetricsEstimator()
    pds = [{'boxes_lidar': np.zeros((0, 7), np.float32), 'score': np.zeros((0,), np.float32), 'name': np.zeros((0,), '<U8'), 'obj_ids': np.zeros((0,), np.int64),
            'sequence_name': 'a', 'frame_id': 0}]
    gts = [{'sequence_name': 'a', 'frame_id': 0, 'annos': {'gt_boxes_lidar': np.zeros((0, 7), np.float32), 'name': np.zeros((0,), '<U8'),
            'difficulty': np.zeros((0,), np.int32), 'num_points_in_gt': np.zeros((0,), np.int64), 'obj_ids': np.zeros((0,), '<U8')}}]
    a = wt.chain_arrays(['object'], *est.waymo_arrays(pds, gts, ['Vehicle'], fake_gt_infos=False))
    assert a['cdesc'].shape == (0, 6) and a['pdesc'].shape == (0, 5) and wt.sequence_groups(a) == []
