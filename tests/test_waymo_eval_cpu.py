"""CPU: the host side of the detection metrics (detzero_amd/waymo_eval.py) and the scenes the GPU tests use.

- metrics_from_counts on count tables written by hand (the areas are worked out in the comments), and the result's keys and order;
- the conversion of info dicts to flat arrays against arrays recorded from the reference's own functions
  (tests/golden/waymo_eval_golden.npz, written by tests/golden/gen_waymo_eval_golden.py), the caller's dicts untouched;
- the sharding / problem layout against the restatement of tests/waymo_eval_ref.py;
- every seed of tests/waymo_eval_cases.py passes the margin conditions and has the properties its docstring claims.
"""
import copy
import os

import numpy as np
import pytest

from detzero_amd import waymo_eval
from detzero_amd.lib import DetZeroHipError
from tests import waymo_eval_cases as cases
from tests import waymo_eval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 32


def _table(n_shards=4):
    return np.zeros((n_shards, 2, 101, 4), dtype=np.int64)


def test_perfect_detector_scores_one():
    t = _table()
    t[0, :, :, 0] = 10                      # every cutoff: 10 TP, no FP, no FN, heading exact
    t[0, :, :, 3] = 10 * ONE
    out = waymo_eval.metrics_from_counts(t)
    for lv in (1, 2):
        assert out['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_%d/AP' % lv] == [1.0] and out['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_%d/APH' % lv] == [1.0]


def test_no_predictions_and_no_ground_truth_score_zero():
    t = _table()
    t[1, :, :, 2] = 7                       # pedestrians: 7 ground truths, nothing predicted
    t[3, :, :50, 1] = 5                     # cyclists: 5 false positives below cutoff 50, no ground truth at all
    out = waymo_eval.metrics_from_counts(t)
    assert all(v == [0.0] for v in out.values())
    assert all(isinstance(v, list) and len(v) == 1 and isinstance(v[0], float) for v in out.values())


def test_two_step_curve():
    # 4 ground truths.  Cutoffs 0..49 hold 4 predictions: 2 TP, 2 FP -> p = 0.5, r = 0.5.  Cutoffs 50..100 hold 1: 1 TP -> p = 1, r = 0.25.
    # Distinct recalls 0.25 < 0.5: AP = (0.25 - 0) * max(p: r >= 0.25) + (0.5 - 0.25) * max(p: r >= 0.5) = 0.25 * 1 + 0.25 * 0.5 = 0.375.
    # Heading: the pair of the high cutoffs has accuracy 0.5, the second pair 1.0 -> HA = 1.5 below 50, 0.5 from 50 on:
    # ph = 1.5/4 = 0.375, rh = 1.5/4 = 0.375 and ph = 0.5, rh = 0.125: APH = 0.125 * 0.5 + (0.375 - 0.125) * 0.375 = 0.15625.
    t = _table()
    t[0, :, :50, :3] = (2, 2, 2)
    t[0, :, 50:, :3] = (1, 0, 3)
    t[0, :, :50, 3] = 3 * ONE // 2
    t[0, :, 50:, 3] = ONE // 2
    out = waymo_eval.metrics_from_counts(t)
    assert out['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_1/AP'][0] == pytest.approx(0.375, abs=1e-15)
    assert out['OBJECT_TYPE_TYPE_VEHICLE_LEVEL_2/APH'][0] == pytest.approx(0.15625, abs=1e-15)


def test_non_monotone_recall():
    # 4 ground truths; recall does not fall with the cutoff (a later, larger matching can lose a level-1 pair to a level-2 one):
    # cutoffs 0..29: TP 2, FP 6 (r 0.5, p 0.25); 30..59: TP 3, FP 1 (r 0.75, p 0.75); 60..100: TP 1, FP 0 (r 0.25, p 1).
    # Distinct recalls 0.25, 0.5, 0.75 with envelope 1, 0.75, 0.75: AP = 0.25 * 1 + 0.25 * 0.75 + 0.25 * 0.75 = 0.625.
    t = _table()
    t[2, 0, :30, :3] = (2, 6, 2)
    t[2, 0, 30:60, :3] = (3, 1, 1)
    t[2, 0, 60:, :3] = (1, 0, 3)
    out = waymo_eval.metrics_from_counts(t)
    assert out['OBJECT_TYPE_TYPE_SIGN_LEVEL_1/AP'][0] == pytest.approx(0.625, abs=1e-15)
    assert out['OBJECT_TYPE_TYPE_SIGN_LEVEL_1/APH'] == [0.0] and out['OBJECT_TYPE_TYPE_SIGN_LEVEL_2/AP'] == [0.0]


def test_keys_and_their_order():
    obj = ['OBJECT_TYPE_TYPE_%s_LEVEL_%d/%s' % (t, lv, m) for t in ('VEHICLE', 'PEDESTRIAN', 'SIGN', 'CYCLIST') for lv in (1, 2) for m in ('AP', 'APH')]
    rng = ['RANGE_TYPE_%s_%s_LEVEL_%d/%s' % (t, r, lv, m) for t in ('VEHICLE', 'PEDESTRIAN', 'SIGN', 'CYCLIST')
           for r in ('[0, 30)', '[30, 50)', '[50, +inf)') for lv in (1, 2) for m in ('AP', 'APH')]
    assert list(waymo_eval.metrics_from_counts(_table(4), ['object'])) == obj
    assert list(waymo_eval.metrics_from_counts(_table(12), ['range'])) == rng
    assert list(waymo_eval.metrics_from_counts(_table(16), ['object', 'range', '3d'])) == obj + rng
    assert list(waymo_eval.metrics_from_counts(_table(16))) == obj + rng
    with pytest.raises(DetZeroHipError):
        waymo_eval.metrics_from_counts(_table(5))


def test_config_is_a_plain_dict_with_float32_cutoffs():
    est = waymo_eval.WaymoDetectionMetricsEstimator()
    cfg = est.build_config(['object', 'range', 'bev'])
    assert type(cfg) is dict and cfg['breakdown_generator_ids'] == ['OBJECT_TYPE', 'RANGE'] and cfg['box_type'] == 'TYPE_2D'
    assert cfg['iou_thresholds'] == [0.0, 0.7, 0.5, 0.5, 0.5] and len(cfg['score_cutoffs']) == 101
    assert est.build_config(['object'])['box_type'] == 'TYPE_3D'            # neither '3d' nor 'bev' means '3d'
    c = waymo_eval.score_cutoffs()
    assert c.dtype == np.float32 and c[0] == 0 and c[100] == 1 and c[50] == np.float32(0.5) and c[7] == np.float32(7 * 0.01)
    assert (c == ref.CUTOFFS).all()


# ------------------------------------------------------------------------------------------------
# conversion golden
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def golden():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'waymo_eval_golden.npz'))
    n = 1 + max(int(k.split('_')[1][2:]) for k in g.files if k.startswith('in_pd'))
    pds = [{k: g['in_pd%d_%s' % (f, k)] for k in ('name', 'score', 'boxes_lidar')} for f in range(n)]
    gts = [{k: g['in_gt%d_%s' % (f, k)] for k in ('name', 'difficulty', 'num_points_in_gt', 'gt_boxes_lidar')} for f in range(n)]
    return g, pds, gts


@pytest.mark.parametrize('fake', [False, True])
@pytest.mark.parametrize('bev', [False, True])
@pytest.mark.parametrize('dist', [30, 1000])
def test_conversion_matches_the_reference(golden, fake, bev, dist):
    g, pds, gts = golden
    before = copy.deepcopy((pds, gts))
    est = waymo_eval.WaymoDetectionMetricsEstimator()
    names = ['Vehicle', 'Pedestrian', 'Cyclist']
    p = est.generate_waymo_type_results(pds, names, is_gt=False, bev=bev)
    q = est.generate_waymo_type_results(gts, names, is_gt=True, fake_gt_infos=fake, bev=bev)
    pb, pf, pt, ps = est.mask_by_distance(dist, p[1], p[0], p[2], p[3])
    gb, gf, gt_, gd = est.mask_by_distance(dist, q[1], q[0], q[2], q[5])
    tag = 'fake%d_bev%d_dist%d' % (fake, bev, dist)
    for key, got in (('pd_frame', pf), ('pd_box', pb), ('pd_type', pt), ('pd_score', ps), ('gt_frame', gf), ('gt_box', gb), ('gt_type', gt_),
                     ('gt_diff', gd)):
        want = g['%s_%s' % (tag, key)]
        assert np.asarray(got).shape == want.shape and np.asarray(got).dtype == want.dtype, (key, np.asarray(got).dtype, want.dtype)
        assert np.array_equal(got, want), key
    assert len(gb) > 0 and len(pb) > 0 and gb.shape[1] == (5 if bev else 7)
    for a, b in zip(before[0] + before[1], pds + gts):            # the caller's dicts are as they were
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def test_missing_point_counts_raise(golden):
    _, _, gts = golden
    bad = [{k: v for k, v in gt.items() if k != 'num_points_in_gt'} for gt in gts]
    with pytest.raises(NotImplementedError):
        waymo_eval.WaymoDetectionMetricsEstimator().generate_waymo_type_results(bad, ['Vehicle'], is_gt=True)


def test_scores_above_one_go_through_a_sigmoid(golden):
    _, pds, gts = golden
    raw = copy.deepcopy(pds)
    for p in raw:
        p['score'] = p['score'] * 6 - 1
    est = waymo_eval.WaymoDetectionMetricsEstimator()
    (_, _, _, score), _ = est.waymo_arrays(raw, gts, ['Vehicle', 'Pedestrian', 'Cyclist'], ['object'], 1000, False)
    (_, _, _, plain), _ = est.waymo_arrays(pds, gts, ['Vehicle', 'Pedestrian', 'Cyclist'], ['object'], 1000, False)
    assert np.allclose(score, 1 / (1 + np.exp(-(plain.astype(np.float64) * 6 - 1))), rtol=1e-6) and plain.max() <= 1


def test_tracking_is_refused():
    with pytest.raises(DetZeroHipError, match='tracking'):
        waymo_eval.main(['--det_result_path', 'x.pkl', '--tracking'])


# ------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scenes():
    return [cases.scene(seed, types) for seed, types in cases.SCENES]


def test_every_seed_passes_the_margin_conditions(scenes):
    for s in scenes:
        for box_type in ('3d', 'bev'):
            assert ref.margins_hold(['object', 'range'], box_type, s)
    for seed, p, g in cases.SINGLES:
        for box_type in ('3d', 'bev'):
            assert ref.margins_hold(['object'], box_type, cases.single(seed, p, g)), (p, g)


def test_scenes_are_what_they_claim(scenes):
    s = scenes[0]
    per_frame = lambda key, f: int((s[key] == f).sum())
    assert per_frame('pd_frame', 0) == 0 and per_frame('gt_frame', 0) > 0 and per_frame('gt_frame', 1) == 0 and per_frame('pd_frame', 1) > 0
    assert per_frame('pd_frame', 2) == 1 and per_frame('pd_frame', 3) > per_frame('gt_frame', 3) and per_frame('pd_frame', 4) < per_frame('gt_frame', 4)
    assert set(s['gt_type']) == {1, 2, 3, 4} and set(scenes[1]['gt_type']) | set(scenes[1]['pd_type']) == {1, 2, 4}
    assert set(s['gt_diff']) == {1, 2}
    for c in (0.0, 0.5, 1.0):
        assert (s['pd_score'] == np.float32(c)).any()
    dist = np.sqrt((s['gt_box'][:, :3].astype(np.float64) ** 2).sum(axis=1))
    assert (dist == 30).any() and (dist == 50).any()
    # IoUs on both sides of the thresholds; a prefix whose optimum is not the greedy choice; a matching that changes as the prefix grows
    below = above = not_greedy = moved = 0
    for _, t, pb, ps, gb, gd in ref.problems(['object'], *cases.flat(s)):
        m = ref.iou(pb, gb, '3d')
        below += int(((m > 0.2) & (m < ref.THR[t])).sum())
        above += int((m >= ref.THR[t]).sum())
        w = np.where(m >= ref.THR[t], m, 0.0)
        order = np.argsort(-ps, kind='stable')
        prev = {}
        for n in range(1, len(order) + 1):
            cur = {int(order[r]): c for r, c in ref.matching(w[order[:n]])}
            moved += int(any(cur.get(r) != c for r, c in prev.items()))      # a pair of the shorter prefix is gone or changed
            prev = cur
        taken, greedy = set(), {}
        for r in order:
            free = [c for c in np.argsort(-w[r]) if w[r, c] > 0 and c not in taken]
            if free:
                greedy[int(r)] = int(free[0])
                taken.add(free[0])
        not_greedy += int(greedy != prev)
    assert below > 20 and above > 20 and not_greedy > 0 and moved > 0


@pytest.mark.parametrize('config_type', [['object'], ['range'], ['object', 'range']])
def test_problem_layout_matches_the_restatement(scenes, config_type):
    """Keys, shards and members of the product's problem arrays against tests/waymo_eval_ref.problems (bin edges 30 and 50 included)."""
    s = scenes[0]
    pk, pb, ps, gk, gb, gd, n_shards = waymo_eval.problem_arrays(config_type, *cases.flat(s))
    assert n_shards == ref.n_shards_of(config_type)
    want = {}
    for f in range(s['n_frames']):
        one = {k: (v[s['pd_frame' if k.startswith('pd') else 'gt_frame'] == f] if k != 'n_frames' else 1) for k, v in s.items()}
        one['pd_frame'], one['gt_frame'] = one['pd_frame'] * 0, one['gt_frame'] * 0
        for shard, t, b, sc, g, d in ref.problems(config_type, *cases.flat(one)):
            want[f * n_shards + shard] = (t, sorted(map(tuple, b.tolist())), sorted(map(tuple, g.tolist())))
    got_keys = sorted(set(pk.tolist()) | set(gk.tolist()))
    assert got_keys == sorted(want)
    for key in got_keys:
        t, b, g = want[key]
        assert sorted(map(tuple, pb[pk == key].tolist())) == b and sorted(map(tuple, gb[gk == key].tolist())) == g
        assert int(waymo_eval.shard_type(config_type, key % n_shards)) == t
