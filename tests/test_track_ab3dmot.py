"""CPU: the tracker with FILTER.NAME AB3DMOT - TrackManager's orchestration (the output rule, the frame ids, the float64 results,
the batched path's packing) on the numpy float64 ops (tests/track_ab3dmot_ref.py) against the reference's own classes
(tests/golden/track_ab3dmot_golden.npz: the reference's AB3DMOT and TrackManager over the generator's filterpy stand-in).

Boxes are within 8 x max(solve_diff, 2^-40 x the largest |coordinate|): solve_diff is the fixture's measured difference between
inv(S) and a Cholesky solve, 2^-40 of the coordinates (thousands of metres) allows 2^13 ulps of float64 for the order of the sums."""
import copy
import json

import numpy as np
import pytest

from tests import track_ab3dmot_ref as ab

RUNS = list(range(ab.N_RUNS))


def _manager(model, solve='inv', **kw):
    from detzero_amd.track_models import TrackManager
    return TrackManager(model.TRACKING, ops_factory=lambda: ab.NumpyAb3dTrackOps(solve), **kw)


def test_fixture_holds_the_shipped_config_and_the_events():
    z = np.load(ab.GOLDEN)
    model = json.loads(str(z['r0_model']))['TRACKING']
    assert model['FILTER']['NAME'] == 'AB3DMOT' and model['TRACK_AGE'] == {'BIRTH_AGE': 3, 'DEATH_AGE': 2}
    assert model['DATA_ASSOCIATION']['STAGE']['NAME'] == 'one_stage' and not model['TRACK_MERGE']['ENABLE'] and not model['REVERSE_TRACKING']['ENABLE']
    second = json.loads(str(z['r1_model']))['TRACKING']
    assert second['DATA_ASSOCIATION']['STAGE']['NAME'] == 'two_stage' and second['TRACK_MERGE']['ENABLE']
    ids = z['r0_frame_ids']
    assert (ids < 3).any() and (ids >= 3).any() and not np.array_equal(ids, np.arange(len(ids)))
    for ri in RUNS:
        counts = json.loads(str(z['r%d_branches' % ri]))
        assert counts['flip'] > 0 and counts['wide'] > 0 and counts['z_wrap'] > 0
        assert float(z['r%d_solve_diff' % ri]) < 1e-10
    assert json.loads(str(z['r1_branches']))['second_stage'] > 0
    assert min(float(z['gap_affinity']), float(z['gap_merge']), float(z['gap_score'])) >= 1e-3


def test_build_model_accepts_the_shipped_ab3dmot_values():
    from detzero_amd.track_models import build_model
    _, model, _, _ = ab.load_run(0)
    tracker = build_model(model)
    mgr = tracker.module_list[0]
    assert mgr.ab3dmot and mgr.birth_age == 3 and mgr.death_age == 2 and not mgr.reverse_enable


def test_ab3dmot_with_reverse_tracking_is_refused_by_name():
    from detzero_amd.lib import DetZeroHipError
    from detzero_amd.track_models import build_model
    _, model, _, _ = ab.load_run(0)
    model.TRACKING.REVERSE_TRACKING.ENABLE = True
    with pytest.raises(DetZeroHipError, match='AB3DMOT'):
        build_model(model)


def test_other_dimensions_are_refused():
    from detzero_amd.lib import DetZeroHipError
    _, model, _, _ = ab.load_run(0)
    model.TRACKING.FILTER.X_DIM = 10
    with pytest.raises(DetZeroHipError, match='AB3DMOT'):
        _manager(model)


@pytest.mark.parametrize('ri', RUNS)
@pytest.mark.parametrize('solve', ['inv', 'cholesky'])
def test_forward_matches_the_reference(ri, solve):
    seq, model, ref, solve_diff = ab.load_run(ri)
    before = copy.deepcopy(seq)
    mine = _manager(model, solve).forward(seq)
    ab.assert_tracks(mine, ref, ab.box_tolerance(ref, solve_diff), 'run %d, %s' % (ri, solve))
    for tk in mine.values():
        assert tk['num_points'].dtype == np.int64 and (tk['num_points'] == -1).all()
        assert set(np.unique(tk['hit'])) <= {0, 1}
        assert tk['boxes_global'].shape[1] == 9
    # the caller's detections are left alone (the reference wraps the matched headings in place)
    for f in before:
        assert np.array_equal(before[f]['boxes_global'], seq[f]['boxes_global'])


@pytest.mark.parametrize('ri', RUNS)
def test_output_rule_reads_the_frame_id_not_the_ordinal(ri):
    """With the keys replaced by the ordinals the first frames' ids change (1, 2, 4 -> 0, 1, 2), and so do the rows logged."""
    seq, model, ref, _ = ab.load_run(ri)
    keys = sorted(seq, key=int)
    renamed = {str(k): seq[f] for k, f in enumerate(keys)}
    mine = _manager(model).forward(renamed)
    rows = lambda res: sorted((int(t), len(tk['hit'])) for t, tk in res.items())
    assert rows(mine) != rows(ref)


@pytest.mark.parametrize('ri', RUNS)
def test_forward_batch_equals_forward(ri):
    seq, model, ref, solve_diff = ab.load_run(ri)
    short = {f: seq[f] for f in sorted(seq, key=int)[:7]}
    batch = [seq, short, {}, copy.deepcopy(seq)]
    one = _manager(model)
    expect = [one.forward(copy.deepcopy(s)) for s in batch]
    mgr = _manager(model, seq_ops_factory=ab.NumpyAb3dSeqTrackOps)
    got = mgr.forward_batch(copy.deepcopy(batch))
    assert mgr.batched == 4 and mgr.fallbacks == 0 and mgr.seq_ops.passes == 1
    for a, b in zip(got, expect):
        ab.same_tracks(a, b)
    ab.assert_tracks(got[0], ref, ab.box_tolerance(ref, solve_diff), 'run %d, forward_batch' % ri)
    assert got[2] == {}


def test_a_track_with_its_birth_row_alone_keeps_float32():
    """np.array over the constructor's float32 bbox alone is float32 in the reference; one frame below BIRTH_AGE gives such tracks."""
    seq, model, _, _ = ab.load_run(0)
    first = sorted(seq, key=int)[0]
    mine = _manager(model).forward({first: seq[first]})
    assert len(mine) == len(seq[first]['score']) > 0
    for tk in mine.values():
        assert tk['boxes_global'].dtype == np.float32 and tk['boxes_global'].shape == (1, 9) and tk['hit'].tolist() == [1]
        assert np.array_equal(tk['boxes_global'][0, 7:], [0, 0])
