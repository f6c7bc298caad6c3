"""CPU: TrackManager.forward_batch on the numpy stand-in of the sequence ops (tests/track_seq_ref.py): packing, the forward-log
regrouping, unpacking and the reverse rows put in front, without a GPU.

The three fixture sequences of tests/golden/track_model_golden.npz go through forward_batch - the two that share a configuration
in one call - and reproduce the golden raw output with difference 0, as the per-sequence test does (tests/test_track_models.py).
A mixed batch (a one-frame sequence, a sequence whose every frame is empty, a sequence under DEATH_AGE 2) equals the per-sequence
path field by field."""
import copy
import json

import pytest

from tests import track_ref, track_seq_ref
from tests.track_seq_ref import assert_tracks, load_sequence, numpy_manager, same_tracks


def batch_manager(model):
    from detzero_amd.track_models import TrackManager
    return TrackManager(model.TRACKING, ops_factory=track_ref.NumpyTrackOps, seq_ops_factory=track_seq_ref.NumpySeqTrackOps)


def _groups():
    """Fixture sequences grouped by their tracking configuration (a batch shares one TrackManager)."""
    loaded = [load_sequence(si) for si in range(3)]
    groups = {}
    for si, item in enumerate(loaded):
        groups.setdefault(json.dumps(item[1].TRACKING, sort_keys=True, default=str), []).append(si)
    return loaded, list(groups.values())


def test_fixture_sequences_in_batches_reproduce_the_golden():
    loaded, groups = _groups()
    assert sorted(si for g in groups for si in g) == [0, 1, 2]
    for group in groups:
        mgr = batch_manager(loaded[group[0]][1])
        results = mgr.forward_batch([copy.deepcopy(loaded[si][0]) for si in group])
        assert len(results) == len(group) and mgr.seq_ops.passes == (2 if mgr.reverse_enable else 1)       # whatever the batch's size
        assert (mgr.batched, mgr.fallbacks) == (len(group), 0)
        for si, mine in zip(group, results):
            assert_tracks(mine, loaded[si][2], 0.0, 'sequence %d raw (batch of %d)' % (si, len(group)))


def test_all_three_in_one_call_under_one_configuration():
    """One call, three sequences, the configuration of sequence 2 (DEATH_AGE 2, IoU3D): the same as three forward() calls."""
    loaded, _ = _groups()
    model = loaded[2][1]
    seqs = [loaded[si][0] for si in range(3)]
    results = batch_manager(model).forward_batch(copy.deepcopy(seqs))
    for si in range(3):
        same_tracks(results[si], numpy_manager(model).forward(copy.deepcopy(seqs[si])))
    assert_tracks(results[2], loaded[2][2], 0.0, 'sequence 2 raw (batch of 3)')


def test_mixed_batch_one_frame_all_empty_and_death_age():
    seq, model, raw, _, _, _ = load_sequence(2)
    assert model.TRACKING.TRACK_AGE.DEATH_AGE == 2
    one_frame = {'0': copy.deepcopy(seq['0'])}
    empty = {f: {key: (val[:0] if key != 'pose' else val) for key, val in frame.items()} for f, frame in copy.deepcopy(seq).items()}
    assert len(one_frame['0']['score']) > 0 and all(len(f['score']) == 0 for f in empty.values())
    batch = [one_frame, empty, copy.deepcopy(seq), {}]
    results = batch_manager(model).forward_batch(copy.deepcopy(batch))
    assert len(results) == 4 and results[1] == {} and results[3] == {}
    for got, dd in zip(results, batch):
        same_tracks(got, numpy_manager(model).forward(copy.deepcopy(dd)))
    assert len(results[0]) > 0 and all(len(t['hit']) == 1 for t in results[0].values())
    assert_tracks(results[2], raw, 0.0, 'sequence 2 raw (mixed batch)')


def test_num_points_default_is_written_as_forward_does():
    """two_stage without num_points: the reference writes zeros into the frame (track_manager.py:166-167); the batch does too."""
    seq, model, _, _, _, _ = load_sequence(0)
    bare = {f: {k: v for k, v in frame.items() if k != 'num_points'} for f, frame in copy.deepcopy(seq).items()}
    a, b = copy.deepcopy(bare), copy.deepcopy(bare)
    got = batch_manager(model).forward_batch([a])[0]
    same_tracks(got, numpy_manager(model).forward(b))
    assert all('num_points' in frame for frame in a.values())


def test_detection_limit_routes_to_the_per_sequence_path(monkeypatch):
    """A sequence with a frame beyond ops.TRACK_SEQ_MAX_DET never reaches the sequence ops; the result is forward()'s."""
    from detzero_amd import ops
    seq, model, raw, _, _, _ = load_sequence(2)
    most = max(len(f['score']) for f in seq.values())
    monkeypatch.setattr(ops, 'TRACK_SEQ_MAX_DET', most - 1)
    mgr = batch_manager(model)
    seen = []
    inner = track_seq_ref.NumpySeqTrackOps.forward_pass
    monkeypatch.setattr(track_seq_ref.NumpySeqTrackOps, 'forward_pass', lambda self, m, pack, seqs: seen.append(list(seqs)) or inner(self, m, pack, seqs))
    small = {f: {key: (val[:1] if key != 'pose' else val) for key, val in frame.items()} for f, frame in copy.deepcopy(seq).items()}
    results = mgr.forward_batch([copy.deepcopy(seq), copy.deepcopy(small)])
    assert seen == [[1]]                                    # the second sequence (one detection per frame) alone went through the batch
    assert (mgr.batched, mgr.fallbacks) == (1, 1)           # ... and the manager says so
    assert_tracks(results[0], raw, 0.0, 'sequence 2 raw (routed)')
    same_tracks(results[1], numpy_manager(model).forward(copy.deepcopy(small)))


def test_reverse_without_two_stage_is_refused_as_in_forward():
    from detzero_amd.lib import DetZeroHipError
    seq, model, _, _, _, _ = load_sequence(0)
    model = copy.deepcopy(model)
    assert model.TRACKING.REVERSE_TRACKING.ENABLE
    model.TRACKING.DATA_ASSOCIATION.STAGE.NAME = 'one_stage'
    with pytest.raises(DetZeroHipError, match='two_stage'):
        numpy_manager(model).forward(copy.deepcopy(seq))
    with pytest.raises(DetZeroHipError, match='two_stage'):
        batch_manager(model).forward_batch([copy.deepcopy(seq)])
