"""GPU: TrackManager.forward_batch on csrc/track_seq.hip - a pass of every sequence of a batch in one launch, the assignment on the
device - against the golden fixture, against the per-sequence path (TrackManager.forward on HipTrackOps) and against the numpy ops.

A TrackManager has one configuration, and the three fixture sequences of tests/golden/track_model_golden.npz have two (sequences 0
and 1 share one; sequence 2 has DEATH_AGE 2, IoU3D, one_stage, no reverse pass).  So: each configuration's sequences go through one
forward_batch call and are compared with the golden; then all three go through ONE call under each configuration and are compared
with forward() per sequence, bit for bit.
"""
import copy
import pickle

import numpy as np
import pytest
import torch

from tests import track_ref, track_seq_ref
from tests.track_seq_ref import KEYS, assert_tracks, load_sequence, same_tracks

pytestmark = pytest.mark.gpu

_cache = {}


def fixtures():
    if 'loaded' not in _cache:
        _cache['loaded'] = [load_sequence(si) for si in range(3)]
    return _cache['loaded']


def manager(model, **seq_ops_args):
    from detzero_amd.track_models import HipSeqTrackOps, TrackManager
    return TrackManager(model.TRACKING, seq_ops_factory=lambda: HipSeqTrackOps(**seq_ops_args))


def batched(key, model, seqs):
    """One forward_batch call per key, shared by the tests (the result is never modified)."""
    if key not in _cache:
        mgr = manager(model)
        _cache[key] = (mgr, mgr.forward_batch(copy.deepcopy(seqs)))
    return _cache[key]


def per_sequence(key, model, seqs):
    if key not in _cache:
        from detzero_amd.track_models import TrackManager
        mgr = TrackManager(model.TRACKING)
        _cache[key] = [mgr.forward(copy.deepcopy(s)) for s in seqs]
    return _cache[key]


def test_fixture_sequences_against_the_golden(device):
    loaded = fixtures()
    for group in ([0, 1], [2]):
        model = loaded[group[0]][1]
        mgr, results = batched(('golden', tuple(group)), model, [loaded[si][0] for si in group])
        assert mgr.seq_ops.reruns == 0 and mgr.fallbacks == 0 and mgr.batched > 0 and mgr.batched % len(group) == 0
        for si, mine in zip(group, results):
            assert_tracks(mine, loaded[si][2], 4 * loaded[si][5], 'sequence %d raw (batch of %d, device)' % (si, len(group)))


@pytest.mark.parametrize('cfg', [0, 2])
def test_three_sequences_in_one_call_equal_the_per_sequence_path(device, cfg):
    """Every field bit-identical to TrackManager.forward on HipTrackOps (scipy's assignment, one launch per op and frame)."""
    loaded = fixtures()
    model, seqs = loaded[cfg][1], [loaded[si][0] for si in range(3)]
    _, results = batched(('three', cfg), model, seqs)
    for got, want in zip(results, per_sequence(('three-per', cfg), model, seqs)):
        same_tracks(got, want)


def _seeded_model(point_threshold=5):
    model = copy.deepcopy(fixtures()[0][1])
    model.TRACKING.DATA_ASSOCIATION.STAGE.SECOND_STAGE.POINT_THRESHOLD = [point_threshold] * 3
    return model


@pytest.mark.parametrize('n_obj,n_frames', [(70, 10), (270, 6)], ids=['70-objects-cross-a-wave', '270-objects-cross-the-workgroup'])
def test_seeded_sequences_against_the_numpy_ops(device, n_obj, n_frames):
    """Discrete fields exact, boxes within 4 x the fp32 - fp64 difference of the numpy ops on the same sequence (the rule of the
    fixture's end-to-end test), with the `gaps` check on: no discrete decision of the run sits within 1e-3 of its threshold."""
    from detzero_amd.track_models import TrackManager
    model = _seeded_model()
    seq = track_seq_ref.seeded_sequence(n_obj, n_frames, seed=n_obj)
    gaps = {}
    ref32 = TrackManager(model.TRACKING, ops_factory=lambda: track_ref.NumpyTrackOps(np.float32, gaps)).forward(copy.deepcopy(seq))
    ref64 = TrackManager(model.TRACKING, ops_factory=lambda: track_ref.NumpyTrackOps(np.float64)).forward(copy.deepcopy(seq))
    for key in ('affinity', 'merge', 'gate'):
        assert key in gaps and min(gaps[key]) >= 1e-3, (key, min(gaps.get(key, [0.0])))
    assert list(ref32) == list(ref64) and len(ref32) >= n_obj
    diff = max(float(np.max(np.abs(ref32[t]['boxes_global'].astype(np.float64) - ref64[t]['boxes_global']))) for t in ref32)
    assert 0.0 < diff < 0.05
    mgr = manager(model)
    mine = mgr.forward_batch([copy.deepcopy(seq)])[0]
    assert_tracks(mine, ref32, 4 * diff, '%d seeded objects (device batch vs numpy ops)' % n_obj)
    assert any((t['hit'] == 2).any() for t in mine.values()) and any(t['hit'][0] != 1 for t in mine.values())
    # more detections in a frame than a wavefront (64) / than the workgroup (128 threads) has lanes, more tracks than 64 / 256
    assert max(len(f['score']) for f in seq.values()) > (64 if n_obj == 70 else 128) and len(mine) > (64 if n_obj == 70 else 256)


def test_small_capacities_overflow_rerun_and_agree(device):
    loaded = fixtures()
    model, seqs = loaded[0][1], [loaded[0][0], loaded[1][0]]
    _, roomy = batched(('golden', (0, 1)), model, seqs)
    mgr = manager(model, track_cap=4, log_cap=16)
    tight = mgr.forward_batch(copy.deepcopy(seqs))
    assert mgr.seq_ops.reruns >= 2                       # the word was set and the sequences were rerun, in both passes
    for got, want in zip(tight, roomy):
        same_tracks(got, want)


def test_overflow_word_names_the_capacity(device):
    """The no-sync entry itself: 3 tracks cannot hold the first frame (tracks), 4 log rows cannot hold the second (log); a roomy
    sequence next to them finishes."""
    from detzero_amd import ops
    from detzero_amd.track_models import HipSeqTrackOps, SeqPack, TrackManager
    seq, model = fixtures()[0][0], fixtures()[0][1]
    mgr = TrackManager(model.TRACKING)
    first = len(seq['0']['score'])
    assert first > 3
    pack = SeqPack(mgr, [copy.deepcopy(seq), {'0': copy.deepcopy(seq['0'])}])
    so = HipSeqTrackOps()
    rows, flags, frame_row, seq_frame = pack.subset([0, 1])
    args = (so._params(mgr), so._dev(rows).reshape(-1, 16), so._dev(flags), so._dev(frame_row), so._dev(seq_frame))
    _, count, ovf = ops.track_seq_pass_nosync(*args, 3, 3, max(pack.max_det), 64)
    assert ovf.cpu().tolist() == [ops.TRACK_SEQ_OVF_TRACKS, ops.TRACK_SEQ_OVF_TRACKS] and count.cpu().tolist() == [0, 0]
    _, count, ovf = ops.track_seq_pass_nosync(*args, 64, 64, max(pack.max_det), first)
    count = count.cpu().tolist()
    assert ovf.cpu().tolist() == [ops.TRACK_SEQ_OVF_LOG, 0] and 0 < count[1] <= first and count[0] == count[1]     # both logged frame 0


def test_doubled_capacity_is_tried_at_the_limit_before_giving_up(device, monkeypatch):
    """A sequence that needs exactly the limit of tracks, started one below it: the doubled capacity passes the limit, the limit
    itself is tried, and the sequence stays on the batched path.  (The limit is lowered on the Python side to what the fixture's
    sequence 2 needs - forward pass only - found with the no-sync entry; the kernel's own limit is untouched.)"""
    from detzero_amd import ops
    from detzero_amd.track_models import HipSeqTrackOps, SeqPack, TrackManager
    seq, model = fixtures()[2][0], fixtures()[2][1]
    assert not model.TRACKING.REVERSE_TRACKING.ENABLE
    plain = TrackManager(model.TRACKING)
    pack = SeqPack(plain, [copy.deepcopy(seq)])
    so = HipSeqTrackOps()
    rows, flags, frame_row, seq_frame = pack.subset([0])
    args = (so._params(plain), so._dev(rows).reshape(-1, 16), so._dev(flags), so._dev(frame_row), so._dev(seq_frame))

    def runs_out(cap):
        return bool(int(ops.track_seq_pass_nosync(*args, cap, cap, max(pack.max_det), 1 << 15)[2].cpu()[0]) & ops.TRACK_SEQ_OVF_TRACKS)

    lo, hi = 2, 256                                     # runs_out(lo), not runs_out(hi); need = the smallest capacity that holds
    assert runs_out(lo) and not runs_out(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if runs_out(mid) else (lo, mid)
    need = hi
    monkeypatch.setattr(ops, 'TRACK_SEQ_MAX_TRACKS', need)
    mgr = manager(model, track_cap=need - 1)
    got = mgr.forward_batch([copy.deepcopy(seq)])[0]
    assert (mgr.batched, mgr.fallbacks, mgr.seq_ops.reruns) == (1, 0, 1)
    same_tracks(got, plain.forward(copy.deepcopy(seq)))
    beyond = manager(model, track_cap=need - 1)         # one below what is needed as the limit: given up, tracked by forward
    monkeypatch.setattr(ops, 'TRACK_SEQ_MAX_TRACKS', need - 1)
    same_tracks(beyond.forward_batch([copy.deepcopy(seq)])[0], got)
    assert (beyond.batched, beyond.fallbacks) == (0, 1)


def test_sequence_beyond_the_detection_limit_takes_the_per_sequence_path(device):
    from detzero_amd import ops
    from detzero_amd.track_models import HipSeqTrackOps, TrackManager
    model = _seeded_model()
    big = track_seq_ref.seeded_sequence(ops.TRACK_SEQ_MAX_DET + 200, 2, seed=5, spacing=12.0)
    assert max(len(f['score']) for f in big.values()) > ops.TRACK_SEQ_MAX_DET
    small = track_seq_ref.seeded_sequence(20, 3, seed=6)
    seen = []

    class Recording(HipSeqTrackOps):
        def forward_pass(self, mgr, pack, seqs):
            seen.append(list(seqs))
            return super().forward_pass(mgr, pack, seqs)

    mgr = TrackManager(model.TRACKING, seq_ops_factory=Recording)
    results = mgr.forward_batch([copy.deepcopy(big), copy.deepcopy(small)])
    assert seen == [[1]] and (mgr.batched, mgr.fallbacks) == (1, 1)
    direct = TrackManager(model.TRACKING)
    same_tracks(results[0], direct.forward(copy.deepcopy(big)))
    same_tracks(results[1], direct.forward(copy.deepcopy(small)))
    assert len(results[0]) > ops.TRACK_SEQ_MAX_DET


def test_two_calls_and_a_second_instance_are_identical(device):
    loaded = fixtures()
    model, seqs = loaded[0][1], [loaded[0][0], loaded[1][0]]
    mgr, first = batched(('golden', (0, 1)), model, seqs)
    again = mgr.forward_batch(copy.deepcopy(seqs))
    other = manager(model).forward_batch(copy.deepcopy(seqs))
    for res in (again, other):
        for got, want in zip(res, first):
            same_tracks(got, want)


def test_run_model_batch_writes_the_same_pickles(device, tmp_path):
    from detzero_amd.config import AttrDict
    from detzero_amd.track_models import build_dataloader, build_model, run_model
    seq, model, _, _, _, _ = load_sequence(2)
    annos = []
    for name, shift in (('seq_one', 0.0), ('seq_two', 25.0), ('seq_three', -40.0)):
        for f, fr in seq.items():
            boxes = fr['boxes_global'].copy()
            boxes[:, 0] += np.float32(shift)
            annos.append({'sequence_name': name, 'frame_id': int(f), 'pose': np.eye(4), 'name': fr['name'], 'score': fr['score'], 'boxes_lidar': boxes})
    det = tmp_path / 'result.pkl'
    det.write_bytes(pickle.dumps(annos))
    cfg = AttrDict({'DATASET': 'WaymoTrackDataset', 'DATA_PATH': 'unused', 'PROCESSED_DATA_TAG': 'waymo_processed_data',
                    'DATA_PROCESSOR': [{'NAME': 'heading_process'}, {'NAME': 'transform_to_global'}]})
    saved = {}
    for batch in (0, 2):
        dataset, loader = build_dataloader(cfg, log_time='20240101-00000%d' % batch, data_path=str(det), batch_size=8, workers=4, split='test',
                                           logger=None, root_path=str(tmp_path))
        run_model(build_model(model), loader, dataset, workers=4, batch=batch)
        saved[batch] = (pickle.load(open(dataset.get_track_path(), 'rb')), pickle.load(open(dataset.get_drop_path(), 'rb')))
    assert list(saved[0][0]) == ['seq_one', 'seq_two', 'seq_three'] == list(saved[2][0])
    assert pickle.dumps(saved[0][1]) == pickle.dumps(saved[2][1])
    for name in saved[0][0]:
        a, b = saved[0][0][name], saved[2][0][name]
        assert list(a) == list(b) and len(a) >= 5
        for tid in a:
            assert a[tid]['state'] == b[tid]['state']
            for key in KEYS:
                assert np.array_equal(a[tid][key], b[tid][key]), (name, tid, key)
