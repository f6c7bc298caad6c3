"""GPU: the AB3DMOT filter on the device (csrc/track_ab3dmot.h through csrc/track.hip and csrc/track_seq.hip).

Op level against the numpy float64 ops (tests/track_ab3dmot_ref.py): tolerance 1e-10 of the largest entry of the compared array,
x and P separately.  Float64 eps 1.1e-16 x cond(S) <= 2e4 (S = P[:7,:7] + I, eigenvalues between 1 and about 1e4 + 11) gives about
2e-12; the tolerance allows x50 over that for the order of the sums.  Float32 arithmetic misses it by two orders and more.
Sequence level against the reference's own classes (tests/golden/track_ab3dmot_golden.npz) with the bound of the CPU test."""
import copy
import pickle

import numpy as np
import pytest
import torch

from tests import track_ab3dmot_ref as ab
from tests.track_ref import ROW_FRAME, ROW_HIT, ROW_ID, ROW_NPTS

gpu = pytest.mark.gpu
TOL = 1e-10
PI = np.pi
# (state theta, measured theta) on every branch of the correction, at -pi and just below pi, and outside [-pi, pi)
THETAS = ((0.3, 0.4), (0.3, 2.3), (3.0, -3.0), (-3.0, 3.0), (-PI, -PI + 0.05), (1.0, float(np.nextafter(PI, 0))), (3.3, 3.5))


def _pair(device, init_cap=256):
    from detzero_amd.track_models import HipTrackOps
    return HipTrackOps(device, init_cap=init_cap, filter='AB3DMOT'), ab.NumpyAb3dTrackOps('inv')


def _detections(n, seed):
    """n detections: (rows, boxes64) with float64 measurements that are NOT float32 values."""
    from detzero_amd.track_models import det_rows
    rng = np.random.default_rng(seed)
    boxes = np.concatenate([rng.uniform(-60, 60, (n, 2)), rng.uniform(-1, 2, (n, 1)), rng.uniform(0.5, 5.0, (n, 3)), rng.uniform(-PI, PI, (n, 1))], axis=1)
    rows = det_rows(boxes, rng.integers(0, 3, n).astype(np.int32), rng.uniform(0.1, 0.9, n).astype(np.float32), np.zeros(n, np.int32))
    return rows, boxes


def _spawn_both(dev, ref, n, seed):
    rows, boxes = _detections(n, seed)
    for o in (dev, ref):
        o.set_detections(rows, boxes)
        o.spawn('det', np.arange(n), 100 + 3 * np.arange(n), None, None, None)
    return rows, boxes


def _live_in(dev, ref, seed):
    """Overwrite both states: full symmetric positive definite P with eigenvalues between 1e-2 and 1e4, velocities, counters."""
    n = ref.n
    rng = np.random.default_rng(seed)
    xs, ps = np.zeros((n, 10)), np.zeros((n, 100))
    for i, t in enumerate(ref.tracks):
        q, _ = np.linalg.qr(rng.normal(size=(10, 10)))
        p = (q * 10.0 ** rng.uniform(-2, 4, 10)) @ q.T
        t.P = (p + p.T) / 2.
        t.x[7:, 0] = rng.uniform(-3, 3, 3)
        t.x[6, 0] = THETAS[i % len(THETAS)][0]
        t.hits, t.miss, t.hit = 1 + i % 4, i % 3, i % 2
        xs[i], ps[i] = t.x[:, 0], t.P.reshape(-1)
    if n:
        dev.ftable.x[:, :n] = torch.from_numpy(xs.T.copy()).to(dev.device)
        dev.ftable.P[:, :n] = torch.from_numpy(ps.T.copy()).to(dev.device)
        dev.ftable.hits[:n] = torch.tensor([t.hits for t in ref.tracks], dtype=torch.int32, device=dev.device)
        dev.table.miss[:n] = torch.tensor([t.miss for t in ref.tracks], dtype=torch.int32, device=dev.device)
        dev.table.hit[:n] = torch.tensor([t.hit for t in ref.tracks], dtype=torch.int32, device=dev.device)


def _dev_state(dev):
    torch.cuda.synchronize()
    n = dev.n
    f, t = dev.ftable, dev.table
    return {'x': f.x[:, :n].T.cpu().numpy(), 'P': f.P[:, :n].T.cpu().numpy(), 'box64': f.box[:, :n].T.cpu().numpy(), 'hits': f.hits[:n].cpu().numpy(),
            'box': t.box[:n].cpu().numpy(), 'cls': t.cls[:n].cpu().numpy(), 'score': t.score[:n].cpu().numpy(), 'num_points': t.num_points[:n].cpu().numpy(),
            'hit': t.hit[:n].cpu().numpy(), 'miss': t.miss[:n].cpu().numpy(), 'id': t.id[:n].cpu().numpy()}


def _ref_state(ref):
    tr = ref.tracks
    return {'x': np.array([t.x[:, 0] for t in tr]).reshape(-1, 10), 'P': np.array([t.P.reshape(-1) for t in tr]).reshape(-1, 100),
            'box64': np.array([np.asarray(t.bbox, dtype=np.float64) for t in tr]).reshape(-1, 9), 'hits': np.array([t.hits for t in tr], dtype=np.int32),
            'cls': np.array([t.cls for t in tr], dtype=np.int32), 'score': np.array([t.score for t in tr], dtype=np.float32),
            'num_points': np.array([t.num_points for t in tr], dtype=np.int32), 'hit': np.array([t.hit for t in tr], dtype=np.int32),
            'miss': np.array([t.miss for t in tr], dtype=np.int32), 'id': np.array([t.track_id for t in tr], dtype=np.int32)}


def _compare(got, exp, what, factor=1.0, rows=None):
    """x and P within TOL x factor of the array's largest entry; the float32 box = the rounding of the device's own float64 box;
    the discrete fields exactly."""
    sel = slice(None) if rows is None else rows
    for key in ('x', 'P', 'box64'):
        if exp[key][sel].size == 0:
            continue
        scale = float(np.max(np.abs(exp[key][sel])))
        err = float(np.max(np.abs(got[key][sel] - exp[key][sel])))
        print('%s: %s max error %.3e of %.3e (relative %.2e, bound %.1e)' % (what, key, err, scale, err / scale, TOL * factor))
        assert err <= TOL * factor * scale, (what, key, err, scale)
    assert np.array_equal(got['box'], got['box64'].astype(np.float32)), what
    for key in ('hits', 'cls', 'score', 'num_points', 'hit', 'miss', 'id'):
        assert np.array_equal(got[key], exp[key]), (what, key, got[key], exp[key])


# ------------------------------------------------------------------------------------------------
# op level
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_spawn_predict_update_one_step(device, n):
    dev, ref = _pair(device)
    _spawn_both(dev, ref, n, 40 + n)
    got, exp = _dev_state(dev), _ref_state(ref)
    assert np.array_equal(got['x'], exp['x']) and np.array_equal(got['P'], exp['P']) and np.array_equal(got['box64'], exp['box64'])
    assert (got['num_points'] == -1).all() and (got['hits'] == 1).all() and (got['box64'][:, 7:] == 0).all()
    _compare(got, exp, 'spawn n=%d' % n)
    assert dev.table.cap >= n and dev.ftable.cap == dev.table.cap

    _live_in(dev, ref, 50 + n)
    for o in (dev, ref):
        o.predict(0)
    _compare(_dev_state(dev), _ref_state(ref), 'predict n=%d' % n)

    # update: about two thirds of the tracks, in unsorted order, each from its own detection; theta on every branch
    _live_in(dev, ref, 60 + n)
    rng = np.random.default_rng(70 + n)
    chosen = rng.permutation(n)[:max(1, (2 * n) // 3)]
    slots = rng.permutation(n)[:len(chosen)]
    boxes = np.zeros((n, 7))
    for i, d in zip(chosen, slots):
        boxes[d] = ref.tracks[i].x[:7, 0] + rng.normal(0, 0.2, 7)
        boxes[d, 6] = THETAS[i % len(THETAS)][1]
    from detzero_amd.track_models import det_rows
    rows = det_rows(boxes, rng.integers(0, 3, n).astype(np.int32), rng.uniform(0.1, 0.9, n).astype(np.float32), np.zeros(n, np.int32))
    match = np.stack([chosen, slots, rng.integers(0, 2, len(chosen))], axis=1)          # the stage column is ignored
    before = _dev_state(dev)
    for o in (dev, ref):
        o.set_detections(rows, boxes)
        o.update(match, 1.0)
    got, exp = _dev_state(dev), _ref_state(ref)
    _compare(got, exp, 'update n=%d' % n)
    assert (got['hit'][chosen] == 1).all() and (got['miss'][chosen] == 0).all()
    assert (got['x'][chosen, 6] >= -PI).all() and (got['x'][chosen, 6] < PI).all()
    rest = np.setdiff1d(np.arange(n), chosen)
    for key in before:
        assert np.array_equal(got[key][rest], before[key][rest]), key


@gpu
def test_compact_by_death_age_carries_the_companion(device):
    dev, ref = _pair(device)
    _spawn_both(dev, ref, 300, 5)
    _live_in(dev, ref, 6)
    before = _dev_state(dev)
    keep = before['miss'] < 2
    for o in (dev, ref):
        assert o.compact(False, 2) == int(keep.sum())
    got = _dev_state(dev)
    for key in before:
        assert np.array_equal(got[key], before[key][keep]), key
    _compare(got, _ref_state(ref), 'compact')


@gpu
def test_log_applies_the_output_rule(device):
    """hits = birth - 1 and birth, miss = death - 1 and death, frame id below and at BIRTH_AGE."""
    birth, death = 3, 2
    dev, ref = _pair(device)
    _spawn_both(dev, ref, 9, 7)
    for o in (dev, ref):
        o.predict(0)
    cases = [(h, m) for h in (birth - 1, birth) for m in (death - 1, death)] * 2 + [(1, 0)]
    for t, (h, m) in zip(ref.tracks, cases):
        t.hits, t.miss = h, m
    dev.ftable.hits[:9] = torch.tensor([c[0] for c in cases], dtype=torch.int32, device=dev.device)
    dev.table.miss[:9] = torch.tensor([c[1] for c in cases], dtype=torch.int32, device=dev.device)
    for ordinal, frame_id in enumerate((birth - 1, birth)):
        for o in (dev, ref):
            o.log(ordinal, frame_id, birth, death)
    rows, _ = dev.fetch_log()
    exp_rows, _ = ref.fetch_log()
    assert np.array_equal(rows, exp_rows)
    assert np.array_equal(dev.fetch_log_boxes(), ref.fetch_log_boxes())
    expect = [k for k, (h, m) in enumerate(cases) if m < death] + [k for k, (h, m) in enumerate(cases) if h >= birth and m < death]
    assert rows[:, ROW_ID].tolist() == [100 + 3 * k for k in expect] and len(expect) == 5 + 2
    assert rows[:, ROW_FRAME].tolist() == [0] * 5 + [1] * 2 and (rows[:, ROW_NPTS] == -1).all()


@gpu
def test_birth_rows_carry_the_float32_box_and_the_flag(device):
    dev, ref = _pair(device)
    rows, boxes = _spawn_both(dev, ref, 5, 8)
    for o in (dev, ref):
        o.log(0, 0, 3, 2)
    got, _ = dev.fetch_log()
    assert (got[:, ab.ROW_AB3D] == ab.ROW_BIRTH).all()
    b64 = dev.fetch_log_boxes()
    assert np.array_equal(b64[:, :7], boxes.astype(np.float32).astype(np.float64)) and (b64[:, 7:] == 0).all()
    assert not np.array_equal(b64[:, :7], boxes)


@gpu
def test_zero_tracks_and_zero_detections(device):
    from detzero_amd.track_models import det_rows
    dev, _ = _pair(device)
    empty = det_rows(np.zeros((0, 7)), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.int32))
    dev.predict(0)
    dev.set_detections(empty, np.zeros((0, 7)))
    dev.update(np.zeros((0, 3), dtype=int), 1.0)
    dev.spawn('det', np.zeros(0, dtype=int), np.zeros(0, dtype=int), None, None, None)
    dev.log(0, 0, 3, 2)
    assert dev.compact(False, 2) == 0 and dev.n == 0
    rows, _ = dev.fetch_log()
    assert rows.shape == (0, 16) and dev.fetch_log_boxes().shape == (0, 9)
    # tracks without detections: a predict-only frame
    rows, boxes = _detections(3, 9)
    dev.set_detections(rows, boxes)
    dev.spawn('det', np.arange(3), np.arange(3), None, None, None)
    dev.predict(0)
    dev.set_detections(empty, np.zeros((0, 7)))
    dev.update(np.zeros((0, 3), dtype=int), 1.0)
    dev.log(1, 1, 3, 2)
    rows, _ = dev.fetch_log()
    assert rows[:, ROW_HIT].tolist() == [0, 0, 0]


@gpu
def test_thirty_step_chain(device):
    n, steps = 65, 30
    dev, ref = _pair(device)
    _, boxes0 = _spawn_both(dev, ref, n, 11)
    from detzero_amd.track_models import det_rows
    rng = np.random.default_rng(12)
    vel = rng.uniform(-1.5, 1.5, (n, 3)) * np.array([1, 1, 0.05])
    spin = rng.uniform(-0.25, 0.25, n)             # headings walk, some across +-pi
    for k in range(1, steps + 1):
        boxes = boxes0.copy()
        boxes[:, :3] += vel * k + rng.normal(0, 0.05, (n, 3))
        boxes[:, 6] = boxes0[:, 6] + spin * k
        if k % 7 == 0:
            boxes[::4, 6] += PI                     # a turned detection
        seen = np.flatnonzero((np.arange(n) + k) % 5 != 0)
        seen = seen[rng.permutation(len(seen))]
        rows = det_rows(boxes, np.zeros(n, np.int32), np.full(n, 0.5, np.float32), np.zeros(n, np.int32))
        match = np.stack([seen, seen, np.zeros_like(seen)], axis=1)
        for o in (dev, ref):
            o.predict(0)
            o.set_detections(rows, boxes)
            o.update(match, 1.0)
    _compare(_dev_state(dev), _ref_state(ref), 'chain of %d steps' % steps, factor=float(steps))


# ------------------------------------------------------------------------------------------------
# sequence level
# ------------------------------------------------------------------------------------------------
_results = {}


def _tracked(ri, device):
    from detzero_amd.track_models import TrackManager
    if ri not in _results:
        seq, model, ref, solve_diff = ab.load_run(ri)
        mgr = TrackManager(model.TRACKING)
        _results[ri] = (mgr, mgr.forward(copy.deepcopy(seq)))
    return _results[ri]


@gpu
@pytest.mark.parametrize('ri', range(ab.N_RUNS))
def test_fixture_sequences_end_to_end(device, ri):
    seq, model, ref, solve_diff = ab.load_run(ri)
    mgr, mine = _tracked(ri, device)
    assert type(mgr.ops).__name__ == 'HipTrackOps' and mgr.ops.ab3d
    ab.assert_tracks(mine, ref, ab.box_tolerance(ref, solve_diff), 'run %d (device, solve_diff %.2e)' % (ri, solve_diff))
    for tk in mine.values():
        assert (tk['num_points'] == -1).all() and set(np.unique(tk['hit'])) <= {0, 1}


def _more_sequences():
    from tests.track_seq_ref import seeded_sequence
    return [seeded_sequence(9, 11, 3), seeded_sequence(14, 5, 4), {}]


@gpu
@pytest.mark.parametrize('ri', range(ab.N_RUNS))
def test_forward_batch_equals_forward_bytewise(device, ri):
    from detzero_amd.track_models import HipSeqTrackOps, TrackManager
    seq, model, ref, solve_diff = ab.load_run(ri)
    batch = [seq] + _more_sequences()
    one = TrackManager(model.TRACKING)
    expect = [one.forward(copy.deepcopy(s)) for s in batch]
    assert len(expect[1]) > 0 and len(expect[2]) > 0 and expect[3] == {}
    mgr = TrackManager(model.TRACKING)
    got = mgr.forward_batch(copy.deepcopy(batch))
    assert mgr.batched == len(batch) and mgr.fallbacks == 0 and mgr.seq_ops.reruns == 0
    for a, b in zip(got, expect):
        ab.same_tracks(a, b)
    ab.assert_tracks(got[0], ref, ab.box_tolerance(ref, solve_diff), 'run %d (forward_batch)' % ri)
    # capacities forced small: the overflow words, the reruns with doubled capacities, the same rows
    small = TrackManager(model.TRACKING, seq_ops_factory=lambda: HipSeqTrackOps(track_cap=4, log_cap=8))
    again = small.forward_batch(copy.deepcopy(batch))
    assert small.seq_ops.reruns > 0 and small.fallbacks == 0
    for a, b in zip(again, expect):
        ab.same_tracks(a, b)


@gpu
def test_rerun_and_second_instance_give_identical_results(device):
    from detzero_amd.track_models import TrackManager
    seq, model, _, _ = ab.load_run(1)
    mgr, first = _tracked(1, device)
    ab.same_tracks(mgr.forward(copy.deepcopy(seq)), first)
    ab.same_tracks(TrackManager(model.TRACKING).forward(copy.deepcopy(seq)), first)
    other = TrackManager(model.TRACKING)
    ab.same_tracks(other.forward_batch([copy.deepcopy(seq)])[0], first)
    ab.same_tracks(other.forward_batch([copy.deepcopy(seq)])[0], first)


@gpu
@pytest.mark.parametrize('batch', [0, 2])
def test_run_model_over_a_result_pickle(device, tmp_path, batch):
    from detzero_amd.config import AttrDict
    from detzero_amd.track_models import build_dataloader, build_model, run_model
    seq, model, _, _ = ab.load_run(0)
    annos = []
    for name, shift in (('seq_one', 0.0), ('seq_two', 25.0)):
        for f, fr in seq.items():
            boxes = fr['boxes_global'].astype(np.float32)
            boxes[:, 0] += np.float32(shift)
            annos.append({'sequence_name': name, 'frame_id': int(f), 'pose': np.eye(4), 'name': fr['name'], 'score': fr['score'], 'boxes_lidar': boxes})
    det = tmp_path / 'result.pkl'
    det.write_bytes(pickle.dumps(annos))
    cfg = AttrDict({'DATASET': 'WaymoTrackDataset', 'DATA_PATH': 'unused', 'PROCESSED_DATA_TAG': 'waymo_processed_data',
                    'DATA_PROCESSOR': [{'NAME': 'heading_process'}, {'NAME': 'low_confidence_box_filter', 'THRESHOLD': 0.1},
                                       {'NAME': 'transform_to_global'}]})
    dataset, loader = build_dataloader(cfg, log_time='20240101-000000', data_path=str(det), batch_size=8, workers=4, split='test', logger=None,
                                       root_path=str(tmp_path))
    tracker = build_model(model)
    run_model(tracker, loader, dataset, workers=4, batch=batch)
    saved = pickle.load(open(dataset.get_track_path(), 'rb'))
    assert list(saved) == ['seq_one', 'seq_two']
    if batch:
        assert tracker.module_list[0].batched == 2 and tracker.module_list[0].fallbacks == 0
    for k in range(2):
        direct = build_model(model).forward(copy.deepcopy(dataset[k][1]['detection']))
        got = saved[dataset.seq_name_list[k]]
        assert list(got) == list(direct) and len(got) >= 5
        for tid in direct:
            assert got[tid]['state'] == direct[tid]['state'] and got[tid]['boxes_global'].dtype == direct[tid]['boxes_global'].dtype
            # (a track whose only row is its birth row keeps the reference's float32)
            assert got[tid]['boxes_global'].dtype == (np.float64 if len(got[tid]['hit']) > 1 else np.float32)
            for key in ab.KEYS:
                assert np.array_equal(got[tid][key], direct[tid][key]), (tid, key)
