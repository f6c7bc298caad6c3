"""Tracker kernels on the device (csrc/track.hip) against tests/track_ref.py, op by op at the smallest shapes where each can go
wrong, then the fixture sequences of tests/golden/track_model_golden.npz end to end through DetZeroTracker.

Tolerances.  eps = 2^-23.
  predict   every output is a sum of at most four products of entries of P / Q (|dt| < 1): both sides are fp32 in another
            order, so they differ by at most 8 eps max(|P|, |Q|) per track; x by 4 eps max|x|.  After k steps against float64 the
            roundings add up: k times those bounds.
  update    S^-1 comes from cofactors here and from LAPACK there; either has a relative error of a small multiple of
            cond(S) eps, and K, x, P are sums of three products of it: 32 cond(S) eps times the magnitude of the terms
            (max|P| for P; max(|v|, 3 max|P| max|z - x|) for the velocities), cond from the float64 restatement.
  Discrete fields, copied values (stage 2 leaves x / P / box alone, a stage-1 box is the detection's, a spawned track's matrices)
  and the cost matrices (the pair bodies are those of dz_boxes_iou_bev / dz_boxes_pairwise_metric) are compared bit for bit.
  End to end: 4 x the fixture's fp32 - fp64 difference of the reference, as the fixture's generator explains.
"""
import copy
import pickle

import numpy as np
import pytest
import torch

from tests import track_ref
from tests.test_track_models import KEYS, assert_tracks, load_sequence

gpu = pytest.mark.gpu
EPS = 2.0 ** -23
P0, Q0 = (50.0, 1000.0), (5.0, 15.0)
FIELDS = ('x', 'P', 'Q', 'dt', 'box', 'cls', 'score', 'update_score', 'num_points', 'hit', 'miss', 'id')


def _dev(a, device, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


def make_tracks(n, seed, dtype=np.float32):
    """n tracks in a lived-in state: full SPD P (condition number of its 3x3 corner below ~50), grown Q, speeds on both sides of the
    gate, both signs of delta_t.  Track 0..2 (when present): a Vehicle just under the gate, just over it, a Pedestrian in the
    same state as the first."""
    from detzero_amd.synth import synth_boxes
    rng = np.random.default_rng(seed)
    boxes = synth_boxes(seed, max(n, 1), xy_range=30.0, near_duplicates=0.4)[:n]
    tracks = []
    for k in range(n):
        dt = -0.1 if k % 3 == 2 else 0.1
        t = track_ref.Track(boxes[k], k % 3, np.float32(rng.uniform(0.05, 0.95)), int(rng.integers(0, 900)), 1000 - 3 * k, P0, Q0, dt, dtype)
        a = rng.normal(0, 1, size=(5, 5))
        t.P = (a @ a.T + 3.0 * np.eye(5)).astype(dtype)
        t.Q = (t.Q * 1.5 ** int(rng.integers(0, 5))).astype(dtype)
        t.x[3:, 0] = rng.uniform(-6, 6, size=2)
        t.hit, t.miss = int(rng.integers(0, 3)), int(rng.integers(0, 4))
        tracks.append(t)
    for k, (cls, factor) in enumerate(((0, 0.99), (0, 1.01), (1, 0.99))):
        if k < n:
            t = tracks[k]
            t.cls = cls
            half = float(np.max(t.size)) / 2.0
            t.x[3:, 0] = np.array([0.6, 0.8]) * half * factor
    for t in tracks:
        t.bbox[7:9] = t.x[3:, 0]
    return tracks


def upload(tracks, device, cap=None):
    from detzero_amd import ops
    n = len(tracks)
    table = ops.TrackTable(cap or max(n, 1), device)
    if n:
        host = {'x': [t.x.reshape(5) for t in tracks], 'P': [t.P.reshape(25) for t in tracks], 'Q': [t.Q.reshape(25) for t in tracks],
                'dt': [t.F[0, 3] for t in tracks], 'box': [t.bbox for t in tracks], 'cls': [t.cls for t in tracks], 'score': [t.score for t in tracks],
                'update_score': [t.update_score for t in tracks], 'num_points': [t.num_points for t in tracks], 'hit': [t.hit for t in tracks],
                'miss': [t.miss for t in tracks], 'id': [t.track_id for t in tracks]}
        for name in FIELDS:
            arr = table.arrays[name]
            arr[:n].copy_(_dev(np.array(host[name]), device, arr.dtype).reshape(arr[:n].shape))
    return table


def download(table, n):
    torch.cuda.synchronize()
    return {name: table.arrays[name][:n].cpu().numpy() for name in FIELDS}


def host_state(tracks):
    return {'x': np.array([t.x.reshape(5) for t in tracks]).reshape(-1, 5), 'P': np.array([t.P.reshape(25) for t in tracks]).reshape(-1, 25),
            'Q': np.array([t.Q.reshape(25) for t in tracks]).reshape(-1, 25), 'box': np.array([t.bbox for t in tracks]).reshape(-1, 9),
            'hit': np.array([t.hit for t in tracks]), 'miss': np.array([t.miss for t in tracks]), 'cls': np.array([t.cls for t in tracks])}


def det_buffer(n, seed, device, near=None):
    """(rows host (n,16) int32, device copy): detections around the boxes `near` (so that pairs overlap) or anywhere."""
    from detzero_amd.synth import synth_boxes
    from detzero_amd.track_models import det_rows
    rng = np.random.default_rng(seed)
    boxes = synth_boxes(seed, max(n, 1), xy_range=30.0, near_duplicates=0.4)[:n]
    if near is not None and len(near) and n:
        src = near[rng.integers(0, len(near), size=n)]
        boxes = src[:, :7] + rng.normal(0, 0.15, size=(n, 7)).astype(np.float32) * np.array([1, 1, 1, 0.3, 0.3, 0.3, 0.2], np.float32)
    score = rng.uniform(0.0, 1.0, size=n).astype(np.float32)
    if n:
        score[0] = 0.01                 # below the 0.03 floor of update_score
    rows = det_rows(boxes.astype(np.float32), rng.integers(0, 3, size=n).astype(np.int32), score, rng.integers(0, 900, size=n))
    return rows, _dev(rows, device, torch.int32).reshape(-1, 16)


# ------------------------------------------------------------------------------------------------
# predict
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 257])
def test_predict_one_step(device, n):
    from detzero_amd import ops
    tracks = make_tracks(n, 10 + n)
    table = upload(tracks, device)
    before = download(table, n)
    ops.track_predict_nosync(table, n, 0)
    got = download(table, n)
    for t in tracks:
        t.predict(0)
    ref = host_state(tracks)
    assert np.array_equal(got['hit'], np.zeros(n)) and np.array_equal(got['miss'], before['miss'] + 1)
    for name in ('cls', 'score', 'update_score', 'num_points', 'id', 'dt'):
        assert np.array_equal(got[name], before[name]), name
    assert np.array_equal(got['box'][:, 3:7], before['box'][:, 3:7])
    assert np.array_equal(got['box'][:, :3], got['x'][:, :3]) and np.array_equal(got['box'][:, 7:9], got['x'][:, 3:5])
    if n >= 3:          # the gate: Vehicle just under -> stopped, just over -> moving, Pedestrian in the first one's state -> moving
        assert np.all(got['x'][0, 3:] == 0) and np.all(got['x'][1, 3:] != 0) and np.all(got['x'][2, 3:] != 0)
        assert np.array_equal(got['x'][0, :2], before['x'][0, :2])
    assert np.array_equal(got['x'][:, 3:] == 0, ref['x'][:, 3:] == 0)
    for k in range(n):
        scale = max(np.abs(ref['P'][k]).max(), np.abs(ref['Q'][k]).max())
        assert np.abs(got['P'][k] - ref['P'][k]).max() <= 8 * EPS * scale
        assert np.array_equal(got['Q'][k], ref['Q'][k])                         # one exact-order product per entry
        assert np.abs(got['x'][k] - ref['x'][k]).max() <= 4 * EPS * np.abs(ref['x'][k]).max()


@gpu
def test_predict_sixty_steps_against_float64(device):
    from detzero_amd import ops
    n, steps = 65, 60
    tracks = make_tracks(n, 7)
    ref = make_tracks(n, 7, np.float64)
    for t32, t64 in zip(tracks, ref):           # the same fp32 start on both sides
        t64.x, t64.P, t64.Q, t64.bbox = t32.x.astype(np.float64), t32.P.astype(np.float64), t32.Q.astype(np.float64), t32.bbox.astype(np.float64)
        t64.size = t32.size.astype(np.float64)
    table = upload(tracks, device)
    for _ in range(steps):
        ops.track_predict_nosync(table, n, 0)
    got = download(table, n)
    for t in ref:
        for _ in range(steps):
            t.predict(0)
    want = host_state(ref)
    assert np.array_equal(got['miss'], np.array([t.miss for t in ref]))
    worst = 0.0
    for k in range(n):
        scale = max(np.abs(want['P'][k]).max(), np.abs(want['Q'][k]).max())
        worst = max(worst, float(np.abs(got['P'][k] - want['P'][k]).max() / (steps * 8 * EPS * scale)))
        assert np.abs(got['Q'][k] - want['Q'][k]).max() <= steps * EPS * np.abs(want['Q'][k]).max()
        assert np.abs(got['x'][k] - want['x'][k]).max() <= steps * 4 * EPS * np.abs(want['x'][k]).max()
    print('60 predicts: worst P error / bound = %.3f, largest Q %.3e' % (worst, float(want['Q'].max())))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------
# affinity
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('shape', [(0, 5), (5, 0), (1, 1), (33, 65), (65, 33)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('metric', ['IoUBEV', 'IoU3D', 'GIoU3D'])
def test_affinity_is_the_pair_matrix_plus_the_host_masking(device, shape, metric):
    from detzero_amd import ops
    from detzero_amd.track_models import METRICS
    t, d = shape
    tracks = make_tracks(t, 40 + t)
    table = upload(tracks, device)
    tbox = np.array([tr.bbox for tr in tracks], dtype=np.float32).reshape(-1, 9)
    n_ext = 9
    ext_rows, ext_dev = det_buffer(n_ext, 5, device, near=tbox if t else None)
    det_rows_h, det_dev = det_buffer(d + 4, 6, device, near=tbox if t else None)
    rng = np.random.default_rng(t * 100 + d)
    # row subset of the table in a scrambled order plus some forward rows (negative = ext row), column subset of the frame
    rows = np.concatenate([rng.permutation(t)[:max(t - 2, min(t, 1))], -rng.permutation(n_ext)[:4] - 1 if t else np.zeros(0, int)]).astype(int)
    cols = rng.permutation(d + 4)[:d] if d else np.zeros(0, int)
    rbox = np.array([tbox[r, :7] if r >= 0 else ext_rows[-r - 1, :7].view(np.float32) for r in rows], dtype=np.float32).reshape(-1, 7)
    rcls = np.array([tracks[r].cls if r >= 0 else ext_rows[-r - 1, 13] for r in rows], dtype=int)
    cbox = det_rows_h[cols, :7].copy().view(np.float32).reshape(-1, 7)
    ccls = det_rows_h[cols, 13]
    thr = [0.2, 0.1, 0.15]
    for distinguish in (True, False):
        got = ops.track_affinity_nosync(table, t, ext_dev, _dev(rows, device, torch.int32), det_dev, _dev(cols, device, torch.int32),
                                        METRICS[metric], distinguish, thr).cpu().numpy()
        assert got.shape == (len(rows), len(cols)) and got.dtype == np.float32
        if got.size == 0:
            continue
        a, b = _dev(rbox, device, torch.float32), _dev(cbox, device, torch.float32)
        aff = (ops.boxes_pairwise(a, b, True) if metric == 'IoUBEV' else
               ops.boxes_pairwise_metric(a, b, ops.BOXM_IOU3D if metric == 'IoU3D' else ops.BOXM_GIOU3D)).cpu().numpy()
        live = int((aff > 0).sum())
        want = track_ref.cost_of(track_ref.mask_affinity(aff, rcls, ccls, distinguish, thr))
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (metric, distinguish, np.abs(got - want).max())
        if min(t, d) >= 33:
            assert live >= 10 and (want < 1).any() and (want == 5000).any()


# ------------------------------------------------------------------------------------------------
# update / spawn
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('m,grown', [(0, 1.0), (1, 1.0), (64, 1.0), (65, 1.0), (65, 2.0 ** 80)], ids=['0', '1', '64', '65', '65-after-a-long-coast'])
def test_update_mixed_stages(device, m, grown):
    """grown: P and Q as they are after some two hundred predicted frames (Q *= 1.5 per frame, matched or not): the products of a
    3x3 inverse's cofactors would leave fp32 unless S is scaled first."""
    from detzero_amd import ops
    n = m + 3
    tracks = make_tracks(n, 70 + m)
    for t in tracks:
        t.P, t.Q = t.P * np.float32(grown), t.Q * np.float32(grown)
    table = upload(tracks, device)
    before = download(table, n)
    tbox = np.array([t.bbox for t in tracks], dtype=np.float32)
    det_h, det_dev = det_buffer(m + 2, 8, device, near=tbox)
    rng = np.random.default_rng(m)
    trk = rng.permutation(n)[:m]
    det = rng.permutation(m + 2)[:m]
    stage = (np.arange(m) % 3 == 0).astype(int)
    match = np.stack([trk, det, stage], axis=1).astype(np.int32).reshape(-1, 3)
    ref64 = make_tracks(n, 70 + m, np.float64)
    if m:
        ops.track_update_nosync(table, n, det_dev, _dev(match, device, torch.int32), 0.1)
    got = download(table, n)
    untouched = np.setdiff1d(np.arange(n), trk)
    for name in FIELDS:
        assert np.array_equal(got[name][untouched], before[name][untouched]), name
    for i, di, st in match:
        d = det_h[di]
        dbox, dscore = d[:7].view(np.float32), d[9:10].view(np.float32)[0]
        assert got['miss'][i] == 0 and got['score'][i] == dscore and got['num_points'][i] == d[11]
        if st:          # second stage: the filter state is untouched bit for bit
            assert got['hit'][i] == 2
            for name in ('x', 'P', 'Q', 'box', 'cls', 'update_score'):
                assert np.array_equal(got[name][i], before[name][i]), name
            continue
        assert got['hit'][i] == 1 and got['cls'][i] == d[13] and got['update_score'][i] == max(dscore, np.float32(0.03))
        assert np.array_equal(got['box'][i, :7], dbox) and np.array_equal(got['x'][i, :3], dbox[:3])
        assert np.array_equal(got['box'][i, 7:9], got['x'][i, 3:5]) and np.array_equal(got['Q'][i], before['Q'][i])
        t32, t64 = tracks[i], ref64[i]
        t64.x, t64.P = t32.x.astype(np.float64), t32.P.astype(np.float64)
        s64 = t64.P[:3, :3] + 0.1 * np.eye(3)
        cond, s_inv = np.linalg.cond(s64), float(np.abs(np.linalg.inv(s64)).max())
        t32.update(dbox, d[13], dscore, d[11], 0, 0.1)
        t64.update(dbox, d[13], dscore, d[11], 0, 0.1)
        # |K| <= 3 max|P| max|S^-1| and |K res| <= 3 |K| max|res|
        pmax = float(np.abs(before['P'][i]).max())
        res = float(np.abs(dbox[:3].astype(np.float64) - before['x'][i, :3]).max())
        tol = 32 * cond * EPS
        assert np.isfinite(got['P'][i]).all() and np.isfinite(got['x'][i]).all()
        for want in (t32, t64):         # the fp32 port and the float64 yardstick
            assert np.abs(got['P'][i] - want.P.reshape(25)).max() <= tol * pmax, (i, cond)
            assert np.abs(got['x'][i, 3:] - want.x[3:, 0]).max() <= tol * max(float(np.abs(before['x'][i, 3:]).max()), 9 * pmax * s_inv * res), (i, cond)


@gpu
@pytest.mark.parametrize('m', [0, 1, 64, 65])
def test_spawn_from_detections_and_from_forward_rows(device, m):
    from detzero_amd import ops
    n = 5
    tracks = make_tracks(n, 3)
    for source, dt in (('det', 0.1), ('ext', -0.1)):
        table = upload(tracks, device, cap=n + m + 1)
        before = download(table, n)
        src_h, src_dev = det_buffer(m + 3, 9, device)
        idx = np.random.default_rng(m).permutation(m + 3)[:m]
        ids = 500 + 7 * np.arange(m)
        if m:
            ops.track_spawn_nosync(table, n, src_dev, _dev(idx, device, torch.int32), _dev(ids, device, torch.int32), P0, Q0, dt)
        got = download(table, n + m)
        for name in FIELDS:
            assert np.array_equal(got[name][:n], before[name]), name
        for k in range(m):
            ref = track_ref.Track(src_h[idx[k], :7].view(np.float32), src_h[idx[k], 13], src_h[idx[k], 9:10].view(np.float32)[0],
                                  src_h[idx[k], 11], ids[k], P0, Q0, dt)
            i = n + k
            assert np.array_equal(got['x'][i], ref.x.reshape(5)) and np.array_equal(got['P'][i], ref.P.reshape(25))
            assert np.array_equal(got['Q'][i], ref.Q.reshape(25)) and np.array_equal(got['box'][i], ref.bbox)
            assert got['dt'][i] == np.float32(dt) and got['cls'][i] == ref.cls and got['id'][i] == ids[k]
            assert got['score'][i] == ref.score and got['update_score'][i] == ref.score and got['num_points'][i] == ref.num_points
            assert got['hit'][i] == 1 and got['miss'][i] == 0
    with pytest.raises(Exception):
        ops.track_spawn_nosync(upload(tracks, device, cap=n), n, src_dev, _dev([0], device, torch.int32), _dev([1], device, torch.int32), P0, Q0, 0.1)


@gpu
def test_ops_object_grows_its_table_and_log(device):
    from detzero_amd.track_models import HipTrackOps
    ops_obj = HipTrackOps(device, init_cap=4)
    rows, _ = det_buffer(70, 2, device)
    ops_obj.set_detections(rows)
    ops_obj.spawn('det', np.arange(3), np.arange(3), P0, Q0, 0.1)
    ops_obj.spawn('det', np.arange(3, 70), np.arange(3, 70), P0, Q0, 0.1)
    assert ops_obj.n == 70 and ops_obj.table.cap >= 70 and ops_obj.spare.cap == ops_obj.table.cap
    for frame in range(3):
        ops_obj.log(frame)
    log, _ = ops_obj.fetch_log()
    assert log.shape == (210, 16)
    assert np.array_equal(log[:70, :7], rows[:, :7]) and np.array_equal(log[140:, 12], np.arange(70)) and np.all(log[70:140, 14] == 1)
    assert np.array_equal(log[:70, 13], rows[:, 13]) and np.all(log[:, 10] == 1) and np.array_equal(log[:70, 11], rows[:, 11])


# ------------------------------------------------------------------------------------------------
# merge + compact
# ------------------------------------------------------------------------------------------------
def _merge_case(tracks, thr, device):
    """Device verdicts and the numpy sweep on the device's own overlap matrix; then the compaction."""
    from detzero_amd import ops
    n = len(tracks)
    table = upload(tracks, device)
    before = download(table, n)
    removed = ops.track_merge_nosync(table, n, thr)
    boxes = _dev(np.array([t.bbox[:7] for t in tracks], np.float32).reshape(-1, 7), device, torch.float32)
    overlap = ops.boxes_pairwise(boxes, boxes, False).cpu().numpy() if n else np.zeros((0, 0), np.float32)
    b = boxes.cpu().numpy()
    want = track_ref.merge_sweep(overlap, b[:, 3] * b[:, 4], [t.cls for t in tracks], [t.track_id for t in tracks], thr)
    got = removed.cpu().numpy().astype(bool)
    assert np.array_equal(got, want), (np.flatnonzero(got), np.flatnonzero(want))
    spare = ops.TrackTable(max(n, 1), device)
    count = int(ops.track_compact_nosync(table, n, removed if n else None, -1, spare).item())
    assert count == int((~want).sum())
    after = download(spare, count)
    for name in FIELDS:         # surviving order preserved in every array
        assert np.array_equal(after[name], before[name][~want]), name
    return want


def _boxes_tracks(boxes, cls, ids):
    return [track_ref.Track(np.asarray(b, np.float32), c, np.float32(0.5), 10, i, P0, Q0, 0.1) for b, c, i in zip(boxes, cls, ids)]


@gpu
@pytest.mark.parametrize('t', [0, 1, 2, 64, 65, 130])
def test_merge_and_compact_random_clusters(device, t):
    tracks = make_tracks(t, 20 + t)
    rng = np.random.default_rng(t)
    for tr, tid in zip(tracks, rng.permutation(t) + 11):        # ids not in list order
        tr.track_id = int(tid)
    for tr in tracks:
        tr.cls = int(rng.integers(0, 2))
    want = _merge_case(tracks, [0.5, 0.4, 0.4], device)
    if t >= 64:
        assert 2 <= want.sum() < t - 2


@gpu
def test_merge_scripted_cases(device):
    car = [0, 0, 0, 4.5, 2.0, 1.6, 0.0]

    def shifted(dx, dy=0.0):
        b = list(car)
        b[0], b[1] = dx, dy
        return b
    thr = [0.5, 0.4, 0.4]
    chain = [shifted(0.0), shifted(1.8), shifted(3.6)]
    assert _merge_case(_boxes_tracks(chain, [0, 0, 0], [0, 1, 2]), thr, device).tolist() == [False, True, False]
    # the middle box carries the lowest id: row A's set {A, B} keeps B and drops A; B's column is cleared, so C is alone and stays
    assert _merge_case(_boxes_tracks(chain, [0, 0, 0], [5, 1, 7]), thr, device).tolist() == [True, False, False]
    # lowest id of C's set (B, id 1) was deprecated by row A (id 0): C keeps itself
    assert _merge_case(_boxes_tracks(chain, [0, 0, 0], [0, 1, 2]), thr, device)[2] == False            # noqa: E712
    # the same geometry in different classes
    assert not _merge_case(_boxes_tracks(chain, [0, 1, 2], [0, 1, 2]), thr, device).any()
    # a small box inside a large one: the ratio is over the ROW's own area, so the order of the two decides
    big, small = [0, 0, 0, 8.0, 4.0, 2.0, 0.3], [0.5, 0.2, 0, 1.0, 1.0, 1.0, 0.3]
    assert _merge_case(_boxes_tracks([big, small], [0, 0], [5, 3]), thr, device).tolist() == [False, False]
    assert _merge_case(_boxes_tracks([small, big], [0, 0], [3, 5]), thr, device).tolist() == [False, True]
    # everything overlapping everything, across three mask words: only the lowest id stays
    n = 130
    ids = np.random.default_rng(0).permutation(n) + 3
    want = _merge_case(_boxes_tracks([shifted(0.001 * k) for k in range(n)], [0] * n, ids), thr, device)
    assert (~want).sum() == 1 and ids[~want][0] == 3
    # two clusters in different words, far apart, plus loners in between
    far = [shifted(0.0)] + [shifted(40.0 * (k + 1)) for k in range(70)] + [shifted(0.3)]
    want = _merge_case(_boxes_tracks(far, [0] * 72, list(range(72))), thr, device)
    assert np.flatnonzero(want).tolist() == [71]


@gpu
def test_compact_by_death_age(device):
    from detzero_amd import ops
    n = 300
    tracks = make_tracks(n, 1)
    table = upload(tracks, device)
    before = download(table, n)
    spare = ops.TrackTable(n, device)
    count = int(ops.track_compact_nosync(table, n, None, 2, spare).item())
    keep = before['miss'] < 2
    assert count == int(keep.sum()) and 0 < count < n
    after = download(spare, count)
    for name in FIELDS:
        assert np.array_equal(after[name], before[name][keep]), name
    assert int(ops.track_compact_nosync(table, n, None, -1, spare).item()) == n


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
_results = {}


def _tracked(si, device):
    """One device run of a fixture sequence, shared by the tests below: (tracker, raw tracks, post-processed tracks)."""
    if si not in _results:
        from detzero_amd.track_models import build_model
        seq, model, _, _, _, _ = load_sequence(si)
        tracker = build_model(model)
        raw = tracker.module_list[0].forward(copy.deepcopy(seq))
        final = tracker.module_list[1].forward(copy.deepcopy(raw))
        _results[si] = (tracker, raw, final)
    return _results[si]


@gpu
@pytest.mark.parametrize('si', [0, 1, 2])
def test_fixture_sequences_end_to_end(device, si):
    seq, model, raw, final, states, diff = load_sequence(si)
    tracker, mine_raw, mine_final = _tracked(si, device)
    assert_tracks(mine_raw, raw, 4 * diff, 'sequence %d raw (device)' % si)
    assert [t['state'] for t in mine_final.values()] == states.tolist()
    assert_tracks(mine_final, final, 4 * diff, 'sequence %d post-processed (device)' % si)


@gpu
def test_rerun_and_second_instance_give_identical_results(device):
    from detzero_amd.track_models import build_model
    seq, model, _, _, _, _ = load_sequence(2)
    tracker, _, first = _tracked(2, device)
    again = tracker.forward(copy.deepcopy(seq))
    other = build_model(model).forward(copy.deepcopy(seq))
    for res in (again, other):
        assert list(res) == list(first)
        for tid in first:
            assert res[tid]['state'] == first[tid]['state']
            for key in KEYS:
                assert np.array_equal(res[tid][key], first[tid][key]), (tid, key)


@gpu
def test_run_model_over_a_result_pickle(device, tmp_path):
    from detzero_amd.config import AttrDict
    from detzero_amd.track_models import build_dataloader, build_model, run_model
    seq, model, _, _, _, _ = load_sequence(2)
    annos = []
    for name, shift in (('seq_one', 0.0), ('seq_two', 25.0)):
        for f, fr in seq.items():
            boxes = fr['boxes_global'].copy()
            boxes[:, 0] += np.float32(shift)
            annos.append({'sequence_name': name, 'frame_id': int(f), 'pose': np.eye(4), 'name': fr['name'], 'score': fr['score'], 'boxes_lidar': boxes})
    det = tmp_path / 'result.pkl'
    det.write_bytes(pickle.dumps(annos))
    cfg = AttrDict({'DATASET': 'WaymoTrackDataset', 'DATA_PATH': 'unused', 'PROCESSED_DATA_TAG': 'waymo_processed_data',
                    'DATA_PROCESSOR': [{'NAME': 'heading_process'}, {'NAME': 'transform_to_global'}]})
    dataset, loader = build_dataloader(cfg, log_time='20240101-000000', data_path=str(det), batch_size=8, workers=4, split='test', logger=None,
                                       root_path=str(tmp_path))
    tracker = build_model(model)
    run_model(tracker, loader, dataset, workers=4)
    saved = pickle.load(open(dataset.get_track_path(), 'rb'))
    drop = pickle.load(open(dataset.get_drop_path(), 'rb'))
    assert list(saved) == ['seq_one', 'seq_two'] and list(drop) == ['seq_one', 'seq_two']
    for k in range(2):
        direct = build_model(model).forward(copy.deepcopy(dataset[k][1]['detection']))
        got = saved[dataset.seq_name_list[k]]
        assert list(got) == list(direct) and len(got) >= 5
        for tid in direct:
            for key in KEYS:
                assert np.array_equal(got[tid][key], direct[tid][key]), (tid, key)
