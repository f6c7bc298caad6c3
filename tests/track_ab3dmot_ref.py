"""Test helper: numpy float64 restatement of the AB3DMOT filter ops (detzero_amd.track_models.HipTrackOps with filter='AB3DMOT').

``Ab3dTrack`` restates kalman_filter/ab3dmot.py:9-149 over the equations of filterpy's ``KalmanFilter(dim_x=10, dim_z=7)``
(predict: x = F x, P = F P F^T + Q; update: y = z - H x, S = H P H^T + R, K = P H^T S^-1, x += K y, Joseph-form P), with S^-1 by
``np.linalg.inv`` as the reference (``solve='inv'``) or through a Cholesky solve as the device (``solve='cholesky'``).
``NumpyAb3dTrackOps`` builds on tests/track_ref.NumpyTrackOps (affinity, merge and compact are the same code: they read the float32
rounding of the box) and implements the AB3DMOT side of the ops interface; ``NumpyAb3dSeqTrackOps`` is forward_batch's stand-in on it.

Also what tests/test_track_ab3dmot.py and tests/test_gpu_track_ab3dmot.py share: the fixture's loader and the track comparison.
"""
import json
import os

import numpy as np

from tests import track_ref
from tests.track_ref import ROW_CLS, ROW_FRAME, ROW_HIT, ROW_ID, ROW_NPTS, ROW_SCORE, ROW_WORDS

ROW_AB3D, ROW_DROP, ROW_BIRTH = 15, 1, 2
PI = np.pi


def wrap(th):
    if th >= PI:
        th -= PI * 2
    if th < -PI:
        th += PI * 2
    return th


class Ab3dTrack:
    def __init__(self, box7_f64, box7_f32, cls, score, track_id, solve='inv'):
        self.solve = solve
        self.cls, self.score, self.update_score, self.num_points, self.track_id = int(cls), score, score, -1, int(track_id)
        self.bbox = np.zeros(9, dtype=np.float32)           # the reference's float32 self.bbox until the first predict
        self.bbox[:7] = box7_f32
        self.x = np.zeros((10, 1))
        self.x[:7, 0] = np.asarray(box7_f64, dtype=np.float64)
        self.F = np.eye(10)
        self.F[0, 7] = self.F[1, 8] = self.F[2, 9] = 1.
        self.H = np.eye(7, 10)
        self.R = np.eye(7)
        self.P = np.diag([10.] * 7 + [10000.] * 3)
        self.Q = np.diag([1.] * 7 + [0.01] * 3)
        self.hits, self.hit, self.miss = 1, 1, 0

    def predict(self):
        self.x = self.F @ self.x
        self.P = (self.F @ self.P) @ self.F.T + self.Q
        self.x[6, 0] = wrap(self.x[6, 0])
        self.miss += 1
        self.hit = 0
        self.bbox = self.x.reshape(-1)[:9].copy()

    def update(self, z7, cls, score):
        self.hit, self.miss = 1, 0
        self.hits += 1
        self.score, self.cls = score, int(cls)
        z = np.array(z7, dtype=np.float64).reshape(7, 1)
        self.x[6, 0] = wrap(self.x[6, 0])
        z[6, 0] = wrap(z[6, 0])
        new, th = z[6, 0], self.x[6, 0]
        if PI / 2.0 < abs(new - th) < PI * 3 / 2.0:
            th += PI
            if th > PI:
                th -= PI * 2
            if th < -PI:
                th += PI * 2
        if abs(new - th) >= PI * 3 / 2.0:
            th = th + PI * 2 if new > 0 else th - PI * 2
        self.x[6, 0] = th
        y = z - self.H @ self.x
        pht = self.P @ self.H.T
        s = self.H @ pht + self.R
        if self.solve == 'inv':
            k = pht @ np.linalg.inv(s)
        else:
            low = np.linalg.cholesky((s + s.T) / 2.)
            k = np.linalg.solve(low.T, np.linalg.solve(low, pht.T)).T
        self.x = self.x + k @ y
        i_kh = np.eye(10) - k @ self.H
        self.P = (i_kh @ self.P) @ i_kh.T + (k @ self.R) @ k.T
        self.x[6, 0] = wrap(self.x[6, 0])
        self.bbox = self.x.reshape(-1)[:9].copy()


class NumpyAb3dTrackOps(track_ref.NumpyTrackOps):
    """HipTrackOps(filter='AB3DMOT')'s interface on a Python list of ``Ab3dTrack``.  ``history`` keeps, per finished pass, the
    log rows that passed the output rule and their float64 boxes."""

    def __init__(self, solve='inv', gaps=None):
        self.solve = solve
        super().__init__(dtype=np.float64, gaps=gaps)

    def start_pass(self, ext=None):
        assert ext is None, 'the AB3DMOT filter has no reverse pass'
        super().start_pass()
        self.det64, self.kept = None, None

    def set_detections(self, rows, boxes64=None):
        super().set_detections(rows)
        self.det64 = np.asarray(boxes64, dtype=np.float64).reshape(-1, 7)
        assert len(self.det64) == len(self.det)

    def predict(self, gate_class):
        for t in self.tracks:
            t.predict()

    def update(self, match, r):
        for i, di, _stage in np.asarray(match).reshape(-1, 3):
            d = self.det[di]
            self.tracks[i].update(self.det64[di], d[ROW_CLS], d[ROW_SCORE:ROW_SCORE + 1].view(np.float32)[0])

    def spawn(self, source, idx, ids, p, q, dt):
        assert source == 'det'
        for si, tid in zip(idx, ids):
            s = self.det[si]
            self.tracks.append(Ab3dTrack(self.det64[si], s[:7].view(np.float32), s[ROW_CLS], s[ROW_SCORE:ROW_SCORE + 1].view(np.float32)[0], tid,
                                         self.solve))

    def log(self, frame, frame_id=None, birth_age=None, death_age=None):
        for t in self.tracks:
            row = np.zeros(ROW_WORDS, dtype=np.int32)
            row[:9] = np.asarray(t.bbox).astype(np.float32).view(np.int32)
            row[ROW_SCORE] = np.float32(t.score).view(np.int32)
            row[ROW_HIT], row[ROW_NPTS], row[ROW_ID], row[ROW_CLS], row[ROW_FRAME] = t.hit, t.num_points, t.track_id, t.cls, frame
            out = (t.hits >= birth_age or frame_id < birth_age) and t.miss < death_age
            row[ROW_AB3D] = (0 if out else ROW_DROP) | (ROW_BIRTH if t.hits == 1 and t.hit == 1 else 0)
            self.rows.append(row)
            self.boxes.append(np.array(t.bbox, dtype=np.float64))

    def fetch_log(self):
        rows = np.array(self.rows, dtype=np.int32).reshape(-1, ROW_WORDS)
        self.kept = (rows[:, ROW_AB3D] & ROW_DROP) == 0
        self.all_rows, self.all_boxes = rows, np.array(self.boxes, dtype=np.float64).reshape(-1, 9)
        self.history.append((rows[self.kept], self.all_boxes[self.kept]))
        return rows[self.kept], None

    def fetch_log_boxes(self):
        return self.all_boxes[self.kept]


class NumpyAb3dSeqTrackOps:
    """HipSeqTrackOps's interface for the AB3DMOT filter on NumpyAb3dTrackOps: a pass walks the sequence's frames through the
    manager's own per-frame module; the packed rows, measurements and frame ids must be the frames' own (asserted)."""

    def __init__(self, solve='inv'):
        self.solve = solve
        self.boxes64 = {}
        self.passes = 0

    def forward_pass(self, mgr, pack, seqs):
        self.passes += 1
        self.boxes64 = {}
        out = {}
        for s in seqs:
            ops = NumpyAb3dTrackOps(self.solve)
            count = mgr.init_track_id
            for ordinal, g in enumerate(pack.frames_of(s)):
                frm_id = pack.frame_lists[s][ordinal]
                det = pack.data_dicts[s][frm_id]
                rows, flags = pack.frame_rows(g)
                cls, mine = mgr._frame_rows(det)
                assert np.array_equal(rows, mine) and int(pack.frame_ids[g]) == int(frm_id)
                assert np.array_equal(pack.boxes64[pack.frame_row[g]:pack.frame_row[g + 1]], mgr._frame_boxes64(det))
                count = mgr.online_track_module(ops, ordinal, det, count, frm_id)
            out[s] = ops.fetch_log()[0]
            self.boxes64[s] = ops.fetch_log_boxes()
        return out

    def reverse_pass(self, mgr, pack, seqs, fwd, groups):
        raise AssertionError('the AB3DMOT filter has no reverse pass')


# ------------------------------------------------------------------------------------------------
# the fixture (tests/golden/gen_track_ab3dmot_golden.py) and the comparison
# ------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'track_ab3dmot_golden.npz')
KEYS = ('boxes_global', 'name', 'score', 'sample_idx', 'hit', 'num_points', 'obj_ids', 'pose')
EXACT = ('sample_idx', 'hit', 'obj_ids', 'name', 'num_points', 'score', 'pose')
FRAME_KEYS = ('boxes_global', 'name', 'score', 'num_points', 'pose')
N_RUNS = 2
_cache = {}


def load_run(ri):
    """(frames dict, model config (AttrDict), the reference's raw tracks, solve_diff) of run ``ri``."""
    from detzero_amd.config import AttrDict
    if 'z' not in _cache:
        _cache['z'] = np.load(GOLDEN)
    z, p = _cache['z'], 'r%d_' % ri
    seq = {}
    for f in z[p + 'frame_ids']:
        seq[str(f)] = {key: z['%sf%s_%s' % (p, f, key)].copy() for key in FRAME_KEYS}
    ids, lens, dts = z[p + 'raw_ids'], z[p + 'raw_len'], z[p + 'raw_box_dtype']
    off = np.concatenate([[0], np.cumsum(lens)])
    tracks = {}
    for k, t in enumerate(ids):
        tracks[int(t)] = {key: z['%sraw_%s' % (p, key)][off[k]:off[k + 1]] for key in KEYS}
        tracks[int(t)]['boxes_global'] = tracks[int(t)]['boxes_global'].astype(str(dts[k]))
    return seq, AttrDict(json.loads(str(z[p + 'model']))), tracks, float(z[p + 'solve_diff'])


def box_tolerance(ref, solve_diff):
    """8 x max(solve_diff, 2^-40 x the largest |coordinate|)."""
    biggest = max([float(np.max(np.abs(t['boxes_global']))) for t in ref.values()] + [0.0])
    return 8.0 * max(solve_diff, 2.0 ** -40 * biggest)


def assert_tracks(mine, ref, box_tol, what):
    """Ids and their order, the discrete fields and every dtype exactly, boxes_global within box_tol; returns the box error."""
    assert list(mine.keys()) == list(ref.keys()), what
    worst = 0.0
    for tid, exp in ref.items():
        got = mine[tid]
        for key in EXACT:
            assert np.array_equal(np.asarray(got[key]), exp[key]), (what, tid, key, got[key], exp[key])
            if exp[key].dtype.kind != 'U':          # (the fixture stores the strings of all tracks in one array: its width is the widest's)
                assert np.asarray(got[key]).dtype == exp[key].dtype, (what, tid, key, np.asarray(got[key]).dtype, exp[key].dtype)
        assert got['boxes_global'].shape == exp['boxes_global'].shape and got['boxes_global'].dtype == exp['boxes_global'].dtype, (what, tid)
        worst = max(worst, float(np.max(np.abs(got['boxes_global'].astype(np.float64) - exp['boxes_global'].astype(np.float64)))))
    print('%s: max |boxes_global - reference| = %.3e (bound %.3e)' % (what, worst, box_tol))
    assert worst <= box_tol, (what, worst, box_tol)
    return worst


def same_tracks(a, b):
    """Every field of every track bit-identical, dtypes included."""
    assert list(a) == list(b)
    for tid in a:
        assert sorted(a[tid]) == sorted(b[tid])
        for key in KEYS:
            assert np.array_equal(a[tid][key], b[tid][key]) and a[tid][key].dtype == b[tid][key].dtype, (tid, key)
