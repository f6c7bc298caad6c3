"""Test helper: the sequence-ops interface of detzero_amd.track_models.HipSeqTrackOps on tests/track_ref.NumpyTrackOps, so that
TrackManager.forward_batch - packing, the forward-log regrouping, unpacking, the reverse rows put in front - runs without a GPU.

A pass walks the sequence's frames through the manager's own per-frame modules; the detections every frame's ops object receives
must be the rows of the packed buffer at the frame's offsets (asserted), and the packed stage flags must be the manager's masks.

Also what tests/test_track_batch_host.py and tests/test_gpu_track_batch.py share: the golden fixture's loader, the two track
comparisons and the seeded sequences.
"""
import json
import os

import numpy as np

from tests import track_ref

# ---- the golden fixture and the comparisons of the batch tests (the rules of tests/test_track_models.py, restated here so that
# ---- collecting a batch test imports no other test module) ----------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'track_model_golden.npz')
KEYS = ('boxes_global', 'name', 'score', 'sample_idx', 'hit', 'num_points', 'obj_ids', 'pose')
EXACT = ('sample_idx', 'hit', 'obj_ids', 'name', 'num_points', 'score', 'pose')

_cache = {}


def load_sequence(si):
    """(frames dict, model config, expected raw tracks, expected final tracks, final states, fp32 - fp64 difference)."""
    from detzero_amd.config import AttrDict
    if 'z' not in _cache:
        _cache['z'] = np.load(GOLDEN)
    z, p = _cache['z'], 's%d_' % si
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
    """Ids and their order, the discrete fields exactly, boxes_global within box_tol."""
    assert list(mine.keys()) == list(ref.keys()), what
    worst = 0.0
    for tid, exp in ref.items():
        got = mine[tid]
        for key in EXACT:
            assert np.array_equal(np.asarray(got[key]), exp[key]), (what, tid, key, got[key], exp[key])
        assert got['boxes_global'].shape == exp['boxes_global'].shape and got['boxes_global'].dtype == np.float32
        worst = max(worst, float(np.max(np.abs(got['boxes_global'].astype(np.float64) - exp['boxes_global']))))
    print('%s: max |boxes_global - reference| = %.3e (bound %.3e)' % (what, worst, box_tol))
    assert worst <= box_tol, (what, worst, box_tol)


def same_tracks(a, b):
    """Every field of every track bit-identical, dtypes included."""
    assert list(a) == list(b)
    for tid in a:
        assert sorted(a[tid]) == sorted(b[tid])
        for key in KEYS:
            assert np.array_equal(a[tid][key], b[tid][key]) and a[tid][key].dtype == b[tid][key].dtype, (tid, key)


def numpy_manager(model):
    from detzero_amd.track_models import TrackManager
    return TrackManager(model.TRACKING, ops_factory=track_ref.NumpyTrackOps)


CLASS_SIZES = {'Vehicle': (4.6, 2.0, 1.6), 'Pedestrian': (0.8, 0.8, 1.7), 'Cyclist': (1.8, 0.7, 1.6)}


def seeded_sequence(n_obj, n_frames, seed, spacing=30.0):
    """``n_obj`` well-separated objects on a grid in global coordinates: a third stand still, the others move along their heading; a
    detection is missing in about one frame of ten, scores spread over both association stages, point counts on both sides of
    a POINT_THRESHOLD of 5."""
    rng = np.random.RandomState(seed)
    side = int(np.ceil(np.sqrt(n_obj)))
    names = np.array(list(CLASS_SIZES))[rng.randint(0, 3, n_obj)]
    centre = np.stack([1000. + spacing * (np.arange(n_obj) % side), 3000. + spacing * (np.arange(n_obj) // side), rng.uniform(0.5, 1.5, n_obj)], axis=1)
    heading = rng.uniform(-3.0, 3.0, n_obj)
    size = np.array([CLASS_SIZES[n] for n in names]) * rng.uniform(0.9, 1.1, (n_obj, 1))
    # 0.1 .. 0.25 lengths per frame along the heading: the first prediction (velocity still 0) overlaps its detection by IoU > 0.6
    speed = np.where(rng.rand(n_obj) < 0.33, 0.0, rng.uniform(1.0, 2.5, n_obj) * size[:, 0])
    velocity = np.stack([speed * np.cos(heading), speed * np.sin(heading)], axis=1)
    seq = {}
    for f in range(n_frames):
        seen = np.flatnonzero(rng.rand(n_obj) > 0.1)
        seen = seen[rng.permutation(len(seen))]
        boxes = np.zeros((len(seen), 7), dtype=np.float32)
        boxes[:, :2] = centre[seen, :2] + velocity[seen] * 0.1 * f + rng.normal(0, 0.02, (len(seen), 2))
        boxes[:, 2] = centre[seen, 2]
        boxes[:, 3:6] = size[seen]
        boxes[:, 6] = heading[seen] + rng.normal(0, 0.01, len(seen))
        seq[str(f)] = {'boxes_global': boxes, 'name': names[seen], 'score': rng.uniform(0.02, 0.98, len(seen)).astype(np.float32),
                       'num_points': rng.randint(0, 60, len(seen)).astype(np.int32), 'pose': np.eye(4)}
    return seq


class _PackedOps(track_ref.NumpyTrackOps):
    expect = None

    def set_detections(self, rows):
        rows = np.asarray(rows, dtype=np.int32).reshape(-1, track_ref.ROW_WORDS)
        assert self.expect is not None and np.array_equal(rows, self.expect), 'the packed rows of the frame differ from its row buffer'
        super().set_detections(self.expect)


class NumpySeqTrackOps:
    def __init__(self, dtype=np.float32, gaps=None):
        self.dtype, self.gaps = dtype, gaps
        self.passes = 0

    def _frames(self, mgr, pack, s):
        for ordinal, g in enumerate(pack.frames_of(s)):
            rows, flags = pack.frame_rows(g)
            det = pack.data_dicts[s][pack.frame_lists[s][ordinal]]
            if mgr.stage != 'one_stage':
                first, enough = mgr._stage_masks(det, rows[:, track_ref.ROW_CLS])
                assert np.array_equal(flags & 1, np.asarray(first).astype(np.int32)) and np.array_equal(flags >> 1, np.asarray(enough).astype(np.int32))
            else:
                assert not flags.any()
            yield ordinal, rows, det

    def forward_pass(self, mgr, pack, seqs):
        self.passes += 1
        out = {}
        for s in seqs:
            ops = _PackedOps(self.dtype, self.gaps)
            count = mgr.init_track_id
            for ordinal, rows, det in self._frames(mgr, pack, s):
                ops.expect = rows
                count = mgr.online_track_module(ops, ordinal, det, count)
            out[s] = ops.fetch_log()[0]
        return out

    def reverse_pass(self, mgr, pack, seqs, fwd, groups):
        self.passes += 1
        out = {}
        for s in seqs:
            ops = _PackedOps(self.dtype, self.gaps)
            ops.start_pass(ext=fwd[s])
            ids, is_start, per_frame = groups[s]
            for ordinal, rows, det in reversed(list(self._frames(mgr, pack, s))):
                ops.expect = rows
                at = per_frame[ordinal]
                mgr.reverse_tracking_module(ops, ordinal, det, at, is_start[at], ids[at].astype(np.int64))
            out[s] = ops.fetch_log()[0]
        return out
