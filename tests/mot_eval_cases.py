"""Test helper: seeded tracking scenes shared by the tracking-evaluation tests (CPU and GPU).

A scene is the dict of flat arrays tests/mot_eval_ref.py describes.  ``scene(seed)``: sequences 0 and 1 of 10 frames and sequence 2
of one frame; all four types, difficulty mixed per track, a few objects per type and frame on a 9 m grid (tracks drift, they never
meet).  Every 10-frame sequence holds, among random tracks with gaps, jittering scores and free false positives:
  A, B   two ground truths whose predictions swap ids at frame 5 (two mismatches at every cutoff that holds both);
  C      its prediction is absent in frames 3 and 4 and returns with the same id (no mismatch);
  D      the same, but it returns under a new id (one mismatch);
  E      two predictions: the closer one has score 0.62 up to frame 4 and 0.38 from frame 5, the looser one 0.5 throughout, so the
         chains of the cutoffs 39..50 lose E's partner at frame 5 and take the other (a mismatch) while those up to 38 keep it;
  F      a loose prediction alone in frame 0, joined from frame 1 by a closer one with a lower score: the carried pair is not the
         higher-IoU one, and it stays;
  scores exactly on c_0 = 0, c_50 = float32(0.5) and c_100 = 1 (three random tracks of sequence 0).
Sequence 1 has no prediction in frame 7 and no ground truth in frame 8.

A seed is kept only if tests/mot_eval_ref.margins_hold says so for both box types; tests/test_waymo_track_eval_cpu.py checks that
for every seed below, so no case is skipped at test time.
"""
import numpy as np

from tests.waymo_eval_cases import _gt_box, _perturbed

TYPE_NAMES = {1: 'Vehicle', 2: 'Pedestrian', 3: 'Sign', 4: 'Cyclist'}      # waymo_eval_tracking.py:18
SEEDS = [1, 2]
N_FRAMES = 10


def _cell(i, dx):
    return ((i % 6 - 2.5) * 9.0 + 1.0 + dx, (i // 6 - 2.5) * 9.0 + 2.0)


def _shifted(box, frac):
    out = box.copy()
    out[0] += frac * box[3] * np.cos(box[6])
    out[1] += frac * box[3] * np.sin(box[6])
    return out


def _sequence(rng, seq, n_frames, ids, pd, gt, special):
    """Appends the sequence's (seq, frame, id, box, type, score) / (seq, frame, id, box, type, difficulty) tuples."""
    dx = 25.0 * seq
    cell = iter(range(36))

    def new_track(t):
        c = _cell(next(cell), dx)
        box = _gt_box(rng, t, (c[0], c[1], float(rng.uniform(-0.5, 1.0))))
        ids[1] += 1
        return box, rng.uniform(-0.3, 0.3, 2), ids[1], int(rng.randint(1, 3))

    def at(box, vel, f):
        out = box.copy()
        out[:2] += vel * f
        return out

    def new_pid():
        ids[0] += 1
        return ids[0]

    frames = range(n_frames)
    if special:
        t = 2
        (ba, va, ga, da), (bb, vb, gb, db) = new_track(t), new_track(t)
        pa, pb = new_pid(), new_pid()
        for f in frames:
            gt.append((seq, f, ga, at(ba, va, f), t, da))
            gt.append((seq, f, gb, at(bb, vb, f), t, db))
            pd.append((seq, f, pa if f < 5 else pb, _shifted(at(ba, va, f), 0.03), t, 0.9))
            pd.append((seq, f, pb if f < 5 else pa, _shifted(at(bb, vb, f), 0.03), t, 0.8))
        for renamed in (False, True):                                           # C, D
            b, v, g, d = new_track(t)
            p, p2 = new_pid(), new_pid()
            for f in frames:
                gt.append((seq, f, g, at(b, v, f), t, d))
                if f not in (3, 4):
                    pd.append((seq, f, p2 if renamed and f > 4 else p, _shifted(at(b, v, f), 0.04), t, 0.85))
        b, v, g, d = new_track(t)                                               # E
        p, p2 = new_pid(), new_pid()
        for f in frames:
            gt.append((seq, f, g, at(b, v, f), t, d))
            pd.append((seq, f, p, _shifted(at(b, v, f), 0.03), t, 0.62 if f < 5 else 0.38))
            pd.append((seq, f, p2, _shifted(at(b, v, f), -0.12), t, 0.5))
        b, v, g, d = new_track(t)                                               # F
        p, p2 = new_pid(), new_pid()
        for f in frames:
            gt.append((seq, f, g, at(b, v, f), t, d))
            pd.append((seq, f, p, _shifted(at(b, v, f), 0.13), t, 0.7))
            if f >= 1:
                pd.append((seq, f, p2, _shifted(at(b, v, f), 0.02), t, 0.6))
    exact = []
    for t in (1, 2, 3, 4):
        for _ in range(int(rng.randint(2, 4))):
            b, v, g, d = new_track(t)
            p, base = new_pid(), float(rng.uniform(0.05, 0.95))
            exact.append(p)
            first = int(rng.randint(0, 3)) if n_frames > 1 else 0
            for f in range(first, n_frames):
                gt.append((seq, f, g, at(b, v, f), t, d))
                if rng.rand() < 0.15:
                    continue
                if rng.rand() < 0.05:
                    p = new_pid()                                               # the tracker lost it: a new id from here on
                score = float(np.clip(base + rng.uniform(-0.04, 0.04), 0.01, 0.99))
                pd.append((seq, f, p, _perturbed(rng, at(b, v, f), int(rng.choice([0, 0, 1]))), t, score))
    for f in frames:                                                            # free false positives, far from every track
        for _ in range(int(rng.randint(0, 3))):
            t = int(rng.choice([1, 2, 3, 4]))
            c = _cell(int(rng.randint(30, 36)), dx)
            pd.append((seq, f, new_pid(), _gt_box(rng, t, (c[0] + rng.uniform(-3, 3), c[1] + rng.uniform(-3, 3), 0.0)), t,
                       float(rng.uniform(0.02, 0.6))))
    return exact


def scene(seed):
    rng = np.random.RandomState(seed)
    pd, gt, ids = [], [], [0, 0]
    exact = _sequence(rng, 0, N_FRAMES, ids, pd, gt, True)
    _sequence(rng, 1, N_FRAMES, ids, pd, gt, True)
    _sequence(rng, 2, 1, ids, pd, gt, False)
    pd = [p for p in pd if not (p[0] == 1 and p[1] == 7)]
    gt = [g for g in gt if not (g[0] == 1 and g[1] == 8)]
    on_cutoff = dict(zip(exact[:3], (0.0, 0.5, 1.0)))                            # float32(0.5) == c_50 exactly, 0 == c_0, 1 == c_100
    pd = [p[:5] + (on_cutoff[p[2]],) if p[0] == 0 and p[2] in on_cutoff else p for p in pd]
    f32 = lambda rows: np.array(rows, dtype=np.float64).reshape(-1, 7).astype(np.float32)
    return {'pd_seq': np.array([p[0] for p in pd], dtype=np.int64), 'pd_frame': np.array([p[1] for p in pd], dtype=np.int64),
            'pd_id': np.array([p[2] for p in pd], dtype=np.int64), 'pd_box': f32([p[3] for p in pd]),
            'pd_type': np.array([p[4] for p in pd], dtype=np.int64), 'pd_score': np.array([p[5] for p in pd], dtype=np.float32),
            'gt_seq': np.array([g[0] for g in gt], dtype=np.int64), 'gt_frame': np.array([g[1] for g in gt], dtype=np.int64),
            'gt_id': np.array([g[2] for g in gt], dtype=np.int64), 'gt_box': f32([g[3] for g in gt]),
            'gt_type': np.array([g[4] for g in gt], dtype=np.int64), 'gt_diff': np.array([g[5] for g in gt], dtype=np.int32)}


def one_frame_sequences(det):
    """A detection scene (tests/waymo_eval_cases.py) as a tracking scene: every frame a sequence of its own and every object an id
    of its own, so nothing is carried and nothing can mismatch."""
    out = {k: det[k] for k in ('pd_frame', 'pd_box', 'pd_type', 'pd_score', 'gt_frame', 'gt_box', 'gt_type', 'gt_diff')}
    out.update(pd_seq=det['pd_frame'].copy(), gt_seq=det['gt_frame'].copy(), pd_id=np.arange(len(det['pd_frame']), dtype=np.int64),
               gt_id=np.arange(len(det['gt_frame']), dtype=np.int64))
    return out


def frames_of(s):
    """The (sequence, frame) pairs of a scene in walking order."""
    return sorted(set(zip(s['pd_seq'].tolist(), s['pd_frame'].tolist())) | set(zip(s['gt_seq'].tolist(), s['gt_frame'].tolist())))


def infos_of(s):
    """The scene as the info dicts WaymoTrackingMetricsEstimator.waymo_evaluation takes: one prediction info and one whole
    ground-truth info per (sequence, frame), in walking order (true-lidar boxes, 10 points per box)."""
    pds, gts = [], []
    for q, f in frames_of(s):
        pm, gm = (s['pd_seq'] == q) & (s['pd_frame'] == f), (s['gt_seq'] == q) & (s['gt_frame'] == f)
        pds.append({'boxes_lidar': s['pd_box'][pm], 'score': s['pd_score'][pm], 'obj_ids': s['pd_id'][pm],
                    'name': np.array([TYPE_NAMES[int(t)] for t in s['pd_type'][pm]], dtype='<U16'), 'sequence_name': 'seq_%d' % q, 'frame_id': f})
        gts.append({'sequence_name': 'seq_%d' % q, 'frame_id': f, 'sample_idx': f,
                    'annos': {'gt_boxes_lidar': s['gt_box'][gm], 'name': np.array([TYPE_NAMES[int(t)] for t in s['gt_type'][gm]], dtype='<U16'),
                              'difficulty': s['gt_diff'][gm].astype(np.int32), 'num_points_in_gt': np.full((int(gm.sum()),), 10, dtype=np.int64),
                              'obj_ids': np.array(['g%d' % i for i in s['gt_id'][gm]], dtype='<U16')}})
    return pds, gts


def cut_of(score):
    """The highest k with score >= c_k (-1 = none), as dz_mot_weights writes it."""
    c = np.array([k * 0.01 for k in range(100)] + [1.0], dtype=np.float32)
    return ((np.asarray(score, dtype=np.float32)[:, None] >= c[None, :]).sum(axis=1) - 1).astype(np.int32)


def device_inputs(probs):
    """Problems (tests/mot_eval_ref.py, sorted by (sequence, shard, frame)) -> what ops.mot_chain_counts takes, as host arrays:
    weights (float32, flat), cut, pred_id, gt_id, gt_diff, pdesc (n, 5), cdesc (c, 6), frames.  Ids are made dense per (sequence,
    side) here."""
    dense = {}
    for side, key in (('p', 'pid'), ('g', 'gid')):
        for pr in probs:
            table = dense.setdefault((side, pr['seq']), {})
            for i in pr[key].tolist():
                table.setdefault(i, len(table))
    w, cut, pid, gid, gd, pdesc, cdesc, frames = [], [], [], [], [], [], [], []
    n_p = n_g = 0
    for i, pr in enumerate(probs):
        P, G = len(pr['pid']), len(pr['gid'])
        w.append(np.asarray(pr['w'], dtype=np.float32).reshape(-1))
        cut.append(cut_of(pr['score']))
        pid += [dense[('p', pr['seq'])][x] for x in pr['pid'].tolist()]
        gid += [dense[('g', pr['seq'])][x] for x in pr['gid'].tolist()]
        gd += pr['gd'].tolist()
        pdesc.append((n_p, P, n_g, G, pr['type']))
        n_p, n_g = n_p + P, n_g + G
        if i == 0 or (probs[i - 1]['seq'], probs[i - 1]['shard']) != (pr['seq'], pr['shard']):
            cdesc.append([len(frames), 0, pr['shard'], len(dense[('p', pr['seq'])]), len(dense[('g', pr['seq'])]), 0])
        cdesc[-1][1] += 1
        cdesc[-1][5] = max(cdesc[-1][5], P + G)
        frames.append(i)
    i32 = lambda x: np.array(x, dtype=np.int32).reshape(-1)
    return (np.concatenate(w) if w else np.zeros((0,), np.float32), np.concatenate(cut) if cut else np.zeros((0,), np.int32), i32(pid), i32(gid),
            i32(gd), np.array(pdesc, dtype=np.int64).reshape(-1, 5), np.array(cdesc, dtype=np.int64).reshape(-1, 6), np.array(frames, dtype=np.int64))


def _hand_problem(frame, w, score, pid, gid, gd, shard=0, seq=0, t=1):
    w = np.asarray(w, dtype=np.float32).astype(np.float64).reshape(len(pid), len(gid))
    return {'seq': seq, 'frame': frame, 'shard': shard, 'type': t, 'w': w, 'score': np.asarray(score, dtype=np.float32),
            'pid': np.asarray(pid, dtype=np.int64), 'gid': np.asarray(gid, dtype=np.int64), 'gd': np.asarray(gd, dtype=np.int32)}


def hand_cases():
    """Chains small enough to count by hand, as problems with their weights given (one sequence, shard 0):
    'perfect'  3 ground truths (difficulty 1, 2, 1) tracked with weight 1 by ids 5, 6, 7 (scores .9, .6, .3) over 4 frames;
    'swap'     2 ground truths (difficulty 1, 1), weight 0.8, scores .9 / .8; the two prediction ids change places at frame 3 of 6;
    'dropped'  the ground truths of 'perfect' and no prediction at all."""
    eye3, eye2 = np.eye(3), 0.8 * np.eye(2)
    perfect = [_hand_problem(f, eye3, [.9, .6, .3], [5, 6, 7], [10, 11, 12], [1, 2, 1]) for f in range(4)]
    swap = [_hand_problem(f, eye2, [.9, .8], [5, 6] if f < 3 else [6, 5], [10, 11], [1, 1]) for f in range(6)]
    dropped = [_hand_problem(f, np.zeros((0, 3)), [], [], [10, 11, 12], [1, 2, 1]) for f in range(4)]
    return {'perfect': perfect, 'swap': swap, 'dropped': dropped}


def without(s, side, seq=None):
    """The scene with the predictions (side 'pd') or ground truths ('gt') of one sequence - or, seq None, of all - left out."""
    keep = np.zeros(len(s[side + '_seq']), dtype=bool) if seq is None else s[side + '_seq'] != seq
    return {k: (v[keep] if k.startswith(side + '_') else v) for k, v in s.items()}
