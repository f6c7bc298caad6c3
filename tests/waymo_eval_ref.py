"""Test helper: the detection-metric protocol of DESIGN.md 7n in its slow, obvious form.

Float64 numpy around one independent ``scipy.optimize.linear_sum_assignment(maximize=True)`` per problem and per score cutoff (the
device makes ONE solve per problem and reads every cutoff off its prefixes: csrc/eval_match.hip).  The IoU is the fp32 restatement
the tracker's tests use (tests/track_ref.py:iou3d, oracle/cref.py for BEV); everything after it is float64.  Nothing here comes
from detzero_amd: the sharding, the cutoffs and the counts are restated.
"""
import numpy as np

from oracle import cref
from tests import track_ref

THR = np.array([0.0, 0.7, 0.5, 0.5, 0.5])
CUTOFFS = np.array([k * 0.01 for k in range(100)] + [1.0], dtype=np.float32)
K = 101


def iou(pb, gb, box_type):
    pb, gb = np.asarray(pb, np.float32).reshape(-1, 7), np.asarray(gb, np.float32).reshape(-1, 7)
    if len(pb) == 0 or len(gb) == 0:
        return np.zeros((len(pb), len(gb)))
    m = track_ref.iou3d(pb, gb) if box_type == '3d' else cref.boxes_iou_bev(np.ascontiguousarray(pb), np.ascontiguousarray(gb))
    return np.asarray(m, dtype=np.float64)


def weights(pb, gb, obj_type, box_type):
    m = iou(pb, gb, box_type)
    return np.where(m >= THR[obj_type], m, 0.0)


def matching(w):
    """Valid pairs (row, col) of a maximum-total-weight matching of w (rows x cols, >= 0): zero-weight pairs discarded."""
    from scipy.optimize import linear_sum_assignment
    if w.shape[0] == 0 or w.shape[1] == 0:
        return set()
    rows, cols = linear_sum_assignment(w, maximize=True)
    return {(int(r), int(c)) for r, c in zip(rows, cols) if w[r, c] > 0}


def heading_accuracy(hp, hg):
    d = float(hp) - float(hg)
    d -= 2 * np.pi * np.floor((d + np.pi) / (2 * np.pi))
    return 1.0 - abs(d) / np.pi


def shards_of(config_type, obj_type, boxes):
    """[(ids per object)] per breakdown; -1 = in no shard.  OBJECT_TYPE: type - 1; RANGE: after them, (type - 1) * 3 + bin."""
    obj_type = np.asarray(obj_type, dtype=np.int64)
    out, first = [], 0
    if 'object' in config_type:
        out.append(np.where((obj_type >= 1) & (obj_type <= 4), obj_type - 1, -1))
        first = 4
    if 'range' in config_type:
        b = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
        dist = np.sqrt(b[:, 0] ** 2 + b[:, 1] ** 2 + b[:, 2] ** 2)
        rbin = np.where(dist < 30, 0, np.where(dist < 50, 1, 2))
        out.append(np.where((obj_type >= 1) & (obj_type <= 4), first + (obj_type - 1) * 3 + rbin, -1))
    return out


def n_shards_of(config_type):
    return (4 if 'object' in config_type else 0) + (12 if 'range' in config_type else 0)


def problems(config_type, n_frames, pd_frame, pd_box, pd_type, pd_score, gt_frame, gt_box, gt_type, gt_diff):
    """[(shard, object type, pred box, pred score f32, gt box, gt difficulty)] of every (frame, shard) with a member."""
    pd_box, gt_box = np.asarray(pd_box, np.float32).reshape(-1, 7), np.asarray(gt_box, np.float32).reshape(-1, 7)
    pd_score = np.asarray(pd_score, dtype=np.float32)
    pd_frame, gt_frame, gt_diff = np.asarray(pd_frame), np.asarray(gt_frame), np.asarray(gt_diff)
    out = []
    for p_ids, g_ids in zip(shards_of(config_type, pd_type, pd_box), shards_of(config_type, gt_type, gt_box)):
        for f in range(n_frames):
            for s in sorted(set(p_ids[pd_frame == f].tolist()) | set(g_ids[gt_frame == f].tolist())):
                if s < 0:
                    continue
                pm, gm = (pd_frame == f) & (p_ids == s), (gt_frame == f) & (g_ids == s)
                n_obj = 4 if 'object' in config_type else 0
                t = s + 1 if s < n_obj else (s - n_obj) // 3 + 1
                out.append((s, t, pd_box[pm], pd_score[pm], gt_box[gm], gt_diff[gm]))
    return out


def problem_counts(w, score, pred_heading, gt_heading, gt_diff, cache=None):
    """One problem -> counts (2, 101, 3) int [TP, FP, FN], HA (2, 101) float64 and HA as the protocol's table holds it (2, 101)
    int64: every term times 2^32, rounded to nearest, then added.  One scipy solve per cutoff (cutoffs that hold the same
    predictions share the same input, so their solve is made once)."""
    counts, ha, fixed = np.zeros((2, K, 3), dtype=np.int64), np.zeros((2, K)), np.zeros((2, K), dtype=np.int64)
    solved = {} if cache is None else cache
    for k in range(K):
        rows = np.flatnonzero(score >= CUTOFFS[k])
        key = tuple(rows.tolist())
        if key not in solved:
            solved[key] = matching(w[rows])
        pairs = solved[key]
        for lv in (1, 2):
            tp = [(rows[r], c) for r, c in pairs if gt_diff[c] <= lv]
            counts[lv - 1, k] = (len(tp), len(rows) - len(pairs), int((gt_diff <= lv).sum()) - len(tp))
            terms = [heading_accuracy(pred_heading[r], gt_heading[c]) for r, c in tp]
            ha[lv - 1, k] = sum(terms)
            fixed[lv - 1, k] = sum(int(np.round(h * 4294967296.0)) for h in terms)
    return counts, ha, fixed


def counts(config_type, box_type, n_frames, pd_frame, pd_box, pd_type, pd_score, gt_frame, gt_box, gt_type, gt_diff):
    """-> (counts (n_shards, 2, 101, 3) int64 [TP, FP, FN], HA (n_shards, 2, 101) float64, HA in fixed point (n_shards, 2, 101) int64)."""
    n = n_shards_of(config_type)
    total, total_ha, total_fixed = np.zeros((n, 2, K, 3), dtype=np.int64), np.zeros((n, 2, K)), np.zeros((n, 2, K), dtype=np.int64)
    for s, t, pb, ps, gb, gd in problems(config_type, n_frames, pd_frame, pd_box, pd_type, pd_score, gt_frame, gt_box, gt_type, gt_diff):
        c, h, x = problem_counts(weights(pb, gb, t, box_type), ps, pb[:, 6], gb[:, 6], gd)
        total[s] += c
        total_ha[s] += h
        total_fixed[s] += x
    return total, total_ha, total_fixed


def table_of(counts_, fixed):
    """The protocol's table (n_shards, 2, 101, 4) int64 [TP, FP, FN, HA in fixed point]: the input of metrics_from_counts."""
    t = np.zeros(counts_.shape[:3] + (4,), dtype=np.int64)
    t[..., :3] = counts_
    t[..., 3] = fixed
    return t


def margins_hold(config_type, box_type, scene, trials=4, eps=1e-5, thr_margin=1e-4):
    """The two conditions under which a differing device answer is a bug and not a tie: (a) no pair of a problem has an IoU within
    thr_margin of its threshold; (b) every prefix matching is unchanged when all weights move by +-eps (four random sign patterns)."""
    rng = np.random.RandomState(4242)
    for s, t, pb, ps, gb, gd in problems(config_type, scene['n_frames'], scene['pd_frame'], scene['pd_box'], scene['pd_type'], scene['pd_score'],
                                         scene['gt_frame'], scene['gt_box'], scene['gt_type'], scene['gt_diff']):
        m = iou(pb, gb, box_type)
        if m.size and (np.abs(m - THR[t]) < thr_margin).any():
            return False
        w = np.where(m >= THR[t], m, 0.0)
        prefixes = sorted({int((ps >= c).sum()) for c in CUTOFFS} - {0})
        order = np.argsort(-ps, kind='stable')
        base = {n: matching(w[order[:n]]) for n in prefixes}
        for _ in range(trials):
            moved = np.maximum(w + eps * np.where(rng.rand(*w.shape) < 0.5, -1.0, 1.0), 0.0)
            for n in prefixes:
                rows = order[:n]
                if {(r, c) for r, c in matching(moved[rows]) if w[rows[r], c] > 0} != base[n]:
                    return False
    return True
