"""Test helper: the tracking-metric protocol of DESIGN.md 7o in its slow, obvious form.

Float64 numpy, a Python dict for ``last`` and one independent ``scipy.optimize.linear_sum_assignment(maximize=True)`` per frame,
chain and match step (the device walks a chain in one workgroup with csrc/lsa.h's solver on the remaining rows and columns:
csrc/mot_chain.hip).  The IoU, the thresholds, the cutoffs and the sharding are those of tests/waymo_eval_ref.py (fp32 IoU
restatements of tests/track_ref.py and oracle/cref.py); everything after the IoU is float64 and integers.  Nothing here comes from
detzero_amd.

A scene is a dict of flat arrays: pd_seq, pd_frame, pd_id, pd_box (float32), pd_type, pd_score (float32), gt_seq, gt_frame, gt_id,
gt_box (float32), gt_type, gt_diff.  A problem is a dict: seq, frame, shard, type, w (P, G) float64, score (P,) float32 in
descending order (ties in input order), pid (P,), gid (G,), gd (G,), and the boxes pb / gb.
"""
import numpy as np

from tests import waymo_eval_ref as det_ref

THR, CUTOFFS, K = det_ref.THR, det_ref.CUTOFFS, det_ref.K
ONE = 4294967296.0
TP, FP, MISS, MISMATCH, COST = range(5)


def problems(config_type, box_type, scene):
    """Every (sequence, frame, shard) with a member, with its weights: sorted by (sequence, shard, frame)."""
    pd_box, gt_box = np.asarray(scene['pd_box'], np.float32).reshape(-1, 7), np.asarray(scene['gt_box'], np.float32).reshape(-1, 7)
    n_obj = 4 if 'object' in config_type else 0
    out = []
    for p_ids, g_ids in zip(det_ref.shards_of(config_type, scene['pd_type'], pd_box), det_ref.shards_of(config_type, scene['gt_type'], gt_box)):
        keys = {(int(q), int(f), int(s)) for q, f, s in zip(scene['pd_seq'], scene['pd_frame'], p_ids) if s >= 0}
        keys |= {(int(q), int(f), int(s)) for q, f, s in zip(scene['gt_seq'], scene['gt_frame'], g_ids) if s >= 0}
        for q, f, s in keys:
            pm = np.flatnonzero((scene['pd_seq'] == q) & (scene['pd_frame'] == f) & (p_ids == s))
            gm = np.flatnonzero((scene['gt_seq'] == q) & (scene['gt_frame'] == f) & (g_ids == s))
            pm = pm[np.argsort(-scene['pd_score'][pm].astype(np.float32), kind='stable')]
            t = s + 1 if s < n_obj else (s - n_obj) // 3 + 1
            out.append({'seq': q, 'frame': f, 'shard': s, 'type': t, 'pb': pd_box[pm], 'gb': gt_box[gm],
                        'w': det_ref.weights(pd_box[pm], gt_box[gm], t, box_type), 'score': scene['pd_score'][pm].astype(np.float32),
                        'pid': np.asarray(scene['pd_id'])[pm], 'gid': np.asarray(scene['gt_id'])[gm], 'gd': np.asarray(scene['gt_diff'])[gm]})
    return sorted(out, key=lambda p: (p['seq'], p['shard'], p['frame']))


def check_ids(scene):
    """An object id is unique within a (sequence, frame) and side."""
    for side in ('pd', 'gt'):
        keys = list(zip(scene[side + '_seq'].tolist(), scene[side + '_frame'].tolist(), scene[side + '_id'].tolist()))
        if len(set(keys)) != len(keys):
            raise ValueError('duplicate %s id in a frame' % side)


def run_chain(frames, k, w_of=None):
    """One chain: the problems of a (sequence, shard) in ascending frame, at cutoff k -> (2, 5) Python-int counts
    [TP, FP, MISS, MISMATCH, COST * 2^32].  w_of(problem) replaces the problem's weights (margins_hold)."""
    last_g, last_p = {}, {}
    out = [[0] * 5, [0] * 5]
    for pr in frames:
        w = pr['w'] if w_of is None else w_of(pr)
        pid, gid, gd = pr['pid'].tolist(), pr['gid'].tolist(), pr['gd'].tolist()
        rows = [r for r in range(len(pid)) if pr['score'][r] >= CUTOFFS[k]]
        row_of = {pid[r]: r for r in rows}
        pool_p, pool_g, pairs = list(rows), list(range(len(gid))), []
        for g in range(len(gid)):                                           # 1. carry
            q = last_g.get(gid[g])
            if q is not None and q in row_of and w[row_of[q], g] > 0:
                pairs.append((row_of[q], g))
                pool_p.remove(row_of[q])
                pool_g.remove(g)
        new = [(pool_p[i], pool_g[j]) for i, j in det_ref.matching(w[np.ix_(pool_p, pool_g)])] if pool_p and pool_g else []   # 2. match
        mismatched = [g for p, g in new if gid[g] in last_g and last_g[gid[g]] != pid[p]]                   # 3. update
        for p, g in new:
            a, b = gid[g], pid[p]
            if a in last_g:
                del last_p[last_g.pop(a)]
            if b in last_p:
                del last_g[last_p.pop(b)]
            last_g[a], last_p[b] = b, a
        pairs += new
        for lv in (1, 2):
            o = out[lv - 1]
            tp = [(p, g) for p, g in pairs if gd[g] <= lv]
            o[TP] += len(tp)
            o[FP] += len(rows) - len(pairs)
            o[MISS] += sum(1 for d in gd if d <= lv) - len(tp)
            o[MISMATCH] += sum(1 for g in mismatched if gd[g] <= lv)
            o[COST] += sum(int(np.round((1.0 - float(w[p, g])) * ONE)) for p, g in tp)
    return out


def table_from_problems(probs, n_shards, w_of=None):
    """The protocol's table (n_shards, 2, 101, 5) int64.  Chains of a (sequence, shard) whose cutoffs hold the same predictions in
    every frame have the same input; such a chain is walked once."""
    table = np.zeros((n_shards, 2, K, 5), dtype=np.int64)
    chains = {}
    for pr in probs:
        chains.setdefault((pr['seq'], pr['shard']), []).append(pr)
    for (_, shard), frames in chains.items():
        frames = sorted(frames, key=lambda p: p['frame'])
        done = {}
        for k in range(K):
            key = tuple(int((pr['score'] >= CUTOFFS[k]).sum()) for pr in frames)
            if key not in done:
                done[key] = np.array(run_chain(frames, k, w_of), dtype=np.int64)
            table[shard, :, k, :] += done[key]
    return table


def counts(config_type, box_type, scene):
    check_ids(scene)
    return table_from_problems(problems(config_type, box_type, scene), det_ref.n_shards_of(config_type))


def metrics(table, names):
    """{'<shard>_LEVEL_<L>/<MOTA|MOTP|MISS|MISMATCH|FP>': [value]} of the best cutoff (highest MOTA, the lowest k among equals)."""
    out = {}
    for s, name in enumerate(names):
        for lv in (1, 2):
            best = None
            for k in range(K):
                tp, fp, miss, mm, cost = (int(v) for v in table[s, lv - 1, k])
                n = tp + miss
                if n == 0:
                    continue
                mota = 1.0 - (miss + mm + fp) / n
                if best is None or mota > best[0]:
                    best = (mota, cost / ONE / tp if tp else 0.0, miss / n, mm / n, fp / n)
            best = best or (0.0, 0.0, 0.0, 0.0, 0.0)
            for key, v in zip(('MOTA', 'MOTP', 'MISS', 'MISMATCH', 'FP'), best):
                out['%s_LEVEL_%d/%s' % (name, lv, key)] = [v]
    return out


def margins_hold(config_type, box_type, scene, trials=4, eps=1e-5, thr_margin=1e-4):
    """The two conditions under which a differing device answer is a bug and not a tie: (a) no pair of a problem has an IoU within
    thr_margin of its threshold; (b) the whole table, COST aside, is unchanged when all non-zero weights move by +-eps (four random
    sign patterns), every chain run again."""
    probs = problems(config_type, box_type, scene)
    for pr in probs:
        m = det_ref.iou(pr['pb'], pr['gb'], box_type)
        if m.size and (np.abs(m - THR[pr['type']]) < thr_margin).any():
            return False
    n = det_ref.n_shards_of(config_type)
    base = table_from_problems(probs, n)
    rng = np.random.RandomState(4242)
    for _ in range(trials):
        moved = {id(pr): np.where(pr['w'] > 0, np.maximum(pr['w'] + eps * np.where(rng.rand(*pr['w'].shape) < 0.5, -1.0, 1.0), 1e-9), 0.0)
                 for pr in probs}
        if not np.array_equal(table_from_problems(probs, n, lambda pr: moved[id(pr)])[..., :4], base[..., :4]):
            return False
    return True
