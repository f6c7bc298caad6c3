"""Test helper: seeded detection scenes shared by the evaluation tests (CPU and GPU).

A scene is a dict of flat arrays (what WaymoDetectionMetricsEstimator.generate_waymo_type_results returns, 7-dof boxes):
n_frames, pd_frame, pd_box (float32), pd_type, pd_score (float32), gt_frame, gt_box (float32), gt_type, gt_diff.

``scene(seed, types)``: 12 frames.  Ground truths of the given types with mixed difficulty; predictions are perturbed ground truths
(shift, stretch and turn chosen so that IoUs land on both sides of 0.5 and 0.7), zero to four per ground truth - with several on
one ground truth the matching changes as the prefix grows and the greedy choice (the first, highest-scoring one) is not the
optimum - plus free false positives.  Scores hold the exact float32 cutoffs c_0 = 0, c_50 and c_100 = 1.  Frame 0 has no
prediction, frame 1 no ground truth, frame 2 one prediction, frame 3 more predictions than ground truths, frame 4 fewer; ground
truths sit exactly on the range-bin edges 30 and 50.
``single(seed, P, G)``: one frame, one type, P predictions on G ground truths (the large shapes of the GPU test).

A seed is kept only if tests/waymo_eval_ref.margins_hold says so for both box types (no IoU within 1e-4 of its threshold, every
prefix matching stable under +-1e-5 on all weights); tests/test_waymo_eval_cpu.py checks that for every seed below, so no case is
skipped at test time.
"""
import numpy as np

SIZES = {1: (4.6, 2.0, 1.7), 2: (0.9, 0.8, 1.75), 3: (0.6, 0.2, 0.9), 4: (1.8, 0.8, 1.7)}
TYPE_NAMES = {1: 'Vehicle', 2: 'Pedestrian', 3: 'Truck', 4: 'Cyclist'}
SCENES = [(1, (1, 2, 3, 4)), (1, (1, 2, 4))]                    # (seed, types): type 3 is absent from every frame of the second
SINGLES = [(1, 280, 20), (1, 900, 200)]                        # (seed, P, G)
N_FRAMES = 12


def _perturbed(rng, box, level):
    """A prediction for ``box``: level 0 close (IoU well above 0.7), 1 middling (around 0.5 .. 0.7), 2 loose (below 0.5)."""
    shift, stretch, turn = ((0.03, 0.03, 0.02), (0.10, 0.08, 0.06), (0.28, 0.2, 0.3))[level]
    out = box.copy()
    out[:3] += rng.uniform(-1, 1, 3) * shift * box[3:6]
    out[3:6] *= 1.0 + rng.uniform(-1, 1, 3) * stretch
    out[6] += rng.uniform(-1, 1) * turn + (np.pi if rng.rand() < 0.15 else 0.0)          # some face the other way: IoU kept, heading lost
    return out


def _gt_box(rng, t, centre=None):
    size = np.array(SIZES[t]) * rng.uniform(0.9, 1.1, 3)
    if centre is None:
        r, a = rng.uniform(3, 70), rng.uniform(-np.pi, np.pi)
        centre = (r * np.cos(a), r * np.sin(a), rng.uniform(-0.5, 1.0))
    return np.array([centre[0], centre[1], centre[2], size[0], size[1], size[2], rng.uniform(-np.pi, np.pi)])


def _pack(n_frames, pd, gt):
    f32 = lambda rows, w: np.array(rows, dtype=np.float64).reshape(-1, w).astype(np.float32)
    return {'n_frames': n_frames,
            'pd_frame': np.array([p[0] for p in pd], dtype=np.int64), 'pd_box': f32([p[1] for p in pd], 7),
            'pd_type': np.array([p[2] for p in pd], dtype=np.int64), 'pd_score': np.array([p[3] for p in pd], dtype=np.float32),
            'gt_frame': np.array([g[0] for g in gt], dtype=np.int64), 'gt_box': f32([g[1] for g in gt], 7),
            'gt_type': np.array([g[2] for g in gt], dtype=np.int64), 'gt_diff': np.array([g[3] for g in gt], dtype=np.int32)}


def scene(seed, types):
    rng = np.random.RandomState(seed)
    pd, gt = [], []
    for f in range(N_FRAMES):
        frame_gt = []
        if f != 1:
            for t in types:
                n = {2: 1, 3: 2, 4: 6}.get(f, rng.randint(2, 6))
                for _ in range(n):
                    frame_gt.append((f, _gt_box(rng, t), t, int(rng.randint(1, 3))))
            if f == 5:                                          # exactly on the bin edges (float32 holds 30 and 50)
                frame_gt.append((f, _gt_box(rng, types[0], (30.0, 0.0, 0.0)), types[0], 1))
                frame_gt.append((f, _gt_box(rng, types[1], (0.0, -50.0, 0.0)), types[1], 2))
        gt += frame_gt
        if f == 0:
            continue
        frame_pd = []
        for _, box, t, _ in frame_gt:
            k = {2: 0, 3: 3, 4: int(rng.rand() < 0.4)}.get(f, rng.randint(0, 5))
            for _ in range(k):
                frame_pd.append((f, _perturbed(rng, box, rng.randint(0, 3)), t, float(rng.uniform(0.02, 0.98))))
        for t in types:                                         # free false positives
            for _ in range({2: 0, 4: 0}.get(f, rng.randint(0, 3))):
                frame_pd.append((f, _gt_box(rng, t), t, float(rng.uniform(0.02, 0.6))))
        if f == 1:
            frame_pd = [(f, _gt_box(rng, t), t, float(rng.uniform(0.1, 0.9))) for t in types for _ in range(2)]
        if f == 2:
            frame_pd = [(f, _perturbed(rng, frame_gt[0][1], 0), frame_gt[0][2], 0.7)]
        pd += frame_pd
    for at, s in zip(rng.choice(len(pd), 6, replace=False), (0.0, 0.0, 0.5, 0.5, 1.0, 1.0)):
        pd[at] = pd[at][:3] + (float(np.float32(s)),)           # float32(0.5) == c_50 exactly, 0 == c_0, 1 == c_100
    return _pack(N_FRAMES, pd, gt)


def single(seed, n_pred, n_gt):
    rng = np.random.RandomState(seed)
    side = int(np.ceil(np.sqrt(n_gt)))
    gt = [(0, _gt_box(rng, 1, ((i % side - side / 2) * 9.0 + 2.0, (i // side - side / 2) * 9.0 + 1.0, 0.0)), 1, int(rng.randint(1, 3)))
          for i in range(n_gt)]
    pd = []
    for i in range(n_pred):
        if i < int(0.9 * n_pred):
            score = rng.uniform(0.0, 1.0)
            if n_pred > 500:                                    # 26 distinct scores: the float64 reference solves once per distinct prefix
                score = np.round(score * 25) / 25
            pd.append((0, _perturbed(rng, gt[rng.randint(0, n_gt)][1], rng.randint(0, 3)), 1, float(score)))
        else:
            pd.append((0, _gt_box(rng, 1), 1, float(rng.uniform(0.0, 0.7))))
    return _pack(1, pd, gt)


def flat(s):
    """The scene's arrays in the order tests/waymo_eval_ref.counts and detzero_amd.waymo_eval.problem_arrays take them."""
    return (s['n_frames'], s['pd_frame'], s['pd_box'], s['pd_type'], s['pd_score'], s['gt_frame'], s['gt_box'], s['gt_type'], s['gt_diff'])


def infos_of(s, beyond=None):
    """The scene as the info dicts waymo_evaluation takes (true-lidar boxes, difficulty as given, 10 points per box).  ``beyond``:
    a distance at which every frame gets one more Vehicle ground truth and prediction (for the distance mask)."""
    pds, gts = [], []
    for f in range(s['n_frames']):
        pm, gm = s['pd_frame'] == f, s['gt_frame'] == f
        pb, pt, ps = s['pd_box'][pm], s['pd_type'][pm], s['pd_score'][pm]
        gb, gtt, gd = s['gt_box'][gm], s['gt_type'][gm], s['gt_diff'][gm]
        if beyond is not None:
            far = np.array([[beyond, 0.0, 0.0, 4.6, 2.0, 1.7, 0.3]], dtype=np.float32)
            pb, pt, ps = np.concatenate([pb, far]), np.concatenate([pt, [1]]), np.concatenate([ps, np.float32([0.9])])
            gb, gtt, gd = np.concatenate([gb, far]), np.concatenate([gtt, [1]]), np.concatenate([gd, np.int32([1])])
        pds.append({'boxes_lidar': pb, 'score': ps, 'name': np.array([TYPE_NAMES[int(t)] for t in pt], dtype='<U16'),
                    'sequence_name': 'seq_%d' % (f // 6), 'frame_id': f % 6})
        gts.append({'gt_boxes_lidar': gb, 'name': np.array([TYPE_NAMES[int(t)] for t in gtt], dtype='<U16'), 'difficulty': gd.astype(np.int32),
                    'num_points_in_gt': np.full((len(gb),), 10, dtype=np.int64)})
    return pds, gts
