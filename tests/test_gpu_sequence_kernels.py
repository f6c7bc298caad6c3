"""The kernels that carry data BETWEEN the stages, one by one against plain references at their edges - the counterpart of
tests/test_gpu_head_post.py / test_gpu_box_ops.py / test_gpu_pdv_kernels.py / test_gpu_refine_kernels.py for csrc/wbf.hip, csrc/waymo_io.hip,
the crop path of csrc/head_post.hip and csrc/object_features.hip.  tests/test_tta.py, test_waymo_dataset.py, test_object_features.py and
test_refine.py hold them at the workload's shapes against goldens; here every input is made by hand, every GPU test hands the entry
point output AND workspace buffers with TAIL sentinel rows behind what the call may write (the entry points are called directly: the
Python wrappers allocate with torch.empty), launches twice and wants the same bits.  References: oracle/wbf.py, oracle/waymo_io.py,
oracle/cref.py, oracle/object_features.py and the float64 / longdouble helpers of oracle/sequence.py.  No goldens.

dz_wbf_fuse_3d (k_wbf_rank -> k_wbf_cluster -> k_wbf_emit; one workgroup of 256 threads = 4 waves per (frame, class)).  Routes of
  k_wbf_cluster's search for the best cluster: thread c % 256 looks at clusters c, c + 256, ...; a 64-lane butterfly; wave leaders write
  red_iou / red_idx; thread 0 reduces the four waves; equal IoUs go to the LOWER cluster index at every level.
    WBF_COUNT_CASES   1 / 63 / 64 / 65 / 255 / 256 / 257 / 300 clusters of one class, two models each (cluster index = creation order =
                      descending score of the first member; the slots are shuffled so that only the scores set it)
    WBF_MATCH_CASES   300 clusters, then ONE further candidate (lowest score, a third model whose other rows are label-0 padding with
                      decoy boxes and scores) that matches cluster 0 / 63 / 64 / 127 / 128 / 255 / 256 / 299: lane 0, the last lane of wave
                      0, each other wave, the second stride of thread 0
    WBF_TIE_CASES     clusters [-0.5,0,0,4,2,2,0] and [+0.5,...] at indices (10, 40) same wave, (10, 70) across waves, (200, 70) the lower
                      index in a later lane group, (5, 261) the same thread two strides apart - each also with the geometry swapped - and
                      a candidate [0,0,0,4,2,2,0] whose IoU with both is the same float32 (0.7777778, class 3: above 0.7)
    'threshold'       float32 IoU == float32(0.6) against the double 0.6 merges; IoU == 0.5 against 0.5 does not
    'gate', 'gate_eq' score x weight against skip_thr: float32(0.1) kept / one ulp below dropped, 0.02f x 0.5 (below 0.01) dropped / one ulp
                      above kept, a threshold EQUAL to the product kept (>=); a class that appears first and is gated away entirely
    WBF_RESCALE       weights None (sum 2) / [1, 0.5, 1] (sum 2.5) x allows_overflow x conf_type: 1 .. 4 members per cluster (below, equal
                      to, above the weight sum; above = one model gives two overlapping boxes), 'max' where the largest weighted score is
                      not the largest raw score
    'ids_*'           object ids: all -1, only the last member has one, the first has none and the second has one, all have one
    'batch_*'         5 frames (a frame without a candidate above the gate between live ones, a frame that lacks a class), 2 frames,
                      cand = 1 (two frames, one of them padding), per_model = 1
  Every new input: within a class no two weighted scores are equal, within a frame no two fused scores of the oracle are equal
  (numpy's argsort()[::-1] has no fixed order among equal values: there is no reference answer) - asserted before comparing.
  test_fusion_cases_are_discriminating: oracle variants with a planted fault (the last maximum, >= at the threshold, the threshold in
  float32, the heading of the last member) each change the expected result of the case built for it.

dz_tta_augment_points / dz_tta_restore_boxes (one grid-stride kernel each).  Every operation alone and all eleven together (flips x /
  y / xy, rotations 0, +-pi/4, pi, 1e-3, scales 0.95 / 1.05), n_ops 1 and 32; 0, 33 and an unknown code are refused.  Points n 0 / 1 / 255 /
  256 / 257 x c 3 / 5 / 6 (extra columns bit for bit, NaN included); boxes frames 1 / 3 x 5 operations x m 1 / 7 x dim 7 / 9 (the (r / m) % n
  mapping; columns 7..8 untouched); m = 0 and frames = 0 return without writing.  Flips and scaling: bit for bit against oracle/wbf.py.
  Rotations: against float64, see ROT_BASE.

dz_merge_sweeps (k_nlz_bits: one ballot word pair per wave -> bitmap_scan in chunks of 256 words = 8192 rows -> k_merge_sweeps).
  MERGE_CASES: n_total 0 / 1 / 63 / 64 / 65 / 255 / 256 / 257 / 8191 / 8192 / 8193 / 16385 (one ballot word, one block, one and two scan chunks)
  x 1 / 2 / 5 / 16 sweeps, empty sweeps first / in the middle / last / two in a row x keep flags all / none / only the first / only the last /
  runs of 64 / mixed (-1.0 keeps; 0, 1, -1.0000001, NaN, -0.0 do not).  Poses 1e5 m from the origin, a few metres apart.  Coordinates:
  float32 of the float64 evaluation bit for bit, one ulp where the longdouble value is within 2^-50 of a rounding midpoint (see
  MIDPOINT_SHARE); intensity (0, -0.0, 1e-8, +-20, 1e30, random) within 2e-7 of tanh; the rest exact.  17 sweeps, decreasing offsets,
  offsets that do not end at n_total and a workspace one byte short are refused.

dz_crop_points_in_boxes / dz_points_in_boxes_count (k_points_in_boxes_bits -> bitmap_scan -> k_crop_gather; k_points_in_boxes_count).
  CROP_CASES: m 1 / 63 / 64 / 65 / 255 / 256 / 257 / 513 x t 1 / 5 / 63 / 64 / 65 / 130 x payload words 1 / 4 / 6 / 8 x cap = total / below / 0;
  families random, 'all' (every box holds every point), 'nothing', 'five' (one point in five boxes: once per box, in box order),
  'faces' (points ON the z face are inside, points at the x / y faces + the 1e-5 margin), 'nan' (NaN points and boxes with a NaN
  centre are inside nothing).  Membership is oracle.cref.points_in_boxes_v2 (the project's bit-exact restatement); the plain float64
  test must agree for every pair farther than 1e-4 from every face (see FACE_SHARE).  cap below the total: d_total is the full
  count, offsets are complete, out / out_index keep their sentinels past cap.  t = 524288 boxes (more boxes than the capped grid of
  k_crop_gather has threads; 4 M bitmap words: the four-words-per-thread scan): offsets[t] == d_total == t.

dz_grm_encode_points / dz_prm_encode_points / dz_draw_subsets.  FEATURE_TRACKS (k = query_pts_num): one object with one box; boxes
  without points first / in the middle / last; a track of empty boxes; point counts k - 1 / k / k + 1; headings +-pi, +-3 pi, pi - 1e-12
  with an initial box that needs wrapping; classes 1 / 2 / 3 and an unknown 0 (all three class channels 0, by the contract stated in include/detzero_hip.h).  PRM: (query_pts_num, memory_pts_num) (5, 3) / (8, 7),
  box_max above every box count (padding slots: zero rows, padding_mask 1), PRM_ENCODINGS with 3 / 1 / 4 / 28 / 31 / 32 / 35 channels (both
  store paths, 'p2co' first), batch x box_max = 42 x 200 = 8400 slots past the 8192-workgroup grid on both store paths, the CRM call
  (no memory rows, no classes).  More than 40 padded channels (a repeated 'p2co') is refused BEFORE the launch - never launched.
  GRM: every subset of the four flags, a query slot of -1, a memory index of -1 between valid ones.  Draws: DRAW_CASES, n 0 / k - 1 / k /
  k + 1 / 5000, k 1 / 5 / 8 / 256, 1 / 63 / 64 / 65 sets, a non-zero first set id: bit for bit against device_draw_subset.

Numbers in this file (each printed by the test named).
  ROT_BASE        7.81e-6 m: the worst |float32 restatement (oracle.wbf.rotate_z_f32) - float64| over the rotation inputs of this
                  module, coordinates up to +-75 m (test_rotation_baseline measures 7.8095e-6 and holds the constant within 2 % above
                  it).  The kernels get 2 x ROT_BASE = 1.562e-5 m: they
                  round sin and cos once on the host and multiply-add without contraction, as the restatement does.
  MIDPOINT_SHARE  share of merged coordinates whose longdouble value lies within 2^-50 (relative to the value) of a float32 rounding
                  midpoint - the only places where two float64 evaluations (another order, fused multiply-adds) may round
                  differently, and where one ulp is allowed.  test_merge_inputs_and_reference measured 0 of 131514 elements; it must
                  stay below 1e-6 (so on these inputs the comparison is bit for bit everywhere).
  FACE_SHARE      share of (box, point) pairs of CROP_CASES closer than 1e-4 to a face, where the float64 test is not asserted:
                  test_crop_cases_on_the_host measured 0.01 %; it must stay below 1 %.
  Fusion: 1e-7 on scores and 1e-6 on boxes, as tests/test_tta.py against the same oracle; features: the tolerances of
  tests/test_object_features.py (2e-6 GRM, 3e-5 PRM points, 1e-5 trajectory, 1e-9 initial box).
"""
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

from detzero_amd import lib as L
from detzero_amd import object_features as OF
from oracle import cref
from oracle import object_features as OO
from oracle import sequence as S
from oracle import waymo_io as OW
from oracle import wbf as W
from tests.test_gpu_dense_conv import SENTINEL

F64, F32, I32 = np.float64, np.float32, np.int32
TAIL = 8                             # sentinel rows behind every buffer
SENT_F = float(np.array([SENTINEL], I32).view(F32)[0])
ROT_BASE = 7.81e-6
PI32 = float(F32(np.pi))


def f32(x):
    return F32(x)


def case_id(c):
    return '-'.join(str(x) for x in c) if isinstance(c, tuple) else str(c)


# ------------------------------------------------------------------------------------------------------------------------
# weighted box fusion: inputs
# ------------------------------------------------------------------------------------------------------------------------
DECOY = np.array([0, 0, 0, 4, 2, 2, 0], F32)         # box and score of the label-0 padding rows: must never be looked at


class Frame:
    """Candidates of one frame, (n_models, per_model) slots; unused slots are label-0 padding carrying a decoy box and a high score."""

    def __init__(self, n_models, per_model):
        self.boxes = np.tile(DECOY, (n_models, per_model, 1))
        self.scores = np.full((n_models, per_model), 0.99, F32)
        self.labels = np.zeros((n_models, per_model), I32)
        self.ids = np.full((n_models, per_model), -1, I32)
        self.free = [list(range(per_model)) for _ in range(n_models)]

    def add(self, model, box, score, label, oid=-1, slot=None):
        j = self.free[model].pop(0) if slot is None else self.free[model].pop(self.free[model].index(slot))
        self.boxes[model, j], self.scores[model, j], self.labels[model, j], self.ids[model, j] = np.asarray(box, F32), F32(score), label, oid


def pack(frames, weights=None, iou_thr=W.IOU_THR, skip_thr=W.SKIP_THR, conf_type='avg', overflow=False, ids=False):
    return {'boxes': np.stack([f.boxes for f in frames]), 'scores': np.stack([f.scores for f in frames]),
            'labels': np.stack([f.labels for f in frames]), 'ids': np.stack([f.ids for f in frames]) if ids else None,
            'weights': weights, 'iou_thr': tuple(iou_thr), 'skip_thr': tuple(skip_thr), 'conf_type': conf_type, 'overflow': overflow}


def grid_box(i, dz=1.6):
    """Object i of a 20-wide grid of well separated boxes with varied headings."""
    return np.array([12.0 * (i % 20) - 114, 8.0 * (i // 20) - 56, 0.0, 4, 2, dz, (i * 0.37) % 3 - 1.5], F32)


def clusters_frame(n, match=None, seed=0):
    """n objects of class 1 seen by two models (model 1: the box 5 cm off, the score x 0.9), in shuffled slots: cluster r is the
    object of score rank r.  match = r: a third model holds one more candidate, on the object of rank r, with the lowest score."""
    rng = np.random.default_rng(seed)
    per_model = n + 3
    fr = Frame(2 if match is None else 3, per_model)
    place = rng.permutation(n)                                     # object of rank r sits on grid position place[r]
    slots = [rng.permutation(per_model)[:n] for _ in range(2)]
    for r in range(n):
        box = grid_box(int(place[r]))
        s0 = f32(0.95 - 0.0015 * r)
        fr.add(0, box, s0, 1, slot=int(slots[0][r]))
        fr.add(1, box + np.array([0.05, 0, 0, 0, 0, 0, 0.01], F32), s0 * f32(0.9), 1, slot=int(slots[1][r]))
    if match is not None and match >= 0:                           # (match = -1: the third model is there and empty)
        fr.add(2, grid_box(int(place[match])) + np.array([0, 0.1, 0, 0, 0, 0, 0], F32), 0.2, 1, slot=per_model // 2)
    return fr


TIE_A, TIE_B, TIE_C = (np.array([x, 0, 0, 4, 2, 2, 0], F32) for x in (-0.5, 0.5, 0.0))
TIE_CLUSTERS = 270


def tie_frame(i_a, i_b, seed=0):
    """One model, class 3: TIE_CLUSTERS single-member clusters, TIE_A the cluster of index i_a and TIE_B of index i_b, then TIE_C."""
    rng = np.random.default_rng(seed)
    per_model = TIE_CLUSTERS + 4
    fr = Frame(1, per_model)
    slots = rng.permutation(per_model)
    k = 0
    for r in range(TIE_CLUSTERS):
        if r == i_a:
            box = TIE_A
        elif r == i_b:
            box = TIE_B
        else:
            box = np.array([10.0 * (k % 20) - 95, 8.0 * (k // 20) + 10, 0, 4, 2, 2, 0], F32)
            k += 1
        fr.add(0, box, f32(0.9 - 0.002 * r), 3, slot=int(slots[r]))
    fr.add(0, TIE_C, 0.0507, 3, slot=int(slots[TIE_CLUSTERS]))           # (off the 0.002 grid: the fused score collides with no other)
    return fr


def threshold_frame():
    fr = Frame(2, 4)
    fr.add(0, [0, 0, 0, 4, 2, 2, 0], 0.9, 2)
    fr.add(1, [1, 0, 0, 4, 2, 2, 0], 0.8, 2)             # IoU float32(0.6) > 0.6: merges
    fr.add(0, [0, 20, 0, 4, 2, 2, 0], 0.7, 1)
    fr.add(1, [0, 20, 0, 2, 2, 2, 0], 0.6, 1)            # IoU 0.5, threshold 0.5: does not
    return fr


def gate_frame():
    """Weights [1, 0.5].  Class 3 appears first and is gated away; every other candidate is an object of its own."""
    fr = Frame(2, 8)
    below = lambda v: np.nextafter(f32(v), f32(0))          # noqa: E731
    above = lambda v: np.nextafter(f32(v), f32(1))          # noqa: E731
    fr.add(0, grid_box(0), 0.001, 3)
    fr.add(1, grid_box(1), 0.015, 3)                     # x 0.5 = 0.0075 < 0.01
    fr.add(0, grid_box(2), f32(0.1), 1, slot=3)          # 0.1000000015 >= 0.1 (and == the threshold of 'gate_eq'): kept
    fr.add(0, grid_box(3), below(0.1), 1)                # one ulp below: dropped
    fr.add(0, grid_box(4), above(0.1), 1, slot=6)
    fr.add(1, grid_box(5), f32(0.02), 2, slot=2)         # 0.02f x 0.5 = 0.00999999977 < 0.01: dropped (== the threshold of 'gate_eq': kept)
    fr.add(1, grid_box(6), above(0.02), 2)               # 0.0100000007: kept
    fr.add(1, grid_box(7), below(0.02), 2, slot=5)       # dropped in both
    fr.add(0, grid_box(9), 0.5, 2)
    return fr


def members_frame(n_models, objects, per_model=None, first=0):
    """objects: (label, [(model, score, id), ...]); member k of an object is its box moved 3 cm and turned 0.02 rad per k.  Every
    third slot of a model stays padding."""
    per_model = per_model or 3 * len(objects) + 2
    fr = Frame(n_models, per_model)
    for m in range(n_models):
        fr.free[m] = [j for j in fr.free[m] if j % 3 != 1] + [j for j in fr.free[m] if j % 3 == 1]
    for o, (label, members) in enumerate(objects):
        base = grid_box(first + 2 * o, dz=(1.6, 1.7, 1.8)[label - 1])
        for k, (model, score, oid) in enumerate(members):
            fr.add(model, base + np.array([0.03 * k, 0, 0, 0, 0, 0, 0.02 * k], F32), score, label, oid)
    return fr


RESCALE_OBJECTS = {2: [(1, [(0, 0.91, -1)]), (1, [(0, 0.83, -1), (1, 0.77, -1)]), (2, [(0, 0.71, -1), (0, 0.66, -1), (1, 0.62, -1)]),
                       (3, [(1, 0.55, -1), (0, 0.52, -1)]), (1, [(1, 0.47, -1), (0, 0.44, -1), (1, 0.41, -1), (0, 0.38, -1)])],
                   # weights [1, 0.5, 1]: the third object's largest raw score 0.9 is model 1's (weighted 0.45), its largest weighted 0.6
                   3: [(1, [(1, 0.93, -1)]), (1, [(0, 0.84, -1), (2, 0.79, -1)]), (2, [(1, 0.9, -1), (0, 0.6, -1), (2, 0.57, -1)]),
                       (3, [(2, 0.53, -1), (1, 0.86, -1)]), (1, [(0, 0.49, -1), (1, 0.75, -1), (2, 0.46, -1), (2, 0.43, -1)])]}
WBF_RESCALE = [(w, ov, ct) for w in ('none', 'w') for ov in (False, True) for ct in ('avg', 'max')]
IDS_OBJECTS = {'ids_none': [(-1, -1, -1), (-1, -1, -1)], 'ids_last': [(-1, -1, 7), (-1, -1, 9)], 'ids_second': [(-1, 4, -1), (-1, 5, 6)],
               'ids_all': [(11, 12, 13), (21, 22, 23)]}
WBF_COUNT_CASES = [1, 63, 64, 65, 255, 256, 257, 300]
WBF_MATCH_CASES = [0, 63, 64, 127, 128, 255, 256, 299]
WBF_TIE_CASES = [(a, b, sw) for a, b in ((10, 40), (10, 70), (200, 70), (5, 261)) for sw in (False, True)]
WBF_OTHER_CASES = ['threshold', 'gate', 'gate_eq'] + sorted(IDS_OBJECTS) + ['batch_5', 'batch_2', 'batch_cand1', 'batch_per_model1']


def live_frame(seed, classes=(1, 2, 3)):
    """A small two-model frame of 2- and 1-member objects with scores that depend on the seed."""
    objs = []
    for o in range(5):
        s = 0.9 - 0.11 * o - 0.003 * seed
        label = classes[o % len(classes)]
        objs.append((label, [(0, s, -1), (1, s - 0.04, -1)] if o % 2 == 0 else [(o % 2, s, -1)]))
    return members_frame(2, objs, per_model=17, first=3 * seed)


@functools.lru_cache(maxsize=None)
def wbf_case(name):
    if isinstance(name, int):
        return pack([clusters_frame(name, seed=name)])
    if name[0] == 'match':
        return pack([clusters_frame(300, match=name[1], seed=300)])
    if name[0] == 'tie':
        _, a, b, sw = name
        return pack([tie_frame(b, a, seed=a) if sw else tie_frame(a, b, seed=a)])
    if name[0] == 'rescale':
        _, w, ov, ct = name
        n_models = 3 if w == 'w' else 2
        return pack([members_frame(n_models, RESCALE_OBJECTS[n_models])], weights=[1.0, 0.5, 1.0] if w == 'w' else None, conf_type=ct, overflow=ov)
    if name == 'threshold':
        return pack([threshold_frame()], iou_thr=(0.5, 0.6, 0.7))
    if name == 'gate':
        return pack([gate_frame()], weights=[1.0, 0.5])
    if name == 'gate_eq':
        return pack([gate_frame()], weights=[1.0, 0.5], skip_thr=(float(f32(0.1)), float(f32(0.02)) * 0.5, 0.01))
    if name in IDS_OBJECTS:
        objs = [(1 + o, [(m, 0.9 - 0.2 * o - 0.05 * m, oid) for m, oid in enumerate(trio)]) for o, trio in enumerate(IDS_OBJECTS[name])]
        return pack([members_frame(3, objs)], ids=True)
    if name == 'batch_5':
        dead = members_frame(2, [(1, [(0, 0.05, -1), (1, 0.09, -1)]), (2, [(0, 0.005, -1)])], per_model=17)
        return pack([live_frame(0), dead, live_frame(1), live_frame(2, classes=(1, 3)), live_frame(3)])
    if name == 'batch_2':
        return pack([live_frame(4), live_frame(5, classes=(2,))], conf_type='max')
    if name == 'batch_cand1':
        a, b = Frame(1, 1), Frame(1, 1)
        a.add(0, grid_box(0), 0.4, 2)
        return pack([a, b])
    if name == 'batch_per_model1':
        fr = Frame(4, 1)
        for m, s in enumerate((0.9, 0.8, 0.05, 0.7)):                 # one object from four models, one below the gate
            fr.add(m, grid_box(1) + np.array([0.02 * m, 0, 0, 0, 0, 0, 0], F32), s, 1)
        return pack([fr])
    raise KeyError(name)


ALL_WBF = (WBF_COUNT_CASES + [('match', k) for k in WBF_MATCH_CASES] + [('tie',) + c for c in WBF_TIE_CASES]
           + [('rescale',) + c for c in WBF_RESCALE] + WBF_OTHER_CASES)


@functools.lru_cache(maxsize=None)
def wbf_expected(name):
    """The oracle per frame, after the two conditions under which it IS a reference (no equal weighted scores within a class, no
    equal fused scores within a frame)."""
    c = wbf_case(name)
    out = []
    for f in range(c['boxes'].shape[0]):
        w = np.ones(c['boxes'].shape[1]) if c['weights'] is None else np.array(c['weights'])
        ws = c['scores'][f].astype(F64) * w[:, None]
        for lab in (1, 2, 3):
            v = ws[c['labels'][f] == lab]
            assert len(np.unique(v)) == len(v), (name, f, lab, 'equal weighted scores')
        res = W.weighted_boxes_fusion_3d(c['boxes'][f], c['scores'][f], c['labels'][f], weights=c['weights'], iou_thr=c['iou_thr'],
                                         skip_box_thr=c['skip_thr'], conf_type=c['conf_type'], allows_overflow=c['overflow'],
                                         obj_ids=None if c['ids'] is None else c['ids'][f])
        assert len(np.unique(res[1])) == len(res[1]), (name, f, 'equal fused scores')
        out.append(res)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# TTA inputs
# ------------------------------------------------------------------------------------------------------------------------
K_ORIG, K_FX, K_FY, K_FXY, K_ROT, K_SCALE = range(6)
ANGLES = [0.0, np.pi / 4, -np.pi / 4, np.pi, 1e-3]
TTA_ALL = [(K_ORIG, 0.0), (K_FX, 0.0), (K_FY, 0.0), (K_FXY, 0.0)] + [(K_ROT, a) for a in ANGLES] + [(K_SCALE, 0.95), (K_SCALE, 1.05)]
TTA_ALONE = [[op] for op in TTA_ALL]
RESTORE_SETS = {'a': [(K_FX, 0.0), (K_ROT, np.pi / 4), (K_SCALE, 0.95), (K_FY, 0.0), (K_FXY, 0.0)],
                'b': [(K_ROT, -np.pi / 4), (K_ROT, np.pi), (K_ROT, 1e-3), (K_SCALE, 1.05), (K_ORIG, 0.0)],
                'c': [(K_ROT, 0.0), (K_FXY, 0.0), (K_ORIG, 0.0), (K_ROT, 1e-3), (K_FY, 0.0)]}
#                 frames m  dim set
RESTORE_CASES = [(1, 1, 7, 'a'), (3, 7, 9, 'a'), (1, 7, 9, 'b'), (3, 1, 7, 'b'), (3, 7, 7, 'c')]
POINT_CASES = [(0, 3), (1, 3), (1, 6), (255, 5), (256, 6), (257, 3), (257, 5)]


def op_name(kind, param):
    p = repr(float(F32(param)))
    return {K_ORIG: 'tta_original', K_FX: 'tta_flip_x', K_FY: 'tta_flip_y', K_FXY: 'tta_flip_xy', K_ROT: 'tta_rot_' + p, K_SCALE: 'tta_scale_' + p}[kind]


def tta_points(n, c, seed=0):
    """xy up to +-75 m (the first rows ARE the corners), z +-4; the extra columns hold NaN, infinities and arbitrary bit patterns."""
    rng = np.random.default_rng(seed)
    p = np.empty((n, c), F32)
    p[:, :2] = rng.uniform(-75, 75, (n, 2))
    p[:, 2] = rng.uniform(-4, 4, n)
    p[:min(n, 4), :2] = np.array([[75, 75], [-75, 75], [75, -75], [-75, -75]], F32)[:min(n, 4)]
    if c > 3:
        extra = rng.integers(-2 ** 31, 2 ** 31, (n, c - 3), dtype=np.int64).astype(I32).view(F32)
        extra[::3, 0] = np.nan
        extra[1::5, -1] = np.inf
        p[:, 3:] = extra
    return p


def tta_boxes(frames, n_ops, m, seed=0):
    rng = np.random.default_rng(seed)
    b = np.empty((frames, n_ops, m, 7), F32)
    b[..., :2] = rng.uniform(-75, 75, b.shape[:-1] + (2,))
    b[..., 2] = rng.uniform(-3, 3, b.shape[:-1])
    b[..., 3:6] = rng.uniform(0.5, 10, b.shape[:-1] + (3,))
    b[..., 6] = rng.uniform(-np.pi, np.pi, b.shape[:-1])
    b[0, :, 0, :2] = 75.0
    return b


def augment_expected(p, ops):
    """-> (n_ops, n, c) float32 restatement (oracle/wbf.py), (n_ops, n, 2) float64 xy of the rotations (NaN elsewhere)."""
    want = np.stack([W.augment_points(p, op_name(k, a)) for k, a in ops]) if p.shape[0] else np.zeros((len(ops), 0, p.shape[1]), F32)
    rot = np.full((len(ops), p.shape[0], 2), np.nan)
    for i, (k, a) in enumerate(ops):
        if k == K_ROT:
            rot[i] = S.rotate_xy_f64(p[:, :2], F32(a))
    return want, rot


def restore_expected(b, ops):
    want = np.stack([W.restore_boxes(b[f], [op_name(k, a) for k, a in ops]) for f in range(b.shape[0])])
    rot = np.full(b.shape[:3] + (2,), np.nan)
    for i, (k, a) in enumerate(ops):
        if k == K_ROT:
            rot[:, i] = S.rotate_xy_f64(b[:, i, :, :2], F32(-float(F32(a))))
    return want, rot


def bits(a):
    return np.ascontiguousarray(a, F32).view(I32)


def check_rotated(got, want32, rot64, ops, axis, what):
    """Rows of rotations: x, y within 2 ROT_BASE of float64, everything else bit for bit; all other rows bit for bit."""
    worst = 0.0
    for i, (k, a) in enumerate(ops):
        g, w = np.take(got, i, axis), np.take(want32, i, axis)
        if k == K_ROT:
            r = np.take(rot64, i, axis)
            if g.size:
                worst = max(worst, float(np.abs(g[..., :2].astype(F64) - r).max()))
            np.testing.assert_array_equal(bits(g[..., 2:]), bits(w[..., 2:]), err_msg='%s, op %d' % (what, i))
        else:
            np.testing.assert_array_equal(bits(g), bits(w), err_msg='%s, op %d' % (what, i))
    print('  %s: rotations worst |got - float64| %.2e (allowed %.2e)' % (what, worst, 2 * ROT_BASE))
    assert worst <= 2 * ROT_BASE, (what, worst)


# ------------------------------------------------------------------------------------------------------------------------
# sweep merge inputs
# ------------------------------------------------------------------------------------------------------------------------
DROP_FLAGS = np.array([0.0, 1.0, -1.0000001, np.nan, -0.0], F32)
INTENSITIES = np.array([0.0, -0.0, 1e-8, 20.0, -20.0, 1e30], F32)
LAYOUTS = {'one': [1], 'two': [3, 2], 'five': [1, 2, 3, 1, 2], 'sixteen': [1] * 16, 'empty_first': [0, 2, 1], 'empty_mid': [2, 0, 3, 1],
           'empty_last': [1, 2, 0], 'empty_two': [2, 0, 0, 1, 3]}
#              n_total layout        keep
MERGE_CASES = [(0, 'one', 'all'), (1, 'one', 'all'), (1, 'empty_first', 'none'), (63, 'two', 'mixed'), (64, 'five', 'all'), (65, 'sixteen', 'mixed'),
               (255, 'empty_mid', 'runs64'), (256, 'empty_two', 'mixed'), (257, 'empty_last', 'first'), (8191, 'five', 'mixed'),
               (8192, 'two', 'last'), (8192, 'one', 'all'), (8193, 'sixteen', 'runs64'), (16385, 'empty_mid', 'mixed'), (16385, 'five', 'none'),
               (16385, 'one', 'all')]


def pose(yaw, t):
    m = np.eye(4)
    m[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    m[:3, 3] = t
    return m


@functools.lru_cache(maxsize=None)
def merge_case(i):
    n, layout, keep = MERGE_CASES[i]
    rng = np.random.default_rng(4000 + i)
    parts = np.array(LAYOUTS[layout], F64)
    offsets = np.concatenate([[0], np.floor(np.cumsum(parts) / parts.sum() * n + 1e-9)]).astype(I32)
    offsets[-1] = n
    raw = np.empty((n, 6), F32)
    raw[:, :2] = rng.uniform(-75, 75, (n, 2))
    raw[:, 2] = rng.uniform(-4, 4, n)
    raw[:, 3] = rng.uniform(0, 3, n)
    raw[:, 3][rng.permutation(n)[:n // 3]] = INTENSITIES[rng.integers(0, len(INTENSITIES), n // 3)]
    raw[:len(INTENSITIES), 3] = INTENSITIES[:n]
    raw[:, 4] = rng.uniform(0, 2, n)
    flag = np.full(n, -1.0, F32)
    drop = DROP_FLAGS[np.arange(n) % len(DROP_FLAGS)]
    if keep == 'none':
        flag = drop
    elif keep in ('first', 'last'):
        flag = drop.copy()
        flag[0 if keep == 'first' else n - 1] = -1.0
    elif keep == 'runs64':
        flag = np.where((np.arange(n) // 64) % 2 == 0, flag, drop)
    elif keep == 'mixed':
        flag = np.where(rng.random(n) < 0.6, flag, drop)
        if n >= 10:                                                   # every dropping value is there, whatever the draw
            flag[:5], flag[5:10] = drop[:5], -1.0
    raw[:, 5] = flag
    n_sweeps = len(parts)
    cur = {'pose': pose(0.3, [1e5, -1e5, 30.0]), 'time_stamp': 1550000000000000}
    infos = [{'pose': pose(0.3 + 0.01 * s, [1e5 + 1.5 * s, -1e5 + 0.3 * s, 30.0 + 0.01 * s]), 'time_stamp': 1550000000000000 - 100000 * s}
             for s in range(n_sweeps)]
    mats = np.stack([(np.linalg.inv(cur['pose']) @ t['pose'])[:3, :] for t in infos])
    dts = np.array([float(int(t['time_stamp']) - int(cur['time_stamp'])) / 1000000. for t in infos])
    # expected rows
    kept = raw[:, 5] == F32(-1.0)
    sweep = np.searchsorted(offsets[1:], np.arange(n), side='right')
    v64, v80 = np.zeros((n, 3)), np.zeros((n, 3), np.longdouble)
    for s in range(n_sweeps):
        sel = sweep == s
        v64[sel] = S.affine_rows(raw[sel, :3], mats[s])
        v80[sel] = S.affine_rows(raw[sel, :3], mats[s], np.longdouble)
    want = np.concatenate([v64.astype(F32), np.tanh(raw[:, 3:4].astype(F64)).astype(F32), raw[:, 4:5], dts[sweep].astype(F32)[:, None]], axis=1)[kept]
    return {'raw': raw, 'offsets': offsets, 'mats': mats, 'dts': dts, 'cur': cur, 'infos': infos, 'want': want, 'tanh64': np.tanh(raw[kept, 3].astype(F64)),
            'loose': S.near_f32_midpoint(v80)[kept]}


def check_merged(got, d, what):
    """got (k, 6) float32 against the case's expected rows."""
    want = d['want']
    assert got.shape == want.shape, (what, got.shape, want.shape)
    steps = S.ulp_steps(got[:, :3], want[:, :3])
    assert (steps[~d['loose']] == 0).all() and (steps <= 1).all(), (what, int(steps.max()), int((steps > 0).sum()))
    np.testing.assert_array_equal(bits(got[:, 4:]), bits(want[:, 4:]), err_msg=what)
    err = np.abs(got[:, 3].astype(F64) - d['tanh64'])
    print('  %s: %d rows kept, %d coordinates off by one ulp (all near a midpoint), tanh worst %.1e' % (what, len(got), int((steps > 0).sum()),
                                                                                                      err.max() if len(err) else 0.0))
    assert (err <= 2e-7).all(), (what, err.max())


# ------------------------------------------------------------------------------------------------------------------------
# crop inputs
# ------------------------------------------------------------------------------------------------------------------------
#              m   t   words cap      family
CROP_CASES = [(1, 1, 1, 'full', 'all'), (63, 63, 4, 'full', 'random'), (64, 64, 6, 'short', 'random'), (65, 65, 8, 'zero', 'random'),
              (255, 130, 4, 'full', 'random'), (256, 1, 1, 'short', 'all'), (257, 5, 6, 'full', 'five'), (513, 130, 8, 'short', 'random'),
              (513, 63, 4, 'full', 'nothing'), (257, 64, 4, 'full', 'faces'), (255, 65, 1, 'full', 'nan'), (1, 130, 4, 'full', 'all'),
              (513, 64, 1, 'short', 'all')]
FACE_BOX = np.array([0, 0, 0, 4, 2, 2, 0], F32)
FACE_POINTS = np.array([[0, 0, 1], [0, 0, -1], [0, 0, np.nextafter(F32(1), F32(2))], [2, 0, 0], [F32(2 + 0.5e-5), 0, 0], [F32(2 + 2e-5), 0, 0],
                        [-2, 0, 0.5], [0, 1, 0], [0, F32(1 + 0.5e-5), 0], [0, F32(-1 - 2e-5), 0], [F32(2 + 2e-5), F32(1 + 2e-5), 1]], F32)
FACE_INSIDE = [1, 1, 0, 1, 1, 0, 1, 1, 1, 0, 0]


@functools.lru_cache(maxsize=None)
def crop_case(i):
    m, t, words, cap_mode, family = CROP_CASES[i]
    rng = np.random.default_rng(5000 + i)
    boxes = np.empty((t, 7), F32)
    boxes[:, :2] = rng.uniform(-20, 20, (t, 2))
    boxes[:, 2] = rng.uniform(-1, 1, t)
    boxes[:, 3:6] = rng.uniform([2, 1, 1], [8, 4, 3], (t, 3))
    boxes[:, 6] = rng.uniform(-np.pi, np.pi, t)
    pts = rng.uniform([-25, -25, -2], [25, 25, 2], (m, 3)).astype(F32)
    owner = rng.integers(0, t, m)
    local = rng.uniform(-0.6, 0.6, (m, 3)) * boxes[owner, 3:6]
    c, s = np.cos(boxes[owner, 6]), np.sin(boxes[owner, 6])
    seeded = np.stack([local[:, 0] * c - local[:, 1] * s, local[:, 0] * s + local[:, 1] * c, local[:, 2]], 1) + boxes[owner, :3]
    half = rng.random(m) < 0.5
    pts[half] = seeded[half].astype(F32)
    if family == 'all':
        boxes[:, :3], boxes[:, 3:6] = 0, [200, 200, 50]
    elif family == 'nothing':
        boxes[:, 0] += 1000
    elif family == 'five':
        pts[:] = rng.uniform([100, 100, -2], [120, 120, 2], (m, 3))
        pts[7] = [3, -2, 0.5]
        boxes[:, :3], boxes[:, 3:6] = pts[7], [0.5, 0.5, 0.5]
    elif family == 'faces':
        boxes[0] = FACE_BOX
        pts[:len(FACE_POINTS)] = FACE_POINTS
    elif family == 'nan':
        pts[::7] = np.nan
        boxes[::5, 0] = np.nan
    payload = rng.integers(-2 ** 31, 2 ** 31, (m, words), dtype=np.int64).astype(I32)
    mask = cref.points_in_boxes_v2(pts, boxes).astype(bool)
    rows, index, offsets = S.crop_rows(mask, payload)
    total = int(offsets[-1])
    cap = {'full': total, 'short': total // 2, 'zero': 0}[cap_mode]
    return {'pts': pts, 'boxes': boxes, 'payload': payload, 'mask': mask, 'rows': rows, 'index': index, 'offsets': offsets, 'total': total, 'cap': cap}


# ------------------------------------------------------------------------------------------------------------------------
# object feature inputs
# ------------------------------------------------------------------------------------------------------------------------
PRM_ENCODINGS = [('xyz',), ('score',), ('xyz', 'intensity'), ('p2co', 'intensity'), ('p2co', 'xyz', 'score'), ('p2co', 'xyz', 'intensity', 'score'),
                 ('class', 'xyz', 'intensity', 'p2co', 'score')]
PRM_CHANNELS = [3, 1, 4, 28, 31, 32, 35]
PRM_SIZES = [(5, 3), (8, 7)]
GRM_SUBSETS = [tuple(e for b, e in enumerate(('xyz', 'intensity', 'p2s', 'score')) if s >> b & 1) for s in range(1, 16)]
#              sets k   first set id
DRAW_CASES = [(1, 1, 0), (63, 256, 0), (64, 5, 7), (65, 8, 1000)]


def make_track(seed, counts, name, headings=None):
    """A hand-made object track: box t holds counts[t] points inside it; scores are distinct."""
    rng = np.random.default_rng(seed)
    t = len(counts)
    boxes = np.zeros((t, 7))
    boxes[:, :3] = np.array([30.0 + seed, -12.0, 1.0]) + np.cumsum(rng.uniform(-0.6, 0.6, (t, 3)), axis=0)
    boxes[:, 3:6] = np.array([4.5, 1.9, 1.6]) + rng.uniform(-0.1, 0.1, (t, 3))
    boxes[:, 6] = rng.uniform(-3, 3, t) if headings is None else headings
    pts = []
    for i, n in enumerate(counts):
        local = rng.uniform(-0.5, 0.5, (n, 3)) * boxes[i, 3:6]
        c, s = np.cos(boxes[i, 6]), np.sin(boxes[i, 6])
        xyz = np.stack([local[:, 0] * c - local[:, 1] * s, local[:, 0] * s + local[:, 1] * c, local[:, 2]], 1) + boxes[i, :3]
        pts.append(np.concatenate([xyz, rng.uniform(0, 1, (n, 1))], axis=1))
    return {'boxes_global': boxes, 'score': 0.3 + 0.6 * rng.permutation(t) / max(t, 1) + 0.01 * rng.random(t), 'pts': pts, 'name': name}


def feature_tracks(k):
    """FEATURE_TRACKS for a selection size k (the docstring's list)."""
    return [make_track(1, [k + 1], 'Vehicle'),
            make_track(2, [0, k - 1, 0, k, k + 1, 0], 'Pedestrian'),
            make_track(3, [0, 0, 0], 'Cyclist'),
            make_track(4, [k, 2, k + 3, 1, 2 * k], 0, headings=[np.pi, -np.pi, 3 * np.pi, -3 * np.pi, np.pi - 1e-12]),
            make_track(5, [3, k], 'Cyclist', headings=[0.5, -3 * np.pi])]


def grid_tracks():
    """42 objects of one tiny box each: with box_max = 200 the PRM point kernel walks 8400 slots with 8192 workgroups."""
    return [make_track(100 + i, [2 + i % 3], ('Vehicle', 'Pedestrian', 'Cyclist')[i % 3]) for i in range(42)]


def prm_expected(tracks, encoding, box_max, q_n, m_n, seed):
    rng = random.Random(seed)
    ref = OO.prm_batch([OO.prm_object(t, encoding, box_max, q_n, m_n, rng) for t in tracks])
    return ref


def close(got, ref, atol, rtol, what):
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    print('  %s: worst |got - want| %.2e (atol %.0e)' % (what, err.max() if err.size else 0.0, atol))
    assert (err <= atol + rtol * np.abs(ref)).all(), (what, err.max())


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the references, the case tables, the measured numbers
# ------------------------------------------------------------------------------------------------------------------------
def test_fusion_inputs_are_what_the_case_tables_say():
    """The arithmetic the cases are built on, checked with the oracle: the three IoU values, the cluster counts, which cluster the
    extra candidate joins, what the gate keeps - and that every case meets the no-equal-scores conditions (wbf_expected)."""
    iou = lambda a, b: W.iou3d_one_to_many(np.asarray(a, F32), np.asarray([b], F32))[0]          # noqa: E731
    both = W.iou3d_one_to_many(TIE_C, np.stack([TIE_A, TIE_B]))
    assert both[0] == both[1] == F32(0.7777778) and float(both[0]) > 0.7 and float(iou(TIE_A, TIE_B)) < 0.7
    v = iou([0, 0, 0, 4, 2, 2, 0], [1, 0, 0, 4, 2, 2, 0])
    assert v == F32(0.6) and float(v) > 0.6 and not F32(v) > F32(0.6)
    assert iou([0, 0, 0, 4, 2, 2, 0], [0, 0, 0, 2, 2, 2, 0]) == F32(0.5)
    for name in ALL_WBF:
        wbf_expected(name)
    for n in WBF_COUNT_CASES:
        c = wbf_case(n)
        assert len(wbf_expected(n)[0][1]) == n and int((c['labels'] == 1).sum()) == 2 * n
    base = wbf_expected(('match', -1))[0]
    for k in WBF_MATCH_CASES:
        b, s, l = wbf_expected(('match', k))[0]
        assert len(s) == 300
        # the fused score of the joined cluster is the only one that changed; its rank among the 300 scores of the plain case = k
        changed = [i for i in range(300) if base[1][i] not in s]
        assert changed == [k], (k, changed)
    for a, b, sw in WBF_TIE_CASES:
        fb, fs, fl = wbf_expected(('tie', a, b, sw))[0]
        assert len(fs) == TIE_CLUSTERS
        grown = fb[(np.abs(fb[:, 1]) < 1) & (np.abs(fb[:, 0]) < 0.49)]                 # the cluster pulled towards the candidate
        assert len(grown) == 1
        low_is_a = (a < b) != sw                                                        # the lower cluster index holds TIE_A (x < 0)
        assert (grown[0, 0] < 0) == low_is_a, (a, b, sw)
    tb, ts, tl = wbf_expected('threshold')[0]
    assert sorted(tl.tolist()) == [1, 1, 2]
    for name, n_kept in (('gate', 4), ('gate_eq', 5)):
        gb, gs, gl = wbf_expected(name)[0]
        assert len(gs) == n_kept and 3 not in gl.tolist() and wbf_case(name)['labels'][0, 0, 0] == 3, (name, len(gs))
    for w, ov, ct in WBF_RESCALE:
        c = wbf_case(('rescale', w, ov, ct))
        wsum = 2.5 if w == 'w' else 2.0
        sizes = [len(m) for _, m in RESCALE_OBJECTS[3 if w == 'w' else 2]]
        assert any(n < wsum for n in sizes) and any(n > wsum for n in sizes) and (w == 'w' or any(n == wsum for n in sizes))
        assert len(wbf_expected(('rescale', w, ov, ct))[0][1]) == len(sizes)
    # 'max' with weights: the largest weighted score of the third object is not its largest raw score
    raw = [s for _, s, _ in RESCALE_OBJECTS[3][2][1]]
    wt = [s * [1.0, 0.5, 1.0][m] for m, s, _ in RESCALE_OBJECTS[3][2][1]]
    assert int(np.argmax(raw)) != int(np.argmax(wt))
    for name in IDS_OBJECTS:
        assert len(wbf_expected(name)[0]) == 4 and len(wbf_expected(name)[0][3]) == 2
    assert wbf_expected('ids_none')[0][3].tolist() == [-1, -1] and sorted(wbf_expected('ids_last')[0][3].tolist()) == [7, 9]
    assert sorted(wbf_expected('ids_second')[0][3].tolist()) == [4, 5] and sorted(wbf_expected('ids_all')[0][3].tolist()) == [11, 21]
    five = wbf_expected('batch_5')
    assert [len(r[1]) for r in five] == [5, 0, 5, 5, 5] and 2 not in five[3][2].tolist() and 2 in five[0][2].tolist()
    assert [len(r[1]) for r in wbf_expected('batch_cand1')] == [1, 0] and len(wbf_expected('batch_per_model1')[0][1]) == 1
    assert wbf_case('batch_cand1')['boxes'].shape[1:3] == (1, 1) and wbf_case('batch_per_model1')['boxes'].shape[1:3] == (4, 1)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_fusion_cases_are_discriminating():
    """oracle.sequence.fusion_variant with its defaults is the oracle; with one planted fault each it changes the expected result
    of the case built for that fault (and so a kernel with that fault fails the case)."""
    def run(name, **fault):
        c = wbf_case(name)
        return S.fusion_variant(c['boxes'][0], c['scores'][0], c['labels'][0], weights=c['weights'], iou_thr=c['iou_thr'], skip_box_thr=c['skip_thr'],
                                conf_type=c['conf_type'], allows_overflow=c['overflow'], **fault)
    for name in [('tie', 10, 70, False), 'threshold', 'gate', ('rescale', 'w', False, 'max'), ('rescale', 'none', True, 'avg'), 65]:
        assert _same(run(name), wbf_expected(name)[0][:3]), name
    for a, b, sw in WBF_TIE_CASES:
        assert not _same(run(('tie', a, b, sw), argmax='last'), wbf_expected(('tie', a, b, sw))[0])
    assert len(run('threshold', compare='ge')[1]) == 2 and len(run('threshold', thr_f32=True)[1]) == 4 and len(wbf_expected('threshold')[0][1]) == 3
    for w, ov, ct in WBF_RESCALE:
        got, want = run(('rescale', w, ov, ct), heading='last'), wbf_expected(('rescale', w, ov, ct))[0]
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0][:, :6], want[0][:, :6]) and (got[0][:, 6] != want[0][:, 6]).sum() == 4


def test_rotation_baseline():
    """ROT_BASE: the float32 restatement of the rotations against float64 over every rotation input of this module."""
    worst = 0.0
    for n, c in POINT_CASES:
        p = tta_points(n, c, seed=n + c)
        want, rot = augment_expected(p, TTA_ALL)
        for i, (k, a) in enumerate(TTA_ALL):
            if k == K_ROT and n:
                worst = max(worst, float(np.abs(want[i, :, :2].astype(F64) - rot[i]).max()))
    for ci, (frames, m, dim, key) in enumerate(RESTORE_CASES):
        b = tta_boxes(frames, 5, m, seed=ci)
        want, rot = restore_expected(b, RESTORE_SETS[key])
        for i, (k, a) in enumerate(RESTORE_SETS[key]):
            if k == K_ROT:
                worst = max(worst, float(np.abs(want[:, i, :, :2].astype(F64) - rot[:, i]).max()))
    print('  rotations, float32 restatement against float64: worst %.2e m (ROT_BASE %.2e, the kernels get %.2e)' % (worst, ROT_BASE, 2 * ROT_BASE))
    assert worst <= ROT_BASE <= 1.02 * worst, (worst, ROT_BASE)
    # a rotation by the angle of the wrong sign, or with one coordinate's sine dropped, is far outside
    p = tta_points(257, 3, seed=1)
    good = S.rotate_xy_f64(p[:, :2], 1e-3)
    assert np.abs(good - S.rotate_xy_f64(p[:, :2], -1e-3)).max() > 1000 * ROT_BASE
    c, sn = np.cos(F64(F32(1e-3))), np.sin(F64(F32(1e-3)))
    no_sine = np.stack([p[:, 0].astype(F64) * c, p[:, 0].astype(F64) * sn + p[:, 1].astype(F64) * c], axis=-1)      # x' without its - y sin term
    assert np.abs(good - no_sine).max() > 1000 * ROT_BASE


def test_tta_case_tables():
    assert {n for n, c in POINT_CASES} == {0, 1, 255, 256, 257} and {c for n, c in POINT_CASES} == {3, 5, 6}
    assert {k for k, a in TTA_ALL} == set(range(6)) and len(TTA_ALL) == 11
    assert {float(a) for k, a in TTA_ALL if k == K_ROT} == {0.0, np.pi / 4, -np.pi / 4, np.pi, 1e-3} and {a for k, a in TTA_ALL if k == K_SCALE} == {0.95, 1.05}
    assert {c[0] for c in RESTORE_CASES} == {1, 3} and {c[1] for c in RESTORE_CASES} == {1, 7} and {c[2] for c in RESTORE_CASES} == {7, 9}
    assert all(len(v) == 5 for v in RESTORE_SETS.values()) and {k for v in RESTORE_SETS.values() for k, a in v} == set(range(6))
    assert op_name(K_ROT, -np.pi / 4) == 'tta_rot_-0.7853981852531433' and op_name(K_SCALE, 0.95).startswith('tta_scale_0.9499999')


def test_merge_inputs_and_reference():
    """MERGE_CASES reach what the docstring names; the float64 evaluation of the affine rows IS oracle.waymo_io.merge_sweeps (up to
    one ulp at the flagged near-midpoint elements); MIDPOINT_SHARE."""
    assert {c[0] for c in MERGE_CASES} == {0, 1, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193, 16385}
    assert {c[1] for c in MERGE_CASES} == set(LAYOUTS) and {len(v) for v in LAYOUTS.values()} >= {1, 2, 5, 16}
    assert {c[2] for c in MERGE_CASES} == {'all', 'none', 'first', 'last', 'runs64', 'mixed'}
    assert [(n + 63) // 64 * 2 > 256 for n in (8191, 8192, 8193)] == [False, False, True]            # bitmap words against one scan chunk
    flagged = elements = 0
    for i, (n, layout, keep) in enumerate(MERGE_CASES):
        d = merge_case(i)
        off = d['offsets']
        assert off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all() and len(off) == len(LAYOUTS[layout]) + 1
        if layout.startswith('empty') and n > 16:
            empty = [s for s, v in enumerate(LAYOUTS[layout]) if v == 0]
            assert all(off[s] == off[s + 1] for s in empty) and (np.diff(off) > 0).sum() == len(off) - 1 - len(empty)
        kept = int((d['raw'][:, 5] == F32(-1.0)).sum())
        assert kept == {'all': n, 'none': 0, 'first': 1, 'last': 1}.get(keep, kept) and d['want'].shape[0] == kept
        if keep in ('runs64', 'mixed') and n > 16:
            assert 0 < kept < n and {repr(float(v)) for v in d['raw'][:, 5]} >= {'-1.0', '0.0', '1.0', '-0.0', 'nan', repr(float(F32(-1.0000001)))}
        if n >= 63:
            assert {float(v) for v in INTENSITIES} <= {float(v) for v in d['raw'][:, 3]}
        parts = [d['raw'][off[s]:off[s + 1]].copy() for s in range(len(off) - 1)]
        ref = OW.merge_sweeps(d['cur'], d['infos'], parts) if n else np.zeros((0, 6))
        check_merged(ref.astype(F32), d, 'oracle.waymo_io.merge_sweeps, case %d' % i)
        flagged += int(d['loose'].sum())
        elements += 3 * kept
    # poses 1e5 m out, a few metres apart: the relative transforms the kernel is handed are small
    m = merge_case(len(MERGE_CASES) - 1)
    assert np.abs(m['mats'][:, :, 3]).max() < 40 and np.abs(m['cur']['pose'][:2, 3]).min() >= 1e5
    share = flagged / elements
    print('  merge: %d of %d coordinates within 2^-50 of a float32 midpoint (share %.1e)' % (flagged, elements, share))
    assert share < 1e-6


def test_merge_midpoint_detector_by_hand():
    """near_f32_midpoint flags exactly the values at a midpoint: 1 + 2^-24 (between 1 and 1 + 2^-23), not 1 + 2^-24 + 2^-40."""
    one = np.longdouble(1)
    v = np.array([one + np.longdouble(2.0 ** -24), one + np.longdouble(2.0 ** -24) + np.longdouble(2.0 ** -40), one, one - np.longdouble(2.0 ** -25)])
    assert S.near_f32_midpoint(v).tolist() == [True, False, False, True]
    assert S.ulp_steps(np.array([1.0, -1.0, 0.0], F32), np.array([np.nextafter(F32(1), F32(2)), -1.0, -0.0], F32)).tolist() == [1, 0, 0]
    val = S.affine_rows(np.array([[1, 2, 3]], F32), np.array([[1, 0, 0, 10], [0, -1, 0, 0], [2, 2, 2, -12.0]]))
    assert val.tolist() == [[11.0, -2.0, 0.0]]


def test_crop_cases_on_the_host():
    """CROP_CASES reach what the docstring names; the restated membership agrees with the plain float64 test away from the faces;
    FACE_SHARE."""
    assert {c[0] for c in CROP_CASES} == {1, 63, 64, 65, 255, 256, 257, 513} and {c[1] for c in CROP_CASES} == {1, 5, 63, 64, 65, 130}
    assert {c[2] for c in CROP_CASES} == {1, 4, 6, 8} and {c[3] for c in CROP_CASES} == {'full', 'short', 'zero'}
    assert {c[4] for c in CROP_CASES} == {'all', 'random', 'nothing', 'five', 'faces', 'nan'}
    near = pairs = 0
    for i, (m, t, words, cap_mode, family) in enumerate(CROP_CASES):
        d = crop_case(i)
        inside, dist = S.inside_f64(d['pts'], d['boxes'])
        far = dist > 1e-4                                             # (NaN distances compare False: those pairs are checked below)
        assert np.array_equal(inside[far], d['mask'][far]), (i, int((inside[far] != d['mask'][far]).sum()))
        valid = ~np.isnan(dist)
        near += int((valid & ~far).sum())
        pairs += int(valid.sum())
        total = d['total']
        if family == 'all':
            assert d['mask'].all() and total == m * t
        elif family == 'nothing':
            assert total == 0
        elif family == 'five':
            assert total == 5 and d['index'].tolist() == [7] * 5 and d['offsets'].tolist() == [0, 1, 2, 3, 4, 5]
        elif family == 'faces':
            assert d['mask'][0, :len(FACE_POINTS)].astype(int).tolist() == FACE_INSIDE
        elif family == 'nan':
            assert not d['mask'][:, ::7].any() and not d['mask'][::5].any() and total > 0
        else:
            assert total > 0 and ((np.diff(d['offsets']) == 0).any() or t < 63)
        if cap_mode == 'short':
            assert 0 < d['cap'] < total
    share = near / pairs
    print('  crop: %d of %d (box, point) pairs within 1e-4 of a face (share %.2f %%)' % (near, pairs, 100 * share))
    assert share < 0.01


def test_feature_case_tables():
    lib_channels = {'xyz': 3, 'intensity': 1, 'p2co': 27, 'score': 1, 'class': 3}
    assert [sum(lib_channels[e] for e in enc) for enc in PRM_ENCODINGS] == PRM_CHANNELS == [3, 1, 4, 28, 31, 32, 35]
    assert {c & 3 == 0 for c in PRM_CHANNELS} == {True, False} and PRM_ENCODINGS[3][0] == 'p2co'
    assert len(GRM_SUBSETS) == 15 and len(set(GRM_SUBSETS)) == 15
    for k, mn in PRM_SIZES:
        tracks = feature_tracks(k)
        counts = [[p.shape[0] for p in t['pts']] for t in tracks]
        assert counts[0] == [k + 1] and counts[1] == [0, k - 1, 0, k, k + 1, 0] and counts[2] == [0, 0, 0]
        assert {t['name'] for t in tracks} == {'Vehicle', 'Pedestrian', 'Cyclist', 0}
        init = tracks[3]['boxes_global'][5 // 2, 6]
        assert init == 3 * np.pi and OO.wrap_heading(np.array([init]))[0] != init
        assert max(len(c) for c in counts) < 7                                           # box_max 7: every object has padding slots
    assert 42 * 200 > 8192 and len(grid_tracks()) == 42
    for sets, k, set0 in DRAW_CASES:
        assert {0, k - 1, k, k + 1, 5000} <= set(draw_counts(sets, k).tolist()) or sets == 1
    assert {c[0] for c in DRAW_CASES} == {1, 63, 64, 65} and {c[1] for c in DRAW_CASES} >= {1, 256} and any(c[2] for c in DRAW_CASES)


def test_repeated_feature_names_are_refused_on_the_host():
    """('xyz', 'p2co', 'p2co') would be 57 channels - past the 40 entries of the point kernel's channel tables."""
    tracks = feature_tracks(5)
    with pytest.raises(L.DetZeroHipError, match='repeats'):
        OF.prm_features(tracks, encoding=('xyz', 'p2co', 'p2co'), device=torch.device('cpu'))
    with pytest.raises(L.DetZeroHipError, match='repeats'):
        OF.crm_features(tracks, encoding=('score', 'xyz', 'score'), device=torch.device('cpu'))


def draw_counts(sets, k):
    base = [0, k - 1, k, k + 1, 5000, 3 * k, k + 7]
    return np.array([k] if sets == 1 else [base[s % len(base)] for s in range(sets)], I32)


# ------------------------------------------------------------------------------------------------------------------------
# GPU plumbing
# ------------------------------------------------------------------------------------------------------------------------
def dev(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


class Buf:
    """(rows + TAIL, cols) elements of `dtype`, every 32-bit word SENTINEL; the entry point under test is handed its start."""

    def __init__(self, rows, cols, dtype, device):
        self.rows, self.cols, self.dtype = rows, cols, dtype
        self.wpe = torch.empty((), dtype=dtype).element_size() // 4
        self.raw = torch.full((rows + TAIL, cols * self.wpe), SENTINEL, dtype=torch.int32, device=device)

    @property
    def ptr(self):
        return self.raw.data_ptr()

    def put(self, a):
        """Input for an in-place call."""
        self.raw.fill_(SENTINEL)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(self.raw.device).reshape(self.rows, -1)
        self.raw[:self.rows, :t.shape[1] * self.wpe] = t.view(torch.int32)

    def np(self):
        return self.raw.view(self.dtype)[:self.rows].cpu().numpy()

    def clean_from(self, row):
        """Every word from row `row` on (the TAIL included) still holds the sentinel."""
        return bool((self.raw[row:] == SENTINEL).all())

    def untouched(self):
        return self.clean_from(0)


def twice(bufs, launch, scratch=()):
    """Launch, keep the bits, refill, launch again: the same bits in every buffer.  `scratch`: workspaces, refilled too but not
    compared (what a call leaves in them is not part of its contract: the fusion ranks through atomics, in any order)."""
    launch()
    first = [b.raw.clone() for b in bufs]
    for b in list(bufs) + list(scratch):
        b.raw.fill_(SENTINEL)
    launch()
    for b, f in zip(bufs, first):
        assert torch.equal(b.raw, f), 'two launches differ'


def refused(rc, bufs, what):
    msg = L.load().dz_last_error()
    assert rc != 0 and msg, what
    assert all(b.untouched() for b in bufs), what
    return msg.decode()


def host(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    return a, a.ctypes.data


# ------------------------------------------------------------------------------------------------------------------------
# GPU: fusion
# ------------------------------------------------------------------------------------------------------------------------
class WbfRun:
    def __init__(self, device, c):
        self.lib = L.load()
        f, t, m = c['boxes'].shape[:3]
        self.c, self.f, self.cand, self.per_model, self.n_models = c, f, t * m, m, t
        self.boxes, self.scores, self.labels = (dev(c[k].reshape((f, t * m) + c[k].shape[3:]), device) for k in ('boxes', 'scores', 'labels'))
        self.ids = None if c['ids'] is None else dev(c['ids'].reshape(f, t * m), device)
        self.w = None if c['weights'] is None else dev(np.asarray(c['weights'], F64), device)
        self.iou, self.p_iou = host(c['iou_thr'], F64)
        self.skip, self.p_skip = host(c['skip_thr'], F64)
        self.wsum = float(np.sum(c['weights'])) if c['weights'] is not None else float(t)
        self.ws_bytes = self.lib.dz_wbf_workspace_bytes(f, self.cand)
        assert self.ws_bytes % 8 == 0
        self.ws = Buf(self.ws_bytes // 8, 1, torch.float64, device)
        self.ob, self.os_ = Buf(f * self.cand, 7, torch.float64, device), Buf(f * self.cand, 1, torch.float64, device)
        self.ol, self.oi, self.oc = (Buf(n, 1, torch.int32, device) for n in (f * self.cand, f * self.cand, f))
        self.outs = [self.ob, self.os_, self.ol, self.oi, self.oc]

    def call(self, ws_bytes=None, ws_shift=0, out_ids=True):
        c = self.c
        return self.lib.dz_wbf_fuse_3d(L.ptr(self.boxes), L.ptr(self.scores), L.ptr(self.labels), L.ptr(self.ids), self.f, self.cand, self.per_model,
                                       L.ptr(self.w), self.n_models, self.p_iou, self.p_skip, self.wsum, int(c['conf_type'] == 'max'), int(c['overflow']),
                                       self.ob.ptr, self.os_.ptr, self.ol.ptr, self.oi.ptr if (self.ids is not None and out_ids) else None, self.oc.ptr,
                                       self.ws.ptr + ws_shift, self.ws_bytes if ws_bytes is None else ws_bytes, L.stream())


def check_fusion(device, name):
    c, want = wbf_case(name), wbf_expected(name)
    r = WbfRun(device, c)
    twice(r.outs, lambda: L.check(r.call(), 'dz_wbf_fuse_3d'), scratch=[r.ws])
    counts = r.oc.np()[:, 0]
    assert r.oc.clean_from(r.f) and r.ws.clean_from(r.ws.rows), 'written behind the counts / the workspace'
    worst_s = worst_b = 0.0
    for f in range(r.f):
        k = int(counts[f])
        assert k == len(want[f][1]), (name, f, k, len(want[f][1]))
        for buf in (r.ob, r.os_, r.ol, r.oi):
            w = buf.raw[:r.f * r.cand].reshape(r.f, r.cand, -1)
            assert bool((w[f, k if (buf is not r.oi or r.ids is not None) else 0:] == SENTINEL).all()), 'rows past out_count written'
        lo = f * r.cand
        np.testing.assert_array_equal(r.ol.np()[lo:lo + k, 0], want[f][2])
        if r.ids is not None:
            np.testing.assert_array_equal(r.oi.np()[lo:lo + k, 0], want[f][3])
        if k:
            worst_s = max(worst_s, float(np.abs(r.os_.np()[lo:lo + k, 0] - want[f][1]).max()))
            worst_b = max(worst_b, float(np.abs(r.ob.np()[lo:lo + k] - want[f][0]).max()))
    assert r.oi.clean_from(r.f * r.cand) and r.ob.clean_from(r.f * r.cand) and r.os_.clean_from(r.f * r.cand) and r.ol.clean_from(r.f * r.cand)
    print('  fusion %s: %s boxes, worst score difference %.1e (1e-7), worst box difference %.1e (1e-6)' % (case_id(name), counts.tolist(), worst_s, worst_b))
    assert worst_s <= 1e-7 and worst_b <= 1e-6, (name, worst_s, worst_b)


@pytest.mark.gpu
@pytest.mark.parametrize('n', WBF_COUNT_CASES)
def test_fusion_cluster_counts(device, n):
    check_fusion(device, n)


@pytest.mark.gpu
@pytest.mark.parametrize('k', WBF_MATCH_CASES)
def test_fusion_best_match_in_every_lane_group(device, k):
    check_fusion(device, ('match', k))


@pytest.mark.gpu
@pytest.mark.parametrize('c', WBF_TIE_CASES, ids=[case_id(c) for c in WBF_TIE_CASES])
def test_fusion_equal_ious_go_to_the_first_cluster(device, c):
    check_fusion(device, ('tie',) + c)


@pytest.mark.gpu
@pytest.mark.parametrize('c', WBF_RESCALE, ids=[case_id(c) for c in WBF_RESCALE])
def test_fusion_rescale_rules(device, c):
    check_fusion(device, ('rescale',) + c)


@pytest.mark.gpu
@pytest.mark.parametrize('name', WBF_OTHER_CASES)
def test_fusion_thresholds_gate_ids_and_batches(device, name):
    check_fusion(device, name)


@pytest.mark.gpu
def test_fusion_contracts(device):
    lib = L.load()
    r = WbfRun(device, wbf_case('ids_all'))
    assert lib.dz_wbf_workspace_bytes(r.f, r.cand) == r.ws_bytes
    refused(r.call(ws_bytes=r.ws_bytes - 1), r.outs + [r.ws], 'a workspace one byte short')
    refused(r.call(ws_shift=4), r.outs + [r.ws], 'a workspace pointer off by 4')
    refused(r.call(out_ids=False), r.outs + [r.ws], 'obj_ids without out_obj_ids')
    r.per_model = 1                                                     # models x per_model < cand
    refused(r.call(), r.outs + [r.ws], 'fewer model slots than candidates')
    check_fusion(device, 'ids_all')                                     # (and nothing of the above broke the next call)


# ------------------------------------------------------------------------------------------------------------------------
# GPU: TTA
# ------------------------------------------------------------------------------------------------------------------------
def run_augment(device, p, ops, expect_refusal=False):
    lib = L.load()
    n, c = p.shape
    kinds, pk = host([k for k, a in ops], I32)
    params, pp = host([a for k, a in ops], F32)
    d_p = dev(p, device) if n else None
    out = Buf(max(len(ops), 1) * n, c, torch.float32, device)
    if expect_refusal:
        return refused(lib.dz_tta_augment_points(L.ptr(d_p), n, c, pk, pp, len(ops), out.ptr, L.stream()), [out], 'augment')
    twice([out], lambda: L.check(lib.dz_tta_augment_points(L.ptr(d_p), n, c, pk, pp, len(ops), out.ptr, L.stream()), 'dz_tta_augment_points'))
    assert out.clean_from(out.rows)
    return out.np().reshape(len(ops), n, c)


@pytest.mark.gpu
@pytest.mark.parametrize('n, c', POINT_CASES, ids=[case_id(c) for c in POINT_CASES])
def test_augment_points_all_operations(device, n, c):
    p = tta_points(n, c, seed=n + c)
    want, rot = augment_expected(p, TTA_ALL)
    check_rotated(run_augment(device, p, TTA_ALL), want, rot, TTA_ALL, 0, 'augment %d x %d' % (n, c))


@pytest.mark.gpu
def test_augment_points_each_operation_alone_and_32(device):
    p = tta_points(257, 5, seed=9)
    for ops in TTA_ALONE + [[TTA_ALL[(3 * i) % len(TTA_ALL)] for i in range(32)]]:
        want, rot = augment_expected(p, ops)
        check_rotated(run_augment(device, p, ops), want, rot, ops, 0, 'augment, %d operation(s) from %s' % (len(ops), op_name(*ops[0])))
    for bad in ([], [TTA_ALL[i % len(TTA_ALL)] for i in range(33)], [(6, 0.0)], [(K_FX, 0.0), (-1, 0.0)]):
        run_augment(device, p, bad, expect_refusal=True)


def run_restore(device, b, ops, dim, expect_refusal=False, frames=None, m=None):
    lib = L.load()
    f0, t, m0 = b.shape[:3]
    frames, m = f0 if frames is None else frames, m0 if m is None else m
    full = np.full((f0, t, m0, dim), SENT_F, F32)
    full[..., :7] = b
    kinds, pk = host([k for k, a in ops], I32)
    params, pp = host([a for k, a in ops], F32)
    buf = Buf(f0 * t * m0, dim, torch.float32, device)
    first = []

    def launch():
        buf.put(bits(full).reshape(-1, dim))
        rc = lib.dz_tta_restore_boxes(buf.ptr, frames, len(ops), m, dim, pk, pp, L.stream())
        first.append(rc)
        if not expect_refusal:
            L.check(rc, 'dz_tta_restore_boxes')
    if expect_refusal:
        launch()
        assert first[0] != 0 and lib.dz_last_error()
    else:
        launch()
        a = buf.raw.clone()
        launch()
        assert torch.equal(a, buf.raw), 'two launches differ'
    assert buf.clean_from(buf.rows)
    got = buf.np().reshape(f0, t, m0, dim)
    np.testing.assert_array_equal(bits(got[..., 7:]), bits(full[..., 7:]), err_msg='columns behind the box written')
    return got[..., :7]


@pytest.mark.gpu
@pytest.mark.parametrize('ci', range(len(RESTORE_CASES)), ids=[case_id(c) for c in RESTORE_CASES])
def test_restore_boxes(device, ci):
    frames, m, dim, key = RESTORE_CASES[ci]
    ops = RESTORE_SETS[key]
    b = tta_boxes(frames, 5, m, seed=ci)
    want, rot = restore_expected(b, ops)
    check_rotated(run_restore(device, b, ops, dim), want, rot, ops, 1, 'restore %s' % case_id(RESTORE_CASES[ci]))


@pytest.mark.gpu
def test_restore_boxes_empty_and_refused(device):
    b = tta_boxes(2, 5, 3, seed=77)
    ops = RESTORE_SETS['a']
    for kw in ({'m': 0}, {'frames': 0}):                                # returns cleanly, writes nothing
        np.testing.assert_array_equal(bits(run_restore(device, b, ops, 9, **kw)), bits(b))
    b1 = tta_boxes(1, 1, 3, seed=78)
    one = [(K_FXY, 0.0)]
    np.testing.assert_array_equal(bits(run_restore(device, b1, one, 7)), bits(W.restore_boxes(b1[0], [op_name(*one[0])])[None]))
    ops32 = [TTA_ALL[(5 * i) % len(TTA_ALL)] for i in range(32)]
    b32 = tta_boxes(1, 32, 2, seed=79)
    want, rot = restore_expected(b32, ops32)
    check_rotated(run_restore(device, b32, ops32, 7), want, rot, ops32, 1, 'restore, 32 operations')
    for bad in ([], [TTA_ALL[i % len(TTA_ALL)] for i in range(33)], [(6, 0.0)]):
        bb = tta_boxes(1, max(len(bad), 1), 2, seed=80)
        np.testing.assert_array_equal(bits(run_restore(device, bb, bad, 7, expect_refusal=True)), bits(bb))


# ------------------------------------------------------------------------------------------------------------------------
# GPU: sweep merge
# ------------------------------------------------------------------------------------------------------------------------
class MergeRun:
    def __init__(self, device, d, n_sweeps=None, offsets=None):
        self.lib = L.load()
        self.n = d['raw'].shape[0]
        self.raw = dev(d['raw'], device) if self.n else None
        self.off, self.p_off = host(d['offsets'] if offsets is None else offsets, I32)
        self.n_sweeps = len(d['offsets']) - 1 if n_sweeps is None else n_sweeps
        mats, dts = np.zeros((max(self.n_sweeps, 16), 3, 4)), np.zeros(max(self.n_sweeps, 16))
        mats[:len(d['mats'])], dts[:len(d['dts'])] = d['mats'], d['dts']
        self.mats, self.p_mats = host(mats, F64)
        self.dts, self.p_dts = host(dts, F64)
        self.ws_bytes = self.lib.dz_merge_sweeps_workspace_bytes(self.n)
        assert self.ws_bytes % 4 == 0
        self.ws = Buf(self.ws_bytes // 4, 1, torch.int32, device)
        self.out, self.cnt = Buf(self.n, 6, torch.float32, device), Buf(1, 1, torch.int32, device)
        self.bufs = [self.out, self.cnt, self.ws]

    def call(self, ws_bytes=None):
        return self.lib.dz_merge_sweeps(L.ptr(self.raw), self.n, self.p_off, self.p_mats, self.p_dts, self.n_sweeps, self.out.ptr, self.cnt.ptr,
                                        self.ws.ptr, self.ws_bytes if ws_bytes is None else ws_bytes, L.stream())


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(MERGE_CASES)), ids=[case_id(c) for c in MERGE_CASES])
def test_merge_sweeps(device, i):
    d = merge_case(i)
    r = MergeRun(device, d)
    twice([r.out, r.cnt], lambda: L.check(r.call(), 'dz_merge_sweeps'), scratch=[r.ws])
    k = int(r.cnt.np()[0, 0])
    assert k == d['want'].shape[0], (k, d['want'].shape[0])
    assert r.out.clean_from(k) and r.cnt.clean_from(1) and r.ws.clean_from(r.ws.rows), 'rows past the count / behind the workspace written'
    check_merged(r.out.np()[:k], d, 'merge %s' % case_id(MERGE_CASES[i]))


@pytest.mark.gpu
def test_merge_sweeps_refusals(device):
    d = merge_case(9)                                                   # 8191 rows, five sweeps
    r = MergeRun(device, d)
    refused(r.call(ws_bytes=r.ws_bytes - 1), r.bufs, 'a workspace one byte short')
    off = d['offsets'].copy()
    off[2], off[3] = off[3], off[2]
    assert off[2] > off[3]
    short = d['offsets'].copy()
    short[-1] -= 1
    off17 = np.linspace(0, d['raw'].shape[0], 18).astype(I32)
    for what, kw in (('decreasing offsets', {'offsets': off}), ('offsets that do not end at n_total', {'offsets': short}),
                     ('17 sweeps', {'n_sweeps': 17, 'offsets': off17}), ('no sweep', {'n_sweeps': 0, 'offsets': off17})):
        bad = MergeRun(device, d, **kw)
        refused(bad.call(), bad.bufs, what)
    r16 = MergeRun(device, merge_case(5))                               # 16 sweeps are accepted (test_merge_sweeps runs them)
    assert r16.n_sweeps == 16


# ------------------------------------------------------------------------------------------------------------------------
# GPU: crop
# ------------------------------------------------------------------------------------------------------------------------
def run_crop(device, pts, boxes, payload, cap):
    lib = L.load()
    m, t, words = pts.shape[0], boxes.shape[0], payload.shape[1]
    d_p, d_b, d_w = dev(pts, device), dev(boxes, device), dev(payload, device)
    ws_bytes = lib.dz_crop_points_workspace_bytes(m, t, cap)
    assert ws_bytes % 4 == 0
    ws = Buf(ws_bytes // 4, 1, torch.int32, device)
    out, idx, off, tot = Buf(cap, words, torch.int32, device), Buf(cap, 1, torch.int32, device), Buf(t + 1, 1, torch.int32, device), Buf(1, 1, torch.int32, device)
    bufs = [out, idx, off, tot, ws]
    refused(lib.dz_crop_points_in_boxes(L.ptr(d_p), m, L.ptr(d_b), t, L.ptr(d_w), words, out.ptr, idx.ptr, off.ptr, tot.ptr, cap, ws.ptr, ws_bytes - 1,
                                        L.stream()), bufs, 'a workspace one byte short')
    twice(bufs[:4], lambda: L.check(lib.dz_crop_points_in_boxes(L.ptr(d_p), m, L.ptr(d_b), t, L.ptr(d_w), words, out.ptr, idx.ptr, off.ptr, tot.ptr, cap,
                                                                ws.ptr, ws_bytes, L.stream()), 'dz_crop_points_in_boxes'), scratch=[ws])
    assert all(b.clean_from(b.rows) for b in bufs), 'written behind a buffer'
    return out, idx, off.np()[:, 0], int(tot.np()[0, 0])


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(CROP_CASES)), ids=[case_id(c) for c in CROP_CASES])
def test_crop_points_in_boxes(device, i):
    d = crop_case(i)
    cap, total = d['cap'], d['total']
    out, idx, offsets, d_total = run_crop(device, d['pts'], d['boxes'], d['payload'], cap)
    assert d_total == total                                             # the full count, whatever the capacity
    np.testing.assert_array_equal(offsets, d['offsets'])                # complete, whatever the capacity
    k = min(cap, total)
    np.testing.assert_array_equal(out.np()[:k], d['rows'][:k])
    np.testing.assert_array_equal(idx.np()[:k, 0], d['index'][:k])
    assert out.clean_from(k) and idx.clean_from(k)
    lib = L.load()
    t, m = d['boxes'].shape[0], d['pts'].shape[0]
    counts = Buf(t, 1, torch.int32, device)
    d_b, d_p = dev(d['boxes'], device), dev(d['pts'], device)
    twice([counts], lambda: L.check(lib.dz_points_in_boxes_count(L.ptr(d_b), L.ptr(d_p), t, m, counts.ptr, L.stream()), 'dz_points_in_boxes_count'))
    assert counts.clean_from(t)
    np.testing.assert_array_equal(counts.np()[:, 0], np.diff(d['offsets']))
    print('  crop %s: %d rows of %d written, counts agree' % (case_id(CROP_CASES[i]), k, total))


@pytest.mark.gpu
def test_crop_offsets_with_more_boxes_than_gather_threads(device):
    """t = 524288 = 2048 workgroups x 256 threads, the cap of the gather's grid: offsets[t] was never written (and read as 0 from the
    wrapper's zero-filled tensor) before the gather wrote the offsets in a grid-stride loop."""
    t = 524288
    boxes = np.tile(np.array([0, 0, 0, 2, 2, 2, 0], F32), (t, 1))
    pts = np.zeros((1, 3), F32)
    payload = np.array([[12345]], I32)
    out, idx, offsets, d_total = run_crop(device, pts, boxes, payload, 1)
    assert d_total == t and offsets[t] == t
    np.testing.assert_array_equal(offsets, np.arange(t + 1, dtype=I32))
    assert out.np()[0, 0] == 12345 and idx.np()[0, 0] == 0 and out.clean_from(1) and idx.clean_from(1)


# ------------------------------------------------------------------------------------------------------------------------
# GPU: object features
# ------------------------------------------------------------------------------------------------------------------------
def run_prm(device, tracks, encoding, box_max, q_n, m_n, seed, crm=False):
    """dz_prm_encode_points on sentinel buffers -> dict of numpy results shaped like oracle.object_features.prm_batch."""
    lib = L.load()
    packed = OF.PackedTracks(tracks, device)
    b = packed.batch
    q_idx, m_idx = OF.prm_selection(packed, q_n, max(m_n, 1), random.Random(seed))
    if crm:
        q_idx = OF.crm_selection(packed, q_n, random.Random(seed))
    d_q, d_m = dev(q_idx, device), None if crm else dev(m_idx, device)
    codes, p_codes = host([OF.PRM_CODES[e] for e in encoding], I32)
    ch = lib.dz_prm_feature_channels(p_codes, len(codes))
    mm = 0 if crm else m_n
    query, memory = Buf(b * box_max * q_n, ch, torch.float32, device), Buf(b * box_max * mm, ch, torch.float32, device)
    traj, mask = Buf(b * box_max, 7, torch.float32, device), Buf(b * box_max, 1, torch.float32, device)
    init, scratch = Buf(b, 7, torch.float64, device), Buf(b * box_max * 27 + 2 * b, 1, torch.float64, device)
    bufs = [query, memory, traj, mask, init, scratch]
    twice(bufs[:5], scratch=[scratch], launch=lambda: L.check(lib.dz_prm_encode_points(
        L.ptr(packed.pts), L.ptr(packed.box_offsets), L.ptr(packed.traj), L.ptr(packed.score), L.ptr(packed.obj_box_offsets),
        None if crm else L.ptr(packed.obj_cls), L.ptr(d_q), L.ptr(d_m), q_n, mm, b, box_max, p_codes, len(codes), query.ptr, None if crm else memory.ptr,
        traj.ptr, mask.ptr, init.ptr, scratch.ptr, L.stream()), 'dz_prm_encode_points'))
    assert all(x.clean_from(x.rows) for x in bufs), 'written behind a buffer'
    return {'pos_query_points': query.np().reshape(b, box_max, q_n, ch), 'pos_memory_points': memory.np().reshape(b, box_max, mm, ch),
            'pos_trajectory': traj.np().reshape(b, box_max, 7), 'padding_mask': mask.np().reshape(b, box_max), 'pos_init_box': init.np()}


def check_prm(got, ref, what, memory=True):
    close(got['pos_init_box'], ref['pos_init_box'], 1e-9, 1e-12, what + ' initial box')
    np.testing.assert_array_equal(got['padding_mask'], ref['padding_mask'])
    close(got['pos_trajectory'], ref['pos_trajectory'], 1e-5, 2e-6, what + ' trajectory')
    close(got['pos_query_points'], ref['pos_query_points'], 3e-5, 2e-6, what + ' query points')
    if memory:
        close(got['pos_memory_points'], ref['pos_memory_points'], 3e-5, 2e-6, what + ' memory points')
    pad = ref['padding_mask'] == 1
    assert pad.any() and not got['pos_query_points'][pad].any() and not got['pos_trajectory'][pad].any()      # padding slots: exactly 0


@pytest.mark.gpu
@pytest.mark.parametrize('q_n, m_n', PRM_SIZES, ids=[case_id(c) for c in PRM_SIZES])
@pytest.mark.parametrize('e', range(len(PRM_ENCODINGS)), ids=['ch%d' % c for c in PRM_CHANNELS])
def test_prm_encode_points(device, e, q_n, m_n):
    tracks, enc = feature_tracks(q_n), PRM_ENCODINGS[e]
    got = run_prm(device, tracks, enc, 7, q_n, m_n, seed=e)
    assert got['pos_query_points'].shape[-1] == PRM_CHANNELS[e]
    check_prm(got, prm_expected(tracks, enc, 7, q_n, m_n, seed=e), 'PRM %s %d/%d' % ('+'.join(enc), q_n, m_n))
    if 'class' in enc:                                                   # one-hot per object: classes 1, 2, 3, none for the unknown 0, 3
        cls = got['pos_query_points'][:, 0, 0, 0:3]                      # (rows without a point carry it too: object 2 has no point at all)
        assert cls.tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0], [0, 0, 1]]


@pytest.mark.gpu
@pytest.mark.parametrize('e', [5, 6], ids=['ch32-float4', 'ch35-scalar'])
def test_prm_encode_points_more_slots_than_workgroups(device, e):
    tracks, enc = grid_tracks(), PRM_ENCODINGS[e]
    got = run_prm(device, tracks, enc, 200, 5, 3, seed=50 + e)
    check_prm(got, prm_expected(tracks, enc, 200, 5, 3, seed=50 + e), 'PRM 42 x 200 slots, %d channels' % PRM_CHANNELS[e])


@pytest.mark.gpu
def test_crm_call_of_the_prm_encoder(device):
    """The confidence model's input: the query half alone (m_n = 0, no memory pointers, no classes)."""
    tracks, enc = feature_tracks(8), ('xyz', 'intensity', 'p2co', 'score')
    got = run_prm(device, tracks, enc, 7, 8, 0, seed=3, crm=True)
    rng = random.Random(3)
    ref = OO.crm_batch([OO.crm_object(t, enc, 7, 8, rng) for t in tracks])
    close(got['pos_query_points'], ref['conf_points'], 3e-5, 2e-6, 'CRM points')


@pytest.mark.gpu
def test_prm_refuses_more_channels_than_its_tables_hold(device):
    """('xyz', 'p2co', 'p2co') = 57 channels: refused before anything is launched, nothing written.  (Never launched: it would write
    past the kernel's 40-entry channel tables.)"""
    lib = L.load()
    packed = OF.PackedTracks(feature_tracks(5), device)
    b = packed.batch
    q_idx, m_idx = OF.prm_selection(packed, 5, 3, random.Random(0))
    d_q, d_m = dev(q_idx, device), dev(m_idx, device)
    bufs = [Buf(b * 7 * 5, 64, torch.float32, device), Buf(b * 7 * 3, 64, torch.float32, device), Buf(b * 7, 7, torch.float32, device),
            Buf(b * 7, 1, torch.float32, device), Buf(b, 7, torch.float64, device), Buf(b * 7 * 27 + 2 * b, 1, torch.float64, device)]
    for enc in (('xyz', 'p2co', 'p2co'), ('p2co', 'class', 'xyz', 'intensity', 'score', 'score', 'xyz', 'xyz')):        # 57 and 42 channels
        codes, p_codes = host([OF.PRM_CODES[e] for e in enc], I32)
        rc = lib.dz_prm_encode_points(L.ptr(packed.pts), L.ptr(packed.box_offsets), L.ptr(packed.traj), L.ptr(packed.score), L.ptr(packed.obj_box_offsets),
                                      L.ptr(packed.obj_cls), L.ptr(d_q), L.ptr(d_m), 5, 3, b, 7, p_codes, len(codes), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr,
                                      bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, L.stream())
        assert 'channels' in refused(rc, bufs, enc)


@pytest.mark.gpu
@pytest.mark.parametrize('q_n, mem_n', PRM_SIZES, ids=[case_id(c) for c in PRM_SIZES])
def test_grm_encode_points_every_flag_subset(device, q_n, mem_n):
    lib = L.load()
    tracks = feature_tracks(q_n)
    packed = OF.PackedTracks(tracks, device)
    b = packed.batch
    for si, enc in enumerate(GRM_SUBSETS):
        mem_idx, query_box, query_idx, qnum, orders = OF.grm_selection(packed, 3, q_n, mem_n, random.Random(si))
        rng = random.Random(si)
        ref = OO.grm_batch([OO.grm_object(t, enc, 3, q_n, mem_n, rng) for t in tracks])
        assert query_box.shape[1] == 3 and (query_box[0, 1:] == -1).all()               # the one-box object: two query slots of -1
        hole = int(np.nonzero(mem_idx[1] >= 0)[0][1])                                   # a memory index of -1 between valid ones
        assert mem_idx[1, hole - 1] >= 0 and mem_idx[1, hole + 1] >= 0
        mem_idx[1, hole] = -1
        ref['geo_memory_points'][1, hole] = 0
        flags = sum(OF.GRM_FLAGS[e] for e in enc)
        cm = lib.dz_grm_feature_channels(flags)
        assert cm == ref['geo_memory_points'].shape[2]
        d_mem, d_qb, d_qi = dev(mem_idx, device), dev(query_box, device), dev(query_idx, device)
        memory, query = Buf(b * mem_n, cm, torch.float32, device), Buf(b * 3 * q_n, 4, torch.float32, device)
        twice([memory, query], lambda: L.check(lib.dz_grm_encode_points(
            L.ptr(packed.pts), L.ptr(packed.box_offsets), L.ptr(packed.traj), L.ptr(packed.score), L.ptr(packed.obj_box_offsets), L.ptr(d_mem), mem_n,
            L.ptr(d_qb), L.ptr(d_qi), 3, q_n, b, flags, memory.ptr, query.ptr, L.stream()), 'dz_grm_encode_points'))
        assert memory.clean_from(memory.rows) and query.clean_from(query.rows)
        close(memory.np().reshape(b, mem_n, cm), ref['geo_memory_points'], 2e-6, 2e-6, 'GRM memory %s' % '+'.join(enc))
        close(query.np().reshape(b, 3, q_n, 4), ref['geo_query_points'], 2e-6, 2e-6, 'GRM query %s' % '+'.join(enc))
        assert not query.np().reshape(b, 3, q_n, 4)[0, 1:].any() and not memory.np().reshape(b, mem_n, cm)[1, hole].any()
    memory, query = Buf(b * mem_n, 11, torch.float32, device), Buf(b * 3 * q_n, 4, torch.float32, device)
    for bad in (0, 16):
        refused(lib.dz_grm_encode_points(L.ptr(packed.pts), L.ptr(packed.box_offsets), L.ptr(packed.traj), L.ptr(packed.score), L.ptr(packed.obj_box_offsets),
                                         L.ptr(d_mem), mem_n, L.ptr(d_qb), L.ptr(d_qi), 3, q_n, b, bad, memory.ptr, query.ptr, L.stream()), [memory, query],
                'encoding flags %d' % bad)


@pytest.mark.gpu
@pytest.mark.parametrize('sets, k, set0', DRAW_CASES, ids=[case_id(c) for c in DRAW_CASES])
def test_draw_subsets(device, sets, k, set0):
    lib = L.load()
    counts = draw_counts(sets, k)
    seed = 0x1234567890ABCDEF + sets
    d_c = dev(counts, device)
    out = Buf(sets, k, torch.int32, device)
    twice([out], lambda: L.check(lib.dz_draw_subsets(L.ptr(d_c), sets, k, seed, set0, out.ptr, L.stream()), 'dz_draw_subsets'))
    assert out.clean_from(sets)
    got = out.np()
    for s in range(sets):
        want = OO.device_draw_subset(int(counts[s]), k, seed, set0 + s)
        np.testing.assert_array_equal(got[s, :len(want)], want, err_msg='set %d of %d rows' % (s, counts[s]))
        assert (got[s, len(want):] == -1).all() and len(want) == min(int(counts[s]), k)
    out.raw.fill_(SENTINEL)
    refused(lib.dz_draw_subsets(L.ptr(d_c), sets, 0, seed, set0, out.ptr, L.stream()), [out], 'k = 0')
