"""The head post stage (csrc/head_post.hip: radix top-K decode, rotated NMS, packing) at its edges.

Decode (`dz_centerhead_decode`): an eight-launch radix select (digit levels of 11 + 11 + 10 bits, a per-frame state block, a
4096-entry tie list and a second tie path when the list overflows or more keys equal the threshold than are needed), a 1024-wide
bitonic sort and an ordered compaction.  The reference here is float64: score = sigmoid(hm) * clamp(iou, 0, 1)^2, global top-K
over class-major flat indices (score descending, ties by ascending flat index), box decode as oracle/dense.py:decode.

  * exact cases: `hm` / `iou` logits come from small finite sets, so every tie is bit-exact by construction and two distinct
    score levels are more than 1e-5 apart (relative) - float32 sigmoid error is a few ulp (1e-7), so the device's order of the
    levels is certain and counts, labels and flat pixel indices must equal the reference exactly and in order.  The pixel of a
    candidate is recovered from its `center_z`, which every input marks with the pixel index.
  * continuous cases: random float32 logits; selection and order are judged with a band of 16 float32 ulp around the float64
    K-th score (derivation at `EPS_ULPS`).

Rotated NMS (`dz_nms_rotated_batched`): ragged batches against single-frame calls bit for bit, every frame against
oracle/cref.py under the on-threshold rule of tests/util.py:nms_on_threshold_rule, the post_max cut, the n_cap limit.
Packing (`dz_pack_detections`): against a numpy gather, exactly, into a sentinel-filled buffer.

CPU-only checks of the references and of the input builders run under `-m "not gpu"`; device tests carry `@pytest.mark.gpu`.
Each device test prints the figures it measured (worst differences, on-threshold decisions).
"""
import math
import os
import types

import numpy as np
import pytest
import torch

from detzero_amd.synth import POINT_CLOUD_RANGE, VOXEL_SIZE_01, VOXEL_SIZE_02, synth_boxes
from tests.util import nms_on_threshold_rule

gpu = pytest.mark.gpu

SCORE_THRESH = 0.03
LIMIT = [-80, -80, -10.0, 80, 80, 10.0]                    # POST_CENTER_LIMIT_RANGE
STRIDE = 8
VOXEL = VOXEL_SIZE_01                                      # 0.8 m per head pixel: a 188 x 188 map spans the point-cloud range
TIE_CAP = 4096                                             # head_post.hip
SENT = 0x7FBADBAD                                          # a NaN as fp32, never a plausible label / count / index
SCORE_TOL, BOX_TOL = 1e-6, 1e-4                            # the tolerances of test_decode_topk_matches_reference_golden

# Continuous maps: the device evaluates s = 1 / (1 + expf(-x)) * (c * c) with c = clamp(iou) in float32.  Five rounded
# operations (negation is exact; the add, the divide, c * c, the product with it, and the conversion of the float64 reference's
# logit path count one half ulp each: 2.5 ulp) plus an expf of 1-2 ulp that passes through 1 / (1 + e) with a gain below 1, i.e.
# under 5 ulp in all; 16 ulp of the K-th score leaves a factor of three.
EPS_ULPS = 16
BAND_MAX = 4                                               # candidates allowed inside the band, per frame (asserted on the inputs)


# ------------------------------------------------------------------------------------------------------------------------
# float64 / integer references
# ------------------------------------------------------------------------------------------------------------------------
def z_marks(hw):
    """center_z value of pixel p: strictly increasing float32 inside the z limits, so the pixel is recoverable from a box."""
    zm = (-9.0 + 18.0 * np.arange(hw, dtype=np.float64) / hw).astype(np.float32)
    assert hw == 1 or np.all(np.diff(zm) > 0)
    return zm


def pix_from_z(z, hw):
    zm = z_marks(hw)
    idx = np.clip(np.searchsorted(zm, z), 0, hw - 1)
    assert np.array_equal(zm[idx], z), 'a box carries a center_z that marks no pixel'
    return idx.astype(np.int64)


def scores64(head, ncls, use_iou):
    """head (hw, 12) float32 -> float64 scores, class-major flat (ncls * hw)."""
    hm = head[:, 9:9 + ncls].astype(np.float64).T
    s = 1.0 / (1.0 + np.exp(-hm))
    if use_iou:
        s = s * np.clip(head[:, 8].astype(np.float64), 0.0, 1.0)[None, :] ** 2
    return np.ascontiguousarray(s).reshape(-1)


def decode_ref(head, h, w, ncls, k, use_iou, thresh=SCORE_THRESH, limit=LIMIT, pc_range=POINT_CLOUD_RANGE, voxel=VOXEL,
               stride=STRIDE):
    """Float64 decode of one frame.  sel_*: the top-K before the masks; flat / scores / boxes / labels: what leaves."""
    hw = h * w
    s = scores64(head, ncls, use_iou)
    kk = min(k, s.size)
    order = np.lexsort((np.arange(s.size), -s))[:kk]
    sc = s[order]
    lab, pix = order // hw, order % hw
    row = head[pix].astype(np.float64)
    xs = (pix % w) + row[:, 0]
    ys = (pix // w) + row[:, 1]
    box = np.stack([xs * stride * float(voxel[0]) + float(pc_range[0]), ys * stride * float(voxel[1]) + float(pc_range[1]), row[:, 2],
                    np.exp(row[:, 3]), np.exp(row[:, 4]), np.exp(row[:, 5]), np.arctan2(row[:, 7], row[:, 6])], axis=1)
    lim = np.asarray(limit, np.float64)
    ok = (box[:, :3] >= lim[:3]).all(1) & (box[:, :3] <= lim[3:]).all(1) & (sc > thresh)
    return types.SimpleNamespace(all_scores=s, order=order, sel_scores=sc, sel_boxes=box, ok=ok, s_k=float(sc[-1]), hw=hw, k=k,
                                 count=int(ok.sum()), flat=order[ok], scores=sc[ok], boxes=box[ok], labels=lab[ok], pix=pix[ok])


def assert_exact_inputs(ref, thresh=SCORE_THRESH, limit=LIMIT):
    """What an exact case's input must satisfy, on the float64 reference alone, before any device call."""
    u = np.unique(ref.all_scores)
    if u.size > 1:
        assert np.all(np.diff(u) > 1e-5 * u[1:]), 'two distinct score levels are within 1e-5 (relative)'
    lim = np.asarray(limit, np.float64)
    for a in range(3):
        d = np.minimum(np.abs(ref.sel_boxes[:, a] - lim[a]), np.abs(ref.sel_boxes[:, a] - lim[a + 3]))
        assert d.size == 0 or d.min() > 1e-3, 'a selected candidate sits on a limit of POST_CENTER_LIMIT_RANGE'
    assert np.all(np.abs(ref.sel_scores - thresh) > 1e-5), 'a selected score sits on score_thresh'


def compare_exact(got, ref):
    """got: dict(count, boxes (K,7), scores (K,), labels (K,)) of one frame.  Counts, labels and flat pixel indices exactly and
    in order, scores within 1e-6, boxes within 1e-4.  Returns (worst score difference, worst box difference)."""
    assert got['count'] == ref.count, 'count %d, reference %d' % (got['count'], ref.count)
    c = ref.count
    if c == 0:
        return 0.0, 0.0
    lab = got['labels'][:c].astype(np.int64)
    pix = pix_from_z(got['boxes'][:c, 2], ref.hw)
    flat = lab * ref.hw + pix
    assert sorted(flat.tolist()) == sorted(ref.flat.tolist()), 'selected set differs from the reference: %d candidates missing' % (
        np.setdiff1d(ref.flat, flat).size)
    assert np.array_equal(flat, ref.flat), 'selected set is right, its order is not (first difference at %d)' % int(
        np.nonzero(flat != ref.flat)[0][0])
    assert np.array_equal(lab, ref.labels)
    ds = np.abs(got['scores'][:c].astype(np.float64) - ref.scores)
    db = np.abs(got['boxes'][:c].astype(np.float64) - ref.boxes)
    assert ds.max() <= SCORE_TOL, ds.max()
    assert db.max() <= BOX_TOL, db.max()
    return float(ds.max()), float(db.max())


def pack_ref(boxes, scores, labels, keep, d_nk, post_max):
    """numpy gather: (B,K,7), (B,K), (B,K) i32, keep (B,K) i32, d_nk (B,) -> (B, post_max, 9) [box | score | label + 1]."""
    b, k = boxes.shape[0], boxes.shape[1]
    out = np.zeros((b, post_max, 9), np.float32)
    for i in range(b):
        m = min(int(d_nk[i]), post_max, k)
        sel = keep[i, :m].astype(np.int64)
        out[i, :m, :7] = boxes[i, sel]
        out[i, :m, 7] = scores[i, sel]
        out[i, :m, 8] = (labels[i, sel] + 1).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# input builders: head maps
# ------------------------------------------------------------------------------------------------------------------------
HI = np.array([3.0, 2.5, 2.0, 1.5], np.float32)            # hm logits of the keys above the tie level
TIE_HM = np.float32(1.0)
LO = np.array([0.0, -1.0, -2.0, -3.0], np.float32)         # ... and below it (sigmoid(-3) * 0.81 = 0.038 > score_thresh)
IOU_ONE, IOU_PART = np.float32(1.5), np.float32(0.9)       # clamp -> weights 1 and 0.81; tied keys sit on IOU_PART pixels


def build_head(h, w, hm, iou, seed, z_shift=0.0):
    """hm (ncls, hw) and iou (hw,) float32 logits -> head (hw, 12): centre offsets in [0.1, 0.9] (so no decoded x / y comes
    near a limit), center_z marking the pixel, dim logits in [-2, 3], headings away from +-pi; the heat-map columns of the
    classes a head does not have hold a large logit, which must never be read."""
    ncls, hw = hm.shape
    assert hw == h * w and iou.shape == (hw,)
    rng = np.random.default_rng(seed)
    head = np.zeros((hw, 12), np.float32)
    head[:, 0:2] = rng.uniform(0.1, 0.9, (hw, 2))
    head[:, 2] = z_marks(hw) + np.float32(z_shift)
    head[:, 3:6] = rng.uniform(-2.0, 3.0, (hw, 3))
    ang, r = rng.uniform(-math.pi + 0.1, math.pi - 0.1, hw), rng.uniform(0.5, 2.0, hw)
    head[:, 6], head[:, 7] = r * np.cos(ang), r * np.sin(ang)
    head[:, 8] = iou
    head[:, 9:] = 30.0
    head[:, 9:9 + ncls] = hm.T
    return head


def tie_map(h, w, ncls, n_hi, m, where, seed, use_iou=True, z_shift=0.0):
    """n_hi keys above the tie level (themselves tied among a few levels), m keys exactly ON it, every other key below.
    where: 'any' (tied keys anywhere), 'last_class', 'highest' (the m highest flat indices)."""
    hw, n = h * w, ncls * h * w
    assert n_hi + m <= n
    rng = np.random.default_rng(seed)
    if where == 'any':
        tie = rng.choice(n, m, replace=False)
    elif where == 'last_class':
        tie = (ncls - 1) * hw + rng.choice(hw, m, replace=False)
    else:
        tie = np.arange(n - m, n)
    hm = rng.choice(LO, n)
    hm[tie] = TIE_HM
    rest = np.setdiff1d(np.arange(n), tie)
    hm[rng.choice(rest, n_hi, replace=False)] = rng.choice(HI, n_hi)
    if use_iou:
        iou = rng.choice(np.array([IOU_ONE, IOU_PART]), hw)
        iou[tie % hw] = IOU_PART
    else:
        iou = rng.choice(np.array([-1.0, 0.3, 2.0], np.float32), hw)                   # must be ignored
    return build_head(h, w, hm.reshape(ncls, hw), iou.astype(np.float32), seed + 1, z_shift)


def const_map(h, w, ncls, hm_logit, iou_logits, seed):
    hw = h * w
    rng = np.random.default_rng(seed)
    hm = np.full((ncls, hw), hm_logit, np.float32) if np.isscalar(hm_logit) else rng.choice(np.asarray(hm_logit, np.float32), (ncls, hw))
    iou = rng.choice(np.asarray(iou_logits, np.float32), hw)
    return build_head(h, w, hm, iou, seed + 1)


def sigmoid32(x):
    one = np.float32(1.0)
    return one / (one + np.exp(-np.float32(x), dtype=np.float32))


def logit_of_bits(bits):
    s = float(np.array([bits], np.uint32).view(np.float32)[0])
    return np.float32(math.log(s / (1.0 - s)))


# level -> (bits of the upper score, bits of the lower score, lowest / highest bit of the digit).  The bits below the digit sit
# mid-range (level 2: 32 ulp inside the digit's ends), so the few ulp by which a float32 sigmoid misses the target carry nowhere.
DIGITS = {0: (0x3F480200, 0x3F280200, 21, 31), 1: (0x3F2A0200, 0x3F29E200, 10, 20), 2: (0x3F2A03E0, 0x3F2A0020, 0, 9)}


def digit_logits(level):
    a, b, lo, hi = DIGITS[level]
    assert (a ^ b).bit_length() - 1 <= hi and ((a ^ b) & ((1 << lo) - 1)) == 0, 'the targets differ outside the digit'
    return logit_of_bits(a), logit_of_bits(b)


def digit_map(level, kth, seed=5):
    """use_iou off, 100 x 100 x 2: 120 keys well above, 150 on the upper level, 160 on the lower one, the rest well below.
    kth 'upper': K ends on the last upper key; 'lower': K ends inside the lower level (its keys tie)."""
    h, w, ncls, n_hi, n_a, n_b = 100, 100, 2, 120, 150, 160
    xa, xb = digit_logits(level)
    n = ncls * h * w
    rng = np.random.default_rng(seed + level)
    pos = rng.choice(n, n_hi + n_a + n_b, replace=False)
    hm = np.full(n, -1.0, np.float32)
    hm[pos[:n_hi]] = 3.0
    hm[pos[n_hi:n_hi + n_a]] = xa
    hm[pos[n_hi + n_a:]] = xb
    iou = rng.choice(np.array([-1.0, 0.3, 2.0], np.float32), h * w)
    k = n_hi + n_a if kth == 'upper' else n_hi + n_a + n_b // 2
    return build_head(h, w, hm.reshape(ncls, h * w), iou, seed), h, w, ncls, k


def _tie(h, w, ncls, k, n_hi, m, where='any', use_iou=True, seed=3):
    return dict(kind='tie', h=h, w=w, ncls=ncls, k=k, n_hi=n_hi, m=m, where=where, use_iou=use_iou, seed=seed)


EXACT_CASES = {
    # --- tie patterns: the K-th score is tied across ... (188 x 188 x 3, K = 500: 300 keys above, need = 200)
    'tie_exactly_need': _tie(188, 188, 3, 500, 300, 200),
    'tie_need_plus_1': _tie(188, 188, 3, 500, 300, 201),
    'tie_TIE_CAP': _tie(188, 188, 3, 500, 300, TIE_CAP),
    'tie_TIE_CAP_plus_1': _tie(188, 188, 3, 500, 300, TIE_CAP + 1),
    'tie_all_keys_flat': dict(kind='const', h=188, w=188, ncls=3, k=500, hm=0.7, iou=[0.9]),
    'tie_all_keys_saturated_1.0': dict(kind='const', h=188, w=188, ncls=3, k=500, hm=40.0, iou=[2.0]),
    'tie_all_keys_zero_iou_le_0': dict(kind='const', h=188, w=188, ncls=3, k=500, hm=[3.0, 0.0, -2.0], iou=[0.0, -1.0]),
    'tie_only_last_class': _tie(188, 188, 3, 500, 300, 300, where='last_class'),
    'tie_only_highest_flat_indices': _tie(188, 188, 3, 500, 300, 300, where='highest'),
    'tie_TIE_CAP_plus_1_highest_flat_indices': _tie(188, 188, 3, 500, 300, TIE_CAP + 1, where='highest'),
    # --- radix digit boundaries: two levels that differ only in bits 31..21 / 20..10 / 9..0, K between them or inside the lower
    'digit_31_21_kth_upper': dict(kind='digit', level=0, kth='upper'),
    'digit_31_21_kth_lower': dict(kind='digit', level=0, kth='lower'),
    'digit_20_10_kth_upper': dict(kind='digit', level=1, kth='upper'),
    'digit_20_10_kth_lower': dict(kind='digit', level=1, kth='lower'),
    'digit_9_0_kth_upper': dict(kind='digit', level=2, kth='upper'),
    'digit_9_0_kth_lower': dict(kind='digit', level=2, kth='lower'),
    # --- sizes
    'K_1': _tie(64, 64, 3, 1, 0, 5),
    'K_2': _tie(64, 64, 3, 2, 1, 4),
    'K_500': _tie(64, 64, 3, 500, 450, 60),
    'K_1023': _tie(64, 64, 3, 1023, 700, 400),
    'K_1024': _tie(64, 64, 3, 1024, 1000, 30),
    'K_1024_all_from_overflowing_ties': _tie(64, 64, 3, 1024, 0, 5000),
    'K_gt_keys': _tie(4, 5, 3, 100, 10, 20),
    'ncls_1': _tie(64, 64, 1, 100, 60, 50),
    'ncls_2': _tie(64, 64, 2, 100, 60, 50),
    'ncls_3': _tie(64, 64, 3, 100, 60, 50),
    'map_1x1': _tie(1, 1, 3, 8, 1, 2),
    'map_4x5': _tie(4, 5, 3, 32, 10, 30),
    'map_188x188': _tie(188, 188, 3, 500, 250, 300),
    'map_376x380_more_keys_than_one_grid_pass': _tie(376, 380, 3, 1024, 600, 4500),
    'map_376x380_ties_at_highest_flat_indices': _tie(376, 380, 3, 1024, 600, 4500, where='highest'),
    'map_37x53_hw_not_multiple_of_256': _tie(37, 53, 3, 500, 200, 400),
    'use_iou_on': _tie(64, 64, 3, 100, 60, 50, use_iou=True, seed=8),
    'use_iou_off': _tie(64, 64, 3, 100, 60, 50, use_iou=False, seed=8),
}


def exact_case(name):
    """-> head (hw,12), h, w, ncls, k, use_iou, regime: dict(n_gt, n_eq) the float64 scores must show (None: not stated)."""
    c = EXACT_CASES[name]
    if c['kind'] == 'tie':
        head = tie_map(c['h'], c['w'], c['ncls'], c['n_hi'], c['m'], c['where'], c['seed'], c['use_iou'])
        n = c['ncls'] * c['h'] * c['w']
        regime = dict(n_gt=c['n_hi'], n_eq=c['m']) if c['n_hi'] + c['m'] >= min(c['k'], n) > c['n_hi'] else None
        return head, c['h'], c['w'], c['ncls'], c['k'], c['use_iou'], regime
    if c['kind'] == 'const':
        head = const_map(c['h'], c['w'], c['ncls'], c['hm'], c['iou'], 4)
        return head, c['h'], c['w'], c['ncls'], c['k'], True, dict(n_gt=0, n_eq=c['ncls'] * c['h'] * c['w'])
    head, h, w, ncls, k = digit_map(c['level'], c['kth'])
    return head, h, w, ncls, k, False, (dict(n_gt=120, n_eq=150) if c['kth'] == 'upper' else dict(n_gt=270, n_eq=160))


def exact_reference(name):
    head, h, w, ncls, k, use_iou, regime = exact_case(name)
    ref = decode_ref(head, h, w, ncls, k, use_iou)
    assert_exact_inputs(ref)
    if regime is not None:                                   # the case is the regime its name states
        assert int((ref.all_scores > ref.s_k).sum()) == regime['n_gt']
        assert int((ref.all_scores == ref.s_k).sum()) == regime['n_eq']
    return head, h, w, ncls, k, use_iou, ref


# the 32-frame batch: neighbouring frames in different regimes
def batch_frames():
    h, w, ncls, k = 188, 188, 3, 500
    regimes = [
        lambda s: tie_map(h, w, ncls, 300, 200, 'any', s),                             # generic: every tied key is taken
        lambda s: const_map(h, w, ncls, 0.7, [0.9], s),                                # flat
        lambda s: tie_map(h, w, ncls, 300, 201, 'any', s),                             # one tie too many
        lambda s: const_map(h, w, ncls, 40.0, [2.0], s),                               # saturated at 1.0
        lambda s: const_map(h, w, ncls, [-5.0, -6.0], [1.5, 0.9], s),                  # everything below score_thresh
        lambda s: tie_map(h, w, ncls, 300, TIE_CAP + 1, 'highest', s),                 # tie list overflows
        lambda s: tie_map(h, w, ncls, 300, 250, 'any', s, z_shift=30.0),               # everything outside the limit range
        lambda s: const_map(h, w, ncls, [3.0, 0.0], [0.0, -1.0], s),                   # all scores zero
    ]
    heads = np.stack([regimes[i % len(regimes)](100 + i) for i in range(32)])
    return heads, h, w, ncls, k


def continuous_frames(seed, batch=8, h=188, w=188, ncls=3):
    hw = h * w
    heads = []
    for b in range(batch):
        rng = np.random.default_rng(1000 * seed + b)
        hm = rng.normal(0.0, 1.5, (ncls, hw)).astype(np.float32)
        iou = rng.uniform(0.6, 1.3, hw).astype(np.float32)
        heads.append(build_head(h, w, hm, iou, 1000 * seed + b + 500))
    return np.stack(heads), h, w, ncls


CONT_SEEDS = (1, 2, 3)
CONT_K = 500


def continuous_reference(head, h, w, ncls, k=CONT_K):
    """Reference of one continuous frame + the condition on the input: at most BAND_MAX candidates inside the band, and every
    candidate that may be selected passes the masks (so the count is K and no mask decision is in play)."""
    ref = decode_ref(head, h, w, ncls, k, True)
    eps = EPS_ULPS * float(np.spacing(np.float32(ref.s_k)))
    s = ref.all_scores
    in_band = int(((s >= ref.s_k - eps) & (s <= ref.s_k + eps)).sum())
    assert in_band <= BAND_MAX, '%d candidates inside the band' % in_band
    assert ref.count == k and ref.s_k - eps > SCORE_THRESH + 1e-5
    return ref, eps, in_band


def compare_band(got, ref, eps):
    """Selection and order of one continuous frame judged with the band.  -> (worst score difference, flat indices selected)."""
    c = got['count']
    assert c == ref.k
    lab = got['labels'][:c].astype(np.int64)
    flat = lab * ref.hw + pix_from_z(got['boxes'][:c, 2], ref.hw)
    assert np.unique(flat).size == c, 'a candidate was selected twice'
    s = ref.all_scores
    s_sel = s[flat]
    assert s_sel.min() >= ref.s_k - eps, 'a selected candidate lies %.3g below the K-th score' % (ref.s_k - s_sel.min())
    above = np.nonzero(s > ref.s_k + eps)[0]
    assert np.isin(above, flat).all(), 'a candidate above the band is missing'
    dev = got['scores'][:c]
    assert np.all(np.diff(dev) <= 0), 'device scores increase along the output'
    inv = s_sel[1:] - np.minimum.accumulate(s_sel)[:-1]      # how far a later entry's float64 score exceeds an earlier one's
    assert inv.size == 0 or inv.max() < eps, 'two entries are swapped although their float64 scores differ by %.3g' % inv.max()
    return float(np.abs(dev.astype(np.float64) - s_sel).max()), flat


def boxes_of_flat(head, h, w, flat):
    """Float64 boxes of given flat indices (the decode formula of decode_ref on chosen pixels)."""
    hw = h * w
    pix = flat % hw
    row = head[pix].astype(np.float64)
    xs, ys = (pix % w) + row[:, 0], (pix // w) + row[:, 1]
    return np.stack([xs * STRIDE * float(VOXEL[0]) + float(POINT_CLOUD_RANGE[0]), ys * STRIDE * float(VOXEL[1]) + float(POINT_CLOUD_RANGE[1]),
                     row[:, 2], np.exp(row[:, 3]), np.exp(row[:, 4]), np.exp(row[:, 5]), np.arctan2(row[:, 7], row[:, 6])], axis=1)


# ------------------------------------------------------------------------------------------------------------------------
# input builders: box sets of the NMS tests (the row order is the score order)
# ------------------------------------------------------------------------------------------------------------------------
NMS_SETS = ('synth', 'dense_cluster', 'long_thin', 'exact_duplicates', 'axis_headings')


def nms_boxes(kind, n, seed=0):
    rng = np.random.default_rng(7919 * seed + n)
    if kind == 'synth':
        return synth_boxes(300 + n + seed, n, xy_range=40.0, near_duplicates=0.5)
    b = np.zeros((n, 7), np.float64)
    b[:, 2] = rng.uniform(-1, 2, n)
    b[:, 5] = rng.uniform(1.0, 2.5, n)
    if kind == 'dense_cluster':
        # 1200 boxes with centres within 1 m of each other at the head of the list: 18 whole row blocks whose waves keep all
        # 16 x 64 pairs through the circle test; the rest of the list is spread out
        m = min(n, 1200)
        ang, r = rng.uniform(-math.pi, math.pi, m), 0.5 * np.sqrt(rng.uniform(0, 1, m))
        b[:m, 0], b[:m, 1] = r * np.cos(ang), r * np.sin(ang)
        b[m:, 0:2] = rng.uniform(-40, 40, (n - m, 2))
        b[:, 3], b[:, 4] = rng.uniform(0.5, 6.0, n), rng.uniform(0.5, 2.5, n)
        b[:, 6] = rng.uniform(-math.pi, math.pi, n)
        dup = rng.random(n) < 0.4                            # near-duplicates of an earlier box: IoUs on both sides of a threshold
        src = (rng.random(n) * np.arange(n)).astype(np.int64)
        j = np.nonzero(dup & (np.arange(n) > 0))[0]
        b[j, :] = b[src[j], :]
        b[j, 0:2] += rng.normal(0, 0.08, (j.size, 2))
        b[j, 3:5] *= rng.uniform(0.93, 1.07, (j.size, 2))
        b[j, 6] += rng.normal(0, 0.03, j.size)
        return b.astype(np.float32)
    if kind == 'long_thin':
        # 15-20 m x 0.3-0.6 m boxes crossing at all angles, centres up to 12 m apart, near-duplicates of them, and clusters of tiny
        # boxes a few centimetres apart: 0.05 m ones, and 0.01 m ones - smaller than the 1 cm margin of the reference's corner
        # test, so that pairs whose circumscribed circles are up to 8 mm APART still have an IoU above every threshold here (what
        # the 0.05 m of slack in the kernel's circle test is for)
        n_tiny = n // 8
        n_thin = n - n_tiny
        ang, r = rng.uniform(-math.pi, math.pi, n_thin), 6.0 * np.sqrt(rng.uniform(0, 1, n_thin))
        b[:n_thin, 0], b[:n_thin, 1] = r * np.cos(ang), r * np.sin(ang)
        b[:n_thin, 3], b[:n_thin, 4] = rng.uniform(15.0, 20.0, n_thin), rng.uniform(0.3, 0.6, n_thin)
        b[:n_thin, 6] = rng.uniform(-math.pi, math.pi, n_thin)
        j = np.nonzero((rng.random(n_thin) < 0.4) & (np.arange(n_thin) > 0))[0]
        src = (rng.random(n_thin) * np.arange(n_thin)).astype(np.int64)
        b[j, :] = b[src[j], :]
        b[j, 0:2] += rng.normal(0, 0.04, (j.size, 2))
        b[j, 3:5] *= rng.uniform(0.95, 1.05, (j.size, 2))
        b[j, 6] += rng.normal(0, 0.004, j.size)
        centres = rng.uniform(-6, 6, (max(n_tiny // 6, 1), 2))
        t = slice(n_thin, n)
        b[t, 0:2] = centres[rng.integers(0, centres.shape[0], n_tiny)] + rng.uniform(-0.06, 0.06, (n_tiny, 2))
        b[t, 3], b[t, 4] = 0.05, 0.05
        b[t, 6] = rng.uniform(-math.pi, math.pi, n_tiny)
        q = n_thin + 2 * np.arange(n_tiny // 4)              # half of the tiny boxes: pairs of 0.01 m boxes, the second one 19-21.5 mm
        d, a = rng.uniform(0.019, 0.0215, q.size), b[q, 6] + rng.integers(0, 4, q.size) * (math.pi / 2)      # along an axis of the first
        b[q + 1, 0], b[q + 1, 1] = b[q, 0] + d * np.cos(a), b[q, 1] + d * np.sin(a)
        b[q + 1, 6] = b[q, 6] + rng.normal(0, 0.05, q.size)
        b[q, 3] = b[q, 4] = b[q + 1, 3] = b[q + 1, 4] = 0.01
        return b[rng.permutation(n)].astype(np.float32)
    if kind == 'exact_duplicates':
        base = synth_boxes(900 + n + seed, (n + 3) // 4, xy_range=30.0, near_duplicates=0.3)
        return np.ascontiguousarray(np.tile(base, (4, 1))[rng.permutation(4 * base.shape[0])[:n]])
    assert kind == 'axis_headings'
    side = int(math.ceil(math.sqrt(n / 3.0)))                # about three boxes per cell of a 2 m grid
    cell = rng.integers(0, side * side, n)
    b[:, 0] = (cell % side) * 2.0 + rng.normal(0, 0.25, n)
    b[:, 1] = (cell // side) * 2.0 + rng.normal(0, 0.25, n)
    b[:, 3], b[:, 4] = rng.uniform(1.0, 4.0, n), rng.uniform(0.8, 2.0, n)
    j = np.nonzero((rng.random(n) < 0.35) & (np.arange(n) > 0))[0]                     # near-duplicates of an earlier box, heading redrawn
    src = (rng.random(n) * np.arange(n)).astype(np.int64)
    b[j, :] = b[src[j], :]
    b[j, 0:2] += rng.normal(0, 0.1, (j.size, 2))
    b[:, 6] = rng.choice(np.array([0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi]), n)
    return b.astype(np.float32)


def circle_near(boxes, i, cols):
    """The circle test of k_nms_mask for row box i against column boxes `cols`, in float32 with the kernel's operation order."""
    f = np.float32
    b = boxes.astype(np.float32)
    ra = np.sqrt(f(0.25) * (b[i, 3] * b[i, 3] + b[i, 4] * b[i, 4]))
    rb = np.sqrt(f(0.25) * (b[cols, 3] * b[cols, 3] + b[cols, 4] * b[cols, 4]))
    reach = ra + rb + f(0.05)
    dx, dy = b[i, 0] - b[cols, 0], b[i, 1] - b[cols, 1]
    return dx * dx + dy * dy <= reach * reach


def circle_test_drops_nothing(boxes, keep, thresh):
    """From cref.boxes_iou_bev: no pair (kept box i, later box j) that the circle test drops has an IoU above the threshold.
    Only the rows the sweep uses (the kept boxes) are evaluated.  Returns the number of dropped pairs examined."""
    from oracle import cref
    n = boxes.shape[0]
    examined = 0
    for i in np.asarray(keep, np.int64):
        cols = np.arange(i + 1, n)
        if cols.size == 0:
            continue
        cols = cols[~circle_near(boxes, i, cols)]
        if cols.size:
            iou = cref.boxes_iou_bev(boxes[i:i + 1], boxes[cols])[0]
            assert iou.max() <= thresh, 'the circle test drops pair (%d, %d) with IoU %.4f' % (i, cols[int(iou.argmax())], iou.max())
            examined += cols.size
    return examined


# ------------------------------------------------------------------------------------------------------------------------
# 1. reference self-checks and input-builder checks (CPU)
# ------------------------------------------------------------------------------------------------------------------------
def _as_got(ref, k):
    """What a correct device would hand back for `ref` (float32 outputs, K-sized buffers)."""
    boxes = np.zeros((k, 7), np.float32)
    scores = np.zeros((k,), np.float32)
    labels = np.zeros((k,), np.int32)
    boxes[:ref.count] = ref.boxes.astype(np.float32)
    boxes[:ref.count, 2] = z_marks(ref.hw)[ref.pix]
    scores[:ref.count] = ref.scores.astype(np.float32)
    labels[:ref.count] = ref.labels
    return dict(count=ref.count, boxes=boxes, scores=scores, labels=labels)


def test_decode_ref_agrees_with_oracle_decode():
    from oracle import dense
    heads, h, w, ncls = continuous_frames(11, batch=2, h=40, w=52)
    maps = heads.reshape(2, h, w, 12).transpose(0, 3, 1, 2)
    pred = {'center': maps[:, 0:2], 'center_z': maps[:, 2:3], 'dim': maps[:, 3:6], 'rot': maps[:, 6:8], 'iou': maps[:, 8:9], 'hm': maps[:, 9:12]}
    pred = {k_: torch.from_numpy(np.ascontiguousarray(v)) for k_, v in pred.items()}
    dec = dense.decode(pred, POINT_CLOUD_RANGE, VOXEL, STRIDE, 200, SCORE_THRESH, LIMIT)
    for b in range(2):
        ref = decode_ref(heads[b], h, w, ncls, 200, True)
        assert np.unique(ref.all_scores).size == ref.all_scores.size                  # tie-free
        assert ref.count == dec[b]['pred_boxes'].shape[0] > 100
        assert np.array_equal(ref.labels, dec[b]['pred_labels'].numpy())
        np.testing.assert_allclose(dec[b]['pred_scores'].numpy(), ref.scores, rtol=0, atol=SCORE_TOL)
        np.testing.assert_allclose(dec[b]['pred_boxes'].numpy(), ref.boxes, rtol=0, atol=BOX_TOL)


def test_decode_ref_reproduces_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'det_golden.npz'))
    maps = np.concatenate([g['head_pred_' + n] for n in ('center', 'center_z', 'dim', 'rot', 'iou', 'hm')], axis=1)
    b, _, h, w = maps.shape
    heads = np.ascontiguousarray(maps.transpose(0, 2, 3, 1).reshape(b, h * w, 12))
    for i in range(b):
        ref = decode_ref(heads[i], h, w, 3, 100, True, voxel=VOXEL_SIZE_02)
        assert ref.count == g['dec_boxes_%d' % i].shape[0]
        assert np.array_equal(ref.labels, g['dec_labels_%d' % i])
        np.testing.assert_allclose(g['dec_scores_%d' % i], ref.scores, rtol=0, atol=SCORE_TOL)
        np.testing.assert_allclose(g['dec_boxes_%d' % i], ref.boxes, rtol=0, atol=BOX_TOL)


@pytest.mark.parametrize('name', list(EXACT_CASES))
def test_exact_case_inputs(name):
    """Every exact case satisfies the conditions on its input and is the regime its name states; the reference's own output,
    rounded to float32, passes the comparison."""
    head, h, w, ncls, k, use_iou, ref = exact_reference(name)
    compare_exact(_as_got(ref, k), ref)


@pytest.mark.parametrize('level', [0, 1, 2])
def test_digit_levels_keep_their_order_in_float32(level):
    """The float32 sigmoid of the stored logits keeps the intended order, and the two scores first differ inside the intended
    digit - also when either moves by 8 ulp (what a device expf may add)."""
    a, b, lo, hi = DIGITS[level]
    xa, xb = digit_logits(level)
    sa, sb = sigmoid32(xa), sigmoid32(xb)
    assert sa > sb
    ba, bb = int(np.array([sa]).view(np.uint32)[0]), int(np.array([sb]).view(np.uint32)[0])
    assert abs(ba - a) <= 4 and abs(bb - b) <= 4
    for da in (-8, 0, 8):
        for db in (-8, 0, 8):
            top = ((ba + da) ^ (bb + db)).bit_length() - 1
            assert lo <= top <= hi and ba + da > bb + db


def test_batch_frames_inputs():
    heads, h, w, ncls, k = batch_frames()
    counts = []
    for b in range(heads.shape[0]):
        ref = decode_ref(heads[b], h, w, ncls, k, True)
        assert_exact_inputs(ref)
        counts.append(ref.count)
        assert b == 0 or not np.array_equal(heads[b, :, 9:], heads[b - 1, :, 9:])
    assert counts[:8] == [500, 500, 500, 500, 0, 500, 0, 0]


@pytest.mark.parametrize('seed', CONT_SEEDS)
def test_continuous_inputs(seed):
    heads, h, w, ncls = continuous_frames(seed)
    for b in range(heads.shape[0]):
        continuous_reference(heads[b], h, w, ncls)


def test_compare_reports_a_dropped_tied_candidate():
    head, h, w, ncls, k, use_iou, ref = exact_reference('tie_need_plus_1')
    got = _as_got(ref, k)
    tied = np.nonzero(ref.sel_scores == ref.s_k)[0]
    assert tied.size == 200 and ref.count == k
    j = int(tied[3])                                         # drop one tied candidate: the rest moves up, the count falls
    for a in ('boxes', 'scores', 'labels'):
        got[a][j:-1] = got[a][j + 1:].copy()
    got['count'] -= 1
    with pytest.raises(AssertionError):
        compare_exact(got, ref)
    # ... or the (need + 1)-th tied key is taken in its place: same count, same scores, another pixel
    got = _as_got(ref, k)
    s = ref.all_scores
    spare = np.nonzero(s == ref.s_k)[0][-1]
    assert spare not in ref.flat
    got['labels'][j] = spare // ref.hw
    got['boxes'][j, 2] = z_marks(ref.hw)[spare % ref.hw]
    with pytest.raises(AssertionError, match='selected set differs'):
        compare_exact(got, ref)


def test_compare_reports_two_swapped_tied_candidates():
    head, h, w, ncls, k, use_iou, ref = exact_reference('tie_need_plus_1')
    got = _as_got(ref, k)
    tied = np.nonzero(ref.sel_scores == ref.s_k)[0]
    i, j = int(tied[5]), int(tied[6])
    for a in ('boxes', 'scores', 'labels'):
        got[a][[i, j]] = got[a][[j, i]]
    with pytest.raises(AssertionError, match='order'):
        compare_exact(got, ref)
    compare_exact(_as_got(ref, k), ref)


def test_nms_rule_reports_a_wrong_decision():
    from oracle import cref
    boxes = nms_boxes('synth', 600)
    ref = cref.nms_sorted(boxes, 0.7)
    assert nms_on_threshold_rule(boxes, ref, 0.7) == 0
    iou = cref.boxes_iou_bev(boxes, boxes[ref])
    iou = np.where(ref[None, :] < np.arange(600)[:, None], iou, 0).max(1)
    dropped = np.setdiff1d(np.arange(600), ref)
    clear = dropped[iou[dropped] > 0.8]                      # suppressed at an IoU clearly above the threshold ...
    assert clear.size > 0
    with pytest.raises(AssertionError, match='kept although'):
        nms_on_threshold_rule(boxes, np.sort(np.append(ref, clear[0])), 0.7)          # ... and wrongly kept
    lonely = ref[iou[ref] < 0.5]                             # kept at an IoU clearly below it, and nothing later depends on it
    later = cref.boxes_iou_bev(boxes[lonely], boxes).max(0)
    with pytest.raises(AssertionError, match='suppressed although'):
        nms_on_threshold_rule(boxes, np.setdiff1d(ref, lonely[-1:]), 0.7)              # ... and wrongly suppressed
    assert later.shape == (600,)
    with pytest.raises(AssertionError, match='score order'):
        nms_on_threshold_rule(boxes, ref[::-1], 0.7)


def test_pack_ref_reports_a_wrong_label_and_a_stale_row():
    rng = np.random.default_rng(0)
    boxes, scores = rng.normal(size=(2, 6, 7)).astype(np.float32), rng.random((2, 6)).astype(np.float32)
    labels = rng.integers(0, 3, (2, 6)).astype(np.int32)
    keep = np.array([[4, 1, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0]], np.int32)
    out = pack_ref(boxes, scores, labels, keep, np.array([2, 5]), 3)
    assert np.array_equal(out[0, :2, :7], boxes[0, [4, 1]]) and np.array_equal(out[0, :2, 8], labels[0, [4, 1]] + 1.0)
    assert np.all(out[0, 2:] == 0) and np.array_equal(out[1, :, 7], scores[1, [2, 0, 0]])
    wrong = out.copy()
    wrong[..., 8] -= 1.0                                     # 0-based labels
    assert not np.array_equal(wrong, out)


def test_long_thin_set_survives_the_circle_test():
    """On the CPU alone: in the long-thin set the circle test (0.05 m margin included) drops no pair above a threshold, and the set
    holds pairs of tiny boxes that a circle test WITHOUT the margin would drop although their IoU is above 0.8."""
    from oracle import cref
    boxes = nms_boxes('long_thin', 4033)
    keep = cref.nms_sorted(boxes, 0.1)
    assert circle_test_drops_nothing(boxes, keep, 0.1) > 1000
    t = boxes[boxes[:, 3] < 0.1]
    d = np.sqrt(((t[:, None, :2] - t[None, :, :2]) ** 2).sum(-1))
    reach = 0.5 * (np.hypot(t[:, 3], t[:, 4])[:, None] + np.hypot(t[:, 3], t[:, 4])[None, :])
    i, j = np.nonzero(np.triu((d > reach * 1.0001) & (d < reach + 0.05), 1))
    iou = np.array([cref.boxes_iou_bev(t[a:a + 1], t[b:b + 1])[0, 0] for a, b in zip(i[:6000], j[:6000])])
    assert (iou > 0.8).sum() >= 20, (iou > 0.8).sum()


# ------------------------------------------------------------------------------------------------------------------------
# device plumbing
# ------------------------------------------------------------------------------------------------------------------------
def _sent(shape, device, dtype=torch.float32):
    t = torch.full(shape, SENT, dtype=torch.int32, device=device)
    return t.view(torch.float32) if dtype == torch.float32 else t


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def device_decode(heads, h, w, ncls, k, use_iou, device, thresh=SCORE_THRESH, ws_short=0, alloc_k=None):
    """dz_centerhead_decode through the C ABI on sentinel-filled outputs and a garbage-filled workspace.
    -> rc, per-frame list of dict(count, boxes, scores, labels), raw arrays."""
    from detzero_amd import lib as L
    lib = L.load()
    heads = np.ascontiguousarray(heads if heads.ndim == 3 else heads[None], np.float32)
    b = heads.shape[0]
    ka = alloc_k or max(k, 1)
    t = torch.from_numpy(heads).to(device)
    boxes, scores = _sent((b, ka, 7), device), _sent((b, ka), device)
    labels, counts = _sent((b, ka), device, torch.int32), _sent((b,), device, torch.int32)
    need = int(lib.dz_centerhead_decode_workspace_bytes(b, h * w, ncls, k))
    ws = torch.full((max(need, 256),), 0xA5, dtype=torch.uint8, device=device)
    rc = lib.dz_centerhead_decode(L.ptr(t), b, h, w, ncls, k, float(thresh), L.f6(LIMIT), L.f6(POINT_CLOUD_RANGE), L.f3(VOXEL), STRIDE,
                                  1 if use_iou else 0, L.ptr(boxes), L.ptr(scores), L.ptr(labels), L.ptr(counts), L.ptr(ws),
                                  need - ws_short, L.stream())
    torch.cuda.synchronize()
    raw = dict(boxes=boxes.cpu().numpy(), scores=scores.cpu().numpy(), labels=labels.cpu().numpy(), counts=counts.cpu().numpy())
    frames = [dict(count=int(raw['counts'][i]), boxes=raw['boxes'][i], scores=raw['scores'][i], labels=raw['labels'][i]) for i in range(b)]
    return rc, frames, raw


def assert_tail_untouched(frame):
    c = frame['count']
    assert 0 <= c <= frame['scores'].shape[0]
    assert np.all(_bits(frame['boxes'][c:]) == SENT) and np.all(_bits(frame['scores'][c:]) == SENT) and np.all(frame['labels'][c:] == SENT)


# ------------------------------------------------------------------------------------------------------------------------
# 2. decode with exact selection (GPU)
# ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('name', list(EXACT_CASES))
def test_decode_exact(device, name):
    head, h, w, ncls, k, use_iou, ref = exact_reference(name)
    rc, frames, _ = device_decode(head, h, w, ncls, k, use_iou, device)
    assert rc == 0
    ds, db = compare_exact(frames[0], ref)
    assert_tail_untouched(frames[0])
    print('\n[head_post] decode_exact %-44s count %4d  tied at K-th %6d  score diff %.2e  box diff %.2e' % (
        name, ref.count, int((ref.all_scores == ref.s_k).sum()), ds, db))


@gpu
def test_decode_batch_of_32_mixed_regimes(device):
    heads, h, w, ncls, k = batch_frames()
    rc, frames, raw = device_decode(heads, h, w, ncls, k, True, device)
    assert rc == 0
    worst_s = worst_b = 0.0
    for b in range(heads.shape[0]):
        rc1, one, _ = device_decode(heads[b], h, w, ncls, k, True, device)
        assert rc1 == 0 and one[0]['count'] == frames[b]['count']
        for a in ('boxes', 'scores', 'labels'):
            assert np.array_equal(_bits(one[0][a]), _bits(frames[b][a])), 'frame %d differs from its single-frame call' % b
        ref = decode_ref(heads[b], h, w, ncls, k, True)
        assert_exact_inputs(ref)
        ds, db = compare_exact(frames[b], ref)
        assert_tail_untouched(frames[b])
        worst_s, worst_b = max(worst_s, ds), max(worst_b, db)
    print('\n[head_post] decode_batch32 counts %s  score diff %.2e  box diff %.2e' % (raw['counts'].tolist(), worst_s, worst_b))


@gpu
@pytest.mark.parametrize('what', ['K_0', 'K_1025', 'ncls_4', 'workspace_too_small'])
def test_decode_refusals(device, what):
    from detzero_amd import lib as L
    head = tie_map(16, 16, 3, 10, 20, 'any', 1)
    k, ncls, short, code = {'K_0': (0, 3, 0, L.ERR_INVALID), 'K_1025': (1025, 3, 0, L.ERR_INVALID), 'ncls_4': (32, 4, 0, L.ERR_INVALID),
                            'workspace_too_small': (32, 3, 1, L.ERR_WORKSPACE)}[what]
    rc, frames, raw = device_decode(head, 16, 16, ncls, k, True, device, ws_short=short, alloc_k=1025)
    assert rc == code
    assert np.all(_bits(raw['boxes']) == SENT) and np.all(_bits(raw['scores']) == SENT)
    assert np.all(raw['labels'] == SENT) and np.all(raw['counts'] == SENT)


# ------------------------------------------------------------------------------------------------------------------------
# 3. decode on continuous maps (GPU)
# ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('seed', CONT_SEEDS)
def test_decode_continuous(device, seed):
    heads, h, w, ncls = continuous_frames(seed)
    refs = [continuous_reference(heads[b], h, w, ncls) for b in range(heads.shape[0])]      # conditions on the input first
    rc, frames, _ = device_decode(heads, h, w, ncls, CONT_K, True, device)
    assert rc == 0
    worst_s = worst_b = 0.0
    bands = []
    for b, (ref, eps, in_band) in enumerate(refs):
        ds, flat = compare_band(frames[b], ref, eps)
        assert ds <= SCORE_TOL, ds
        db = float(np.abs(frames[b]['boxes'][:CONT_K].astype(np.float64) - boxes_of_flat(heads[b], h, w, flat)).max())
        assert db <= BOX_TOL, db
        worst_s, worst_b = max(worst_s, ds), max(worst_b, db)
        bands.append(in_band)
    print('\n[head_post] decode_continuous seed %d  in-band candidates per frame %s  score diff %.2e  box diff %.2e' % (
        seed, bands, worst_s, worst_b))


# ------------------------------------------------------------------------------------------------------------------------
# 4. rotated NMS (GPU)
# ------------------------------------------------------------------------------------------------------------------------
def _dev(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(device).contiguous()


def device_nms(boxes, device, thresh, post_max):
    """One frame through the batched entry point (d_n = all rows).  -> kept indices."""
    from detzero_amd import ops
    n = boxes.shape[0]
    keep, d_nk = ops.nms_rotated_batched_nosync(_dev(boxes[None], device), _dev(np.array([n], np.int32), device), thresh, post_max)
    nk = int(d_nk[0].item())
    return keep[0, :nk].cpu().numpy().astype(np.int64), nk


@gpu
@pytest.mark.parametrize('n_cap', [200, 4096])
def test_nms_batched_equals_single_frame_calls(device, n_cap):
    from detzero_amd import ops
    d_n = [0, 1, 63, 64, 65, n_cap, n_cap + 50, 64, 0, n_cap - 1]
    boxes = np.stack([nms_boxes('synth', n_cap, seed=b) for b in range(len(d_n))])
    for b, d in enumerate(d_n):
        boxes[b, min(d, n_cap):] = np.nan                    # rows past d_n[b] must never be read into a decision
    keep, d_nk = ops.nms_rotated_batched_nosync(_dev(boxes, device), _dev(np.array(d_n, np.int32), device), 0.7, n_cap)
    keep, d_nk = keep.cpu().numpy(), d_nk.cpu().numpy()
    for b, d in enumerate(d_n):
        d = min(d, n_cap)                                    # a count above n_cap clamps
        k1, n1 = ops.nms_rotated_nosync(_dev(boxes[b, :d], device), None, 0.7, n_cap)
        n1 = int(n1.item())
        assert int(d_nk[b]) == n1, (b, d, int(d_nk[b]), n1)
        assert np.array_equal(keep[b, :n1], k1[:n1].cpu().numpy()), (b, d)
        assert n1 == d or d > 2
    print('\n[head_post] nms_batched n_cap %d  d_n %s  kept %s' % (n_cap, d_n, d_nk.tolist()))


@gpu
@pytest.mark.parametrize('thresh', [0.1, 0.7, 0.8])
@pytest.mark.parametrize('n_cap', [4033, 4095, 4096])
@pytest.mark.parametrize('kind', NMS_SETS)
def test_nms_vs_cref(device, kind, n_cap, thresh):
    boxes = nms_boxes(kind, n_cap)
    got, nk = device_nms(boxes, device, thresh, n_cap)
    flips = nms_on_threshold_rule(boxes, got, thresh)
    dropped = circle_test_drops_nothing(boxes, got, thresh) if kind == 'long_thin' else 0
    assert 0 < nk < n_cap
    print('\n[head_post] nms_vs_cref %-17s n_cap %d thr %.1f  kept %4d  on-threshold decisions %d%s' % (
        kind, n_cap, thresh, nk, flips, '  circle-dropped pairs examined %d' % dropped if dropped else ''))


@gpu
@pytest.mark.parametrize('post_max', [0, 1, 3, 500, 1500])
def test_nms_post_max(device, post_max):
    n = 1500
    boxes = nms_boxes('synth', n)
    uncut, nu = device_nms(boxes, device, 0.7, n)
    assert nu > 500
    got, nk = device_nms(boxes, device, 0.7, post_max)
    assert nk == min(post_max, nu)
    assert np.array_equal(got, uncut[:post_max])


@gpu
def test_nms_refuses_n_cap_4097(device):
    from detzero_amd import lib as L
    lib = L.load()
    boxes = _dev(nms_boxes('synth', 4097), device)
    keep, d_nk = _sent((4097,), device, torch.int32), _sent((1,), device, torch.int32)
    ws = torch.empty((int(lib.dz_nms_workspace_bytes(4097)) + 256,), dtype=torch.uint8, device=device)
    d_n = _dev(np.array([4097], np.int32), device)
    rc = lib.dz_nms_rotated_batched(L.ptr(boxes), L.ptr(d_n), 1, 4097, 0.7, 500, L.ptr(keep), L.ptr(d_nk), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    assert rc == L.ERR_INVALID
    assert bool((keep == SENT).all()) and int(d_nk.item()) == SENT


# ------------------------------------------------------------------------------------------------------------------------
# 5. packing and the chain (GPU)
# ------------------------------------------------------------------------------------------------------------------------
def device_pack(boxes, scores, labels, keep, d_nk, post_max, device):
    """dz_pack_detections into a sentinel-filled buffer with a sentinel guard row behind it."""
    from detzero_amd import lib as L
    lib = L.load()
    b, k = boxes.shape[0], boxes.shape[1]
    buf = _sent((b * post_max * 9 + 9,), device)
    t = [_dev(boxes, device), _dev(scores, device), _dev(labels, device), _dev(keep, device), _dev(d_nk, device)]
    rc = lib.dz_pack_detections(L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]), L.ptr(t[4]), b, k, int(post_max), L.ptr(buf), L.stream())
    torch.cuda.synchronize()
    assert rc == 0
    raw = buf.cpu().numpy()
    assert np.all(_bits(raw[b * post_max * 9:]) == SENT), 'written past the end of the output'
    return raw[:b * post_max * 9].reshape(b, post_max, 9)


# name -> (batch, k, post_max, d_nk per frame (cycled))
PACK_CASES = {
    'label_plus_1': (2, 64, 16, [16, 9]),
    'zero_rows_after_the_kept': (3, 500, 500, [7, 499, 130]),
    'd_nk_above_post_max': (3, 500, 100, [500, 101, 100]),
    'k_below_post_max': (3, 40, 500, [40, 39, 1]),
    'frame_with_d_nk_0': (4, 300, 200, [150, 0, 0, 200]),
    'batch_32': (32, 500, 500, [500, 0, 1, 257, 499, 64, 3, 311]),
}


@gpu
@pytest.mark.parametrize('name', list(PACK_CASES))
def test_pack_detections(device, name):
    b, k, post_max, cyc = PACK_CASES[name]
    rng = np.random.default_rng(len(name))
    boxes, scores = rng.normal(0, 20, (b, k, 7)).astype(np.float32), rng.random((b, k)).astype(np.float32)
    labels = rng.integers(0, 3, (b, k)).astype(np.int32)
    d_nk = np.array([cyc[i % len(cyc)] for i in range(b)], np.int32)
    keep = np.zeros((b, k), np.int32)                        # past d_nk: a valid index that must not be gathered
    for i in range(b):
        m = min(int(d_nk[i]), k)
        keep[i, :m] = np.sort(rng.choice(k, m, replace=False))
    ref = pack_ref(boxes, scores, labels, keep, d_nk, post_max)
    out = device_pack(boxes, scores, labels, keep, d_nk, post_max, device)
    assert not np.any(_bits(out) == SENT), 'a row of the output was not written'
    assert np.array_equal(_bits(out), _bits(ref))
    assert set(np.unique(ref[..., 8]).tolist()) <= {0.0, 1.0, 2.0, 3.0}
    print('\n[head_post] pack %-26s batch %2d k %3d post_max %3d  rows gathered %d, zero rows %d' % (
        name, b, k, post_max, int(np.minimum(np.minimum(d_nk, post_max), k).sum()), b * post_max - int(np.minimum(np.minimum(d_nk, post_max), k).sum())))


def _center_head(device, k, post_max):
    from detzero_amd.config import AttrDict
    from detzero_amd.det_modules import CenterHead
    from oracle import voxelize as ov
    names = ['Vehicle', 'Pedestrian', 'Cyclist']
    branch = lambda c: {'out_channels': c, 'num_conv': 2}
    hcfg = AttrDict({
        'CLASS_NAMES_EACH_HEAD': [names], 'SHARED_CONV_CHANNEL': 32, 'USE_BIAS_BEFORE_NORM': True, 'NUM_HM_CONV': 2, 'IOU_WEIGHT': 1,
        'SEPARATE_HEAD_CFG': {'HEAD_ORDER': ['center', 'center_z', 'dim', 'rot', 'iou'],
                              'HEAD_DICT': {'center': branch(2), 'center_z': branch(1), 'dim': branch(3), 'rot': branch(2), 'iou': branch(1)}},
        'TARGET_ASSIGNER_CONFIG': {'FEATURE_MAP_STRIDE': STRIDE},
        'POST_PROCESSING': {'SCORE_THRESH': SCORE_THRESH, 'POST_CENTER_LIMIT_RANGE': LIMIT, 'MAX_OBJ_PER_SAMPLE': k,
                            'NMS_CONFIG': {'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.7, 'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': post_max}}})
    grid = ov.grid_size_of(POINT_CLOUD_RANGE, VOXEL)
    return CenterHead(hcfg, 64, 3, names, grid, POINT_CLOUD_RANGE, VOXEL).to(device).eval()


@gpu
def test_chain_decode_nms_pack(device):
    """decode -> batched NMS -> pack on the 32-frame batch of mixed regimes, against the reference chain (float64 decode, cref NMS
    on the reference's boxes, numpy gather) and against CenterHead.decode_batched_nosync on the same head maps."""
    from detzero_amd import ops
    from oracle import cref
    heads, h, w, ncls, k = batch_frames()
    post_max = 500
    t = _dev(heads, device)
    boxes, scores, labels, counts = ops.centerhead_decode(t, h, w, ncls, k, SCORE_THRESH, LIMIT, POINT_CLOUD_RANGE, VOXEL, STRIDE, use_iou=True)
    keep, d_nk = ops.nms_rotated_batched_nosync(boxes, counts, 0.7, post_max)
    out = ops.pack_detections(boxes, scores, labels, keep, d_nk, post_max).cpu().numpy()
    hb, hs, hl, hk, hn = _center_head(device, k, post_max).decode_batched_nosync(t, h, w)
    boxes_n, scores_n, labels_n = boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy()
    keep_n, d_nk_n, counts_n = keep.cpu().numpy(), d_nk.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(out.view(np.int32), pack_ref(boxes_n, scores_n, labels_n, keep_n, d_nk_n, post_max).view(np.int32))
    flips_all, kept_all, worst = 0, [], 0.0
    for b in range(heads.shape[0]):
        c, nk = int(counts_n[b]), int(d_nk_n[b])
        # the detector's own route: the same bits
        assert int(hn[b].item()) == nk and np.array_equal(hk[b, :nk].cpu().numpy(), keep_n[b, :nk])
        assert np.array_equal(_bits(hb[b, :c].cpu().numpy()), _bits(boxes_n[b, :c])) and np.array_equal(hl[b, :c].cpu().numpy(), labels_n[b, :c])
        assert np.array_equal(_bits(hs[b, :c].cpu().numpy()), _bits(scores_n[b, :c]))
        # the reference chain
        ref = decode_ref(heads[b], h, w, ncls, k, True)
        compare_exact(dict(count=c, boxes=boxes_n[b], scores=scores_n[b], labels=labels_n[b]), ref)
        flips = 0
        if not np.array_equal(keep_n[b, :nk], cref.nms_sorted(ref.boxes.astype(np.float32), 0.7) if c else np.zeros((0,), np.int64)):
            # the device's boxes are within 1e-4 of the reference's (just checked), which can move an IoU that sits on 0.7: then the
            # sweep is judged on the boxes it was given
            flips = nms_on_threshold_rule(boxes_n[b, :c], keep_n[b, :nk], 0.7)
        sel = keep_n[b, :nk].astype(np.int64)
        assert nk == min(post_max, nk) and np.all(out[b, nk:] == 0)
        if nk:
            assert np.array_equal(out[b, :nk, 8], (ref.labels[sel] + 1).astype(np.float32))
            ds = float(np.abs(out[b, :nk, 7] - ref.scores[sel]).max())
            db = float(np.abs(out[b, :nk, :7] - ref.boxes[sel]).max())
            assert ds <= SCORE_TOL and db <= BOX_TOL, (ds, db)
            worst = max(worst, ds, db)
        flips_all += flips
        kept_all.append(nk)
    print('\n[head_post] chain batch32 kept per frame %s  on-threshold decisions %d  worst difference %.2e' % (kept_all, flips_all, worst))
