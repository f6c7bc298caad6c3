"""Box ops on the device (csrc/box_ops.hip): dz_boxes_pairwise_metric, dz_nms_normal(_batched) and the Python surface above them
(iou3d_nms_utils, CenterHead / PDVHead NMS_TYPE dispatch, the detzero_utils.ops shim).  References, input regimes and tolerances
are those of tests/test_box_ops.py (checked there on the CPU); each test prints the figures it measured.

GIoU and the unit range.  The textbook quantity (DZ_BOXM_GIOU3D_EXACT) lies in [-1, 1], and that is asserted for every pair.
The reference's formula (DZ_BOXM_GIOU3D) takes min(tops) - min(bottoms) as the enclosing height, which can be SMALLER than
either box: same footprint and bottom, heights 1 and 10, gives 0.1 - (4 - 40) / 4 = 9.1 (test_box_ops.py:test_giou_ref_values,
and on the device in test_giou_reference_height_term below).  For that variant the range is therefore asserted where it is a
property of the formula - the pairs with equal tops, on which the two variants are the same expression - and the extremes
over the other pairs are printed.  The per-pair tolerance (hull bound / hull area) + 16 * 2^-24 is derived for values of the
unit range; it is used as it stands for the exact variant and for equal tops, and scaled by max(1, U / C) of the float64
reference where the reference's height term makes U / C exceed 1 (tests/test_box_ops.py:giou_tol has the derivation; measured
with the unscaled tolerance: every regime of ordinary boxes passes it, worst error / tolerance 0.48 at values up to 7.1, and the
zero-size boxes of `tiny`, whose C is clamped at 1e-6 under a U of 100, reach 2.2e8 with an error of 17.5 = 8e-8 relative).
"""
import math

import numpy as np
import pytest
import torch

from tests.test_box_ops import (REGIMES, SHAPES, _head, giou_ref, giou_tol, heights64, nms_boxes, nms_normal_ref, on_threshold_pair,
                                pair_case)

gpu = pytest.mark.gpu

PAIR_CASES = [('random', s) for s in SHAPES[:3]] + [(r, s) for s in SHAPES[3:] for r in REGIMES]
PAIR_IDS = ['%s-%dx%d' % (r, s[0], s[1]) for r, s in PAIR_CASES]


def _dev(a, device, dtype=torch.float32):
    return torch.from_numpy(np.array(a, order='C')).to(device=device, dtype=dtype)          # (a copy: the shared references are read-only)


def _metric(a, b, metric, device):
    from detzero_amd import ops
    out = ops.boxes_pairwise_metric(_dev(a, device), _dev(b, device), metric)
    assert out.shape == (a.shape[0], b.shape[0]) and out.dtype == torch.float32
    return out


# ------------------------------------------------------------------------------------------------------------------------
# pair matrices
# ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('regime,shape', PAIR_CASES, ids=PAIR_IDS)
def test_union_bev(device, regime, shape):
    from detzero_amd import iou3d_nms_utils, ops
    a, b, area, bound = pair_case(regime, shape)
    got = _metric(a, b, ops.BOXM_UNION_BEV, device).cpu().numpy().astype(np.float64)
    assert np.array_equal(got, iou3d_nms_utils.boxes_union_bev_gpu(_dev(a, device), _dev(b, device)).cpu().numpy())
    err = np.abs(got - area)
    assert np.all(err <= bound), (float(err.max()), np.unravel_index(np.argmax(err - bound), err.shape))
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0
    if regime == 'inside' and shape[0]:
        j = np.arange(shape[1])
        i = j % shape[0]
        outer = a[i, 3].astype(np.float64) * a[i, 4].astype(np.float64)
        assert np.all(np.abs(got[i, j] - outer) <= bound[i, j])            # a box inside another: the outer dx * dy
    print('\n[box_ops] union %-9s %3dx%-3d worst error %.2e m^2, worst error / bound %.3f' % (
        regime, shape[0], shape[1], float(err.max()) if err.size else 0.0, ratio))


def _iou3d_parent_composition(boxes_a, boxes_b):
    """boxes_iou3d_gpu as it was before the fused kernel: torch dispatches around dz_boxes_overlap_bev."""
    from detzero_amd import iou3d_nms_utils
    a_max = (boxes_a[:, 2] + boxes_a[:, 5] / 2).reshape(-1, 1)
    a_min = (boxes_a[:, 2] - boxes_a[:, 5] / 2).reshape(-1, 1)
    b_max = (boxes_b[:, 2] + boxes_b[:, 5] / 2).reshape(1, -1)
    b_min = (boxes_b[:, 2] - boxes_b[:, 5] / 2).reshape(1, -1)
    overlaps_bev = iou3d_nms_utils.boxes_overlap_bev_gpu(boxes_a, boxes_b)
    overlaps_h = torch.clamp(torch.min(a_max, b_max) - torch.max(a_min, b_min), min=0)
    overlaps_3d = overlaps_bev * overlaps_h
    vol_a = (boxes_a[:, 3] * boxes_a[:, 4] * boxes_a[:, 5]).reshape(-1, 1)
    vol_b = (boxes_b[:, 3] * boxes_b[:, 4] * boxes_b[:, 5]).reshape(1, -1)
    return overlaps_3d / torch.clamp(vol_a + vol_b - overlaps_3d, min=1e-6)


@gpu
@pytest.mark.parametrize('regime,shape', PAIR_CASES, ids=PAIR_IDS)
def test_iou3d_equals_the_torch_composition(device, regime, shape):
    from detzero_amd import iou3d_nms_utils, ops
    a, b, _, _ = pair_case(regime, shape)
    ta, tb = _dev(a, device), _dev(b, device)
    got = _metric(a, b, ops.BOXM_IOU3D, device)
    want = _iou3d_parent_composition(ta, tb)
    assert torch.equal(got, want), float((got - want).abs().max())
    assert torch.equal(iou3d_nms_utils.boxes_iou3d_gpu(ta, tb), want)
    # far-apart pairs: exactly 0 (centre distance beyond both circumscribed circles and the 5 cm of the skip, with 5 cm to spare)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    dist = np.hypot(a64[:, None, 0] - b64[None, :, 0], a64[:, None, 1] - b64[None, :, 1])
    reach = 0.5 * np.hypot(a64[:, 3], a64[:, 4])[:, None] + 0.5 * np.hypot(b64[:, 3], b64[:, 4])[None, :]
    far = dist > reach + 0.1
    g = got.cpu().numpy()
    assert np.all(g[far] == 0)
    if regime == 'far' and shape == (129, 65):
        assert far.sum() > 1000 and (g > 0).sum() > 100
    print('\n[box_ops] iou3d %-9s %3dx%-3d bit-equal; far pairs %d (all exactly 0), positive %d, max %.4f' % (
        regime, shape[0], shape[1], int(far.sum()), int((g > 0).sum()), float(g.max()) if g.size else 0.0))


@gpu
@pytest.mark.parametrize('regime,shape', PAIR_CASES, ids=PAIR_IDS)
def test_giou3d(device, regime, shape):
    from detzero_amd import iou3d_nms_utils, ops
    a, b, area, bound = pair_case(regime, shape)
    ta, tb = _dev(a, device), _dev(b, device)
    overlap = ops.boxes_pairwise(ta, tb, iou=False).cpu().numpy()          # dz_boxes_overlap_bev (existing, tested)
    a_max, _, b_max, _ = heights64(a, b)
    tops_equal = np.broadcast_to(a_max == b_max, area.shape)
    unit = giou_tol(area, bound)                                           # the tolerance for values of the unit range
    got = {}
    for exact, metric in ((False, ops.BOXM_GIOU3D), (True, ops.BOXM_GIOU3D_EXACT)):
        g = _metric(a, b, metric, device)
        assert torch.equal(g, iou3d_nms_utils.boxes_giou3d_gpu(ta, tb, exact_height=exact))
        g = g.cpu().numpy().astype(np.float64)
        ref, ratio = giou_ref(a, b, overlap, area, exact, with_ratio=True)
        # exact height, or equal tops: U / C <= 1, `unit` as it stands; the reference's height term elsewhere: scaled by U / C (giou_tol)
        tol = unit if exact else np.where(tops_equal, unit, giou_tol(area, bound, ratio))
        err = np.abs(g - ref)
        print('\n[box_ops] giou%s %-9s %3dx%-3d worst error %.2e, worst error / tolerance %.3f, range [%.4f, %.4f]' % (
            '_exact' if exact else '      ', regime, shape[0], shape[1], float(err.max()) if err.size else 0.0,
            float((err / tol).max()) if err.size else 0.0, float(g.min()) if g.size else 0.0, float(g.max()) if g.size else 0.0))
        assert np.all(err <= tol), (exact, float((err / tol).max()), np.unravel_index(np.argmax(err / tol), err.shape))
        where = np.ones_like(tops_equal) if exact else tops_equal          # (module docstring: the reference's height term)
        assert np.all(g[where] >= -1 - unit[where]) and np.all(g[where] <= 1 + unit[where])
        got[exact] = g
    # the two variants differ where, and only where, one box's top is above the other's
    assert np.array_equal(got[False][tops_equal], got[True][tops_equal])
    if regime != 'tiny':                                                    # (zero-volume pairs clamp U and C on both sides)
        assert np.all(a[:, 3:6] > 0.2) and np.all(b[:, 3:6] > 0.08) and np.all(area > 0)
        assert np.all(got[False][~tops_equal] != got[True][~tops_equal])
    if regime == 'identical' and shape[0]:
        j = np.arange(shape[1])
        i = j % shape[0]
        assert np.all(np.abs(got[True][i, j] - 1.0) <= unit[i, j])         # EXACT of a box with itself


@gpu
def test_giou_reference_height_term(device):
    """Same footprint and bottom, heights 1 and 10: the reference's formula gives 9.1 (outside [-1, 1]), the textbook one 0.1."""
    from detzero_amd import iou3d_nms_utils
    lo = np.array([[0, 0, 0.5, 2, 2, 1.0, 0]], np.float32)
    hi = np.array([[0, 0, 5.0, 2, 2, 10.0, 0]], np.float32)
    g = float(iou3d_nms_utils.boxes_giou3d_gpu(_dev(lo, device), _dev(hi, device)).item())
    ge = float(iou3d_nms_utils.boxes_giou3d_gpu(_dev(lo, device), _dev(hi, device), exact_height=True).item())
    print('\n[box_ops] giou of heights 1 / 10 on one footprint: reference formula %.7f, exact height %.7f' % (g, ge))
    assert abs(g - 9.1) <= 16 * 2.0 ** -24 and abs(ge - 0.1) <= 16 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------------
# axis-aligned NMS
# ------------------------------------------------------------------------------------------------------------------------
def _nms(boxes, device, thresh, post_max, d_n=None):
    from detzero_amd import ops
    keep, d_nk = ops.nms_normal_nosync(_dev(boxes, device), None if d_n is None else torch.tensor([d_n], dtype=torch.int32, device=device),
                                       thresh, post_max)
    nk = int(d_nk.item())
    return keep[:nk].cpu().numpy().astype(np.int64), nk


@gpu
@pytest.mark.parametrize('n', [0, 1, 2, 63, 64, 65, 130, 500])
def test_nms_normal_vs_numpy_sweep(device, n):
    boxes = nms_boxes(n, seed=n)
    turned = boxes.copy()
    turned[:, 6] = np.random.default_rng(n).uniform(-math.pi, math.pi, n)
    kept = []
    for post_max in sorted({1, 5, n}):
        want = nms_normal_ref(boxes, 0.5, post_max)
        got, nk = _nms(boxes, device, 0.5, post_max)
        assert nk == len(want) and np.array_equal(got, want), (n, post_max)
        assert np.array_equal(_nms(turned, device, 0.5, post_max)[0], want)           # the heading is ignored
        kept.append((post_max, nk))
    print('\n[box_ops] nms_normal n %3d: (post_max, kept) %s' % (n, kept))


@gpu
def test_nms_normal_on_the_threshold(device):
    pair = on_threshold_pair()
    third = np.float32(1 / 3)
    at, _ = _nms(pair, device, float(third), 2)
    below, _ = _nms(pair, device, float(np.nextafter(third, np.float32(0))), 2)
    print('\n[box_ops] nms_normal IoU == thresh == float32(1/3): kept %s; thresh one ulp lower: kept %s' % (at.tolist(), below.tolist()))
    assert at.tolist() == [0, 1] and below.tolist() == [0]


@gpu
def test_nms_normal_ragged_count(device):
    """d_n < n_cap with NaN rows behind d_n (no influence), d_n > n_cap (clamped)."""
    n_cap, n = 130, 70
    boxes = nms_boxes(n_cap, seed=5)
    want = nms_normal_ref(boxes[:n], 0.5, n_cap)
    dirty = boxes.copy()
    dirty[n:] = np.nan
    got, nk = _nms(dirty, device, 0.5, n_cap, d_n=n)
    assert np.array_equal(got, want)
    full = nms_normal_ref(boxes, 0.5, n_cap)
    over, nk_over = _nms(boxes, device, 0.5, n_cap, d_n=n_cap + 1000)
    assert np.array_equal(over, full)
    print('\n[box_ops] nms_normal d_n %d of n_cap %d with NaN rows behind: kept %d; d_n > n_cap: kept %d' % (n, n_cap, nk, nk_over))


@gpu
def test_nms_normal_batched_equals_single_frame_calls(device):
    from detzero_amd import ops
    n_cap = 130
    counts = [0, 1, 64, 65, n_cap]
    boxes = np.stack([nms_boxes(n_cap, seed=20 + i) for i in range(len(counts))])
    for i, c in enumerate(counts):
        boxes[i, c:] = np.nan
    t = _dev(boxes, device)
    d_n = torch.tensor(counts, dtype=torch.int32, device=device)
    keep, d_nk = ops.nms_normal_batched_nosync(t, d_n, 0.5, n_cap)
    keep, d_nk = keep.cpu().numpy(), d_nk.cpu().numpy()
    for i, c in enumerate(counts):
        k1, n1 = ops.nms_normal_nosync(t[i].contiguous(), d_n[i:i + 1].contiguous(), 0.5, n_cap)
        nk = int(n1.item())
        assert int(d_nk[i]) == nk and np.array_equal(keep[i, :nk], k1[:nk].cpu().numpy())
        assert np.array_equal(keep[i, :nk], nms_normal_ref(boxes[i, :c], 0.5, n_cap))
    print('\n[box_ops] nms_normal batched counts %s kept %s' % (counts, d_nk.tolist()))


@gpu
def test_nms_normal_gpu_on_unsorted_scores(device):
    from detzero_amd import iou3d_nms_utils
    n = 300
    boxes = nms_boxes(n, seed=9)
    scores = np.random.default_rng(9).permutation(n).astype(np.float32) / n          # distinct
    order = np.argsort(-scores, kind='stable')
    want = order[nms_normal_ref(boxes[order], 0.4, n)]
    got, none = iou3d_nms_utils.nms_normal_gpu(_dev(boxes, device), _dev(scores, device), 0.4, NMS_PRE_MAXSIZE=7)
    assert none is None and got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    empty, _ = iou3d_nms_utils.nms_normal_gpu(_dev(boxes[:0], device), _dev(scores[:0], device), 0.4)
    assert empty.shape == (0,)
    print('\n[box_ops] nms_normal_gpu %d unsorted boxes: kept %d' % (n, len(want)))


# ------------------------------------------------------------------------------------------------------------------------
# NMS_TYPE in the head and in the proposal layer
# ------------------------------------------------------------------------------------------------------------------------
def _head_maps(batch, h, w, seed):
    """(B, H*W, 12) random head output: center 0:2 | center_z 2 | dim 3:6 | rot 6:8 | iou 8 | hm 9:12; 4.5 m boxes at 0.8 m pitch."""
    rng = np.random.default_rng(seed)
    head = rng.normal(0, 1, (batch, h * w, 12)).astype(np.float32)
    head[..., 0:2] = rng.uniform(0, 1, (batch, h * w, 2))
    head[..., 3:5] = rng.normal(1.5, 0.3, (batch, h * w, 2))
    head[..., 5] = rng.normal(0.5, 0.1, (batch, h * w))
    head[..., 8] = rng.normal(2.0, 1.0, (batch, h * w))
    return head


@gpu
def test_center_head_nms_type(device):
    from detzero_amd import ops
    from detzero_amd.synth import POINT_CLOUD_RANGE, VOXEL_SIZE_01
    batch, h, w, k = 3, 24, 24, 128
    t = _dev(_head_maps(batch, h, w, 1), device)
    head = _head('nms_normal_gpu').to(device)
    post = head.model_cfg.POST_PROCESSING
    thr, post_max = post.NMS_CONFIG.NMS_THRESH, post.NMS_CONFIG.NMS_POST_MAXSIZE
    boxes, scores, labels, counts = ops.centerhead_decode(t, h, w, 3, k, post.SCORE_THRESH, post.POST_CENTER_LIMIT_RANGE, POINT_CLOUD_RANGE,
                                                          VOXEL_SIZE_01, 8, use_iou=True)
    hb, hs, hl, hk, hn = head.decode_batched_nosync(t, h, w)
    assert torch.equal(hb, boxes) and torch.equal(hs, scores) and torch.equal(hl, labels)
    boxes_n, counts_n = boxes.cpu().numpy(), counts.cpu().numpy()
    kept = []
    for b in range(batch):
        want = nms_normal_ref(boxes_n[b, :counts_n[b]], thr, post_max)
        nk = int(hn[b].item())
        assert nk == len(want) and np.array_equal(hk[b, :nk].cpu().numpy(), want)
        assert not np.array_equal(want, np.arange(len(want)))                          # candidates were suppressed, not only cut
        kept.append((int(counts_n[b]), nk))
    assert all(0 < nk < c for c, nk in kept)                                          # candidates were suppressed
    # nms_gpu: the rotated wrapper, bit for bit
    rb, rs, rl, rk, rn = _head('nms_gpu').to(device).decode_batched_nosync(t, h, w)
    keep, d_nk = ops.nms_rotated_batched_nosync(boxes, counts, thr, post_max)
    assert torch.equal(rb, boxes) and torch.equal(rn, d_nk)
    for b in range(batch):
        assert torch.equal(rk[b, :int(d_nk[b].item())], keep[b, :int(d_nk[b].item())])
    print('\n[box_ops] CenterHead 24x24 batch 3 K 128: (candidates, kept) axis-aligned %s, rotated kept %s' % (kept, d_nk.tolist()))


def _proposals(device, nms_type):
    from detzero_amd.config import AttrDict
    rng = np.random.default_rng(4)
    boxes = np.stack([nms_boxes(40, seed=30 + i) for i in range(2)])
    cls = rng.permutation(2 * 40 * 3).reshape(2, 40, 3).astype(np.float32) / 240.0          # distinct scores
    cfg = AttrDict({'NMS_TYPE': nms_type, 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 32, 'NMS_POST_MAXSIZE': 16, 'NMS_THRESH': 0.4})
    batch = {'batch_size': 2, 'batch_box_preds': _dev(boxes, device), 'batch_cls_preds': _dev(cls, device)}
    return boxes, cls, cfg, batch


@gpu
def test_pdv_proposal_layer_nms_type(device):
    from detzero_amd import iou3d_nms_utils
    from detzero_amd.pdv_modules import PDVHead
    kept = {}
    for nms_type in ('nms_normal_gpu', 'nms_gpu'):
        boxes, cls, cfg, batch = _proposals(device, nms_type)
        out = PDVHead.proposal_layer(None, batch, cfg)
        assert out['rois'].shape == (2, 16, 7) and out['has_class_labels']
        for i in range(2):
            scores, labels = cls[i].max(axis=1), cls[i].argmax(axis=1)
            if nms_type == 'nms_normal_gpu':          # no pre_maxsize, as in the reference
                order = np.argsort(-scores, kind='stable')
                sel = order[nms_normal_ref(boxes[i][order], cfg.NMS_THRESH, 40)][:16]
            else:
                sel = iou3d_nms_utils.nms_gpu(_dev(boxes[i], device), _dev(scores, device), cfg.NMS_THRESH, pre_maxsize=32)[0][:16].cpu().numpy()
            m = len(sel)
            assert 0 < m
            assert np.array_equal(out['rois'][i, :m].cpu().numpy(), boxes[i][sel]) and not out['rois'][i, m:].any()
            assert np.array_equal(out['roi_scores'][i, :m].cpu().numpy(), scores[sel])
            assert np.array_equal(out['roi_labels'][i, :m].cpu().numpy(), labels[sel] + 1)
            kept[(nms_type, i)] = m
    print('\n[box_ops] PDVHead.proposal_layer 2 x 40 proposals: RoIs kept %s' % kept)


# ------------------------------------------------------------------------------------------------------------------------
# the detzero_utils.ops shim
# ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_shim_iou3d_nms_cuda_calling_convention(device):
    from detzero_amd import iou3d_nms_utils, ops, shim
    shim.install()
    from detzero_utils.ops.iou3d_nms import iou3d_nms_cuda
    a, b, _, _ = pair_case('random', (7, 3))
    ta, tb = _dev(a, device), _dev(b, device)
    for fn, want in ((iou3d_nms_cuda.boxes_overlap_bev_gpu, iou3d_nms_utils.boxes_overlap_bev_gpu(ta, tb)),
                     (iou3d_nms_cuda.boxes_iou_bev_gpu, iou3d_nms_utils.boxes_iou_bev(ta, tb)),
                     (iou3d_nms_cuda.boxes_union_bev_gpu, iou3d_nms_utils.boxes_union_bev_gpu(ta, tb))):
        out = torch.full((7, 3), -7.0, device=device)
        assert fn(ta, tb, out) == 1 and torch.equal(out, want) and float(want.max()) > 0
    boxes = _dev(nms_boxes(130, seed=2), device)
    for fn, route in ((iou3d_nms_cuda.nms_gpu, ops.nms_rotated_nosync), (iou3d_nms_cuda.nms_normal_gpu, ops.nms_normal_nosync)):
        keep = torch.full((130,), -1, dtype=torch.int64)
        num = fn(boxes, keep, 0.5)
        d_keep, d_nk = route(boxes, None, 0.5, 130)
        assert isinstance(num, int) and num == int(d_nk.item()) and 0 < num < 130
        assert not keep.is_cuda and keep.dtype == torch.int64 and torch.equal(keep[:num], d_keep[:num].cpu().long())
    assert iou3d_nms_cuda.nms_normal_gpu(boxes[:0], torch.zeros(0, dtype=torch.int64), 0.5) == 0


@gpu
def test_shim_points_in_boxes_num(device):
    from detzero_amd import shim
    shim.install()
    from detzero_utils.ops.roiaware_pool3d import roiaware_pool3d_utils
    rng = np.random.default_rng(0)
    pts = _dev(rng.uniform(-10, 10, (2, 700, 3)), device)
    boxes = _dev(np.stack([nms_boxes(9, seed=i) for i in range(2)]) * np.array([0.2, 0.2, 1, 2, 2, 8, 1], np.float32), device)
    num = roiaware_pool3d_utils.points_in_boxes_num_gpu(pts, boxes)
    want = roiaware_pool3d_utils.points_in_boxes_gpu_v2(pts, boxes).sum(dim=2).int()
    assert num.shape == (2, 9) and torch.equal(num, want) and int(want.sum()) > 0
