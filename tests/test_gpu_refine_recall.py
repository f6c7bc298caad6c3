"""The refining models' recall kernels on the device (csrc/box_ops.hip): dz_boxes_paired_metric and dz_track_recall_iou3d.

The paired metric shares its pair body with dz_boxes_pairwise_metric, so the reference of the first test is that kernel's
diagonal, bit for bit (the matrix itself is checked against float64 in tests/test_gpu_box_ops.py).  The recall table is an
integer function of the paired IoUs of the same run: the reference is a numpy count over them, `>` taken in float32, exactly.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from detzero_amd.synth import synth_boxes

gpu = pytest.mark.gpu


def edge_pairs(n, seed):
    """(a, b) of n pairs: seeded near-duplicates, then - as far as n allows - the edge cases, cycled through the rows."""
    rng = np.random.default_rng(seed)
    a = synth_boxes(seed, max(n, 1), near_duplicates=0.0)[:n].astype(np.float32)
    b = a.copy()
    b[:, :3] += (rng.normal(0, 1, (n, 3)) * np.array([0.3, 0.2, 0.1])).astype(np.float32)
    b[:, 3:6] *= rng.uniform(0.85, 1.15, (n, 3)).astype(np.float32)
    b[:, 6] += rng.normal(0, 0.2, n).astype(np.float32)
    for i in range(n):
        kind = i % 9
        if kind == 1:                                   # identical boxes
            b[i] = a[i]
        elif kind == 2:                                 # disjoint
            b[i, :2] = a[i, :2] + 40.0
        elif kind == 3:                                 # shared edge, headings on the axes
            a[i, 6], b[i] = 0.0, a[i]
            b[i, 6], b[i, 0] = 0.0, a[i, 0] + a[i, 3]
        elif kind == 4:                                 # headings on the axes, overlapping
            a[i, 6], b[i, 6] = np.float32(math.pi / 2), np.float32(-math.pi)
        elif kind == 5:                                 # zero-size boxes: the 1e-6 clamp of the union volume
            a[i, 3:6], b[i] = 0.0, a[i]
            b[i, 3:6] = 0.0
        elif kind == 6:                                 # centres at 5 000 m
            shift = np.float32(5000.0)
            a[i, :2] += shift
            b[i, :2] += shift
        elif kind == 7:                                 # same footprint, disjoint in height
            b[i] = a[i]
            b[i, 2] = a[i, 2] + a[i, 5] * 2
    return a, b


def _dev(x, device):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


@gpu
@pytest.mark.parametrize('n', [1, 63, 64, 65, 129, 1000])
def test_paired_iou_is_the_matrix_diagonal(device, n):
    from detzero_amd import iou3d_nms_utils, ops
    a, b = edge_pairs(n, 100 + n)
    da, db = _dev(a, device), _dev(b, device)
    got = iou3d_nms_utils.boxes_iou3d_paired_gpu(da, db)
    assert got.shape == (n,) and got.dtype == torch.float32
    want = ops.boxes_pairwise_metric(da, db, ops.BOXM_IOU3D).diag()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))             # bit for bit
    got = got.cpu().numpy()
    assert np.all(np.isfinite(got)) and got.min() >= 0.0 and got.max() <= 1.0 + 1e-3
    for i in range(n):
        if i % 9 == 1 and a[i, 3:6].min() > 0:
            assert abs(got[i] - 1.0) < 1e-3, (i, got[i])                          # identical boxes (at 70 m: overlap area to ~1e-4 relative)
        if i % 9 in (2, 7):
            assert got[i] == 0.0, (i, got[i])                                     # disjoint in the plane / in height
    for metric in (ops.BOXM_UNION_BEV, ops.BOXM_GIOU3D, ops.BOXM_GIOU3D_EXACT):   # the other codes run the same shared body
        pm = ops.boxes_paired_metric(da, db, metric)
        assert torch.equal(pm.view(torch.int32), ops.boxes_pairwise_metric(da, db, metric).diag().view(torch.int32)), metric
    print('\n[refine_recall] paired IoU n=%d: bit-equal to the matrix diagonal, range [%.3f, %.3f]' % (n, got.min(), got.max()))


@gpu
def test_paired_metric_empty_and_refusals(device):
    from detzero_amd import lib as L
    from detzero_amd import iou3d_nms_utils, ops
    e = torch.zeros((0, 7), device=device)
    out = iou3d_nms_utils.boxes_iou3d_paired_gpu(e, e)
    assert out.shape == (0,) and out.dtype == torch.float32
    fn = L.load().dz_boxes_paired_metric
    assert fn(None, None, 0, ops.BOXM_IOU3D, None, None) == 0                     # n == 0: no pointer is looked at, nothing launched
    assert fn(None, None, 4, 7, None, None) == L.ERR_UNSUPPORTED and b'7' in L.load().dz_last_error()
    assert fn(None, None, 2 ** 31 // 7 + 1, ops.BOXM_IOU3D, None, None) == L.ERR_UNSUPPORTED
    assert fn(None, None, 4, ops.BOXM_IOU3D, None, None) == L.ERR_INVALID
    with pytest.raises(L.DetZeroHipError):
        ops.boxes_paired_metric(torch.zeros((3, 7), device=device), torch.zeros((2, 7), device=device), ops.BOXM_IOU3D)


def recall_case(b, t, n_thr, seed):
    """Padded tracks with NaN wherever the kernel must not look: outside the mask, at or beyond the length."""
    rng = np.random.default_rng(seed)
    a, g = edge_pairs(b * t, seed)
    o = g.copy()
    o[:, :3] += (rng.normal(0, 1, (b * t, 3)) * 0.05).astype(np.float32)
    lens = rng.integers(0, t + 1, b).astype(np.int32)
    lens[0] = t                                             # a full track; a length of 0 where the batch has room
    if b > 1:
        lens[1] = 0
    mask = (rng.random((b, t)) < 0.7).astype(np.uint8)
    mask[0, 0] = 1                                          # (so that the 1 x 1 case counts its row)
    if b > 2:
        mask[2] = 0                                         # an all-zero mask
    boxes = [x.reshape(b, t, 7).copy() for x in (a, o, g)]
    counted = (mask != 0) & (np.arange(t)[None, :] < lens[:, None])
    for x in boxes:
        x[~counted] = np.nan
    thr = [float(v) for v in np.sort(rng.uniform(0.05, 0.95, n_thr))]
    return boxes, mask, lens, counted, thr


def table_from_ious(iou_in, iou_out, counted, thr):
    want = np.zeros((counted.shape[0], 2, len(thr) + 1), np.int32)
    for s, v in enumerate((iou_in, iou_out)):
        want[:, s, 0] = counted.sum(1)
        for k, th in enumerate(thr):
            want[:, s, 1 + k] = ((v.astype(np.float32) > np.float32(th)) & counted).sum(1)
    return want


@gpu
@pytest.mark.parametrize('b,t,n_thr', [(1, 1, 1), (3, 5, 3), (70, 200, 8), (2, 257, 3), (3, 129, 1)])
def test_recall_table_is_the_count_over_the_paired_ious(device, b, t, n_thr):
    from detzero_amd import ops
    (bi, bo, bg), mask, lens, counted, thr = recall_case(b, t, n_thr, 7 * b + t)
    d = [_dev(x, device) for x in (bi, bo, bg)]
    d_mask, d_len = _dev(mask, device), _dev(lens, device)
    # the paired IoUs of the counted rows, from the paired kernel: the recall kernel must store the same bits
    flat = counted.reshape(-1)
    idx = _dev(np.nonzero(flat)[0], device)
    ref = [np.zeros(b * t, np.float32), np.zeros(b * t, np.float32)]
    for s in range(2):
        v = ops.boxes_paired_metric(d[s].reshape(-1, 7)[idx].contiguous(), d[2].reshape(-1, 7)[idx].contiguous(), ops.BOXM_IOU3D)
        ref[s][flat] = v.cpu().numpy()
    equal_thr = False
    if flat.any():
        # a threshold that equals one pair's IoU exactly: equality is not counted
        inner = ref[0][flat][(ref[0][flat] > 0) & (ref[0][flat] < 1)]
        if inner.size:
            thr[-1], equal_thr = float(inner[inner.size // 2]), True
    counts, iou_in, iou_out = ops.track_recall_iou3d_nosync(d[0], d[1], d[2], d_mask, d_len, thr)
    assert counts.shape == (b, 2, n_thr + 1) and counts.dtype == torch.int32
    got_in, got_out = iou_in.cpu().numpy(), iou_out.cpu().numpy()
    assert np.array_equal(got_in.reshape(-1).view(np.int32), ref[0].view(np.int32))       # bit for bit; 0 on every row not counted
    assert np.array_equal(got_out.reshape(-1).view(np.int32), ref[1].view(np.int32))
    want = table_from_ious(got_in, got_out, counted, thr)
    assert np.array_equal(counts.cpu().numpy(), want)
    hit = int((got_in[counted] == np.float32(thr[-1])).sum())
    assert hit >= 1 or not equal_thr          # the pair that sits on the threshold exists and (by the table above) is not counted
    # two runs, one without the IoU outputs: identical tables; lengths beyond t_cap are clamped
    again, none_in, none_out = ops.track_recall_iou3d_nosync(d[0], d[1], d[2], d_mask, d_len, thr, want_iou=False)
    assert none_in is None and none_out is None and torch.equal(again, counts)
    long_len = _dev(np.where(lens == t, t + 1000, lens).astype(np.int32), device)
    assert torch.equal(ops.track_recall_iou3d_nosync(d[0], d[1], d[2], d_mask, long_len, thr, want_iou=False)[0], counts)
    print('\n[refine_recall] table (%d, %d) x %d thresholds: %d counted rows, %d on the equal threshold, per-threshold totals in %s out %s' % (
        b, t, n_thr, int(counted.sum()), int(hit), want[:, 0, 1:].sum(0).tolist(), want[:, 1, 1:].sum(0).tolist()))


@gpu
def test_recall_argument_refusals(device):
    """Refused before any pointer is looked at and before any launch: sizes only, null pointers."""
    from detzero_amd import lib as L
    fn = L.load().dz_track_recall_iou3d
    thr = (ctypes.c_double * 9)(*([0.5] * 9))
    for n_thr in (0, 9):
        assert fn(None, None, None, None, None, 2, 4, thr, n_thr, None, None, None, None) == L.ERR_UNSUPPORTED
        assert str(n_thr).encode() in L.load().dz_last_error()
    big_b, big_t = 1 << 20, 1 << 9                          # 2^29 rows x 7 floats: beyond 32-bit offsets
    assert fn(None, None, None, None, None, big_b, big_t, thr, 1, None, None, None, None) == L.ERR_UNSUPPORTED
    assert fn(None, None, None, None, None, -1, 4, thr, 1, None, None, None, None) == L.ERR_INVALID
    assert fn(None, None, None, None, None, 2, 4, None, 1, None, None, None, None) == L.ERR_INVALID
    assert fn(None, None, None, None, None, 2, 4, thr, 1, None, None, None, None) == L.ERR_INVALID          # null counts / boxes
    assert fn(None, None, None, None, None, 0, 4, thr, 1, None, None, None, None) == 0                      # empty batch: nothing to do
    counts = torch.full((2, 2, 2), 7, dtype=torch.int32, device=device)
    assert fn(None, None, None, None, None, 2, 0, thr, 1, None, None, counts.data_ptr(), None) == 0          # t_cap 0: the table is zeroed
    assert int(counts.abs().sum()) == 0
