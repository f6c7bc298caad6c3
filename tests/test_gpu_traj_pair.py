"""Trajectory-pair kernels on the device (csrc/traj_pair.hip): dz_traj_pair_table / dz_traj_pair_rows against the composition they
replace, then the fixture of tests/golden/track_assign_golden.npz end to end through assign_track_target, TrackRecall.eval_single_seq
and run_model on HipTrajOps.

Composition.  Per frame, the matrices of dz_boxes_iou_bev and dz_boxes_pairwise_metric(DZ_BOXM_IOU3D) over the boxes present, the
host's class mask and threshold, and a float32 sum with one add per frame in frame order: the kernel uses the same pair bodies and
adds in the same order, so all four tables and the rows are compared BIT FOR BIT.

Tolerances against the reference's CPU values (the fixture), eps = 2^-23:
  per-frame BEV IoU   2e-5, the project's bound for this pair body against the reference's C++ (test_gpu_kernels.py:592: sin / cos /
                      atan2 are ocml here and libm there).
  per-frame 3-D IoU   J = s h / (W - s h) with s the BEV overlap, h the height overlap and W = Va + Vb >= h (A + B): dJ/ds =
                      h W / (W - s h)^2 falls as W grows, and at W = h (A + B) it equals the BEV IoU's (A + B) / (A + B - s)^2.
                      An error of the overlap area therefore moves J by no more than it moves the BEV IoU: 2e-5 again, plus the
                      four fp32 roundings each side makes on a value <= 1 (8 * 2^-24).  test_gpu_box_ops.py holds DZ_BOXM_IOU3D
                      bit-equal to that composition around the overlap kernel, which adds nothing.
  similarity          that bound + n eps, n = the frames the pair shares: each side makes n sequential fp32 adds of values <= 1
                      (partial sums <= n, rounding <= n eps / 2 each) and divides by a length >= n.
"""
import copy
import pickle

import numpy as np
import pytest
import torch

from tests import traj_ref
from tests.test_box_ops import REGIMES, pair_boxes
from tests.test_track_assign import _val_dataset, diff, golden, plain, recall_thr

gpu = pytest.mark.gpu
EPS = 2.0 ** -23
BEV_TOL = 2e-5
IOU3D_TOL = 2e-5 + 8 * 2.0 ** -24
SHAPES = [(1, 1, 1), (3, 67, 5), (65, 2, 24), (129, 65, 7), (40, 50, 200)]
THR = [0.3, 0.1, 0.5]


def _dev(a, device, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


# ------------------------------------------------------------------------------------------------
# inputs and the composition
# ------------------------------------------------------------------------------------------------
def make_sides(n_a, n_b, n_frames, seed=0):
    """Two row tables with frame-major slots.  Frame f takes its boxes from regime REGIMES[f % 7] of tests/test_box_ops.pair_boxes;
    about a third of the slots are absent; trajectory a[0] lives in the first half of the frames only and b[0] in the second half
    (no common frame when there are two frames or more); every fifth trajectory changes class on every third frame; the rows of a
    frame sit in the table in a shuffled order."""
    rng = np.random.default_rng(50 + seed)
    a_traj_cls, b_traj_cls = rng.integers(0, 3, n_a), rng.integers(0, 3, n_b)
    a_slot = np.full((n_frames, n_a), -1, np.int32)
    b_slot = np.full((n_frames, n_b), -1, np.int32)
    boxes = {'a': [], 'b': []}
    cls = {'a': [], 'b': []}
    for f in range(n_frames):
        fa, fb = pair_boxes(REGIMES[f % len(REGIMES)], n_a, n_b, seed=seed + f)
        for side, full, traj_cls, slot, n in (('a', fa, a_traj_cls, a_slot, n_a), ('b', fb, b_traj_cls, b_slot, n_b)):
            here = rng.random(n) >= 1.0 / 3.0
            if n_frames >= 2:
                here[0] = (f < n_frames // 2) if side == 'a' else (f >= n_frames // 2)
            else:
                here[:] = True
            at = rng.permutation(np.flatnonzero(here))
            base = sum(len(x) for x in boxes[side])
            slot[f, at] = base + np.arange(len(at))
            c = traj_cls[at].copy()
            change = (at % 5 == 4) & (f % 3 == 2)
            c[change] = (c[change] + 1) % 3
            boxes[side].append(full[at])
            cls[side].append(c.astype(np.int32))
    cat = lambda parts, w, dt: np.concatenate(parts).astype(dt) if parts else np.zeros((0, w) if w else (0,), dt)      # noqa: E731
    return (cat(boxes['a'], 7, np.float32), cat(cls['a'], 0, np.int32), a_slot, cat(boxes['b'], 7, np.float32), cat(cls['b'], 0, np.int32), b_slot)


def frame_matrices(sides, metric, device):
    """per frame: (a trajectories present, b trajectories present, the device's own per-frame matrix over them)"""
    from detzero_amd import ops
    a_box, _, a_slot, b_box, _, b_slot = sides
    out = []
    for f in range(a_slot.shape[0]):
        ia, ib = np.flatnonzero(a_slot[f] >= 0), np.flatnonzero(b_slot[f] >= 0)
        mat = np.zeros((len(ia), len(ib)), np.float32)
        if len(ia) and len(ib):
            a, b = _dev(a_box[a_slot[f, ia]], device, torch.float32), _dev(b_box[b_slot[f, ib]], device, torch.float32)
            mat = (ops.boxes_pairwise(a, b, True) if metric == ops.TRACK_AFF_IOU_BEV else ops.boxes_pairwise_metric(a, b, ops.BOXM_IOU3D)).cpu().numpy()
        out.append((ia, ib, mat))
    return out


def compose(sides, mats, distinguish, thr, pairs):
    """The host composition: class mask, threshold, one float32 add per frame in frame order."""
    _, a_cls, a_slot, _, b_cls, b_slot = sides
    n_frames, n_a, n_b = a_slot.shape[0], a_slot.shape[1], b_slot.shape[1]
    thr = np.asarray(thr, np.float32)
    sum_all, sum_hit = np.zeros((n_a, n_b), np.float32), np.zeros((n_a, n_b), np.float32)
    n_hit, n_same = np.zeros((n_a, n_b), np.int32), np.zeros((n_a, n_b), np.int32)
    rows = np.zeros((len(pairs), n_frames), np.float32)
    for f, (ia, ib, mat) in enumerate(mats):
        if len(ia) == 0 or len(ib) == 0:
            continue
        ca, cb = a_cls[a_slot[f, ia]], b_cls[b_slot[f, ib]]
        m = mat.copy()
        if distinguish:
            m[ca[:, None] != cb[None, :]] = 0.
        hit = m >= thr[ca][:, None]
        sub = np.ix_(ia, ib)
        n_same[sub] += 1
        sum_all[sub] = sum_all[sub] + m
        n_hit[sub] += hit
        sum_hit[sub] = sum_hit[sub] + np.where(hit, m, np.float32(0))
        full = np.zeros((n_a, n_b), np.float32)
        full[sub] = m
        if len(pairs):
            rows[:, f] = full[pairs[:, 0], pairs[:, 1]]
    return sum_all, sum_hit, n_hit, n_same, rows


def device_sides(sides, device):
    dt = (torch.float32, torch.int32, torch.int32) * 2
    return [_dev(x, device, t) for x, t in zip(sides, dt)]


# ------------------------------------------------------------------------------------------------
# composition, bit for bit
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('metric_name', ['bev', '3d'])
@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%dx%d' % s for s in SHAPES])
def test_tables_and_rows_equal_the_composition_bit_for_bit(device, shape, metric_name):
    from detzero_amd import ops
    from detzero_amd.track_assign import METRIC_OF
    n_a, n_b, n_frames = shape
    metric = METRIC_OF[metric_name]
    sides = make_sides(n_a, n_b, n_frames, seed=n_a + n_frames)
    d = device_sides(sides, device)
    mats = frame_matrices(sides, metric, device)
    rng = np.random.default_rng(3)
    pairs = np.stack([rng.integers(0, n_a, 11), rng.integers(0, n_b, 11)], axis=1).astype(np.int32)
    pairs[0] = (0, 0)
    for distinguish in (True, False):
        want = compose(sides, mats, distinguish, THR, pairs)
        got = [t.cpu().numpy() for t in ops.traj_pair_table(*d, metric, distinguish, THR)]
        got.append(ops.traj_pair_rows(*d, metric, distinguish, _dev(pairs, device, torch.int32)).cpu().numpy())
        for name, g, w in zip(('sum_all', 'sum_hit', 'n_hit', 'n_same', 'rows'), got, want):
            assert g.dtype == w.dtype and g.shape == w.shape, name
            assert np.array_equal(g.view(np.int32), w.view(np.int32)), (name, distinguish, float(np.max(np.abs(g.astype(np.float64) - w))))
    sum_all, sum_hit, n_hit, n_same, rows = want          # distinguish off
    if n_frames >= 2:
        assert n_same[0, 0] == 0 and sum_all[0, 0] == 0 and not rows[0].any()         # the pair without a common frame
    if shape == (40, 50, 200):
        assert n_same.max() > 80 and n_hit.sum() > 1000 and 0 < (n_hit > 0).sum() < n_hit.size and sum_hit.max() > 1.0
    print('\n[traj_pair] %s %dx%dx%d bit-equal; common frames <= %d, hits %d, largest sum %.3f' % (
        metric_name, n_a, n_b, n_frames, int(n_same.max()), int(n_hit.sum()), float(sum_all.max())))


# ------------------------------------------------------------------------------------------------
# empty and refused inputs, determinism
# ------------------------------------------------------------------------------------------------
@gpu
def test_empty_sides_and_no_pairs_return_empty_results(device):
    from detzero_amd import ops
    sides = make_sides(4, 5, 3)
    d = device_sides(sides, device)
    none = [torch.zeros((0, 7), device=device), torch.zeros((0,), dtype=torch.int32, device=device), torch.zeros((3, 0), dtype=torch.int32, device=device)]
    for args, shape in ((none + d[3:], (0, 5)), (d[:3] + none, (4, 0))):
        out = ops.traj_pair_table(*args, ops.TRACK_AFF_IOU_BEV, True, THR)
        assert [tuple(t.shape) for t in out] == [shape] * 4
        assert tuple(ops.traj_pair_rows(*args, ops.TRACK_AFF_IOU_BEV, True, torch.zeros((0, 2), dtype=torch.int32, device=device)).shape) == (0, 3)
    rows = ops.traj_pair_rows(*d, ops.BOXM_IOU3D, True, torch.zeros((0, 2), dtype=torch.int32, device=device))
    assert tuple(rows.shape) == (0, 3) and rows.dtype == torch.float32


@gpu
def test_invalid_arguments_are_refused_on_the_host(device):
    """Nothing here reaches a kernel: every refusal is raised by the wrapper before the launch."""
    from detzero_amd import ops
    from detzero_amd.lib import DetZeroHipError
    sides = make_sides(4, 5, 3)
    d = device_sides(sides, device)
    pairs = torch.zeros((1, 2), dtype=torch.int32, device=device)
    for thr in ([0.3, 0.0, 0.5], [0.3, -1.0, 0.5], []):
        with pytest.raises(DetZeroHipError, match='threshold'):
            ops.traj_pair_table(*d, ops.TRACK_AFF_IOU_BEV, True, thr)
    for metric in (ops.BOXM_GIOU3D, ops.BOXM_UNION_BEV, 7):
        with pytest.raises(DetZeroHipError, match='metric'):
            ops.traj_pair_table(*d, metric, True, THR)
        with pytest.raises(DetZeroHipError, match='metric'):
            ops.traj_pair_rows(*d, metric, True, pairs)
    for k, bad in ((2, sides[0].shape[0]), (2, -2), (5, sides[3].shape[0])):
        slot = sides[k].copy()
        slot[1, 1] = bad
        args = list(d)
        args[k] = _dev(slot, device, torch.int32)
        with pytest.raises(DetZeroHipError, match='slot holds'):
            ops.traj_pair_table(*args, ops.TRACK_AFF_IOU_BEV, True, THR)
        with pytest.raises(DetZeroHipError, match='slot holds'):
            ops.traj_pair_rows(*args, ops.TRACK_AFF_IOU_BEV, True, pairs)
    args = list(d)
    args[1] = torch.full_like(d[1], 3)
    with pytest.raises(DetZeroHipError, match='a_cls holds'):                 # a ground-truth class outside the threshold table
        ops.traj_pair_table(*args, ops.TRACK_AFF_IOU_BEV, True, THR)
    with pytest.raises(DetZeroHipError, match='outside the 4 x 5 table'):
        ops.traj_pair_rows(*d, ops.TRACK_AFF_IOU_BEV, True, torch.tensor([[0, 5]], dtype=torch.int32, device=device))
    with pytest.raises(DetZeroHipError):                                      # CPU tensors
        ops.traj_pair_table(*[_dev(x, 'cpu', t.dtype) for x, t in zip(sides, d)], ops.TRACK_AFF_IOU_BEV, True, THR)


@gpu
def test_a_second_call_and_a_second_ops_object_give_the_same_bytes(device):
    from detzero_amd.track_assign import METRIC_OF, HipTrajOps
    sides = make_sides(40, 50, 24, seed=5)
    pairs = np.array([[1, 2], [39, 49], [7, 7]])
    outs = []
    for ops_obj in (HipTrajOps(device), HipTrajOps(device)):
        ops_obj.set_sides(*sides)
        for _ in range(2):
            outs.append(ops_obj.table(METRIC_OF['3d'], True, THR) + (ops_obj.rows(METRIC_OF['3d'], True, pairs),))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------
# the fixture end to end
# ------------------------------------------------------------------------------------------------
class Recording:
    """an ops object that keeps the tables it returned"""

    def __init__(self, inner):
        self.inner, self.tables = inner, []

    def set_sides(self, *sides):
        self.inner.set_sides(*sides)

    def table(self, *args):
        self.tables.append(self.inner.table(*args))
        return self.tables[-1]

    def rows(self, *args):
        return self.inner.rows(*args)


def rec_metric(method):
    from detzero_amd.track_assign import METRIC_OF
    return METRIC_OF[method]


def _similarity_gap(dev_tables, ref_tables, lens, which):
    """largest (error - n eps) of the normalised similarities; n = the frames a pair shares"""
    d, r = dev_tables[which].astype(np.float64) / lens, ref_tables[which].astype(np.float64) / lens
    return np.abs(d - r) - dev_tables[3] * EPS


@gpu
@pytest.mark.parametrize('si', [0, 1])
def test_fixture_through_assign_on_the_device(device, si):
    from detzero_amd.track_assign import HipTrajOps, assign_track_target, get_gt_id_data
    g = golden()
    e = g['sequences'][si]
    rec, ref = Recording(HipTrajOps(device)), traj_ref.NumpyTrajOps()
    out = assign_track_target((copy.deepcopy(e['det']), copy.deepcopy(e['tracks']), copy.deepcopy(e['gt'])), g['iou_thresholds'], ops=rec)
    assign_track_target((copy.deepcopy(e['det']), copy.deepcopy(e['tracks']), copy.deepcopy(e['gt'])), g['iou_thresholds'], ops=ref)
    # every discrete output exact - membership and order of label / unlabel, ids, state, every array of the ground truth - and the rows within the bound
    assert diff(e['assign'], plain(out), close={'iou': BEV_TOL}) is None
    worst = max(float(np.max(np.abs(v['track']['iou'] - e['assign']['label'][k]['track']['iou']))) for k, v in out['label'].items())
    assert np.array_equal(rec.tables[0][2], ref.tables[0][2]) and np.array_equal(rec.tables[0][3], ref.tables[0][3])
    lens = np.array([[len(v['sample_idx'])] for v in get_gt_id_data(e['gt'], ['name'], g['class_names']).values()], np.float64)
    gap = _similarity_gap(rec.tables[0], ref.tables[0], lens, 1)
    print('\n[traj_pair] assign seq %d: worst per-frame BEV IoU error %.2e (bound %.0e); worst similarity error %.2e' % (
        si, worst, BEV_TOL, float(np.max(gap + rec.tables[0][3] * EPS))))
    assert np.all(gap <= BEV_TOL)


@gpu
@pytest.mark.parametrize('method,tol', [('3d', IOU3D_TOL), ('bev', BEV_TOL)])
@pytest.mark.parametrize('si', [0, 1])
def test_fixture_through_recall_on_the_device(device, si, method, tol):
    from detzero_amd.track_assign import HipTrajOps, get_gt_id_data
    from detzero_amd.track_recall import TrackRecall
    g = golden()
    e = g['sequences'][si]
    rec, ref = Recording(HipTrajOps(device)), traj_ref.NumpyTrajOps()
    data = lambda: {'gt': copy.deepcopy(e['gt']), 'pred': copy.deepcopy(e['tracks'])}      # noqa: E731
    out = TrackRecall.eval_single_seq(data(), g['class_names'], g['difficultys'], recall_thr(), method, ops=rec)
    TrackRecall.eval_single_seq(data(), g['class_names'], g['difficultys'], recall_thr(), method, ops=ref)
    assert diff(e['recall'][method], plain(out)) is None              # every entry of the recall dict
    assert np.array_equal(rec.tables[0][2], ref.tables[0][2]) and np.array_equal(rec.tables[0][3], ref.tables[0][3])
    lens = np.array([[len(v['sample_idx'])] for v in get_gt_id_data(e['gt'], ['name'], g['class_names']).values()], np.float64)
    gap = _similarity_gap(rec.tables[0], ref.tables[0], lens, 0)
    # the per-frame values of every pair that counts a frame, against the CPU values the reference summed
    pairs = np.argwhere(ref.tables[0][2] > 0)
    frame_err = float(np.max(np.abs(rec.rows(rec_metric(method), True, pairs).astype(np.float64) - ref.rows(rec_metric(method), True, pairs))))
    print('\n[traj_pair] recall %s seq %d: worst per-frame IoU error %.2e over %d pairs, worst similarity error %.2e (bound %.1e, + n eps)' % (
        method, si, frame_err, len(pairs), float(np.max(gap + rec.tables[0][3] * EPS)), tol))
    assert len(pairs) >= 15 and frame_err <= tol
    assert np.all(gap <= tol)


@gpu
@pytest.mark.parametrize('method,tol', [('3d', IOU3D_TOL), ('bev', BEV_TOL)])
def test_get_iou_mat_dict_on_the_box_ops(device, method, tol):
    """The shim-level per-frame matrices (one box-op call per frame) against the same function on the CPU IoUs."""
    from oracle import cref
    from tests import track_ref
    from detzero_amd.track_adapter import frame_list_to_dict, tracklets_to_frames
    from detzero_amd.track_assign import get_iou_mat_dict
    g = golden()
    e = g['sequences'][0]
    frames = frame_list_to_dict(tracklets_to_frames({'reference': e['gt'], 'source': e['tracks']}))
    cpu = lambda a, b, iou: (cref.boxes_iou_bev(np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32))      # noqa: E731
                             if iou == 'bev' else track_ref.iou3d(a, b))
    got = get_iou_mat_dict(e['gt'], frames, g['class_names'], True, method)
    want = get_iou_mat_dict(e['gt'], frames, g['class_names'], True, method, iou_fn=cpu)
    assert list(got) == list(e['gt']) == list(want)
    worst = 0.0
    for key in got:
        assert got[key].shape == want[key].shape and got[key].dtype == np.float32
        assert np.array_equal(got[key] == 0, want[key] == 0)            # the class mask and the far pairs
        worst = max(worst, float(np.max(np.abs(got[key] - want[key]))) if got[key].size else 0.0)
    assert worst <= tol, worst


@gpu
def test_run_model_over_a_result_pickle_in_assign_mode(device, tmp_path):
    """The assign-mode twin of test_gpu_track.py::test_run_model_over_a_result_pickle: tracker and assignment on the device."""
    from detzero_amd.config import AttrDict
    from detzero_amd.track_assign import assign_track_target
    from detzero_amd.track_models import build_model, run_model
    from tests.test_track_models import load_sequence
    g = golden()
    model = load_sequence(0)[1]
    dataset, loader = _val_dataset(tmp_path, g['sequences'], g['sequences'])
    cfgs = AttrDict({'REFINING': {'IOU_THRESHOLDS': dict(g['iou_thresholds'])}})
    run_model(build_model(model), loader, dataset, workers=4, cfgs=cfgs)
    saved = pickle.load(open(dataset.get_track_path(), 'rb'))
    assert dataset.get_track_path().endswith('tracking-val-20240101-000000.pkl') and list(saved) == ['seq_a', 'seq_b']
    for k, e in enumerate(g['sequences']):
        item = dataset[k][1]
        tracks = build_model(model).forward(copy.deepcopy(item['detection']))
        direct = assign_track_target((item['detection'], tracks, copy.deepcopy(item['gt'])), g['iou_thresholds'])
        got = saved[dataset.seq_name_list[k]]
        assert diff(plain(direct), plain(got)) is None
        # the object removed from the ground truth sits 16 m from every other: its track cannot be labelled; most others are
        assert len(got['label']) >= 15 and len(got['unlabel']) >= 1
        assert {v['track']['state'] for v in got['label'].values()} == {'static', 'dynamic'}
        assert all(v['track']['iou'].dtype == np.float32 and len(v['track']['iou']) == len(v['track']['sample_idx']) for v in got['label'].values())
