"""GPU: CenterHead targets and losses on the device (csrc/head_loss.hip) against the reference's own classes
(tests/golden/head_loss_golden.npz, target_golden.npz), the host route of assign_targets and float64."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import head_loss_ref as hr
from tests.test_head_loss_cpu import CASES, EPS32, NAMES, WEIGHTS, class_table, scalar_tol, tb_keys

RANGE_S, VOXEL = [-9.2, -7.6, -2.0, 9.2, 7.6, 4.0], [0.1, 0.1, 0.15]
W_S, H_S, STRIDE = 23, 19, 8


@pytest.fixture(scope='module')
def g(golden_dir):
    return np.load(os.path.join(golden_dir, 'head_loss_golden.npz'))


def random_gt(n_boxes, seed=5, frames=8, half=(9.6, 8.0)):
    """(frames, M, 8) seeded boxes on the small map: centres up to 0.4 m beyond the range (clamped), all three classes,
    padding rows, dx = 0 and dy < 0 rows, a few very large boxes."""
    rng = np.random.default_rng(seed)
    m = n_boxes // frames
    gt = np.zeros((frames, m, 8), np.float32)
    size = np.array([[4.6, 2.0, 1.7], [0.9, 0.8, 1.75], [1.8, 0.8, 1.6]])
    cls = rng.integers(0, 4, (frames, m))
    gt[..., 0] = rng.uniform(-half[0], half[0], (frames, m))
    gt[..., 1] = rng.uniform(-half[1], half[1], (frames, m))
    gt[..., 2] = rng.uniform(-1, 2, (frames, m))
    gt[..., 3:6] = size[np.maximum(cls, 1) - 1] * rng.uniform(0.6, 1.6, (frames, m, 3))
    gt[..., 3:6] *= np.where(rng.random((frames, m, 1)) < 0.03, 9.0, 1.0)
    gt[..., 6] = rng.uniform(-3.2, 3.2, (frames, m))
    gt[..., 7] = cls
    gt[..., 3] = np.where(rng.random((frames, m)) < 0.03, 0.0, gt[..., 3])
    gt[..., 4] = np.where(rng.random((frames, m)) < 0.02, -gt[..., 4], gt[..., 4])
    return gt


def small_head(each_head, nmax, iou_weight=1):
    from detzero_amd.config import centerpoint_1sweep_cfg
    from detzero_amd.det_modules import CenterHead
    cfg = centerpoint_1sweep_cfg()
    cfg.MODEL.DENSE_HEAD.CLASS_NAMES_EACH_HEAD = each_head
    cfg.MODEL.DENSE_HEAD.IOU_WEIGHT = iou_weight
    cfg.MODEL.DENSE_HEAD.TARGET_ASSIGNER_CONFIG.NUM_MAX_OBJS = nmax
    return CenterHead(cfg.MODEL.DENSE_HEAD, 8, 3, NAMES, np.array([W_S * STRIDE, H_S * STRIDE, 40]), RANGE_S, VOXEL)


def check_targets(dev_t, ref_heat, ref_tb, ref_inds, ref_masks, gt_rows=None):
    heat, tb, inds, masks = [t.cpu().numpy() for t in dev_t[:4]]
    np.testing.assert_array_equal(inds, ref_inds)
    np.testing.assert_array_equal(masks, ref_masks)
    np.testing.assert_array_equal(tb[..., 0:3], ref_tb[..., 0:3])
    np.testing.assert_array_equal(heat > 0, ref_heat > 0)                    # the support
    worst = hr.ulps32(heat, ref_heat).max()
    print('heat map: worst %.2f ulp, %d cells' % (worst, (ref_heat > 0).sum()))
    assert worst <= 1
    rec = dev_t[4].cpu().numpy()
    assert rec[0] == (ref_heat == 1).sum() and rec[1] == ref_masks.sum()
    return tb


# ---- targets ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('tag', sorted(CASES))
def test_device_targets_equal_the_fixture(device, g, tag):
    from detzero_amd import ops
    gt = torch.from_numpy(g[tag + '_gt_boxes']).to(device)
    for i, names in enumerate(CASES[tag]):
        out = ops.centerhead_targets(gt, class_table(names), len(names), H_S, W_S, STRIDE, RANGE_S, VOXEL, 16, 0.1, 2)
        ref_tb = g['%s_h%d_target_boxes' % (tag, i)]
        tb = check_targets(out, g['%s_h%d_heatmaps' % (tag, i)], ref_tb, g['%s_h%d_inds' % (tag, i)], g['%s_h%d_masks' % (tag, i)])
        exact = hr.targets(g[tag + '_gt_boxes'], class_table(names), len(names), H_S, W_S, STRIDE, RANGE_S, VOXEL, 16, 0.1, 2)[1]
        assert hr.ulps32(tb[..., 3:8], exact[..., 3:8]).max() <= 4 and hr.ulps32(ref_tb[..., 3:8], exact[..., 3:8]).max() <= 4


@pytest.mark.gpu
@pytest.mark.parametrize('each_head', [[NAMES], [['Vehicle'], ['Pedestrian', 'Cyclist']]], ids=['one_head', 'two_heads'])
def test_device_targets_equal_the_host_route(device, each_head):
    """About 2000 seeded boxes, 250 rows per frame against NUM_MAX_OBJS 150: the device route and target_assign.py."""
    head = small_head(each_head, 150)
    gt = random_gt(2000)
    host = head.assign_targets(torch.from_numpy(gt).clone(), feature_map_size=(H_S, W_S))
    dev = head.assign_targets(torch.from_numpy(gt).to(device), feature_map_size=(H_S, W_S), on_device=True)
    assert sorted(dev) == sorted(list(host) + ['records'])
    for i, names in enumerate(each_head):
        ref = [host[k][i].numpy() for k in ('heatmaps', 'target_boxes', 'inds', 'masks')]
        assert (np.isin(gt[..., 7], [NAMES.index(n) + 1 for n in names]).sum(1) > 150).any() or len(names) < 3      # a frame overflows
        tb = check_targets([dev[k][i] for k in ('heatmaps', 'target_boxes', 'inds', 'masks', 'records')], *ref)
        exact = hr.targets(gt, class_table(names), len(names), H_S, W_S, STRIDE, RANGE_S, VOXEL, 150, 0.1, 2)[1]
        print('log/cos/sin ulps: device %.2f host %.2f' % (hr.ulps32(tb[..., 3:8], exact[..., 3:8]).max(), hr.ulps32(ref[1][..., 3:8], exact[..., 3:8]).max()))
        assert hr.ulps32(tb[..., 3:8], exact[..., 3:8]).max() <= 4 and hr.ulps32(ref[1][..., 3:8], exact[..., 3:8]).max() <= 4


@pytest.mark.gpu
def test_device_targets_188(device, golden_dir):
    from detzero_amd import ops
    from detzero_amd.config import centerpoint_1sweep_cfg
    t = np.load(os.path.join(golden_dir, 'target_golden.npz'))
    cfg = centerpoint_1sweep_cfg()
    out = ops.centerhead_targets(torch.from_numpy(t['gt_boxes']).to(device), [1, 2, 3], 3, 188, 188, 8, cfg.DATA_CONFIG.POINT_CLOUD_RANGE,
                                 [0.1, 0.1, 0.15], 500, 0.1, 2)
    ref = np.zeros((2, 3, 188, 188), np.float32)
    ref[tuple(t['heatmap_nz_idx'].T)] = t['heatmap_nz_val']
    tb = check_targets(out, ref, t['target_boxes'], t['inds'], t['masks'])
    m = t['masks'] > 0
    rows = [np.nonzero(t['gt_boxes'][b, :, 7] > 0)[0] for b in range(2)]
    for b in range(2):
        gt = t['gt_boxes'][b, rows[b]].astype(np.float64)
        exact = np.concatenate([np.log(np.where(gt[:, 3:6] > 0, gt[:, 3:6], 1)), np.cos(gt[:, 6:7]), np.sin(gt[:, 6:7])], axis=1)
        k = m[b, :len(rows[b])]
        assert hr.ulps32(tb[b, :len(rows[b]), 3:8][k], exact[k]).max() <= 4


# ---- losses and gradients ---------------------------------------------------------------------------------------
def run_case(device, g, tag, want_grad=True):
    from detzero_amd import ops
    iou_w = float(g[tag + '_iou_weight'])
    gt = torch.from_numpy(g[tag + '_gt_boxes']).to(device)
    recs, grads = [], []
    for i, names in enumerate(CASES[tag]):
        heat, tb, inds, masks, rec = ops.centerhead_targets(gt, class_table(names), len(names), H_S, W_S, STRIDE, RANGE_S, VOXEL, 16, 0.1, 2)
        head = torch.from_numpy(g['%s_h%d_head' % (tag, i)]).to(device)
        out, grad = ops.centerhead_loss_nosync(head, heat, torch.from_numpy(g['%s_h%d_target_boxes' % (tag, i)]).to(device), inds, masks, rec,
                                               H_S, W_S, WEIGHTS + (iou_w,), STRIDE, RANGE_S, VOXEL, want_grad=want_grad)
        recs.append(out)
        grads.append(grad)
    return recs, grads, iou_w


@pytest.mark.gpu
@pytest.mark.parametrize('tag', sorted(CASES))
def test_losses_equal_the_reference(device, g, tag):
    recs, grads, iou_w = run_case(device, g, tag)
    tb = hr.tb_dict_of([dict(zip(hr.REC_KEYS, r.cpu().numpy().tolist())) for r in recs], iou_w)
    assert sorted(tb) == tb_keys(g, tag)
    bad = []
    for k, v in sorted(tb.items()):
        ref, tol = float(g['%s_tb_%s' % (tag, k)]), scalar_tol(g, tag, k)
        print('%s %-22s device %.9g reference %.9g |d| %.3g tol %.3g' % (tag, k, v, ref, abs(v - ref), tol))
        if not abs(v - ref) <= tol:
            bad.append(k)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('tag', sorted(CASES))
def test_gradients_equal_the_reference(device, g, tag):
    recs, grads, iou_w = run_case(device, g, tag)
    for i, grad in enumerate(grads):
        grad = grad.cpu().numpy().astype(np.float64)
        ref = g['%s_h%d_grad' % (tag, i)].astype(np.float64)
        assert np.isfinite(grad).all() and not grad[ref == 0].any()          # unwritten columns, the clamp, masked slots, the zero residual
        peak = np.abs(ref).max(axis=(0, 1))
        tol = np.maximum(2 * g['%s_h%d_dist_grad' % (tag, i)], 8 * EPS32) * peak
        err = np.abs(grad - ref).max(axis=(0, 1))
        print(tag, i, 'gradient error / tolerance per column', np.array2string(err / np.where(tol > 0, tol, 1), precision=2))
        assert (err <= tol).all()
        if tag == 'c1':                                                      # the two slots of a shared cell add up
            inds, masks = g['c1_h0_inds'], g['c1_h0_masks']
            assert inds[0, 3] == inds[0, 4] and masks[0, 3] and masks[0, 4]
            row = np.abs(grad[0, inds[0, 3], 0:8]) / (2.0 / masks.sum())     # in units of loc_weight / num: the signs add to 0 or 2
            assert np.allclose(row, np.round(row), atol=1e-5) and set(np.round(row)) <= {0.0, 2.0}


@pytest.mark.gpu
def test_autograd_scales_the_fused_gradient(device, g):
    from detzero_amd import ops
    gt = torch.from_numpy(g['c2_gt_boxes']).to(device)
    names = CASES['c2'][1]
    tgt = ops.centerhead_targets(gt, class_table(names), 2, H_S, W_S, STRIDE, RANGE_S, VOXEL, 16, 0.1, 2)
    args = (*tgt, H_S, W_S, WEIGHTS + (1.0,), STRIDE, RANGE_S, VOXEL)
    head = torch.from_numpy(g['c2_h1_head']).to(device)
    rec, grad = ops.centerhead_loss_nosync(head, *args, want_grad=True)
    leaf = head.clone().requires_grad_(True)
    total, rec2 = ops.centerhead_loss(leaf, *args)
    (total * 0.5).backward()
    assert torch.equal(leaf.grad, grad * 0.5) and torch.equal(rec, rec2) and not rec2.requires_grad
    assert float(total.detach()) == float(rec[11].float())
    total3, rec3 = ops.centerhead_loss(head, *args)                          # no grad asked for: no buffer, same bytes
    assert not total3.requires_grad and torch.equal(rec3, rec)


@pytest.mark.gpu
def test_two_runs_give_the_same_bytes(device, g):
    a = run_case(device, g, 'c1')
    b = run_case(device, g, 'c1')
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[1][0], b[1][0])


@pytest.mark.gpu
def test_record_free_call_and_mask(device, g):
    """rec = None makes the call count num_pos / num itself; a heat-map mask of ones changes nothing, a mask that hides frames
    gives the float64 restatement's value."""
    from detzero_amd import ops
    t = {k: g['c1_h0_' + k] for k in ('heatmaps', 'target_boxes', 'inds', 'masks', 'head')}
    d = {k: torch.from_numpy(v).to(device) for k, v in t.items()}
    args = (d['head'], d['heatmaps'], d['target_boxes'], d['inds'], d['masks'])
    tail = (H_S, W_S, WEIGHTS + (1.0,), STRIDE, RANGE_S, VOXEL)
    counts = torch.tensor([int((t['heatmaps'] == 1).sum()), int(t['masks'].sum())], dtype=torch.int32, device=device)
    base = ops.centerhead_loss_nosync(*args, counts, *tail)[0]
    free = ops.centerhead_loss_nosync(*args, None, *tail)[0]
    ones = ops.centerhead_loss_nosync(*args, None, *tail, hm_mask=torch.ones((3, H_S, W_S), device=device))[0]
    assert torch.equal(free, base) and torch.equal(ones, base)
    mask = np.ones((3, H_S, W_S), np.float32)
    mask[1] = 0
    mask[2, :, :7] = 0
    got, grad = ops.centerhead_loss_nosync(*args, None, *tail, hm_mask=torch.from_numpy(mask).to(device), want_grad=True)
    ref, ref_grad = hr.losses(t['head'], t['heatmaps'], t['target_boxes'], t['inds'], t['masks'], WEIGHTS + (1.0,), H_S, W_S, STRIDE, RANGE_S,
                              VOXEL, hm_mask=mask)
    assert abs(float(got[0]) - ref['hm']) <= 1e-9 * abs(ref['hm'])           # both sides sum in float64
    assert np.abs(grad.cpu().numpy()[:, :, 9:] - ref_grad[:, :, 9:]).max() <= 8 * EPS32 * np.abs(ref_grad[:, :, 9:]).max()


@pytest.mark.gpu
def test_loss_modules_on_head_map_views(device, g):
    head = small_head([NAMES], 16)
    hm = torch.from_numpy(g['c1_h0_head']).to(device)
    img = hm.view(3, H_S, W_S, 12)
    heat, tb = torch.from_numpy(g['c1_h0_heatmaps']).to(device), torch.from_numpy(g['c1_h0_target_boxes']).to(device)
    inds, masks = torch.from_numpy(g['c1_h0_inds']).to(device), torch.from_numpy(g['c1_h0_masks']).to(device)
    focal = head.hm_loss_func(img[..., 9:12].permute(0, 3, 1, 2), heat)
    reg = head.reg_loss_func(img[..., 3:6].permute(0, 3, 1, 2), masks, inds, tb[..., 3:6])
    assert abs(float(focal) - float(g['c1_tb_hm_loss_head_0'])) <= scalar_tol(g, 'c1', 'hm_loss_head_0')
    assert focal.dim() == 0 and tuple(reg.shape) == (3,)
    assert abs(float(reg.sum()) - float(g['c1_tb_dim_loss_head_0'])) <= scalar_tol(g, 'c1', 'dim_loss_head_0')


# ---- the module route --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_module_route_host_and_device_targets(device, golden_dir):
    from detzero_amd.centerpoint import synth_detector
    from detzero_amd.lib import DetZeroHipError
    from detzero_amd.synth import VOXEL_SIZE_01
    model, cfg, info = synth_detector(VOXEL_SIZE_01, seed=0)
    model = model.to(device)
    head = model.dense_head
    with pytest.raises(DetZeroHipError):
        head.get_loss()
    torch.manual_seed(3)
    x = torch.randn((2, 512, 188, 188), device=device) * 0.1
    gt = torch.from_numpy(np.load(os.path.join(golden_dir, 'target_golden.npz'))['gt_boxes']).to(device)
    res = {}
    for on_device in (False, True):
        head.targets_on_device = on_device
        out = head({'spatial_features_2d': x, 'gt_boxes': gt.clone(), 'batch_size': 2})
        assert ('records' in head.forward_ret_dict['target_dicts']) == on_device
        loss, tb = model.get_training_loss()[:2]
        loss2, tb2 = head.get_loss()
        assert loss.dim() == 0 and loss.is_cuda and float(loss) == float(loss2) and tb == tb2            # hm is not overwritten
        assert abs(float(loss) - tb['rpn_loss']) <= 4 * float(np.spacing(np.float32(tb['rpn_loss'])))
        res[on_device] = (tb, [d['pred_boxes'].clone() for d in out['final_box_dicts']])
    for k in sorted(res[False][0]):
        a, b = res[False][0][k], res[True][0][k]
        print('%-22s host targets %.9g device targets %.9g' % (k, a, b))
        assert abs(a - b) <= 8 * float(np.spacing(np.float32(abs(a))))
    for a, b in zip(res[False][1], res[True][1]):
        assert torch.equal(a, b)


# ---- refusals ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_launch_nothing(device):
    from detzero_amd import lib as L
    lib = L.load()
    gt = torch.zeros((2, 4, 8), device=device)
    gt10 = torch.zeros((2, 4, 10), device=device)
    heat = torch.full((2, 3, H_S, W_S), 7.0, device=device)
    tb = torch.full((2, 16, 8), 7.0, device=device)
    inds = torch.full((2, 16), 7, dtype=torch.int64, device=device)
    masks = torch.full((2, 16), 7, dtype=torch.int64, device=device)
    rec = torch.full((2,), 7, dtype=torch.int32, device=device)
    table, rng, vox = (ctypes.c_int * 3)(1, 2, 3), (ctypes.c_double * 2)(-9.2, -7.6), (ctypes.c_double * 2)(0.1, 0.1)

    def targets(gt_=gt, cols=8, ncls=3, nmax=16, heat_=heat):
        return lib.dz_centerhead_targets(L.ptr(gt_), 2, 4, cols, table, 3, ncls, H_S, W_S, 8.0, rng, vox, nmax, 0.1, 2, L.ptr(heat_), L.ptr(tb),
                                         L.ptr(inds), L.ptr(masks), L.ptr(rec), L.stream())
    assert targets(heat_=None) == -1 and b'null' in lib.dz_last_error()
    assert targets(ncls=4) == -1 and targets(nmax=0) == -1
    assert targets(gt_=gt10, cols=10) == -4 and b'vel' in lib.dz_last_error()

    head = torch.zeros((2, H_S * W_S, 12), device=device)
    out = torch.full((12,), 7.0, dtype=torch.float64, device=device)
    ws_bytes = lib.dz_centerhead_loss_ws_bytes(2, H_S, W_S)
    ws = torch.zeros((ws_bytes,), dtype=torch.uint8, device=device)
    weights = (ctypes.c_double * 11)(*([1.0] * 11))

    def loss(head_=head, ncls=3, nmax=16, ws_bytes_=ws_bytes):
        return lib.dz_centerhead_loss(L.ptr(head_), L.ptr(heat), L.ptr(tb), L.ptr(inds), L.ptr(masks), L.ptr(rec), None, 2, H_S, W_S, ncls, nmax,
                                      weights, 8.0, rng, vox, L.ptr(out), None, L.ptr(ws), ws_bytes_, L.stream())
    assert loss(head_=None) == -1 and loss(ncls=4) == -1 and loss(nmax=0) == -1 and loss(ws_bytes_=8) == -2
    torch.cuda.synchronize()
    for t in (heat, tb, inds, masks, rec, out):
        assert bool((t == 7).all())
