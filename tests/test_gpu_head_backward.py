"""GPU: the model layer of the head's backward (detzero_amd/head_backward.py, CenterHead.loss_backward,
CenterPoint.head_loss_backward) against the head deep-copied to float64 on the CPU (tests/head_backward_ref.py)."""
import copy

import numpy as np
import pytest
import torch

from tests import head_backward_ref as R

BATCH = 2
# the longest chain of nested float32 sums behind any gradient element (the pixels of the weight gradient, the 9 x 384 products of
# the data gradient at the shared map, the 27 of the output layer's) plus the handful of roundings of the BatchNorm formulas
N_CHAIN = BATCH * R.H_S * R.W_S + 9 * 384 + 27 + 16


@pytest.fixture(scope='module', params=sorted(R.EACH_HEAD))
def case(request, device):
    """Head, inputs, the device's gradients and the float64 reference with the device's masks: computed once, shared, not modified."""
    from detzero_amd import head_backward as hb
    from detzero_amd.det_modules import nchw_to_padded_nhwc
    tag = request.param
    seed = R.SEEDS[tag]
    head_cpu = R.small_head32(R.EACH_HEAD[tag], seed)
    x = R.seeded_input(seed, BATCH)
    gh = R.seeded_grad_heads(head_cpu, seed, BATCH)
    head = copy.deepcopy(head_cpu).to(device)
    concat = nchw_to_padded_nhwc(x.to(device))
    gh_dev = [g.to(device) for g in gh]
    state = hb.head_forward_f32(head, concat)
    grads, grad_in = hb.head_gradients(head, concat, gh_dev, input_grad=True)
    h64 = R.module64(head_cpu)
    x64, gh64 = x.double(), [g.double() for g in gh]
    masks = R.masks_from_device(state[0], state[1], 64)
    own = R.module_backward(h64, x64, gh64)[2]
    ref, ref_in, _ = R.module_backward(h64, x64, gh64, masks=masks)
    bound, bound_in = R.graph_backward(h64, x64, gh64, masks, absolute=True)
    return dict(tag=tag, head=head, head_cpu=head_cpu, x=x, concat=concat, gh=gh_dev, state=state, grads=grads, grad_in=grad_in, masks=masks,
                own=own, ref=ref, ref_in=ref_in, bound=bound, bound_in=bound_in)


def small_gt(device, frames=BATCH):
    from tests.test_gpu_head_loss import random_gt
    return torch.from_numpy(random_gt(32 * frames, seed=7, frames=frames)).to(device)


@pytest.mark.gpu
def test_masks_of_the_device_forward(case):
    """The condition of the comparison: the float64 graph's own ReLUs differ from the device's in at most 1 in 10^4 cells."""
    diff, total = R.mask_mismatch(case['masks'], case['own'])
    print('%s: %d of %d mask cells differ' % (case['tag'], diff, total))
    assert diff * 10 ** 4 <= total


@pytest.mark.gpu
def test_every_gradient_within_the_derived_bound(case):
    """|got - ref| <= gamma_N * A elementwise: A = the sum of the absolute values of all monomials (the float64 graph run on absolute
    values with the masks kept), N = N_CHAIN.  Every name of `grads`, and grad_input."""
    params = dict(case['head'].named_parameters())
    assert set(case['grads']) == set(params) == set(case['ref'])
    gam = R.gamma_n(N_CHAIN)
    failed = []
    for name in sorted(case['grads']):
        got = case['grads'][name]
        assert got.shape == params[name].shape and got.dtype == params[name].dtype and got.device == params[name].device, name
        err = (got.cpu().double() - case['ref'][name]).abs()
        lim = gam * case['bound'][name]
        ratio = float((err / lim.clamp_min(1e-300)).max())
        print('%-34s worst |err| / (gamma_N A) = %.4f' % (name, ratio))
        if not bool((err <= lim).all()):
            failed.append((name, ratio))
    err = (case['grad_in'].permute(0, 3, 1, 2).cpu().double() - case['ref_in']).abs()
    lim = gam * case['bound_in']
    print('%-34s worst |err| / (gamma_N A) = %.4f' % ('grad_input', float((err / lim.clamp_min(1e-300)).max())))
    assert case['grad_in'].shape == (BATCH, R.H_S, R.W_S, R.CIN)
    assert not failed and bool((err <= lim).all()), failed
    zname, zc = R.ZERO_GAMMA
    assert float(params[zname + '.weight'][zc].detach()) == 0.0
    assert all(bool(torch.isfinite(g).all()) for g in case['grads'].values())
    assert float(case['grads'][zname + '.weight'][zc].abs()) > 0


@pytest.mark.gpu
def test_names_shapes_and_determinism(case):
    from detzero_amd import head_backward as hb
    head = case['head']
    want = {k: v.shape for k, v in head.state_dict().items() if v.is_floating_point() and 'running_' not in k}
    assert {k: v.shape for k, v in case['grads'].items()} == want
    assert 'shared_conv.0.weight' in want and 'shared_conv.1.bias' in want and 'heads_list.0.center.0.0.weight' in want and 'heads_list.0.hm.1.bias' in want
    again, none = hb.head_gradients(head, case['concat'], case['gh'], state=case['state'])
    assert none is None
    for name, g in case['grads'].items():
        assert torch.equal(again[name], g), name
    # the module's inference mode does not reach the backward: the masks are those of the fp32 forward
    head.set_math('f16x2')
    try:
        other, _ = hb.head_gradients(head, case['concat'], case['gh'])
    finally:
        head.set_math('f32')
    for name, g in case['grads'].items():
        assert torch.equal(other[name], g), name


@pytest.mark.gpu
def test_frame_groups_add_up_in_group_order(case, monkeypatch):
    """A batch cut into frame groups (the 2 GiB rule, here forced to one frame per group) gives the groups' sums."""
    from detzero_amd import head_backward as hb
    head = case['head']
    parts = [hb.head_gradients(head, case['concat'][b:b + 1], [g[b:b + 1] for g in case['gh']], input_grad=True) for b in range(BATCH)]
    monkeypatch.setattr(hb, 'frames_per_group', lambda *a: 1)
    grads, grad_in = hb.head_gradients(head, case['concat'], case['gh'], input_grad=True)
    for name in grads:
        assert torch.equal(grads[name], parts[0][0][name] + parts[1][0][name]), name
    assert torch.equal(grad_in, torch.cat([p[1] for p in parts], dim=0))


def head_state(head):
    return {k: v.clone() for k, v in head.state_dict().items()}


@pytest.mark.gpu
def test_loss_backward_equals_get_loss_and_accumulates(case, device):
    from detzero_amd import head_backward as hb
    from detzero_amd import ops
    from detzero_amd.head_loss import device_targets, loss_weights
    head = copy.deepcopy(case['head'])
    gt = small_gt(device)
    batch = {'spatial_features_2d': case['x'].to(device), 'gt_boxes': gt, 'batch_size': BATCH}
    head.targets_on_device = True
    before = head(dict(batch))
    maps_before = [d['hm'].clone() for d in head.forward_ret_dict['pred_dicts']]
    loss_fwd, tb_fwd = head.get_loss()
    boxes_before = [d['pred_boxes'].clone() for d in before['final_box_dicts']]
    state_before = head_state(head)

    loss, tb = head.loss_backward(dict(batch))
    assert loss.dim() == 0 and loss.is_cuda and float(loss) == float(loss_fwd) and tb == tb_fwd
    assert not head.training and all(p.grad is not None for p in head.parameters())
    # .grad is head_gradients of the loss's own gradient
    state = case['state']
    targets = device_targets(head, gt, (R.H_S, R.W_S))
    grad_heads = []
    for i, hm in enumerate(state[2]):
        hm = hm.clone().requires_grad_(True)
        total, _ = ops.centerhead_loss(hm, targets['heatmaps'][i], targets['target_boxes'][i], targets['inds'][i], targets['masks'][i],
                                       targets['records'][i], R.H_S, R.W_S, loss_weights(head.model_cfg), head.feature_map_stride,
                                       head.point_cloud_range, head.voxel_size)
        total.backward()
        grad_heads.append(hm.grad)
    want, _ = hb.head_gradients(head, case['concat'], grad_heads)
    first = {}
    for name, prm in head.named_parameters():
        assert torch.equal(prm.grad, want[name]), name
        first[name] = prm.grad.clone()
    # a second call accumulates
    head.loss_backward(dict(batch))
    for name, prm in head.named_parameters():
        assert torch.equal(prm.grad, first[name] + first[name]), name
    # forward and get_loss give the same bytes before and after (no optimiser step was taken)
    after = head(dict(batch))
    for a, b in zip(maps_before, [d['hm'] for d in head.forward_ret_dict['pred_dicts']]):
        assert torch.equal(a, b)
    for a, b in zip(boxes_before, [d['pred_boxes'] for d in after['final_box_dicts']]):
        assert torch.equal(a, b)
    loss_again, tb_again = head.get_loss()
    assert float(loss_again) == float(loss_fwd) and tb_again == tb_fwd
    for k, v in head_state(head).items():
        assert torch.equal(v, state_before[k]), k


@pytest.mark.gpu
def test_sgd_step_lowers_the_loss(case, device):
    """Plain SGD on dense_head.parameters() with lr such that the predicted first-order decrease lr * |g|^2 is 1 % of the loss, then
    invalidate(): the device loss on the same batch drops, forward's head maps change, statistics and mode do not."""
    head = copy.deepcopy(case['head'])
    batch = {'spatial_features_2d': case['x'].to(device), 'gt_boxes': small_gt(device), 'batch_size': BATCH}
    head(dict(batch))
    maps0 = [d['hm'].clone() for d in head.forward_ret_dict['pred_dicts']]
    stats0 = {k: v.clone() for k, v in head.state_dict().items() if 'running_' in k or 'num_batches' in k}
    loss0, _ = head.loss_backward(dict(batch))
    g2 = float(sum((p.grad.double() ** 2).sum() for p in head.parameters()))
    lr = 0.01 * float(loss0) / g2
    with torch.no_grad():
        for p in head.parameters():
            p -= lr * p.grad
            p.grad = None
    head.invalidate()
    loss1, _ = head.loss_backward(dict(batch))
    print('%s: loss %.9g -> %.9g (lr %.3g, predicted decrease %.3g)' % (case['tag'], float(loss0), float(loss1), lr, 0.01 * float(loss0)))
    assert float(loss1) < float(loss0)
    head(dict(batch))
    assert any(not torch.equal(a, d['hm']) for a, d in zip(maps0, head.forward_ret_dict['pred_dicts']))
    assert not head.training
    for k, v in head.state_dict().items():
        if k in stats0:
            assert torch.equal(v, stats0[k]), k


@pytest.mark.gpu
def test_refusals(case, device):
    from detzero_amd.centerpoint import synth_detector
    from detzero_amd.lib import DetZeroHipError
    head = copy.deepcopy(case['head'])
    x = case['x'].to(device)
    gt10 = torch.zeros((BATCH, 4, 10), dtype=torch.float32, device=device)
    with pytest.raises(DetZeroHipError, match='`vel` head'):
        head.loss_backward({'spatial_features_2d': x, 'gt_boxes': gt10, 'batch_size': BATCH})
    with pytest.raises(DetZeroHipError, match='gt_boxes'):
        head.loss_backward({'spatial_features_2d': x, 'batch_size': BATCH})
    assert all(p.grad is None for p in head.parameters())
    head.train()
    with pytest.raises(DetZeroHipError, match='eval'):
        head.loss_backward({'spatial_features_2d': x, 'gt_boxes': small_gt(device), 'batch_size': BATCH})
    if case['tag'] == 'one_head':
        model, _, _ = synth_detector((0.2, 0.2, 0.15), seed=0, second_stage=True)
        with pytest.raises(DetZeroHipError, match='ROI_HEAD'):
            model.head_loss_backward({})
        model.train()
        with pytest.raises(DetZeroHipError, match='eval'):
            model.head_loss_backward({})


@pytest.mark.gpu
def test_detector_head_loss_backward(device):
    """CenterPoint.head_loss_backward: the frozen stages as in forward, then the head's loss_backward - the same bytes as running the
    stages by hand; only dense_head's parameters receive a gradient."""
    from detzero_amd.data_processor import DataProcessor
    from detzero_amd.synth import VOXEL_SIZE_02
    from tests.util import make_model, masked_frame
    model, cfg, info = make_model(VOXEL_SIZE_02, seed=0)
    model = model.to(device)
    pts = masked_frame(0, 20000)
    dp = DataProcessor(cfg.DATA_CONFIG.DATA_PROCESSOR, info.point_cloud_range, training=False, num_point_features=5)
    d = dp.forward({'points': torch.from_numpy(pts).to(device), 'use_lead_xyz': True})
    coords = torch.cat([d['voxel_coords'].new_zeros((d['voxel_coords'].shape[0], 1)), d['voxel_coords']], 1)
    gt = torch.tensor([[[10.0, 5.0, 0.5, 4.6, 2.0, 1.7, 0.3, 1.0], [-20.0, 12.0, 0.4, 0.9, 0.8, 1.75, 1.0, 2.0], [30.0, -25.0, 0.6, 1.8, 0.8, 1.6, -2.0, 3.0],
                        [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]], dtype=torch.float32, device=device)

    def batch():
        return {'voxels': d['voxels'], 'voxel_coords': coords.float(), 'voxel_num_points': d['voxel_num_points'].float(), 'batch_size': 1,
                'gt_boxes': gt.clone()}

    loss, tb, disp = model.head_loss_backward(batch())
    assert loss.dim() == 0 and bool(torch.isfinite(loss)) and disp == {} and abs(float(loss) - tb['rpn_loss']) <= 1e-5 * abs(tb['rpn_loss'])
    head_ids = {id(p) for p in model.dense_head.parameters()}
    for p in model.parameters():
        assert (p.grad is not None) == (id(p) in head_ids)
    got = {k: p.grad.clone() for k, p in model.dense_head.named_parameters()}
    assert all(bool(torch.isfinite(g).all()) for g in got.values()) and any(float(g.abs().max()) > 0 for g in got.values())
    model.dense_head.zero_grad(set_to_none=True)
    bd = batch()
    for mod in (model.vfe, model.backbone3d, model.map_to_bev, model.backbone2d):
        bd = mod(bd)
    loss2, tb2 = model.dense_head.loss_backward(bd)
    assert float(loss2) == float(loss) and tb2 == tb
    for k, p in model.dense_head.named_parameters():
        assert torch.equal(p.grad, got[k]), k
    assert not model.training
