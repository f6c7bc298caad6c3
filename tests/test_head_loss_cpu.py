"""CPU: the CenterHead loss layer's restatement against the reference's own classes (tests/golden/head_loss_golden.npz,
gen_head_loss_golden.py), CenterHead.get_loss with a faked ops layer, the config values and the new C ABI names."""
import os
import re

import numpy as np
import pytest
import torch

from tests import head_loss_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['Vehicle', 'Pedestrian', 'Cyclist']
CASES = {'c1': [NAMES], 'c2': [['Vehicle'], ['Pedestrian', 'Cyclist']], 'c3': [NAMES], 'c4': [NAMES]}
WEIGHTS = (1.0, 2.0) + (1.0,) * 8
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope='module')
def g(golden_dir):
    return np.load(os.path.join(golden_dir, 'head_loss_golden.npz'))


def scalar_tol(g, tag, key):
    """2 x the reference's own float32-against-float64 distance of the scalar, floor 8 float32 ulps."""
    v = float(g['%s_tb_%s' % (tag, key)])
    return max(2 * float(g['%s_dist_%s' % (tag, key)]) * (abs(v) if v != 0 else 1.0), 8 * float(np.spacing(np.float32(abs(v)))))


def tb_keys(g, tag):
    return sorted(k[len(tag) + 4:] for k in g.files if k.startswith(tag + '_tb_'))


def class_table(names):
    return [names.index(n) + 1 if n in names else 0 for n in NAMES]


@pytest.mark.parametrize('tag', sorted(CASES))
def test_restated_targets_equal_the_reference(g, tag):
    w, h, nmax, nb, stride = [int(v) for v in g['geometry']]
    for i, names in enumerate(CASES[tag]):
        heat, tb, inds, masks = hr.targets(g[tag + '_gt_boxes'], class_table(names), len(names), h, w, stride, g['range'], g['voxel'], nmax, 0.1, 2)
        ref_tb = g['%s_h%d_target_boxes' % (tag, i)]
        np.testing.assert_array_equal(inds, g['%s_h%d_inds' % (tag, i)])
        np.testing.assert_array_equal(masks, g['%s_h%d_masks' % (tag, i)])
        np.testing.assert_array_equal(heat, g['%s_h%d_heatmaps' % (tag, i)])
        np.testing.assert_array_equal(tb[..., 0:3].astype(np.float32), ref_tb[..., 0:3])
        assert hr.ulps32(ref_tb[..., 3:8], tb[..., 3:8]).max() <= 4          # the reference's float32 log / cos / sin


def test_fixture_holds_the_cases_the_issue_names(g):
    w, h, nmax, nb, stride = [int(v) for v in g['geometry']]
    assert (w, h, nmax, nb) == (23, 19, 16, 3)
    inds, masks, heat, gt = g['c1_h0_inds'], g['c1_h0_masks'], g['c1_h0_heatmaps'], g['c1_gt_boxes']
    assert inds[0, 0] == h * w - 1 and masks[0, 0] == 1                      # clamped into the last cell
    assert (heat[0, 0] > 0).all()                                            # the huge box covers its whole plane, clipped on all sides
    assert masks[0, 2] == 0 and gt[0, 2, 3] == 0 and masks[0, 3] == 1        # dx = 0 leaves its slot empty, the next slot is not moved up
    assert (gt[0, :, 7] == 0).any() and (gt[1, :, 7] > 0).sum() > nmax and masks[1].sum() == nmax
    assert inds[0, 3] == inds[0, 4] and inds[0, 5] == inds[0, 6]             # shared cells: one class, two classes
    assert (heat == 1).sum() < masks.sum()                                   # num_pos counts the shared cell once
    head = g['c1_h0_head']
    assert (np.abs(head[:, :, 9:12]) > 9.3).any()
    hit = [(b, k) for b in range(nb) for k in range(nmax) if masks[b, k] and np.array_equal(head[b, inds[b, k], 0:8], g['c1_h0_target_boxes'][b, k])]
    assert len(hit) == 1 and not g['c1_h0_grad'][hit[0][0], inds[hit[0]], 0:8].any()
    assert np.isnan(g['c2_h0_head'][:, :, 10:]).all() and np.isnan(g['c2_h1_head'][:, :, 11]).all() and not g['c2_h0_grad'][:, :, 10:].any()
    assert g['c3_h0_masks'].sum() == 0 and not (g['c3_h0_heatmaps'] == 1).any()
    assert 'c4_tb_iou_loss_head_0' not in g.files and not g['c4_h0_grad'][:, :, 8].any()


@pytest.mark.parametrize('tag', sorted(CASES))
def test_restated_losses_equal_the_reference(g, tag):
    w, h, nmax, nb, stride = [int(v) for v in g['geometry']]
    iou_w = float(g[tag + '_iou_weight'])
    recs = []
    for i in range(len(CASES[tag])):
        t = {k: g['%s_h%d_%s' % (tag, i, k)] for k in ('heatmaps', 'target_boxes', 'inds', 'masks')}
        rec, grad = hr.losses(np.nan_to_num(g['%s_h%d_head' % (tag, i)]), t['heatmaps'], t['target_boxes'], t['inds'], t['masks'],
                              WEIGHTS + (iou_w,), h, w, stride, g['range'], g['voxel'])
        recs.append(rec)
        ref = g['%s_h%d_grad' % (tag, i)].astype(np.float64)
        assert not grad[ref == 0].any()                                      # the zeros are exact: clamp, masked slots, unwritten columns
        peak = np.abs(ref).max(axis=(0, 1))
        tol = np.maximum(2 * g['%s_h%d_dist_grad' % (tag, i)], 8 * EPS32) * peak
        assert (np.abs(grad - ref).max(axis=(0, 1)) <= tol).all()
    tb = hr.tb_dict_of(recs, iou_w)
    assert sorted(tb) == tb_keys(g, tag)
    for k, v in tb.items():
        assert abs(v - float(g['%s_tb_%s' % (tag, k)])) <= scalar_tol(g, tag, k), k


def test_host_side_log_cos_sin_are_within_4_ulps():
    """The bound the GPU test puts on both sides' log / cos / sin columns holds for the host route on the inputs it uses."""
    from tests.test_gpu_head_loss import random_gt
    gt = random_gt(2000)
    x = torch.from_numpy(gt.reshape(-1, 8))
    x = x[(x[:, 3] > 0) & (x[:, 4] > 0)]
    host = torch.cat([x[:, 3:6].log(), x[:, 6:7].cos(), x[:, 6:7].sin()], dim=1).numpy()
    d = x.numpy().astype(np.float64)
    exact = np.concatenate([np.log(d[:, 3:6]), np.cos(d[:, 6:7]), np.sin(d[:, 6:7])], axis=1)
    assert hr.ulps32(host, exact).max() <= 4


class _FakeOps:
    """Stands in for detzero_amd.ops in head_loss.py: records the calls, returns host tensors."""

    def __init__(self):
        self.calls = []

    def centerhead_loss(self, head, heat, tb, inds, masks, rec, h, w, weights, stride, pc_range, voxel, hm_mask=None):
        self.calls.append((tuple(head.shape), tuple(heat.shape), rec, h, w, tuple(weights)))
        out = torch.arange(12, dtype=torch.float64) + 100 * len(self.calls)
        return out[11].float(), out


def _head(each_head=None):
    from detzero_amd.config import centerpoint_1sweep_cfg
    from detzero_amd.det_modules import CenterHead
    cfg = centerpoint_1sweep_cfg()
    if each_head is not None:
        cfg.MODEL.DENSE_HEAD.CLASS_NAMES_EACH_HEAD = each_head
    return CenterHead(cfg.MODEL.DENSE_HEAD, 8, 3, NAMES, np.array([184, 152, 40]), [-9.2, -7.6, -2, 9.2, 7.6, 4], [0.1, 0.1, 0.15])


def test_get_loss_keys_and_errors(monkeypatch):
    from detzero_amd import head_loss
    from detzero_amd.lib import DetZeroHipError
    head = _head(CASES['c2'])
    assert isinstance(head.hm_loss_func, head_loss.FocalLossCenterNet) and isinstance(head.reg_loss_func, head_loss.RegLossCenterNet)
    assert not [k for k in head.state_dict() if 'loss_func' in k] and head.targets_on_device is False
    with pytest.raises(DetZeroHipError, match='pred_dicts'):
        head.get_loss()
    fake = _FakeOps()
    monkeypatch.setattr(head_loss, 'ops', fake)
    monkeypatch.setattr(head_loss, 'head_map_of', lambda view: (view, 9, 19, 23))
    maps = [torch.zeros((3, 19 * 23, 12)) for _ in range(2)]
    head.forward_ret_dict = {'pred_dicts': [{'hm': m} for m in maps]}
    with pytest.raises(DetZeroHipError, match='target_dicts'):
        head.get_loss()
    head.forward_ret_dict['target_dicts'] = {
        'heatmaps': [torch.zeros((3, n, 19, 23)) for n in (1, 2)], 'target_boxes': [torch.zeros((3, 500, 8))] * 2,
        'inds': [torch.zeros((3, 500), dtype=torch.int64)] * 2, 'masks': [torch.zeros((3, 500), dtype=torch.int64)] * 2}
    loss, tb = head.get_loss({'kept': 1.0})
    keys = ['%s_loss_head_%d' % (n, i) for i in range(2) for n in ('hm', 'loc', 'center', 'center_z', 'dim', 'rot', 'iou')]
    assert sorted(tb) == sorted(keys + ['rpn_loss', 'kept'])
    assert loss.dim() == 0 and float(loss) == 111.0 + 211.0 and tb['rpn_loss'] == 322.0
    assert tb['center_loss_head_1'] == 201.0 + 202.0 and tb['iou_loss_head_0'] == 110.0 and tb['hm_loss_head_1'] == 200.0
    assert [c[1][1] for c in fake.calls] == [1, 2] and fake.calls[0][2] is None            # host targets carry no record
    assert fake.calls[0][5] == (1.0, 2.0) + (1.0,) * 8 + (1.0,)
    del head.model_cfg['LOSS_CONFIG']
    with pytest.raises(DetZeroHipError, match='LOSS_CONFIG'):
        head.get_loss()


def test_loss_config_in_builtin_configs():
    from detzero_amd import config
    for make in (config.centerpoint_1sweep_cfg, config.centerpoint_3sweeps_cfg, config.centerpoint_pdv_cfg):
        lw = make().MODEL.DENSE_HEAD.LOSS_CONFIG.LOSS_WEIGHTS
        assert lw['cls_weight'] == 1.0 and lw['loc_weight'] == 2.0 and list(lw['code_weights']) == [1.0] * 8


def test_new_symbols_in_header_and_table():
    from detzero_amd import lib as L
    header = open(os.path.join(ROOT, 'include', 'detzero_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in ('dz_centerhead_targets', 'dz_centerhead_loss', 'dz_centerhead_loss_ws_bytes'):
        assert name + '(' in header and name in L.exported_symbols()
    assert 'dz_centerhead_loss' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_training_loss_refuses_two_stage():
    from detzero_amd.centerpoint import SyntheticDatasetInfo, build_network
    from detzero_amd.config import centerpoint_pdv_cfg
    from detzero_amd.lib import DetZeroHipError
    cfg = centerpoint_pdv_cfg()
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), SyntheticDatasetInfo(cfg))
    with pytest.raises(DetZeroHipError, match='PDV'):
        model.get_training_loss()


def test_kernels_have_no_scratch(tmp_path):
    """The six kernels of csrc/head_loss.hip from the compiler's resource report: no scratch, no spilled register, static LDS
    within the 64 KiB a launch gets without asking."""
    import subprocess
    src = os.path.join(ROOT, 'detzero_amd', 'csrc', 'head_loss.hip')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-c', src, '-o', str(tmp_path / 'hl.o'), '-Rpass-analysis=kernel-resource-usage']
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    kernels, cur = [], None
    for line in run.stderr.splitlines():
        m = re.search(r'remark: +([A-Za-z \[\]/]+): +(\S+)', line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == 'Function Name':
            cur = {'name': v}
            kernels.append(cur)
        elif cur is not None:
            cur[k] = v
    names = [k['name'] for k in kernels]
    for want in ('k_cht_clear', 'k_cht_assign', 'k_chl_count', 'k_chl_dense', 'k_chl_slots', 'k_chl_final'):
        assert sum(want in n for n in names) == 1, (want, names)
    for k in kernels:
        assert int(k['ScratchSize [bytes/lane]']) == 0 and int(k['VGPRs Spill']) == 0, k
        assert int(k['LDS Size [bytes/block]']) <= 64 * 1024, k
