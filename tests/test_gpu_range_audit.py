"""GPU (MI355X): the range audit end to end on the synthetic detector (20 000-point frame, 0.2 m grid): coverage of every stored
tensor, agreement with the stage calibration, no interference with the results, the hidden-layer saturation the feature exists for,
and graph capture."""
import math
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F16_MAX = 65504.0


def _frame(seed, n):
    from detzero_amd.synth import POINT_CLOUD_RANGE, synth_waymo_frame
    pts = synth_waymo_frame(seed, n)
    r = POINT_CLOUD_RANGE
    keep = (pts[:, 0] >= r[0]) & (pts[:, 0] <= r[3]) & (pts[:, 1] >= r[1]) & (pts[:, 1] <= r[4])
    return pts[keep]


def _detector(device, seed=0):
    from detzero_amd.centerpoint import synth_detector
    from detzero_amd.synth import VOXEL_SIZE_02
    model, cfg, info = synth_detector(VOXEL_SIZE_02, seed)
    return model.to(device), info


def _boxes(pipe, pts):
    o, n = pipe(pts)
    return o.clone(), n.clone()


def _matched(a, b, tol=1e-3):
    """Greedy one-to-one match of boxes9 rows by centre; a pair counts when all 7 box parameters (heading modulo 2 pi) and the score
    agree within tol.  Returns the number of matched rows of `a`."""
    if a.shape[0] == 0 or b.shape[0] == 0:
        return 0
    d = np.abs(a[:, None, :3] - b[None, :, :3]).max(-1)
    used, n = set(), 0
    for i in range(a.shape[0]):
        j = int(np.argmin(d[i]))
        if d[i, j] <= tol and j not in used:
            diff = np.abs(a[i, :7] - b[j, :7])
            diff[6] = min(diff[6], abs(diff[6] - 2 * np.pi))
            if diff.max() <= tol and abs(float(a[i, 7]) - float(b[j, 7])) <= tol:
                used.add(j)
                n += 1
    return n


@pytest.fixture(scope='module')
def det(device):
    model, info = _detector(device)
    pts = torch.from_numpy(_frame(0, 20000)).to(device)
    return model, info, pts


@pytest.fixture(scope='module')
def f32_report(det):
    """The calibration measurement of every stored tensor (computed once, shared, not modified)."""
    from detzero_amd.centerpoint import range_audit
    model, info, pts = det
    return range_audit(model, info, [pts], math='f32')


def test_every_stored_tensor_has_one_record(det, f32_report):
    from detzero_amd.centerpoint import PRESCALE_STAGES, FramePipeline
    model, info, pts = det
    names = [r['name'] for r in f32_report]
    assert len(set(names)) == len(names)
    by = {r['name']: r for r in f32_report}
    sparse = [n for n in names if n.startswith('backbone3d.')]
    bev = [n for n in names if n.startswith('backbone2d.')]
    head = [n for n in names if n.startswith('dense_head.')]
    assert len(sparse) + len(bev) + len(head) == len(names)
    bb3, bb2, hd = model.backbone3d, model.backbone2d, model.dense_head
    n_sparse = sum(1 for m in bb3.modules() if type(m).__name__ in ('SubMConv3d', 'SparseConv3d'))
    assert len(sparse) == n_sparse == 21
    layer_nums = list(bb2.model_cfg.LAYER_NUMS)
    assert len(bev) == sum(layer_nums) + len(layer_nums) + len(bb2.deblocks)
    # the dense stage of FramePipeline: the shared map, one hidden and one final map per head it runs (one head: every DetZero config)
    assert len(head) == 1 + 2 * len(hd.heads_list)
    for r in f32_report:
        assert r['storage'] == 'f32' and r['exp'] == 0 and r['saturated'] == 0 and r['nonfinite'] == 0 and r['headroom_bits'] is None
        assert r['peak'] == r['peak_stored'] and (r['stage'] in PRESCALE_STAGES or r['stage'] is None)
        assert r['elements'] > 0 and (r['peak'] > 0 or r['stage'] is None)
    assert [r['name'] for r in f32_report if r['stage'] is None] == [n for n in head if n.endswith('final')]
    # names follow the module path: each one resolves to the module that writes the tensor
    mods = dict(model.named_modules())
    for n in sparse + bev:
        assert n in mods or n.rsplit('.', 1)[0] in mods, n
    # elements: rows below the level's device count x channels (sparse); the zero-bordered image of the pass x the slice's channels (dense)
    pipe = FramePipeline(model, info, math='f32')
    res = pipe.backbone_stage(pipe.prepare([pts]))
    level_of = {'conv_input': 'x_conv1', 'conv1': 'x_conv1', 'conv2': 'x_conv2', 'conv3': 'x_conv3', 'conv4': 'x_conv4', 'conv_out': 'encoded'}
    for n in sparse:
        stage = level_of[n.split('.')[1]]
        feats, lvl = res[stage]
        assert by[n]['stage'] == stage
        assert by[n]['elements'] == lvl.num_active() * feats.shape[1] and lvl.num_active() > 0, n
    enc = res['encoded'][1]
    h, w = enc.shape[1], enc.shape[2]
    filters, up, strides = list(bb2.model_cfg.NUM_FILTERS), list(bb2.model_cfg.NUM_UPSAMPLE_FILTERS), list(bb2.model_cfg.LAYER_STRIDES)
    xh, xw = h, w
    for li, nl in enumerate(layer_nums):
        xh, xw = (xh + 2 - 3) // strides[li] + 1, (xw + 2 - 3) // strides[li] + 1
        for ci in range(nl + 1):
            r = by['backbone2d.blocks.%d.%d' % (li, 1 + 3 * ci)]
            assert r['stage'] == 'spatial_features_2d' and r['elements'] == (xh + 2) * (xw + 2) * filters[li], r
        r = by['backbone2d.deblocks.%d' % li]
        assert r['stage'] == 'spatial_features_2d' and r['elements'] == (h + 2) * (w + 2) * up[li], r
    c = hd.model_cfg.SHARED_CONV_CHANNEL
    assert by['dense_head.shared_conv']['elements'] == (h + 2) * (w + 2) * c
    hidden = [n for n in head if n.endswith('hidden')]
    assert len(hidden) == 1 and by[hidden[0]]['elements'] % ((h + 2) * (w + 2) * c) == 0 and by[hidden[0]]['stage'] == 'spatial_features_2d'
    final = [n for n in head if n.endswith('final')]
    assert by[final[0]]['elements'] == h * w * 8            # the written columns (at most 4: iou, hm) in a zero-padded 8-column image


def test_peaks_of_the_stage_outputs_equal_the_stage_calibration(det, f32_report):
    from detzero_amd.centerpoint import PRESCALE_STAGES, activation_range, group_peaks
    model, info, pts = det
    rng = activation_range(model, info, [pts])
    by = {r['name']: r for r in f32_report}
    last = {'x_conv1': 'backbone3d.conv1.1.conv2', 'x_conv2': 'backbone3d.conv2.2.conv2', 'x_conv3': 'backbone3d.conv3.2.conv2',
            'x_conv4': 'backbone3d.conv4.2.conv2', 'encoded': 'backbone3d.conv_out'}
    for stage, name in last.items():
        assert by[name]['peak'] == rng[stage], (stage, by[name]['peak'], rng[stage])
    concat = max(r['peak'] for r in f32_report if r['name'].startswith('backbone2d.deblocks.'))
    assert concat == rng['spatial_features_2d']
    assert set(rng) == set(PRESCALE_STAGES)
    # probe='all': the group maxima of the same measurement, never below the stage outputs'
    allp = activation_range(model, info, [pts], probe='all')
    assert allp == group_peaks(f32_report)
    assert all(allp[k] >= rng[k] for k in PRESCALE_STAGES)


@pytest.mark.parametrize('mode', ['f32', 'f16x2'])
def test_recording_changes_no_bit_of_the_results(det, mode):
    from detzero_amd.centerpoint import FramePipeline, RangeAudit, set_math
    model, info, pts = det
    plain = FramePipeline(model, info, math=mode)
    o0, n0 = _boxes(plain, pts)
    audit = RangeAudit()
    audited = FramePipeline(model, info, math=mode, audit=audit)
    o1, n1 = _boxes(audited, pts)
    o2, n2 = _boxes(plain, pts)
    assert int(n0.item()) > 0
    assert torch.equal(n0, n1) and torch.equal(o0, o1) and torch.equal(n0, n2) and torch.equal(o0, o2)
    rep = audit.report()
    assert len(rep) > 21 and all(r['elements'] > 0 for r in rep)
    want = {'f32': 'f32', 'f16x2': 'f16x2'}[mode]
    assert all(r['storage'] == (want if r['stage'] is not None else 'f32') for r in rep)
    audited.check_range()                                   # nothing saturated: passes, and clears the records
    assert all(r['elements'] == 0 and r['peak_stored'] == 0.0 for r in audit.report())
    with pytest.raises(Exception, match='audit'):
        plain.check_range()
    set_math(model, 'f32')


def test_hidden_layer_hotter_than_its_stage_output(device):
    """A hidden layer of the first BEV block scaled up by 2^k (its BatchNorm) and the next convolution scaled down by 2^-k: the fp32
    network is unchanged bit for bit, the stage outputs - all that probe='stages' measures - too, but the hidden tensor now saturates
    its fp16 pairs under the 'stages' exponents.  The audit sees it, check_range() and verify=True refuse it, probe='all' fixes it."""
    from detzero_amd.centerpoint import (PRESCALE_STAGES, FramePipeline, RangeAudit, activation_range, prescale_exponents, range_audit,
                                         select_math, set_math, set_prescale)
    from detzero_amd.lib import DetZeroHipError
    model, info = _detector(device)
    pts = torch.from_numpy(_frame(0, 20000)).to(device)
    blk = model.backbone2d.blocks[0]
    ci = 2                                                   # conv -> BN -> ReLU at Sequential indices 7, 8, 9; the next conv at 10
    conv, bn, nxt = blk[1 + 3 * ci], blk[2 + 3 * ci], blk[4 + 3 * ci]
    assert isinstance(conv, torch.nn.Conv2d) and isinstance(bn, torch.nn.BatchNorm2d) and isinstance(nxt, torch.nn.Conv2d)
    name = 'backbone2d.blocks.0.%d' % (1 + 3 * ci)
    o_ref, n_ref = _boxes(FramePipeline(model, info, math='f32'), pts)
    by = {r['name']: r for r in range_audit(model, info, [pts], math='f32')}
    e_stage = prescale_exponents(activation_range(model, info, [pts]))['spatial_features_2d']
    stored = by[name]['peak'] * 2.0 ** e_stage               # the hidden tensor's stored peak under the 'stages' exponents
    k = max(0, math.ceil(math.log2(4 * F16_MAX / stored)))
    print('hidden tensor %s: peak %.4g, stage exponent %d, stored peak %.4g -> k = %d' % (name, by[name]['peak'], e_stage, stored, k))
    assert 0 < k < 16 and stored * 2.0 ** k >= 4 * F16_MAX > stored * 2.0 ** (k - 1)
    with torch.no_grad():
        bn.weight.mul_(2.0 ** k)
        bn.bias.mul_(2.0 ** k)
        nxt.weight.mul_(2.0 ** -k)
    model.backbone2d.invalidate()
    o_f32, n_f32 = _boxes(FramePipeline(model, info, math='f32'), pts)
    assert torch.equal(n_f32, n_ref) and torch.equal(o_f32, o_ref)          # exact powers of two: the same network
    # ---- calibrated on the stage outputs alone: the hidden tensor clips
    mode, rng = select_math(model, info, [pts], probe='stages')
    exps_stages = dict(model.prescale)
    assert mode == 'f16x2' and exps_stages['spatial_features_2d'] == e_stage
    audit = RangeAudit()
    pipe = FramePipeline(model, info, math='f16x2', audit=audit)
    pipe(pts)
    rep = {r['name']: r for r in audit.report()}
    assert rep[name]['saturated'] > 0 and rep[name]['storage'] == 'f16x2' and rep[name]['exp'] == e_stage, rep[name]
    assert rep[name]['peak_stored'] >= F16_MAX and rep[name]['headroom_bits'] <= 0
    with pytest.raises(DetZeroHipError, match=re.escape(name)):
        pipe.check_range()
    pipe.check_range()                                       # the records were cleared by the failed check
    with pytest.raises(DetZeroHipError, match=re.escape(name)):
        select_math(model, info, [pts], probe='stages', verify=True)
    # ---- calibrated on every stored tensor: it fits
    mode, rng_all = select_math(model, info, [pts], probe='all', verify=True)
    exps_all = dict(model.prescale)
    assert mode == 'f16x2'
    assert all(exps_all[s] <= exps_stages[s] for s in PRESCALE_STAGES), (exps_all, exps_stages)
    assert exps_all['spatial_features_2d'] <= e_stage - 7          # the group's peak is now >= 4 x 65504 x 2^-e_stage, the target 2^11
    pipe(pts)
    rep = audit.report()
    assert all(r['saturated'] == 0 and r['nonfinite'] == 0 for r in rep), [r for r in rep if r['saturated'] or r['nonfinite']]
    assert all(r['headroom_bits'] > 0 for r in rep if r['storage'] == 'f16x2')
    pipe.check_range()
    o16, n16 = _boxes(pipe, pts)
    a, b = o_f32[:int(n_f32.item())].cpu().numpy(), o16[:int(n16.item())].cpu().numpy()
    nm = _matched(a, b, tol=1e-3)
    print('probe=all: exponents %s (stages: %s); %d / %d boxes of the f32 engine matched within 1e-3' % (exps_all, exps_stages, nm, a.shape[0]))
    assert a.shape[0] > 50 and abs(a.shape[0] - b.shape[0]) <= 2 and nm >= a.shape[0] - 2, (a.shape, b.shape, nm)
    set_prescale(model, None)
    set_math(model, 'f32')


def test_audited_pass_in_a_captured_graph(det):
    """After one eager pass (slots, table and staging images exist) an audited pass captures like any other: two replays after a reset
    leave `elements` at exactly twice a single pass's value in every record, peaks and boxes are those of the eager pass."""
    from detzero_amd.centerpoint import FramePipeline, RangeAudit, set_math
    model, info, pts = det
    f1 = torch.from_numpy(_frame(1, 20000)).to(pts.device)
    n = min(pts.shape[0], f1.shape[0])
    static = torch.stack([pts[:n], f1[:n]]).contiguous()
    audit = RangeAudit()
    pipe = FramePipeline(model, info, math='f16x2', audit=audit)
    o1, n1 = _boxes(pipe, static)
    once = audit.report()
    assert once and all(r['elements'] > 0 for r in once)
    torch.cuda.synchronize()
    cap = pipe.capture(static)
    audit.reset()
    cap.replay()
    cap.replay()
    torch.cuda.synchronize()
    twice = audit.report()
    assert [r['name'] for r in twice] == [r['name'] for r in once]
    for a, b in zip(once, twice):
        assert b['elements'] == 2 * a['elements'] and b['peak_stored'] == a['peak_stored'], (a, b)
        assert b['saturated'] == 2 * a['saturated'] == 0 and b['nonfinite'] == 0
    assert int(n1.min().item()) > 0
    assert torch.equal(cap.counts, n1.view(-1)) and torch.equal(cap.boxes, o1.view(cap.boxes.shape))
    set_math(model, 'f32')
