"""GPU (MI355X): the opt-in bf16x3 engine of the f32 mode's dense 3x3 layers (centerpoint.set_dense_engine, csrc/conv3x3_t.hip)
through the detector - which layers it takes, its error against float64 next to the f32 engine's, boxes, graph capture, and that
switching it on and off leaves the default path's bits alone.  The small synthetic detector of tests/test_gpu_e2e.py (20k-point frame,
0.2 m voxels, the full CenterPoint-1stage network) in f32 mode.

Error budget: the project's own rule (tests/test_gpu_full_parity.py::test_error_budget_against_float64) applied to the dense stage - the
yardstick is the stage evaluated in FLOAT64 from the BEV image the f32 engine's sparse backbone produced (same fp32 weights), every
error in units of the stage's standard deviation, and the three-limb engine may not exceed TWICE the f32 engine's error.
"""

import pytest
import torch

from detzero_amd import ops
from detzero_amd.synth import VOXEL_SIZE_02
from tests.util import make_model, masked_frame, match_boxes

pytestmark = pytest.mark.gpu
BOX_TOL_F32 = 1e-3              # tests/test_gpu_full_parity.py: BOX_TOL['f32']


@pytest.fixture(scope='module')
def small(device):
    model, cfg, info = make_model(VOXEL_SIZE_02, seed=0)
    pts = masked_frame(0, 20000)
    return model.to(device), cfg, info, pts


@pytest.fixture()
def engine(small):
    """set_dense_engine on the module's model, back to the default afterwards whatever the test did."""
    from detzero_amd.centerpoint import set_dense_engine, set_math
    model = small[0]
    set_math(model, 'f32')
    yield lambda name: set_dense_engine(model, name)
    set_dense_engine(model, 'mfma32')


def _bev(small, device):
    """The module path up to the BEV image (f32 sparse backbone; the dense engine plays no part in it)."""
    from tests.test_gpu_e2e import _batch_dict
    model, cfg, info, pts = small
    bd = _batch_dict(model, cfg, info, pts, device)
    return model.map_to_bev(model.backbone3d(model.vfe(bd)))


def _dense_stage(small, bd):
    """backbone2d + dense_head of the module path on a copy of the batch dict -> {'spatial_features_2d', 'head/<branch>'} (NCHW)."""
    model = small[0]
    bd = model.dense_head(model.backbone2d(dict(bd)))
    out = {'spatial_features_2d': bd['spatial_features_2d'].clone()}
    for k, v in model.dense_head.forward_ret_dict['pred_dicts'][0].items():
        out['head/' + k] = v.clone()
    return out


# ---- float64 restatement of the dense stage on the device (torch.nn.functional has no float64 convolution there): per-tap matmuls
def _conv64(x, w, stride=1, pad=1):
    """x (N, C, H, W), w (Co, C, kh, kw) float64 -> (N, Co, Ho, Wo): torch.nn.functional.conv2d(x, w, stride=stride, padding=pad)."""
    x = torch.nn.functional.pad(x, (pad, pad, pad, pad)).permute(0, 2, 3, 1)
    n, hp, wp, c = x.shape
    kh, kw = w.shape[2], w.shape[3]
    ho, wo = (hp - kh) // stride + 1, (wp - kw) // stride + 1
    acc = torch.zeros((n * ho * wo, w.shape[0]), dtype=torch.float64, device=x.device)
    for ky in range(kh):
        for kx in range(kw):
            xt = x[:, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride, :].reshape(-1, c)
            acc.addmm_(xt, w[:, :, ky, kx].t())
    return acc.view(n, ho, wo, -1).permute(0, 3, 1, 2)


def _deconv64(x, w, s):
    """ConvTranspose2d with kernel == stride == s: w (C, Co, s, s)."""
    n, c, h, wd = x.shape
    xt = x.permute(0, 2, 3, 1).reshape(-1, c)
    out = torch.zeros((n, w.shape[1], h * s, wd * s), dtype=torch.float64, device=x.device)
    for dy in range(s):
        for dx in range(s):
            out[:, :, dy::s, dx::s] = (xt @ w[:, :, dy, dx]).view(n, h, wd, -1).permute(0, 3, 1, 2)
    return out


def _bn64(x, sd, p, eps):
    scale = sd[p + '.weight'] / torch.sqrt(sd[p + '.running_var'] + eps)
    return (x - sd[p + '.running_mean'].view(1, -1, 1, 1)) * scale.view(1, -1, 1, 1) + sd[p + '.bias'].view(1, -1, 1, 1)


def _dense_stage_f64(model, bev):
    """oracle/dense.py's bev_backbone_forward + center_head_forward, float64 on the device, from the model's own modules."""
    sd = {k: v.detach().double() for k, v in model.state_dict().items() if v.is_floating_point()}
    b2 = model.backbone2d
    x, ups = bev.double(), []
    for lvl, blk in enumerate(b2.blocks):
        p = 'backbone2d.blocks.%d.' % lvl
        x = torch.relu(_bn64(_conv64(x, sd[p + '1.weight'], stride=b2.layer_strides[lvl]), sd, p + '2', 1e-3))
        for k in range((len(blk) - 4) // 3):
            x = torch.relu(_bn64(_conv64(x, sd[p + '%d.weight' % (4 + 3 * k)]), sd, p + '%d' % (5 + 3 * k), 1e-3))
        d = 'backbone2d.deblocks.%d.' % lvl
        ups.append(torch.relu(_bn64(_deconv64(x, sd[d + '0.weight'], b2.upsample_strides[lvl]), sd, d + '1', 1e-3)))
    f2d = torch.cat(ups, dim=1)
    out = {'spatial_features_2d': f2d}
    bias = lambda k: sd[k].view(1, -1, 1, 1) if k in sd else 0.0          # noqa: E731  (the hidden layers' bias is optional, as in the oracle)
    p = 'dense_head.shared_conv.'
    x = torch.relu(_bn64(_conv64(f2d, sd[p + '0.weight']) + bias(p + '0.bias'), sd, p + '1', 1e-5))
    for name in model.dense_head.head_names:
        h = 'dense_head.heads_list.0.%s.' % name
        y = torch.relu(_bn64(_conv64(x, sd[h + '0.0.weight']) + bias(h + '0.0.bias'), sd, h + '0.1', 1e-5))
        out['head/' + name] = _conv64(y, sd[h + '1.weight']) + sd[h + '1.bias'].view(1, -1, 1, 1)
    return out


def test_float64_restatement_is_the_oracle(small, device):
    """The yardstick above against oracle/dense.py (torch fp32 on the CPU) on a crop of the BEV image: the same network up to fp32 noise."""
    from oracle import dense
    model = small[0]
    bev = _bev(small, device)['spatial_features'][:, :, :24, :32].contiguous()
    got = _dense_stage_f64(model, bev)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    f2d = dense.bev_backbone_forward(sd, bev.cpu())
    pred = dense.center_head_forward(sd, f2d)
    torch.testing.assert_close(got['spatial_features_2d'].float().cpu(), f2d, rtol=1e-4, atol=1e-4)
    for k, v in pred.items():
        torch.testing.assert_close(got['head/' + k].float().cpu(), v, rtol=1e-4, atol=1e-4)


def test_routing(small, device, engine, monkeypatch):
    """With the engine on, LaunchProfiler lists k_conv3x3_t<...> for exactly the layers dz_conv3x3_limb3_supported takes and
    k_conv2d<...> for the rest (strided layers, deblocks, the grouped output layer); with the default engine no k_conv3x3_t at all."""
    bd = _bev(small, device)
    calls = []
    real = ops.conv2d

    def spy(desc, **kw):
        calls.append((dict(desc), kw.get('f32_engine')))
        return real(desc, **kw)
    monkeypatch.setattr(ops, 'conv2d', spy)

    def profiled():
        del calls[:]
        ops.PROFILER = ops.LaunchProfiler()
        try:
            _dense_stage(small, bd)
            names = [r[0] for r in ops.PROFILER.records]
            return list(calls), names, ops.PROFILER.summary()
        finally:
            ops.PROFILER = None
    c0, n0, s0 = profiled()
    assert len(c0) == len(n0) > 0 and all(n.startswith('k_conv2d<') for n in n0) and all(e is None for _, e in c0)
    engine('bf16x3')
    c1, n1, s1 = profiled()
    assert len(c1) == len(c0) == len(n1)
    taken = 0
    for (desc, eng), name, name0 in zip(c1, n1, n0):
        ok = ops.conv3x3_limb3_supported(desc)
        plain = desc['kh'] == 3 and desc['stride'] == 1 and desc['groups'] == 1
        assert ok == plain, desc                                   # every plain 3 x 3 stride-1 layer of this network, and nothing else
        assert (eng == 'bf16x3') == ok
        assert name.startswith('k_conv3x3_t<' if ok else 'k_conv2d<') and (ok or name == name0), (name, name0, desc)
        taken += ok
    # 6 + 5 stride-1 backbone layers, the head's shared and hidden convolutions | 1 strided layer, 1 + 4 deblock launches, the output layer
    assert taken == 13 and len(c1) - taken == 7, (taken, len(c1))
    # same algorithmic flop / byte counts under the new names
    tot = lambda s, key: sum(v[key] for v in s.values())          # noqa: E731
    assert tot(s0, 'launches') == tot(s1, 'launches')
    for key in ('flops', 'bytes'):                                 # (summed per variant name: equal up to the order of the additions)
        assert abs(tot(s0, key) - tot(s1, key)) <= 1e-9 * tot(s0, key), key
    print('  bf16x3 routing: ' + ', '.join('%s x%d' % (k, v['launches']) for k, v in sorted(s1.items())))
    engine('mfma32')
    c2, n2, _ = profiled()
    assert n2 == n0


def test_error_budget_against_float64(small, device, engine):
    model = small[0]
    bd = _bev(small, device)
    yard = _dense_stage_f64(model, bd['spatial_features'])
    f32 = _dense_stage(small, bd)
    engine('bf16x3')
    l3 = _dense_stage(small, bd)
    engine('mfma32')
    err = lambda t, k: float((t[k].double() - yard[k]).abs().max()) / float(yard[k].std())      # noqa: E731
    print('\n  dense stage, max |error| against float64, in units of the stage standard deviation')
    print('  %-22s %12s %12s %12s' % ('stage', 'f32 engine', 'bf16x3', 'bf16x3/f32'))
    for k in yard:
        e32, e3 = err(f32, k), err(l3, k)
        print('  %-22s %12.2e %12.2e %12.2f' % (k, e32, e3, e3 / max(e32, 1e-30)))
    for k in yard:
        e32, e3 = err(f32, k), err(l3, k)
        assert e3 <= 2.0 * e32, (k, e3, e32)


def _boxes(small, device):
    from detzero_amd.centerpoint import FramePipeline
    model, cfg, info, pts = small
    pipe = FramePipeline(model, info, math='f32')
    out, d_n = pipe(torch.from_numpy(pts).to(device))
    torch.cuda.synchronize()
    return pipe, out.clone(), int(d_n.item())


def test_boxes_and_default_path_bits(small, device, engine):
    """FramePipeline boxes with the engine on against the default: same count, every box within 1e-3; and the default engine's
    output is bit-identical before and after the engine was switched on and off again."""
    _, ref, n = _boxes(small, device)
    assert n > 20
    engine('bf16x3')
    _, got, m = _boxes(small, device)
    engine('mfma32')
    _, again, n2 = _boxes(small, device)
    assert n2 == n and torch.equal(again[:n], ref[:n])
    a, b = ref[:n].cpu().numpy(), got[:m].cpu().numpy()
    nm, worst = match_boxes(a[:, :7], a[:, 7], b[:, :7], b[:, 7], tol=BOX_TOL_F32)
    print('  boxes: %d default / %d bf16x3, %d matched within %.0e (worst %.2e)' % (n, m, nm, BOX_TOL_F32, worst))
    assert m == n and nm == n, (n, m, nm, worst)


def test_captured_pass_replays_to_the_eager_bits(small, device, engine):
    engine('bf16x3')
    model, cfg, info, pts = small
    pipe, ref_out, n = _boxes(small, device)
    static_in = torch.from_numpy(pts).to(device)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):
            pipe(static_in)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_out, g_n = pipe(static_in)
    g.replay()
    torch.cuda.synchronize()
    assert int(g_n.item()) == n and torch.equal(g_out[:n], ref_out[:n])
