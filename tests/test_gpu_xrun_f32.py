"""GPU (MI355X): the exact-fp32 x-run sparse convolution (csrc/sparse_conv_xf.hip, dz_spconv_forward_x_f32: submanifold 3 x 3 x 3
convolutions at 32 / 64 / 128 channels from the packed table + windows of the pair16 x-run engine) against the CPU oracle, the fp32
gather kernel and a float64 evaluation of the same rulebook; its write contract, its refusals, and the detector on it.
Levels are built as in tests/test_gpu_xrun.py (`_level`)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_xrun import K3, P1, S1, _level, _t

pytestmark = pytest.mark.gpu
COVERED = (32, 64, 128)
TOL = 2e-4              # the bound of the fp32 sparse engine on these weight scales (test_gpu_kernels.test_spconv_forward_vs_oracle)
SENTINEL = -12345.0


def _tables(lvl, channels, sort, monkeypatch):
    """(plain table, packed table with windows); sort: the rows of a unit in tap-set order (nbr_sorted + perm) or not."""
    from detzero_amd import ops
    monkeypatch.setattr(ops, 'XRUN_SORT', True)
    monkeypatch.setattr(ops, 'XRUN_SORT_MIN_CHANNELS', 0 if sort else 1 << 20)
    plain = lvl.neighbors_to(lvl, K3, S1, P1)
    xt = ops.build_windows(lvl.neighbors_to(lvl, K3, S1, P1, packed=True), lvl, channels)
    assert getattr(xt, 'xwin', None) is not None and (xt.xwin[3] is not None) == sort
    return plain, xt


def _inputs(rng, lvl, m, channels, device):
    feats = rng.standard_normal((m, channels)).astype(np.float32)
    w = (rng.standard_normal((27, channels, channels)) / np.sqrt(channels * 8)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, channels).astype(np.float32)
    shift = (rng.standard_normal(channels) * 0.1).astype(np.float32)
    res = rng.standard_normal((m, channels)).astype(np.float32)
    pad = lambda a: np.concatenate([a, np.zeros((lvl.cap - m, a.shape[1]), np.float32)], 0)          # noqa: E731
    return feats, w, scale, shift, res, _t(pad(feats), device), _t(pad(res), device)


@pytest.mark.parametrize('channels', COVERED)
def test_xrun_f32_vs_oracle_and_gather(device, channels, monkeypatch):
    """Mixed densities in a batch of two; a 90 %-full slab beside 1 %-full ones (some window exceeds the staging capacity: the
    gather-mode arm runs); a small level that is not a multiple of the unit.  With / without residual and ReLU, with scale / shift
    null, with and without the tap-set order."""
    from detzero_amd import lib as L
    from detzero_amd import ops
    from oracle import sparse as osp
    rng = np.random.default_rng(500 * channels)
    rcap = L.load().dz_spconv_x_f32_window_rows(channels, channels)
    assert rcap > 0
    for shape, dens, batch, gather in (([6, 36, 50], (0.3, 0.35, 0.25), 2, None), ([4, 48, 64], (0.01, 0.9, 0.02, 0.5), 1, True),
                                       ([3, 20, 33], (0.08,), 1, False)):
        lvl, coords = _level(rng, batch, shape, dens, device)
        m = coords.shape[0]
        feats, w, scale, shift, res, x, r = _inputs(rng, lvl, m, channels, device)
        rb = osp.build_rulebook(coords, lvl.shape, coords, K3, S1, P1)
        acc = osp.sparse_conv(torch.from_numpy(feats), rb, torch.from_numpy(w), m)
        for sort in (True, False):
            plain, xt = _tables(lvl, channels, sort, monkeypatch)
            if gather is not None:
                longest = int(xt.xwin[0][:-16].view(-1, 3, 2)[..., 1].max().item())
                assert (longest > rcap) == gather, (channels, longest, rcap)
            for with_res, relu, affine in ((True, True, True), (False, False, True), (True, False, False)):
                ref = acc * torch.from_numpy(scale) + torch.from_numpy(shift) if affine else acc.clone()
                if with_res:
                    ref = ref + torch.from_numpy(res)
                if relu:
                    ref = torch.relu(ref)
                sc, sh = (_t(scale, device), _t(shift, device)) if affine else (None, None)
                wd = _t(w, device)
                a = ops.spconv_forward(x, plain, lvl, wd, sc, sh, r if with_res else None, relu=relu)
                b = ops.spconv_forward(x, xt, lvl, wd, sc, sh, r if with_res else None, relu=relu)
                ga, gb = a[:m].cpu(), b[:m].cpu()
                print('  %3d ch %s sort=%d res=%d relu=%d affine=%d: max |x-run - oracle| %.2e, |x-run - gather| %.2e'
                      % (channels, shape, sort, with_res, relu, affine, float((gb - ref).abs().max()), float((gb - ga).abs().max())))
                torch.testing.assert_close(gb, ref, rtol=TOL, atol=TOL)
                torch.testing.assert_close(gb, ga, rtol=TOL, atol=TOL)


def _ref64(x, tab, w, m):
    """float64 evaluation of the rulebook `tab` (27, m; -1 = absent) on the device: (sum x.w, sum |x.w|)."""
    x64, w64 = x.double(), w.double()
    acc = torch.zeros((m, w.shape[2]), dtype=torch.float64, device=x.device)
    aacc = torch.zeros_like(acc)
    for t in range(27):
        idx = tab[t].long()
        rows = torch.nonzero(idx >= 0).squeeze(1)
        src = x64[idx[rows]]
        acc.index_add_(0, rows, src @ w64[t])
        aacc.index_add_(0, rows, src.abs() @ w64[t].abs())
    return acc, aacc


@pytest.mark.parametrize('channels', COVERED)
def test_xrun_f32_error_class(device, channels, monkeypatch):
    """e = max |got - ref64| / (|scale| * sum|x.w| + |shift| + |residual|) (the metric of tests/test_gpu_dense_conv.py) of the fp32
    gather kernel and of the x-run kernel on the same inputs.  Both are chains of the same number of fp32 fmaf roundings in another
    order: the x-run kernel gets 2 x the gather kernel's e of this very run."""
    from detzero_amd import ops
    rng = np.random.default_rng(77 * channels)
    lvl, coords = _level(rng, 2, [6, 36, 50], (0.3, 0.35, 0.25), device)
    m = coords.shape[0]
    feats, w, scale, shift, res, x, r = _inputs(rng, lvl, m, channels, device)
    plain, xt = _tables(lvl, channels, channels >= 64, monkeypatch)
    wd, sc, sh = _t(w, device), _t(scale, device), _t(shift, device)
    acc, aacc = _ref64(x, plain.words[:, :m], wd, m)
    ref = acc * sc.double() + sh.double() + r[:m].double()
    den = aacc * sc.double().abs() + sh.double().abs() + r[:m].double().abs()
    e = {}
    for name, tab in (('gather', plain), ('xrun', xt)):
        got = ops.spconv_forward(x, tab, lvl, wd, sc, sh, r, relu=False)[:m].double()
        e[name] = float(((got - ref).abs() / den.clamp_min(1e-30)).max())
    print('  error class %3d ch: gather fp32 e = %.3e, x-run fp32 e = %.3e (ratio %.2f)' % (channels, e['gather'], e['xrun'], e['xrun'] / e['gather']))
    assert e['gather'] > 0 and e['xrun'] <= 2.0 * e['gather'], e


@pytest.mark.parametrize('channels', COVERED)
def test_xrun_f32_write_contract(device, channels, monkeypatch):
    """Rows at or beyond *d_m_out and the capacity padding keep what they held; two launches agree bit for bit; the queue words behind
    the windows stay zero, and the pair16 x-run kernel on the same windows right after repeats its own earlier result bit for bit."""
    from detzero_amd import ops
    rng = np.random.default_rng(9 * channels)
    lvl, coords = _level(rng, 1, [4, 48, 64], (0.01, 0.9, 0.02, 0.5), device, cap_extra=700)
    m = coords.shape[0]
    feats, w, scale, shift, res, x, r = _inputs(rng, lvl, m, channels, device)
    plain, xt = _tables(lvl, channels, channels >= 64, monkeypatch)
    wd, sc, sh = _t(w, device), _t(scale, device), _t(shift, device)
    xp, rp, wp = ops.pair16_from_f32(x, channels, 1), ops.pair16_from_f32(r, channels, 1), ops.pack_weight_split(wd, 1)
    p0 = ops.spconv_forward(xp, xt, lvl, wp, sc, sh, rp, relu=True, math=1).clone()
    outs = []
    for _ in range(2):
        out = torch.full((lvl.cap, channels), SENTINEL, dtype=torch.float32, device=device)
        got = ops.spconv_forward(x, xt, lvl, wd, sc, sh, r, relu=True, out=out)
        assert got.data_ptr() == out.data_ptr()
        outs.append(out)
    torch.cuda.synchronize(device)
    assert lvl.cap - m >= 700 and bool((outs[0][m:] == SENTINEL).all()) and bool((outs[0][:m] != SENTINEL).all())
    assert torch.equal(outs[0], outs[1])
    assert not bool(xt.xwin[0][-16:].any())
    p1 = ops.spconv_forward(xp, xt, lvl, wp, sc, sh, rp, relu=True, math=1)
    assert torch.equal(p0[:m], p1[:m])


def test_xrun_f32_refusals(device):
    """Width 16, cin != cout, windows of another unit size, buffers at the 2 GiB limit (described, not allocated: the check precedes
    the launch), a packed table without windows: non-zero return with a message, nothing launched, the output untouched."""
    from detzero_amd import lib as L
    from detzero_amd import ops
    lib = L.load()
    rng = np.random.default_rng(3)
    lvl, coords = _level(rng, 1, [3, 16, 16], (0.3,), device)
    packed = lvl.neighbors_to(lvl, K3, S1, P1, packed=True)
    xt = ops.build_windows(packed, lvl, 64)
    win, tr = xt.xwin[0], xt.xwin[1]
    x = torch.zeros((lvl.cap, 128), device=device)
    w = torch.zeros((27 * 128 * 128,), device=device)
    out = torch.full((lvl.cap, 128), SENTINEL, device=device)

    def call(cin, cout, tile_rows, in_rows=None, cap=None):
        rc = lib.dz_spconv_forward_x_f32(L.ptr(x), lvl.cap if in_rows is None else in_rows, cin, L.ptr(packed.words), None, L.ptr(win), tile_rows,
                                         lvl.cap if cap is None else cap, L.ptr(lvl.d_m), L.ptr(w), None, None, None, 0, L.ptr(out), cout, L.stream())
        msg = lib.dz_last_error().decode()
        torch.cuda.synchronize(device)
        print('  %3d -> %3d, tile_rows %d, in_rows %s, cap %s -> rc %d: %s' % (cin, cout, tile_rows, in_rows, cap, rc, msg))
        assert rc != 0 and 'dz_spconv_forward_x_f32' in msg and bool((out == SENTINEL).all())
        return rc, msg
    assert 'channels' in call(16, 16, tr)[1]
    assert 'channels' in call(32, 64, tr)[1]
    assert 'tiles' in call(64, 64, tr // 2)[1]
    rc, msg = call(64, 64, tr, in_rows=2 ** 31 // (64 * 4))                  # an input of exactly 2^31 bytes
    assert rc == L.ERR_UNSUPPORTED and '2 GiB' in msg
    rc, msg = call(64, 64, tr, cap=2 ** 31 // (64 * 4))                      # an output of exactly 2^31 bytes
    assert rc == L.ERR_UNSUPPORTED and '2 GiB' in msg
    rc = lib.dz_spconv_forward_x_f32(L.ptr(x), lvl.cap, 64, L.ptr(packed.words), None, None, tr, lvl.cap, L.ptr(lvl.d_m), L.ptr(w), None, None, None, 0,
                                     L.ptr(out), 64, L.stream())
    assert rc != 0 and b'null' in lib.dz_last_error() and bool((out == SENTINEL).all())
    # the Python mirror: a packed table without windows has no fp32 kernel
    bare = lvl.neighbors_to(lvl, K3, S1, P1, packed=True)
    with pytest.raises(L.DetZeroHipError, match='packed neighbour table'):
        ops.spconv_forward(x[:, :64].contiguous(), bare, lvl, w[:27 * 64 * 64].view(27, 64, 64), None, None, None, relu=False)


def _stage_rows(res):
    out = {}
    for name, (feats, lvl) in res.items():
        out[name] = feats[:lvl.num_active()].clone()
    return out


def test_detector_fp32_on_the_xrun_engine_160k(device):
    """The whole detector at the headline configuration (160k points, 0.1 m voxels) in exact fp32 with the fp32 engine 'gather', then
    'xrun': boxes within 1e-3 of the CPU oracle on each, the backbone stages of the two engines within the fp32 per-stage tolerances
    of tests/test_gpu_full_parity.py; once through a captured FramePipeline at 8 frames (replay == eager, bit for bit)."""
    from detzero_amd.centerpoint import FramePipeline, set_sparse_engine
    from detzero_amd.synth import VOXEL_SIZE_01
    from tests.test_gpu_full_parity import REL
    from tests.util import cpu_state_dict, make_model, masked_frame, match_boxes, oracle_detect
    model, cfg, info = make_model(VOXEL_SIZE_01, seed=0)
    sd = cpu_state_dict(model)
    pts = masked_frame(0, 160000)
    rb = oracle_detect(sd, pts, info)['final'][0]
    n_ref = rb['pred_boxes'].shape[0]
    model = model.to(device)
    bb = model.backbone3d
    before = (bb.engine, bb.f32_engine)
    try:
        stages = {}
        for eng in ('gather', 'xrun'):
            set_sparse_engine(model, before[0], f32_engine=eng)
            pipe = FramePipeline(model, info, math='f32')
            dpts = torch.from_numpy(pts).to(device)
            prep = pipe.prepare([dpts])
            tabs = [st[1] for st in prep['steps'][1:4]]
            assert all((getattr(t, 'xwin', None) is not None) == (eng == 'xrun') for t in tabs), eng
            assert getattr(prep['steps'][0][1], 'xwin', None) is None            # the 16-channel level keeps the gather kernel
            stages[eng] = _stage_rows(pipe.backbone_stage(prep))
            out, d_n = pipe(dpts)
            k = int(d_n.item())
            nm, worst = match_boxes(rb['pred_boxes'].numpy(), rb['pred_scores'].numpy(), out[:k, :7].cpu().numpy(), out[:k, 7].cpu().numpy(), tol=1e-3)
            print('%s [f32]: %d boxes, %d/%d within 1e-3 of the oracle (worst %.2e)' % (eng, k, nm, n_ref, worst))
            assert n_ref > 50 and abs(k - n_ref) <= 2 and nm >= n_ref - 2, (eng, k, n_ref, nm, worst)
        for name in ('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4', 'encoded'):
            g, x = stages['gather'][name], stages['xrun'][name]
            assert g.shape == x.shape
            amp, err = float(g.std()), float((g - x).abs().max())
            print('  stage %-8s x-run vs gather (fp32): max abs %.3e = %.2e of the stage std (tolerance %.1e)' % (name, err, err / amp, REL[name][0]))
            assert err <= REL[name][0] * amp, (name, err, amp)
        assert torch.equal(stages['gather']['x_conv1'], stages['xrun']['x_conv1'])         # level 1 never leaves the gather kernel
        # captured, 8 frames, fp32 engine 'xrun' (still set)
        frames = [torch.from_numpy(masked_frame(20 + i, 40000)).to(device) for i in range(8)]
        pipe = FramePipeline(model, info, math='f32')
        pipe.calibrate(frames[:2], margin=2.0)
        for _ in range(2):
            o1, n1 = pipe(frames)
        torch.cuda.synchronize(device)
        pipe.check_overflow()
        o1, n1 = o1.clone(), n1.clone()
        cp = pipe.capture(frames)
        cp.replay()
        torch.cuda.synchronize(device)
        assert int(n1.sum().item()) > 0
        assert torch.equal(cp.counts, n1.view(-1)) and torch.equal(cp.boxes, o1.view(cp.boxes.shape))
    finally:
        set_sparse_engine(model, before[0], f32_engine=before[1])
