"""GPU (MI355X): the bf16x3 x-run sparse convolution of the exact-fp32 mode (csrc/sparse_conv_xt.hip, dz_spconv_forward_x_limb3:
submanifold 3 x 3 x 3 convolutions at 32 / 64 / 128 channels from the packed table + windows of the x-run engines, every operand as
three exact bf16 limbs) against a float64 evaluation of the same rulebook, the fp32 gather kernel and k_spconv_xf; its limb terms
bit for bit on one-product outputs; the same on inputs whose lower limbs are bf16 subnormals (a measurement: asserted to 2^-124 only);
its write contract, its refusals, and the detector on it.  (Its row-count edges, the staging boundary and the detector's own launches
are cases of tests/test_gpu_sparse_conv.py.)
Levels are built as in tests/test_gpu_xrun.py (`_level`), tables and the float64 reference as in tests/test_gpu_xrun_f32.py."""
import numpy as np
import pytest
import torch

from tests.test_gpu_conv3x3_limb3 import _patterned, _patterned_tiny, _pow2, _subnormal_report
from tests.test_gpu_xrun import K3, P1, S1, _level, _t
from tests.test_gpu_xrun_f32 import SENTINEL, _inputs, _ref64, _stage_rows, _tables

pytestmark = pytest.mark.gpu
COVERED = (32, 64, 128)
BOUND = 2.0 ** -19          # the dense bf16x3 engine's bound: fp32 accumulation of at most 27 * 128 terms + 2^-26 for the dropped terms


def _limb(w):
    from detzero_amd import ops
    return ops.pack_weight_limb3(w, cout_mult=32)


def _xt(x, tab, lvl, w, sc=None, sh=None, res=None, relu=False, out=None):
    from detzero_amd import ops
    return ops.spconv_forward(x, tab, lvl, _limb(w), sc, sh, res, relu=relu, out=out, f32_engine='xrun_bf16x3')


@pytest.mark.parametrize('channels', COVERED)
def test_xrun_limb3_vs_float64_gather_and_xf(device, channels, monkeypatch):
    """The three level shapes of test_xrun_f32_vs_oracle_and_gather, with / without the tap-set order, residual, ReLU and scale /
    shift: e = max |got - ref64| / (|scale| * sum|x.w| + |shift| + |residual|) of the gather kernel, k_spconv_xf and k_spconv_xt on the
    same inputs; the new kernel within 2^-19 and within 2 x the gather kernel's e of the same launch set.  Between them the cases
    hold windows above the kernel's staging capacity (gather-mode arm) and at or below it (staged arm)."""
    from detzero_amd import lib as L
    from detzero_amd import ops
    rng = np.random.default_rng(500 * channels)
    rcap = L.load().dz_spconv_x_limb3_window_rows(channels, channels)
    assert rcap > 0
    above = below = False
    for shape, dens, batch in (([6, 36, 50], (0.3, 0.35, 0.25), 2), ([4, 48, 64], (0.01, 0.9, 0.02, 0.5), 1), ([3, 20, 33], (0.08,), 1)):
        lvl, coords = _level(rng, batch, shape, dens, device)
        m = coords.shape[0]
        feats, w, scale, shift, res, x, r = _inputs(rng, lvl, m, channels, device)
        wd = _t(w, device)
        for sort in (True, False):
            plain, xt = _tables(lvl, channels, sort, monkeypatch)
            if sort:
                acc, aacc = _ref64(x, plain.words[:, :m], wd, m)
            wins = xt.xwin[0][:-16].view(-1, 3, 2)[..., 1]
            longest, shortest = int(wins.max().item()), int(wins[wins > 0].min().item())
            above, below = above or longest > rcap, below or shortest <= rcap
            print('  %3d ch %s sort=%d: unit of %d rows, windows of %d .. %d rows, staging capacity %d' % (channels, shape, sort, xt.xwin[1], shortest, longest, rcap))
            for with_res, relu, affine in ((True, True, True), (False, False, True), (True, False, False)):
                sc, sh = (_t(scale, device), _t(shift, device)) if affine else (None, None)
                scd = sc.double() if affine else torch.ones(channels, dtype=torch.float64, device=device)
                shd = sh.double() if affine else torch.zeros(channels, dtype=torch.float64, device=device)
                ref = acc * scd + shd
                den = aacc * scd.abs() + shd.abs()
                if with_res:
                    ref, den = ref + r[:m].double(), den + r[:m].double().abs()
                if relu:
                    ref = ref.clamp_min(0.0)
                rr = r if with_res else None
                got = {'gather': ops.spconv_forward(x, plain, lvl, wd, sc, sh, rr, relu=relu),
                       'xf': ops.spconv_forward(x, xt, lvl, wd, sc, sh, rr, relu=relu),
                       'xt': _xt(x, xt, lvl, wd, sc, sh, rr, relu=relu)}
                e = {}
                for name, g in got.items():
                    err = (g[:m].double() - ref).abs() / den.clamp_min(1e-30)
                    e[name] = float(torch.where(torch.isnan(g[:m]), torch.full_like(err, float('inf')), err).max())
                print('  %3d ch %s sort=%d res=%d relu=%d affine=%d: e gather %.3e  xf %.3e  xt %.3e (%.2f x gather, %.2f x 2^-24)'
                      % (channels, shape, sort, with_res, relu, affine, e['gather'], e['xf'], e['xt'], e['xt'] / e['gather'], e['xt'] * 2 ** 24))
                assert e['xt'] <= BOUND, (shape, sort, with_res, relu, affine, e)
                assert e['gather'] > 0 and e['xt'] <= 2.0 * e['gather'], (shape, sort, with_res, relu, affine, e)
    assert above and below, 'the cases must run the gather-mode arm and the staged arm (staging capacity %d)' % rcap


# ------------------------------------------------------------------------------------------------------------------------
# limb terms: one product per output, bit for bit (the one-hot cases of tests/test_gpu_conv3x3_limb3.py on a rulebook)
# ------------------------------------------------------------------------------------------------------------------------
def _small_level(device, seed):
    """~500 rows: two units at 256 rows, four at 128, the last one ragged."""
    rng = np.random.default_rng(seed)
    lvl, coords = _level(rng, 1, [5, 12, 14], (0.6, 0.55), device)
    return lvl, coords, coords.shape[0]


def _same_bits(got, exp, what):
    diff = got.contiguous().view(torch.int32) != exp.contiguous().view(torch.int32)
    if bool(diff.any()):
        i = torch.nonzero(diff)[0].tolist()
        raise AssertionError('%s: %d of %d outputs differ in bits, first at (row, channel) = %s: got %r, expected %r'
                             % (what, int(diff.sum()), diff.numel(), i, float(got[tuple(i)]), float(exp[tuple(i)])))


def _one_hot_expect(x, tab, tap, ci, val):
    """out[row, o] = x[tab[tap_o, row], ci_o] * val_o (0 where the neighbour is absent), in float64 -> fp32; exact there (checked)."""
    idx = tab[tap].long()                                              # (cout, m)
    src = x.double()[idx.clamp_min(0), ci.view(-1, 1)]                 # (cout, m)
    e64 = torch.where(idx >= 0, src * val.double().view(-1, 1), torch.zeros_like(src)).t().contiguous()
    e32 = e64.float()
    assert torch.equal(e32.double(), e64)
    return e32


@pytest.mark.parametrize('channels', COVERED)
def test_input_limbs_bit_exact(device, channels, monkeypatch):
    """Patterned 24-bit features, ONE non-zero (tap, cin) weight of value +-1, 0.5 or 2 per output channel; over the launches the
    entries cover all 27 taps x the first and last channel of every 16-channel chunk."""
    lvl, coords, m = _small_level(device, 31 * channels)
    gen = torch.Generator(device=device)
    gen.manual_seed(21 + channels)
    x = torch.zeros((lvl.cap, channels), device=device)
    x[:m] = _patterned((m, channels), gen, device)
    plain, xt = _tables(lvl, channels, channels >= 64, monkeypatch)
    tab = plain.words[:, :m]
    edge = [c for k in range(channels // 16) for c in (16 * k, 16 * k + 15)]
    combos = [(t, c) for t in range(27) for c in edge]
    order = torch.randperm(len(combos), generator=torch.Generator().manual_seed(channels)).tolist()
    values = torch.tensor([1.0, -1.0, 0.5, 2.0, -2.0], device=device)
    launches = -(-len(combos) // channels)
    for k in range(launches):
        pick = [combos[order[(k * channels + o) % len(combos)]] for o in range(channels)]
        tap = torch.tensor([p[0] for p in pick], device=device)
        ci = torch.tensor([p[1] for p in pick], device=device)
        val = values[(torch.arange(channels, device=device) + k) % values.numel()]
        w = torch.zeros((27, channels, channels), device=device)
        w[tap, ci, torch.arange(channels, device=device)] = val
        got = _xt(x, xt, lvl, w)[:m]
        _same_bits(got, _one_hot_expect(x, tab, tap, ci, val), 'input limbs %d ch, launch %d' % (channels, k))


def test_subnormal_limbs_are_measured(device, monkeypatch):
    """test_input_limbs_bit_exact's launches at 64 channels with features of exponent [-120, -104]: their m and / or l limbs are bf16
    subnormals while every product (weights +-1, 0.5, 2) stays a normal fp32.  Asserted: |got - x w| <= 2^-124, which holds whether or
    not the matrix pipe flushes subnormal inputs; printed (and recorded in DESIGN.md 2a-ter): the share of bit-exact outputs."""
    channels = 64
    lvl, coords, m = _small_level(device, 43 * channels)
    gen = torch.Generator(device=device)
    gen.manual_seed(25 + channels)
    x = torch.zeros((lvl.cap, channels), device=device)
    x[:m] = _patterned_tiny((m, channels), gen, device)
    plain, xt = _tables(lvl, channels, True, monkeypatch)
    tab = plain.words[:, :m]
    ar = torch.arange(channels, device=device)
    tap, ci = ar % 27, (ar * 7 + 3) % channels
    val = torch.tensor([1.0, -1.0, 0.5, 2.0, -2.0], device=device)[ar % 5]
    w = torch.zeros((27, channels, channels), device=device)
    w[tap, ci, ar] = val
    got = _xt(x, xt, lvl, w)[:m]
    xsel = _one_hot_expect(x, tab, tap, ci, torch.ones_like(val))
    # (rows without the tap's neighbour hold an exact zero: no subnormal limb, not counted)
    _subnormal_report('k_spconv_xt<%d>' % channels, got, xsel, val)


@pytest.mark.parametrize('channels', COVERED)
def test_weight_limbs_bit_exact(device, channels, monkeypatch):
    """Patterned 24-bit weights; features non-zero only on the voxels whose (z, y, x) are all multiples of 3, on one channel each (a
    first or last channel of a chunk) with value +-1, 0.5 or 2: a 3 x 3 x 3 window holds at most one such voxel, so every output is
    one product; every one of the 27 taps is reached."""
    lvl, coords, m = _small_level(device, 37 * channels)
    gen = torch.Generator(device=device)
    gen.manual_seed(22 + channels)
    w = _patterned((27, channels, channels), gen, device)
    c = torch.from_numpy(coords).to(device)
    lattice = ((c[:, 1] % 3 == 0) & (c[:, 2] % 3 == 0) & (c[:, 3] % 3 == 0))
    rows = torch.nonzero(lattice).squeeze(1)
    edge = torch.tensor([ch for k in range(channels // 16) for ch in (16 * k, 16 * k + 15)], device=device)
    values = torch.tensor([1.0, -1.0, 0.5, 2.0, -2.0], device=device)
    ch = edge[torch.arange(rows.numel(), device=device) % edge.numel()]
    val = values[torch.arange(rows.numel(), device=device) % values.numel()]
    x = torch.zeros((lvl.cap, channels), device=device)
    x[rows, ch] = val
    row_ch = torch.zeros(m, dtype=torch.long, device=device)
    row_val = torch.zeros(m, dtype=torch.float64, device=device)
    row_ch[rows], row_val[rows] = ch, val.double()
    plain, xt = _tables(lvl, channels, channels >= 64, monkeypatch)
    tab = plain.words[:, :m].long()
    e64 = torch.zeros((m, channels), dtype=torch.float64, device=device)
    hits = torch.zeros(m, dtype=torch.long, device=device)
    for t in range(27):
        idx = tab[t]
        live = (idx >= 0) & lattice[idx.clamp_min(0)]
        assert bool(live.any()), 'tap %d is reached by no output row' % t
        src = idx.clamp_min(0)
        e64 += torch.where(live.view(-1, 1), w[t].double()[row_ch[src]] * row_val[src].view(-1, 1), torch.zeros_like(e64))
        hits += live.long()
    assert int(hits.max()) == 1                      # one product per output
    e32 = e64.float()
    assert torch.equal(e32.double(), e64)
    _same_bits(_xt(x, xt, lvl, w)[:m], e32, 'weight limbs %d ch' % channels)


@pytest.mark.parametrize('channels', COVERED)
def test_mm_term_bit_exact(device, channels, monkeypatch):
    """x = (1 + 2^-10) 2^e, one-hot w = (1 + 2^-10) 2^e': the product (1 + 2^-9 + 2^-20) 2^(e + e') is exact in fp32 and is 2^-20 off
    without the m.m term."""
    lvl, coords, m = _small_level(device, 41 * channels)
    gen = torch.Generator(device=device)
    gen.manual_seed(23 + channels)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=gen, device=device)          # noqa: E731
    one = torch.tensor(1.0 + 2.0 ** -10, device=device)
    x = torch.zeros((lvl.cap, channels), device=device)
    x[:m] = one * _pow2(ri(-40, 16, (m, channels)))
    tap, ci = ri(0, 26, (channels,)), ri(0, channels - 1, (channels,))
    tap[:27] = torch.arange(27, device=device)
    val = one * _pow2(ri(-40, 16, (channels,)))
    w = torch.zeros((27, channels, channels), device=device)
    w[tap, ci, torch.arange(channels, device=device)] = val
    plain, xt = _tables(lvl, channels, channels >= 64, monkeypatch)
    exp = _one_hot_expect(x, plain.words[:, :m], tap, ci, val)
    assert bool((exp != 0).any())
    _same_bits(_xt(x, xt, lvl, w)[:m], exp, 'm.m term %d ch' % channels)


@pytest.mark.parametrize('channels', COVERED)
def test_xrun_limb3_write_contract(device, channels, monkeypatch):
    """Rows at or beyond *d_m_out and the capacity padding keep what they held; two launches agree bit for bit; the queue words behind
    the windows stay zero; the pair16 x-run kernel and k_spconv_xf on the same windows right after repeat their own earlier results
    bit for bit."""
    from detzero_amd import ops
    rng = np.random.default_rng(9 * channels)
    lvl, coords = _level(rng, 1, [4, 48, 64], (0.01, 0.9, 0.02, 0.5), device, cap_extra=700)
    m = coords.shape[0]
    feats, w, scale, shift, res, x, r = _inputs(rng, lvl, m, channels, device)
    plain, xt = _tables(lvl, channels, channels >= 64, monkeypatch)
    wd, sc, sh = _t(w, device), _t(scale, device), _t(shift, device)
    xp, rp, wp = ops.pair16_from_f32(x, channels, 1), ops.pair16_from_f32(r, channels, 1), ops.pack_weight_split(wd, 1)
    p0 = ops.spconv_forward(xp, xt, lvl, wp, sc, sh, rp, relu=True, math=1).clone()
    f0 = ops.spconv_forward(x, xt, lvl, wd, sc, sh, r, relu=True).clone()
    wl = _limb(wd)
    outs = []
    for _ in range(2):
        out = torch.full((lvl.cap, channels), SENTINEL, dtype=torch.float32, device=device)
        got = ops.spconv_forward(x, xt, lvl, wl, sc, sh, r, relu=True, out=out, f32_engine='xrun_bf16x3')
        assert got.data_ptr() == out.data_ptr()
        outs.append(out)
    torch.cuda.synchronize(device)
    assert lvl.cap - m >= 700 and bool((outs[0][m:] == SENTINEL).all()) and bool((outs[0][:m] != SENTINEL).all())
    assert torch.equal(outs[0], outs[1])
    assert not bool(xt.xwin[0][-16:].any())
    p1 = ops.spconv_forward(xp, xt, lvl, wp, sc, sh, rp, relu=True, math=1)
    assert torch.equal(p0[:m], p1[:m])
    f1 = ops.spconv_forward(x, xt, lvl, wd, sc, sh, r, relu=True)
    assert torch.equal(f0[:m], f1[:m])


def test_xrun_limb3_refusals(device):
    """Width 16, cin != cout, windows of another unit size, buffers at the 2 GiB limit (described, not allocated: the check precedes
    the launch), a null window pointer: non-zero return with a message that names the entry point, the output untouched; an unknown
    engine name raises."""
    from detzero_amd import lib as L
    from detzero_amd import ops
    lib = L.load()
    rng = np.random.default_rng(3)
    lvl, coords = _level(rng, 1, [3, 16, 16], (0.3,), device)
    packed = lvl.neighbors_to(lvl, K3, S1, P1, packed=True)
    xt = ops.build_windows(packed, lvl, 64)
    win, tr = xt.xwin[0], xt.xwin[1]
    x = torch.zeros((lvl.cap, 128), device=device)
    w = torch.zeros((27 * 128 * 128 * 3 // 2,), device=device)
    out = torch.full((lvl.cap, 128), SENTINEL, device=device)

    def call(cin, cout, tile_rows, in_rows=None, cap=None, windows=win):
        rc = lib.dz_spconv_forward_x_limb3(L.ptr(x), lvl.cap if in_rows is None else in_rows, cin, L.ptr(packed.words), None, L.ptr(windows), tile_rows,
                                           lvl.cap if cap is None else cap, L.ptr(lvl.d_m), L.ptr(w), None, None, None, 0, L.ptr(out), cout, L.stream())
        msg = lib.dz_last_error().decode()
        torch.cuda.synchronize(device)
        print('  %3d -> %3d, tile_rows %d, in_rows %s, cap %s -> rc %d: %s' % (cin, cout, tile_rows, in_rows, cap, rc, msg))
        assert rc != 0 and 'dz_spconv_forward_x_limb3' in msg and bool((out == SENTINEL).all())
        return rc, msg
    assert 'channels' in call(16, 16, tr)[1]
    assert 'channels' in call(32, 64, tr)[1]
    assert 'tiles' in call(64, 64, tr // 2)[1]
    rc, msg = call(64, 64, tr, in_rows=2 ** 31 // (64 * 4))                  # an input of exactly 2^31 bytes
    assert rc == L.ERR_UNSUPPORTED and '2 GiB' in msg
    rc, msg = call(64, 64, tr, cap=2 ** 31 // (64 * 4))                      # an output of exactly 2^31 bytes
    assert rc == L.ERR_UNSUPPORTED and '2 GiB' in msg
    assert 'null' in call(64, 64, tr, windows=None)[1]
    w64 = torch.zeros((27, 64, 64), device=device)
    with pytest.raises(L.DetZeroHipError, match='nonsense'):
        ops.spconv_forward(x[:, :64].contiguous(), xt, lvl, w64, None, None, None, relu=False, f32_engine='nonsense')
    # the Python mirror of the kernel's refusals: limb weights on a table without windows
    bare = lvl.neighbors_to(lvl, K3, S1, P1, packed=True)
    with pytest.raises(L.DetZeroHipError, match='xrun_bf16x3'):
        ops.spconv_forward(x[:, :64].contiguous(), bare, lvl, _limb(w64), None, None, None, relu=False, f32_engine='xrun_bf16x3')


def test_detector_fp32_on_the_limb3_xrun_engine_40k(device):
    """The detector at one 40 000-point frame (0.1 m voxels) in exact fp32 with the fp32 sparse engine 'gather', then 'xrun_bf16x3',
    then 'xrun_bf16x3' with the dense bf16x3 engine: the stage tables carry windows only on the x-run engine, level 1 is bit-identical,
    the deeper stages within the fp32 per-stage tolerances of tests/test_gpu_full_parity.py of the gather run, the boxes within 1e-3
    of the gather run's; then 2 frames through a captured FramePipeline (replay == eager, bit for bit)."""
    from detzero_amd.centerpoint import FramePipeline, set_dense_engine, set_sparse_engine
    from detzero_amd.synth import VOXEL_SIZE_01
    from tests.test_gpu_full_parity import REL
    from tests.util import make_model, masked_frame, match_boxes
    model, cfg, info = make_model(VOXEL_SIZE_01, seed=0)
    pts = masked_frame(0, 40000)
    model = model.to(device)
    bb = model.backbone3d
    before = (bb.engine, bb.f32_engine)
    dense_before = [mod.f32_dense_engine for mod in model.modules() if hasattr(mod, 'set_dense_engine')]
    assert len(set(dense_before)) == 1
    try:
        stages, boxes = {}, {}
        for eng, dense in (('gather', dense_before[0]), ('xrun_bf16x3', dense_before[0]), ('xrun_bf16x3', 'bf16x3')):
            set_sparse_engine(model, before[0], f32_engine=eng)
            set_dense_engine(model, dense)
            key = (eng, dense)
            pipe = FramePipeline(model, info, math='f32')
            dpts = torch.from_numpy(pts).to(device)
            prep = pipe.prepare([dpts])
            tabs = [st[1] for st in prep['steps'][1:4]]
            assert all((getattr(t, 'xwin', None) is not None) == (eng != 'gather') for t in tabs), eng
            assert getattr(prep['steps'][0][1], 'xwin', None) is None            # the 16-channel level keeps the gather kernel
            stages[key] = _stage_rows(pipe.backbone_stage(prep))
            out, d_n = pipe(dpts)
            k = int(d_n.item())
            boxes[key] = (out[:k, :7].cpu().numpy(), out[:k, 7].cpu().numpy())
        ref_key = ('gather', dense_before[0])
        rb, rs = boxes[ref_key]
        n_ref = rb.shape[0]
        for key in list(boxes)[1:]:
            gb, gs = boxes[key]
            nm, worst = match_boxes(rb, rs, gb, gs, tol=1e-3)
            print('%s [f32]: %d boxes, %d/%d within 1e-3 of the gather engine (worst %.2e)' % (key, gb.shape[0], nm, n_ref, worst))
            assert n_ref > 0 and abs(gb.shape[0] - n_ref) <= 2 and nm >= n_ref - 2, (key, gb.shape[0], n_ref, nm, worst)
            assert torch.equal(stages[ref_key]['x_conv1'], stages[key]['x_conv1'])         # level 1 never leaves the gather kernel
            for name in ('x_conv2', 'x_conv3', 'x_conv4', 'encoded'):
                g, x = stages[ref_key][name], stages[key][name]
                assert g.shape == x.shape
                amp, err = float(g.std()), float((g - x).abs().max())
                print('  stage %-8s %s vs gather (fp32): max abs %.3e = %.2e of the stage std (tolerance %.1e)' % (name, key[0], err, err / amp, REL[name][0]))
                assert err <= REL[name][0] * amp, (key, name, err, amp)
        # captured, 2 frames, the engines still on
        frames = [torch.from_numpy(masked_frame(20 + i, 40000)).to(device) for i in range(2)]
        pipe = FramePipeline(model, info, math='f32')
        pipe.calibrate(frames, margin=2.0)
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
        set_dense_engine(model, dense_before[0])
