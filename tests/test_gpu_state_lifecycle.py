"""GPU (MI355X): the detector's cached device state - kernel-layout plans, packed pair / limb weights, the fp16-pair pre-scale, the
zero-response images of the first BEV block, captured graphs that point at all of them - across weight reloads, math / pre-scale /
engine switches, device moves, captures and cache evictions.  A model driven through a sequence of such changes must give the bits of
a model built directly in the state it ends in; what cannot stay valid (exponents calibrated for other weights, a graph over a dropped
plan) must refuse.  Every stale-pointer condition is asserted on the host before a graph is replayed.  The host-side rules alone:
tests/test_state_lifecycle.py.  Smallest detector of the suite throughout (0.2 m voxels, 20 000-point frames)."""
import copy
import time

import numpy as np
import pytest
import torch

from detzero_amd.synth import VOXEL_SIZE_02
from tests.test_gpu_split import _scaled_model, _stage_features
from tests.util import canon_order, cpu_state_dict, make_model, masked_frame, match_boxes, oracle_features_f64

pytestmark = pytest.mark.gpu
SPARSE_STAGES = ('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4', 'encoded')


@pytest.fixture(scope='module')
def seeds():
    """Pristine CPU detectors of seed 0 and 1 (never planned, never moved: a deep copy of one is a freshly built model), their state
    dicts and the dataset info."""
    m0, _, info = make_model(VOXEL_SIZE_02, seed=0)
    m1 = make_model(VOXEL_SIZE_02, seed=1)[0]
    return {'model': {0: m0, 1: m1}, 'sd': {0: cpu_state_dict(m0), 1: cpu_state_dict(m1)}, 'info': info}


def _fresh(seeds, seed, device):
    return copy.deepcopy(seeds['model'][seed]).to(device)


def _packed(model, info, frames, math, ways=None):
    """(boxes9 rows below the counts, counts) of one FramePipeline pass, cloned."""
    from detzero_amd.centerpoint import FramePipeline
    out, n = FramePipeline(model, info, math=math, ways=ways)(frames)
    return out.clone(), n.clone()


def _same_packed(a, b):
    (oa, na), (ob, nb) = a, b
    if not torch.equal(na.view(-1), nb.view(-1)):
        return False
    oa, ob = oa.view(na.numel(), -1, 9), ob.view(nb.numel(), -1, 9)
    return all(torch.equal(oa[i, :int(k)], ob[i, :int(k)]) for i, k in enumerate(na.view(-1).tolist()))


# ------------------------------------------------------------------------------------------------ C1
def test_reload_after_select_math_refuses_stale_exponents_then_recalibrates(device):
    """Weights of a detector whose activations are 3e4 x larger loaded into a model that went through select_math: the f16x2 pass
    refuses (the exponents would saturate the pairs at 65504 without a sign), the f32 pass runs, and after a new select_math the
    stage features are within 2e-5 of each stage's peak of the f32 engine and the boxes within 1e-3 - the bounds of
    tests/test_gpu_split.py::test_select_math_keeps_fp16_pairs_at_any_activation_scale.
    Data-dependent preconditions: the two weight sets calibrate to different exponents at every stage; more than 50 boxes."""
    from detzero_amd.centerpoint import FramePipeline, select_math, set_math
    from detzero_amd.lib import DetZeroHipError
    from tests.test_gpu_split import _boxes
    model, info = _scaled_model(device, 1.0, homogeneous=True)
    hot, _ = _scaled_model(device, 3.0e4, homogeneous=True)
    pts = torch.from_numpy(masked_frame(0, 20000)).to(device)
    mode, _ = select_math(model, info, [pts])
    first = dict(model.prescale)
    assert mode == 'f16x2' and model.backbone2d.math == 1
    model.load_state_dict(hot.state_dict())
    with pytest.raises(DetZeroHipError, match='select_math'):
        FramePipeline(model, info, math='f16x2')(pts)
    a = _boxes(model, info, pts, 'f32')                                   # the exact-fp32 engine takes no pre-scale: it runs ...
    assert np.array_equal(a, _boxes(hot, info, pts, 'f32'))              # ... on the new weights
    with pytest.raises(DetZeroHipError):                                  # (and an f32 pass does not clear the mark)
        FramePipeline(model, info, math='f16x2')(pts)
    mode, rng = select_math(model, info, [pts])
    second = dict(model.prescale)
    print('exponents before the reload %s, after %s' % (first, second))
    assert mode == 'f16x2' and all(second[k] < first[k] - 10 for k in first), (first, second)      # (3e4 ~ 2^15)
    ref = _stage_features(model, info, pts, 'f32')
    got = _stage_features(model, info, pts, 'f16x2')
    for name in ref:
        scale = float(ref[name].abs().max())
        err = float((got[name] - ref[name]).abs().max()) / scale
        print('  %-8s after reload + select_math: %.2e of the stage peak %.3g (bound 2e-5)' % (name, err, scale))
        assert err < 2e-5, (name, err, scale)
    b = _boxes(model, info, pts, 'f16x2')
    nm, wbox = match_boxes(a[:, :7], a[:, 7], b[:, :7], b[:, 7], tol=1e-3)
    print('  %d / %d boxes of the f32 engine matched within 1e-3 (worst %.2e)' % (nm, a.shape[0], wbox))
    assert a.shape[0] > 50 and abs(a.shape[0] - b.shape[0]) <= 2 and nm >= a.shape[0] - 2, (a.shape, b.shape, nm, wbox)
    set_math(model, 'f32')


# ------------------------------------------------------------------------------------------------ C2
def _canonical_rows(model, info, pts, math):
    """{stage: (rows in canonical order as fp32 CPU tensors, their coordinates)} of the sparse backbone on one frame."""
    from detzero_amd import ops
    from detzero_amd.centerpoint import FramePipeline
    pipe = FramePipeline(model, info, math=math)
    res = pipe.backbone_stage(pipe.prepare([pts]))
    out = {}
    for name, (feats, lvl) in res.items():
        m = lvl.num_active()
        coords = lvl.coords[:m].cpu().numpy()
        o = canon_order(coords, lvl.shape)
        out[name] = (ops.level_rows_f32(feats[:m], lvl, ops.math_id(math)).cpu()[torch.from_numpy(o)], coords[o])
    return out


def test_a_model_driven_through_state_changes_equals_a_fresh_one_bit_for_bit(device, seeds):
    """One model through: f32 -> select_math f16x2 -> bf16x2 -> f16x2 again (cached pair weights) -> pre-scale shifted by +1 -> no
    pre-scale -> the bf16x3 dense / x-run / gather engines in f32 -> load_state_dict(seed 1) in f32, then in f16x2 after a new
    select_math (first pass: a SPLIT pass of 12 frames, equal to the unsplit one) -> .cpu() / .to(device) -> load_state_dict(seed 0),
    default engines.  After every step the five stage tensors and the packed boxes are torch.equal to those of a FRESH model (a copy of
    a never-used CPU model) put directly into that state; the end equals steps 1 and 2, and sits inside the float64 budgets of
    tests/test_gpu_full_parity.py (REL).  Preconditions: seed 0 and seed 1 give different bits; more than 50 boxes per state."""
    from detzero_amd.centerpoint import select_math, set_dense_engine, set_math, set_prescale, set_sparse_engine
    from tests.test_gpu_full_parity import REL
    info = seeds['info']
    pts_np = masked_frame(0, 20000)
    pts = torch.from_numpy(pts_np).to(device)
    fresh_results = {}
    times = []

    def observe(m, math):
        return _stage_features(m, info, pts, math), _packed(m, info, pts, math)

    def fresh(state, build):
        """Results of a fresh model built in `state` (once per distinct state)."""
        if state not in fresh_results:
            m, math = build()
            fresh_results[state] = observe(m, math)
            assert int(fresh_results[state][1][1].item()) > 50, state
        return fresh_results[state]

    def check(step, math, state, build, t0):
        got = observe(model, math)
        want = fresh(state, build)
        for name in SPARSE_STAGES:
            assert torch.equal(got[0][name], want[0][name]), (step, name, float((got[0][name] - want[0][name]).abs().max()))
        assert _same_packed(got[1], want[1]), step
        torch.cuda.synchronize()
        times.append((step, time.perf_counter() - t0))
        return got

    def engines_on(m):
        set_dense_engine(m, 'bf16x3')
        set_sparse_engine(m, m.backbone3d.engine, f32_engine='xrun_bf16x3', f32_gather='bf16x3')
        return m

    def build_plain(seed, math, exps=None, engines=False):
        def build():
            m = _fresh(seeds, seed, device)
            if engines:
                engines_on(m)
            set_prescale(m, exps)
            set_math(m, math)
            return m, math
        return build

    def build_selected(seed, engines=False):
        def build():
            m = _fresh(seeds, seed, device)
            if engines:
                engines_on(m)
            select_math(m, info, [pts])
            return m, 'f16x2'
        return build

    model = _fresh(seeds, 0, device)
    default_engines = (model.backbone3d.f32_engine, model.backbone3d.f32_gather, model.backbone2d.f32_dense_engine)
    # 1. f32
    t0 = time.perf_counter()
    set_math(model, 'f32')
    step1 = check('1 f32', 'f32', (0, 'f32'), build_plain(0, 'f32'), t0)
    # 2. select_math: f16x2 with the calibrated exponents (the fresh model calibrates for itself: the same exponents)
    t0 = time.perf_counter()
    select_math(model, info, [pts])
    exps0 = dict(model.prescale)
    step2 = check('2 select_math f16x2', 'f16x2', (0, 'f16x2', 'selected'), build_selected(0), t0)
    assert any(exps0.values()), exps0
    assert not torch.equal(step1[0]['encoded'], step2[0]['encoded'])            # (the two arithmetics differ in bits: the steps can tell them apart)
    # 3. bf16 pairs (the pre-scale stays installed and is ignored)
    t0 = time.perf_counter()
    set_math(model, 'bf16x2')
    check('3 bf16x2', 'bf16x2', (0, 'bf16x2'), build_plain(0, 'bf16x2'), t0)
    # 4. back to fp16 pairs: the packed pair weights of step 2 are still in the plan
    t0 = time.perf_counter()
    set_math(model, 'f16x2')
    assert any('_pre' in e for e in (model.backbone3d.plan()['conv_input'], model.backbone3d.plan()['conv_out']))
    check('4 f16x2 again', 'f16x2', (0, 'f16x2', 'selected'), None, t0)
    # 5. every exponent + 1
    t0 = time.perf_counter()
    shifted = {k: v + 1 for k, v in exps0.items()}
    set_prescale(model, shifted)
    check('5 exponents + 1', 'f16x2', (0, 'f16x2', 'shifted'), build_plain(0, 'f16x2', shifted), t0)
    # 6. no pre-scale
    t0 = time.perf_counter()
    set_prescale(model, None)
    check('6 no pre-scale', 'f16x2', (0, 'f16x2', None), build_plain(0, 'f16x2'), t0)
    # 7. the three bf16x3 engines of the exact-fp32 mode
    t0 = time.perf_counter()
    set_math(model, 'f32')
    engines_on(model)
    step7 = check('7 bf16x3 engines, f32', 'f32', (0, 'f32', 'bf16x3'), build_plain(0, 'f32', engines=True), t0)
    assert not torch.equal(step7[0]['encoded'], step1[0]['encoded'])            # (another accumulation order: the engines did run)
    assert any('w_xlimb3' in e for e in (model.backbone3d.plan()['conv_input'], model.backbone3d.plan()['conv_out']))
    # 8a. other weights, still f32 on the bf16x3 engines
    t0 = time.perf_counter()
    model.load_state_dict(seeds['sd'][1])
    step8 = check('8a seed 1, f32', 'f32', (1, 'f32', 'bf16x3'), build_plain(1, 'f32', engines=True), t0)
    assert not torch.equal(step8[0]['x_conv1'], step7[0]['x_conv1'])            # (seed 1 is another network)
    # 8b. ... and f16x2 after a new select_math; the FIRST f16x2 pass on the new weights is a split pass (12 frames of 5000 points, two
    # concurrent sub-passes that both need the packed weights and zero-response images nobody has built yet) and equals the unsplit one
    t0 = time.perf_counter()
    select_math(model, info, [pts])
    exps1 = dict(model.prescale)
    twelve = [torch.from_numpy(masked_frame(40 + i, 5000)).to(device) for i in range(12)]
    from detzero_amd.centerpoint import FramePipeline
    two = FramePipeline(model, info, math='f16x2', ways=2)
    assert two.splits(len(twelve))
    split = tuple(t.clone() for t in two(twelve))
    assert two._subs is not None and len(two._subs) == 2
    unsplit = _packed(model, info, twelve, 'f16x2', ways=1)
    assert int(unsplit[1].min().item()) > 0 and _same_packed(split, unsplit)
    check('8b seed 1, select_math f16x2 (split pass first)', 'f16x2', (1, 'f16x2', 'selected'), build_selected(1, engines=True), t0)
    # 9. a round trip through the host: the values did not change, so the exponents stay valid
    t0 = time.perf_counter()
    model = model.cpu().to(device)
    assert model.backbone3d._plan is None and dict(model.prescale) == exps1
    check('9 .cpu() / .to(device)', 'f16x2', (1, 'f16x2', 'selected'), None, t0)
    # 10. seed 0 again, default engines: steps 1 and 2
    t0 = time.perf_counter()
    model.load_state_dict(seeds['sd'][0])
    set_dense_engine(model, default_engines[2])
    set_sparse_engine(model, model.backbone3d.engine, f32_engine=default_engines[0], f32_gather=default_engines[1])
    set_math(model, 'f32')
    end32 = check('10a seed 0 again, f32', 'f32', (0, 'f32'), None, t0)
    t0 = time.perf_counter()
    select_math(model, info, [pts])
    assert dict(model.prescale) == exps0
    end16 = check('10b seed 0 again, select_math f16x2', 'f16x2', (0, 'f16x2', 'selected'), None, t0)
    for name in SPARSE_STAGES:
        assert torch.equal(end32[0][name], step1[0][name]) and torch.equal(end16[0][name], step2[0][name]), name
    assert _same_packed(end32[1], step1[1]) and _same_packed(end16[1], step2[1])
    # ... and the end state against float64 on the same weights
    t0 = time.perf_counter()
    r64 = oracle_features_f64(seeds['sd'][0], pts_np, info)
    for col, math in ((0, 'f32'), (1, 'f16x2')):
        rows = _canonical_rows(model, info, pts, math)
        for name in SPARSE_STAGES:
            rf, rc, rs = r64['backbone'][name]
            got, coords = rows[name]
            assert np.array_equal(coords[:, 1:], np.asarray(rc)[:, 1:]), name
            amp = float(rf.std())
            err = float((got.double() - rf.double()).abs().max())
            print('  end state %-8s [%-5s] max abs err %.3e = %.2e of the stage std %.3g (budget %.1e)' % (name, math, err, err / amp, amp, REL[name][col]))
            assert err <= REL[name][col] * amp, (name, math, err, amp)
    times.append(('float64 yardstick', time.perf_counter() - t0))
    set_math(model, 'f32')
    print('  wall time per step: ' + '; '.join('%s %.2f s' % t for t in times))


# ------------------------------------------------------------------------------------------------ C3
def _zero_keys(lvl):
    return [k for k in lvl if isinstance(k, tuple) and k[0] == 'zero_resp']


def test_zero_response_images_of_a_capture_survive_other_batch_sizes(device, seeds):
    """A graph captured at 2 frames reads the zero-response images of that key; eager passes at 1, 3, 4, 5, (1 again) and 6 frames add
    five keys to a cache that keeps four.  The captured key is pinned: it stays in the plan with the same images (asserted on the
    host BEFORE the replay), the replay equals the eager pass bit for bit, at most four unpinned keys remain, and the key that was hit
    again between the insertions (1 frame) is not the one evicted (3 frames is).
    Preconditions: frames masked to x > 0, so whole pixel tiles are empty - at least one skippable tile at layer 2 of the first block."""
    from detzero_amd import det_modules, ops
    from detzero_amd.centerpoint import FramePipeline
    info = seeds['info']
    model = _fresh(seeds, 0, device)
    frames = []
    for i in range(6):
        p = masked_frame(60 + i, 20000)
        frames.append(torch.from_numpy(p[p[:, 0] > 0.0].copy()).to(device))
    assert det_modules.SKIP_EMPTY_TILES
    pipe = FramePipeline(model, info, math='f16x2')
    static = [f.clone() for f in frames[:2]]
    pipe.calibrate(frames, margin=2.0)                    # (capacities for every frame the eager passes below will see)
    for _ in range(2):
        ref = pipe(static)
    ref = tuple(t.clone() for t in ref)
    torch.cuda.synchronize()
    pipe.check_overflow()
    assert int(ref[1].min().item()) > 50
    # preconditions: the images exist under a 2-frame key, and tiles ARE skipped below the first layer
    lvl = model.backbone2d.plan()[0]
    keys = _zero_keys(lvl)
    assert len(keys) == 1 and keys[0][5] == 2, keys
    key2 = keys[0]
    x, enc = pipe.backbone_stage(pipe.prepare(static))['encoded']
    ridx = ops.bev_row_index(enc, x.shape[0], pad=1)
    lists = ops.bev_tile_list(ridx, ridx.shape[1] - 2, ridx.shape[2] - 2, 6).cpu()
    print('  skippable tiles per layer: %s of %d' % (lists[:, 1].tolist(), int(lists[0, 0] + lists[0, 1])))
    assert int(lists[1, 1]) >= 1 and int(lists[5, 1]) >= 1
    cache = lvl['_zero_resp_cache']
    assert cache.unpinned() == [key2] and not cache.pinned()
    cp = pipe.capture(static)
    assert cache.pinned() == {key2} and cache.unpinned() == []
    images = lvl[key2]
    ptrs = [t.data_ptr() for t in images]
    for nb in (1, 3, 4, 5, 1, 6):
        pipe(frames[:nb])
        assert len(cache.unpinned()) <= 4
    # host-side, before anything is replayed: the captured key and its images are where the graph expects them
    assert key2 in lvl and lvl[key2] is images and [t.data_ptr() for t in lvl[key2]] == ptrs and cache.pinned() == {key2}
    assert [k[5] for k in cache.unpinned()] == [4, 5, 1, 6]                   # 3 went: least recently USED, not first inserted
    assert sorted(k[5] for k in _zero_keys(lvl)) == [1, 2, 4, 5, 6]
    assert not cp.stale()
    torch.cuda.synchronize()
    cp.replay()
    torch.cuda.synchronize()
    eager = tuple(t.clone() for t in pipe(static))
    assert _same_packed(eager, ref) and _same_packed((cp.boxes, cp.counts), eager)
    pipe.check_overflow()
    # ... and the skipped tiles did matter: without them every tile is computed, and the bits are the same
    det_modules.SKIP_EMPTY_TILES = False
    try:
        full = tuple(t.clone() for t in FramePipeline(model, info, math='f16x2')(static))
    finally:
        det_modules.SKIP_EMPTY_TILES = True
    assert _same_packed(full, eager)


# ------------------------------------------------------------------------------------------------ C4
def test_captured_passes_refuse_to_replay_after_a_reload(device, seeds):
    """CapturedPass and StreamingDetector(use_graph=True) over a select_math'd f16x2 model: a reload of ANOTHER model instance leaves
    them fresh, math and pre-scale switches on their own model leave the replay at the capture-time bits, a reload of their model makes
    stale() true and replay() / feed() / flush() raise before launching anything; a new capture after a new select_math works.
    Preconditions: the streaming slots were captured as graphs; more than 50 boxes per frame."""
    from detzero_amd.centerpoint import FramePipeline, StreamingDetector, select_math, set_math, set_prescale
    from detzero_amd.lib import DetZeroHipError
    info = seeds['info']
    model, other = _fresh(seeds, 0, device), _fresh(seeds, 0, device)
    n = 12000
    batch = [torch.from_numpy(masked_frame(70 + j, 20000)[:n].copy()).to(device) for j in range(2)]
    select_math(model, info, batch)
    exps = dict(model.prescale)
    pipe = FramePipeline(model, info, math='f16x2')
    pipe.calibrate(batch, margin=2.0)
    for _ in range(2):
        ref = pipe(batch)
    ref = tuple(t.clone() for t in ref)
    torch.cuda.synchronize()
    assert int(ref[1].min().item()) > 50
    FramePipeline(other, info, math='f16x2')(batch)                            # (the other instance has plans of its own)
    cp = pipe.capture(batch)
    sdet = StreamingDetector(pipe, batch, use_graph=True)
    assert sdet.graph_note.startswith('hipGraph') and all(s['gb'] is not None and s['plans'] for s in sdet.slots), sdet.graph_note
    assert len(cp.plans) >= 3 and not cp.stale() and not sdet.stale()

    def replayed():
        cp.replay()
        torch.cuda.synchronize()
        return cp.boxes.clone(), cp.counts.clone()
    assert _same_packed(replayed(), ref)
    # another model's reload: global counters move, this capture's plans do not
    other.load_state_dict(seeds['sd'][1])
    assert other.backbone3d._plan is None and not cp.stale() and not sdet.stale()
    assert _same_packed(replayed(), ref)
    assert sdet.feed(batch) is None
    got = sdet.feed(batch)
    torch.cuda.synchronize()
    assert _same_packed((got[0].clone(), got[1].clone()), ref)
    # switches that keep the plan: the graph stays at its capture-time configuration
    set_math(model, 'f32')
    assert not cp.stale() and _same_packed(replayed(), ref)
    set_prescale(model, {k: v + 1 for k, v in exps.items()})
    assert not cp.stale() and _same_packed(replayed(), ref)
    set_prescale(model, exps)
    set_math(model, 'f16x2')
    # the capture's own model gets other weights
    model.load_state_dict(seeds['sd'][1])
    assert cp.stale() and sdet.stale()                                         # first: nothing below may launch
    with pytest.raises(DetZeroHipError, match='capture again'):
        cp.replay()
    with pytest.raises(DetZeroHipError, match='capture again'):
        sdet.feed(batch)
    with pytest.raises(DetZeroHipError, match='capture again'):
        sdet.flush()
    assert all(p is not None for _, p in cp.plans)                             # (what the old graph points at is still held)
    torch.cuda.synchronize()
    # capture again: new exponents, new eager pass, new graph
    select_math(model, info, batch)
    pipe2 = FramePipeline(model, info, math='f16x2')
    pipe2.calibrate(batch, margin=2.0)
    for _ in range(2):
        ref2 = pipe2(batch)
    ref2 = tuple(t.clone() for t in ref2)
    cp2 = pipe2.capture(batch)
    cp2.replay()
    torch.cuda.synchronize()
    assert not cp2.stale() and cp.stale()
    assert int(ref2[1].min().item()) > 50 and not _same_packed(ref2, ref) and _same_packed((cp2.boxes, cp2.counts), ref2)
    set_math(model, 'f32')
