"""CPU: the host-side rules that keep the detector's cached device state consistent with its weights - the eviction policy of the
zero-response cache (det_modules.PinnedLRU), the stale mark of the fp16-pair pre-scale after load_state_dict (det_modules._Cached._e)
and the staleness predicate of captured passes (det_modules.plan_snapshot / plans_changed).  No device is touched: the GPU side of the
same rules is tests/test_gpu_state_lifecycle.py."""
import pytest
import torch

from detzero_amd.synth import VOXEL_SIZE_02
from tests.util import cpu_state_dict, make_model

MODULES = ('backbone3d', 'backbone2d', 'dense_head')
STAGES = ('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4', 'encoded', 'spatial_features_2d')
EXPS = {s: 3 + i for i, s in enumerate(STAGES)}          # (all different and none 0: a wrong stage or a reset shows)


# ------------------------------------------------------------------------------------------------ cache policy
def test_lru_evicts_the_least_recently_used_key_one_at_a_time():
    from detzero_amd.det_modules import PinnedLRU
    c = PinnedLRU(4)
    for k in 'abcd':
        assert c.put(k, k.upper()) == []
    assert c.unpinned() == list('abcd') and len(c) == 4
    assert c.put('e', 'E') == [('a', 'A')]               # beyond the bound: exactly one entry, the oldest, comes back
    assert 'a' not in c and 'a' not in c.store and c.get('a') is None
    assert c.put('f', 'F') == [('b', 'B')]
    assert c.unpinned() == list('cdef') and sorted(c.store) == list('cdef')


def test_lru_hit_refreshes_recency():
    from detzero_amd.det_modules import PinnedLRU
    c = PinnedLRU(4)
    for k in 'abcd':
        c.put(k, k.upper())
    # 'a' is the oldest INSERTION; a key that keeps being hit between insertions is never the one that goes
    for new, gone in (('e', 'b'), ('f', 'c'), ('g', 'd'), ('h', 'e'), ('i', 'f')):
        assert c.get('a') == 'A'
        assert c.put(new, new.upper()) == [(gone, gone.upper())]
        assert 'a' in c and len(c.unpinned()) == 4
    assert c.get('missing') is None and c.get('missing', 7) == 7
    assert c.put('a', 'A2') == [] and c.get('a') == 'A2' and len(c.unpinned()) == 4          # replacing a key evicts nothing


def test_lru_pinned_keys_survive_and_do_not_count():
    from detzero_amd.det_modules import PinnedLRU
    store = {'not a cache key': 1}                        # (the detector keeps the values in the plan entry next to other things)
    c = PinnedLRU(4, store=store)
    c.put('p', 'P')
    c.put('q', 'Q')
    c.pin('p')
    c.pin('p')                                            # (again: no-op)
    with pytest.raises(KeyError):
        c.pin('never inserted')
    evicted = []
    for i in range(100):
        out = c.put(i, str(i))
        assert len(out) <= 1                              # never more than one entry per insertion
        evicted += [k for k, _ in out]
        assert len(c.unpinned()) <= 4 and 'p' in c and store['p'] == 'P' and c.get('p') == 'P'
    assert c.pinned() == {'p'} and c.unpinned() == [96, 97, 98, 99] and len(c) == 5
    assert evicted == ['q'] + list(range(96))             # in order of use, each exactly once
    assert sorted(k for k in store if k != 'not a cache key' and k != 'p') == [96, 97, 98, 99] and store['not a cache key'] == 1
    c.pin(97)                                             # a pin frees a slot of the unpinned population
    assert c.put('x', 'X') == [] and c.put('y', 'Y') == [(96, '96')]
    assert c.put('p', 'P2') == [] and c.get('p') == 'P2' and c.pinned() == {'p', 97}          # a pinned key can be rewritten, stays pinned


# ------------------------------------------------------------------------------------------------ stale pre-scale
@pytest.fixture(scope='module')
def weights():
    """State dicts of the seed-0 and seed-1 detectors (CPU) and a factory of fresh seed-0 models."""
    sd1 = cpu_state_dict(make_model(VOXEL_SIZE_02, seed=1)[0])
    return sd1, (lambda: make_model(VOXEL_SIZE_02, seed=0)[0])


def _set_math(model, mid):
    for name in MODULES:
        getattr(model, name).set_math(mid)


def test_reload_marks_the_prescale_stale_in_fp16_pair_storage_only(weights):
    from detzero_amd.centerpoint import set_prescale
    from detzero_amd.lib import DetZeroHipError
    sd1, fresh = weights
    model = fresh()
    set_prescale(model, EXPS)
    _set_math(model, 1)
    for name in MODULES:
        assert [getattr(model, name)._e(s) for s in STAGES] == [EXPS[s] for s in STAGES]
    model.load_state_dict(sd1)
    for name in MODULES:
        mod = getattr(model, name)
        assert mod._plan is None and mod.act_exp == EXPS              # marked, not reset: no one-sided change of the exponents
        for mid in (1, 3):                                            # ('f16' computes on the tensors of 'f16x2': the same storage)
            mod.set_math(mid)
            for s in STAGES:
                with pytest.raises(DetZeroHipError) as ei:
                    mod._e(s)
                assert type(mod).__name__ in str(ei.value) and 'select_math' in str(ei.value) and 'set_prescale' in str(ei.value)
        for mid in (0, 2):                                            # f32 / bf16 pairs take no pre-scale: select_math's calibration pass runs
            mod.set_math(mid)
            assert [mod._e(s) for s in STAGES] == [0] * len(STAGES)
    # set_prescale(exps) clears the mark ...
    _set_math(model, 1)
    shifted = {s: e + 1 for s, e in EXPS.items()}
    set_prescale(model, shifted)
    for name in MODULES:
        assert [getattr(model, name)._e(s) for s in STAGES] == [shifted[s] for s in STAGES]
    # ... and so does set_prescale(None)
    model.load_state_dict(sd1)
    with pytest.raises(DetZeroHipError):
        model.backbone2d._e('encoded')
    set_prescale(model, None)
    for name in MODULES:
        assert [getattr(model, name)._e(s) for s in STAGES] == [0] * len(STAGES)
    # a device move keeps the values, so it keeps the exponents too
    set_prescale(model, EXPS)
    model.float()                                                     # (goes through _apply, as .to(device) does)
    for name in MODULES:
        assert getattr(model, name)._plan is None and getattr(model, name)._e('x_conv2') == EXPS['x_conv2']


def test_reload_without_a_prescale_and_into_one_submodule(weights):
    from detzero_amd.centerpoint import set_prescale
    from detzero_amd.lib import DetZeroHipError
    sd1, fresh = weights
    model = fresh()
    _set_math(model, 1)
    model.load_state_dict(sd1)                                        # never had a pre-scale: nothing to go stale
    for name in MODULES:
        assert [getattr(model, name)._e(s) for s in STAGES] == [0] * len(STAGES)
    set_prescale(model, EXPS)
    sub = {k[len('backbone2d.'):]: v for k, v in sd1.items() if k.startswith('backbone2d.')}
    model.backbone2d.plan()
    model.dense_head.plan()
    model.backbone2d.load_state_dict(sub)                             # one submodule: only it is marked, only its plan goes
    with pytest.raises(DetZeroHipError):
        model.backbone2d._e('spatial_features_2d')
    assert model.backbone2d._plan is None and model.dense_head._plan is not None
    assert model.backbone3d._e('encoded') == EXPS['encoded'] and model.dense_head._e('spatial_features_2d') == EXPS['spatial_features_2d']


# ------------------------------------------------------------------------------------------------ staleness of a capture
class _Mod:
    def __init__(self, plan):
        self._plan = plan


class _Model:
    def __init__(self, *mods):
        self.mods = list(mods)

    def modules(self):
        return iter(self.mods)


def test_capture_staleness_is_plan_identity_per_model():
    from detzero_amd.det_modules import plan_snapshot, plans_changed
    a = _Model(_Mod({'w': 1}), _Mod([{'w': 2}]), _Mod(None), object())       # (a module without a plan yet, one that has none at all)
    b = _Model(_Mod({'w': 1}))
    snap_a, snap_b = plan_snapshot(a), plan_snapshot(b)
    assert [m for m, _ in snap_a] == a.mods[:2] and all(p is m._plan for m, p in snap_a)     # strong references to the very objects
    assert not plans_changed(snap_a) and not plans_changed(snap_b) and not plans_changed([])
    a.mods[0]._plan['_pre'] = {}                          # lazily packed weights are added to the SAME plan object: not a change
    a.mods[2]._plan = {'built': 'later'}                  # a module that was not part of the capture builds its plan: not a change
    assert not plans_changed(snap_a)
    b.mods[0]._plan = None                                # another model drops its plan
    assert plans_changed(snap_b) and not plans_changed(snap_a)
    b.mods[0]._plan = {'w': 1}                            # rebuilt with equal contents: still another object
    assert plans_changed(snap_b)
    kept = snap_a[1][1]
    a.mods[1]._plan = None
    assert plans_changed(snap_a) and kept == [{'w': 2}]   # ... and the snapshot still holds what the graph points at


def test_capture_staleness_on_the_detector_modules(weights):
    """The same on the real modules: load_state_dict, invalidate() and a device-move _apply drop the plan; math, pre-scale and engine
    switches keep the object."""
    from detzero_amd.centerpoint import set_prescale
    from detzero_amd.det_modules import plan_snapshot, plans_changed
    sd1, fresh = weights
    model, other = fresh(), fresh()
    for m in (model, other):
        for name in MODULES:
            getattr(m, name).plan()
    snap = plan_snapshot(model)
    assert sorted(type(m).__name__ for m, _ in snap) == ['BaseBEVBackbone', 'CenterHead', 'VoxelResBackBone8x']
    _set_math(model, 2)
    set_prescale(model, EXPS)
    model.backbone2d.set_dense_engine('bf16x3')
    model.backbone3d.set_engine('xrun', 'xrun_bf16x3', 'bf16x3')
    other.load_state_dict(sd1)
    assert not plans_changed(snap)
    model.dense_head.invalidate()
    assert plans_changed(snap)
    snap = plan_snapshot(model)                           # (two modules left with a plan)
    assert len(snap) == 2 and not plans_changed(snap)
    model.load_state_dict(sd1)
    assert plans_changed(snap)
    for name in MODULES:
        getattr(model, name).plan()
    snap = plan_snapshot(model)
    model.double().float()
    assert plans_changed(snap)
