"""GPU: dz_mot_chain_counts (csrc/mot_chain.hip, k_mot_chain) on weights the test supplies, against the float64 restatement of the
protocol (tests/mot_eval_ref.py) - integer for integer, COST included.

The weights are float32 values handed to both sides (the restatement widens them to float64, as the kernel does), so nothing here
depends on the IoU's rounding: every count, and every fixed-point cost term round((1 - w) * 2^32), has one right value.  The scenes
(tests/mot_eval_cases.py) keep every matching stable under +-1e-5 on all weights (checked on the CPU for every seed), so a
differing table is a bug and not a tie.
"""
import numpy as np
import pytest

from tests import mot_eval_cases as cases
from tests import mot_eval_ref as ref

pytestmark = pytest.mark.gpu

CONFIGS = (['object'], ['range'])


def _f32(probs):
    for p in probs:
        p['w'] = p['w'].astype(np.float32).astype(np.float64)
    return probs


@pytest.fixture(scope='module')
def scene_tables():
    """{(seed, config)}: (problems with float32-valued weights, n_shards, the restatement's table) - computed once, read-only."""
    out = {}
    for seed in cases.SEEDS:
        s = cases.scene(seed)
        for config_type in CONFIGS:
            probs = _f32(ref.problems(config_type, '3d', s))
            n = ref.det_ref.n_shards_of(config_type)
            table = ref.table_from_problems(probs, n)
            table.setflags(write=False)
            out[(seed, tuple(config_type))] = (probs, n, table)
    return out


def _run(device, probs, n_shards, mapping='wave', merge=True, edit=None, nosync=False):
    import torch
    from detzero_amd import ops
    w, cut, pid, gid, gd, pdesc, cdesc, frames = cases.device_inputs(probs)
    if edit is not None:
        pdesc, cdesc, frames = edit(pdesc, cdesc, frames)
    pdesc6, w_len = ops.mot_problem_desc(pdesc)
    assert w_len == w.size
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    args = (t(w), t(cut), t(pid), t(gid), t(gd), pdesc6, cdesc, frames, n_shards, mapping, merge)
    if nosync:
        table, status = ops.mot_chain_counts_nosync(*args)
        return table.cpu().numpy(), int(status.item())
    return ops.mot_chain_counts(*args)


@pytest.mark.parametrize('config_type', CONFIGS, ids=['object', 'range'])
@pytest.mark.parametrize('seed', cases.SEEDS)
def test_table_equals_the_restatement(device, scene_tables, seed, config_type):
    probs, n, want = scene_tables[(seed, tuple(config_type))]
    got = _run(device, probs, n)
    assert got.shape == want.shape and got.dtype == np.int64
    diff = np.argwhere(got != want)
    assert diff.size == 0, (len(diff), diff[:5].tolist(), got[tuple(diff[0])], want[tuple(diff[0])])
    assert want[..., 3].max() >= 3 and want[..., 4].max() > 0


def test_hand_counted_chains(device):
    hand = cases.hand_cases()
    cost = int(np.round((1.0 - float(np.float32(0.8))) * 4294967296.0))
    for name, probs in hand.items():
        got = _run(device, probs, 4)
        assert np.array_equal(got, ref.table_from_problems(probs, 4)), name
        assert not got[1:].any()
        if name == 'perfect':
            assert got[0, 1, 0].tolist() == [12, 0, 0, 0, 0] and got[0, 0, 31].tolist() == [4, 0, 4, 0, 0] and got[0, 1, 91].tolist() == [0, 0, 12, 0, 0]
        if name == 'swap':
            assert all(got[0, 0, k].tolist() == [12, 0, 0, 2, 12 * cost] for k in range(81))
            assert all(got[0, 0, k].tolist() == [6, 0, 6, 1, 6 * cost] for k in range(81, 91))
        if name == 'dropped':
            assert (got[0, 1] == np.array([0, 0, 12, 0, 0])).all()


def _big_chain():
    """One type, two frames of P = 100 predictions and G = 93 ground truths: P + G = 193 is the smallest size above the LDS column
    bound (DZ_MOT_LDS_DIM = 192).  Random weights on a band, so the optimum is not the diagonal; the second frame keeps the ids,
    moves the weights and drops every third prediction's overlap, so carry, match and update all run on workspace vectors."""
    rng = np.random.RandomState(7)
    P, G = 100, 93
    probs = []
    for f in range(2):
        w = np.zeros((P, G))
        for i in range(P):
            for j in range(max(0, i - 2), min(G, i + 3)):
                if rng.rand() < 0.7:
                    w[i, j] = rng.uniform(0.5, 0.99)
        if f == 1:
            w[::3] = 0.0
        score = np.sort(rng.uniform(0.0, 1.0, P).astype(np.float32))[::-1]
        probs.append(cases._hand_problem(f, w, score, np.arange(P) if f == 0 else rng.permutation(P), np.arange(G), rng.randint(1, 3, G)))
    probs[1]['score'] = probs[0]['score']
    return probs


def test_a_frame_above_the_lds_bound(device):
    from detzero_amd import ops
    probs = _big_chain()
    assert len(probs[0]['pid']) + len(probs[0]['gid']) == ops.MOT_LDS_DIM + 1
    want = ref.table_from_problems(probs, 4)
    for mapping in ('wave', 'workgroup'):
        assert np.array_equal(_run(device, probs, 4, mapping), want), mapping
    assert want[0, 1, 0, 3] > 0 and want[0, 1, 0, 0] > 100


def test_an_empty_chain_among_full_ones(device, scene_tables):
    probs, n, want = scene_tables[(cases.SEEDS[0], ('object',))]

    def edit(pdesc, cdesc, frames):
        empty = np.array([[int(cdesc[2, 0]), 0, 3, 0, 0, 0]], dtype=np.int64)              # no frame, no id, in the middle
        return pdesc, np.concatenate([cdesc[:2], empty, cdesc[2:]]), frames
    assert np.array_equal(_run(device, probs, n, edit=edit), want)


def test_same_input_same_bits_and_both_mappings(device, scene_tables):
    probs, n, want = scene_tables[(cases.SEEDS[1], ('range',))]
    first = _run(device, probs, n, 'wave')
    assert np.array_equal(first, _run(device, probs, n, 'wave'))
    assert np.array_equal(first, _run(device, probs, n, 'workgroup'))
    assert np.array_equal(first, want)


def test_unmerged_cutoffs_give_the_same_table(device, scene_tables):
    probs, n, want = scene_tables[(cases.SEEDS[0], ('object',))]
    assert np.array_equal(_run(device, probs, n, merge=False), want)
    hand = cases.hand_cases()['swap']
    assert np.array_equal(_run(device, hand, 4, merge=False), _run(device, hand, 4, merge=True))


@pytest.mark.parametrize('what', ['frames', 'ids', 'problem', 'size'])
def test_a_bad_descriptor_sets_the_status_and_adds_nothing(device, scene_tables, what):
    from detzero_amd import ops
    probs, n, want = scene_tables[(cases.SEEDS[0], ('object',))]
    victim = 1                                                                  # the second chain: (sequence 0, shard 1)
    key = (probs[cases.device_inputs(probs)[6][victim, 0]]['seq'], probs[cases.device_inputs(probs)[6][victim, 0]]['shard'])
    others = ref.table_from_problems([p for p in probs if (p['seq'], p['shard']) != key], n)
    assert not np.array_equal(others, want)

    def edit(pdesc, cdesc, frames):
        pdesc, cdesc, frames = pdesc.copy(), cdesc.copy(), frames.copy()
        if what == 'frames':
            cdesc[victim, 1] = len(frames) + 5                                  # its frame list leaves `frames`
        elif what == 'ids':
            cdesc[victim, 3] = 1                                                # fewer prediction ids than its predictions name
        elif what == 'problem':
            frames[cdesc[victim, 0] + 1] = len(pdesc) + 3                       # a frame that names no problem
        else:
            cdesc[victim, 5] = 1                                                # its frames are larger than it says
        return pdesc, cdesc, frames
    got, status = _run(device, probs, n, edit=edit, nosync=True)
    assert status == 1 and np.array_equal(got, others)
    with pytest.raises(ops.L.DetZeroHipError):
        _run(device, probs, n, edit=edit)


def test_a_frame_beyond_the_limit_is_unsupported(device):
    from detzero_amd import ops
    probs = [cases._hand_problem(0, np.zeros((4000, 97)), np.zeros(4000), np.arange(4000), np.arange(97), np.ones(97))]
    with pytest.raises(ops.L.DetZeroHipError):
        _run(device, probs, 4)
