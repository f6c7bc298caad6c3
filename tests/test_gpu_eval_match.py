"""GPU: ops.eval_match_counts (csrc/eval_match.hip, one workgroup and ONE solve per problem) against the float64 restatement of
tests/waymo_eval_ref.py (one scipy solve per problem and per cutoff), on the scenes of tests/waymo_eval_cases.py.

The integer counts TP / FP / FN are asked to be EQUAL.  The scenes pass the margin conditions (tests/test_waymo_eval_cpu.py): no IoU
within 1e-4 of its threshold and every prefix matching stable under +-1e-5 on all weights, far above the difference between the
device's fp32 IoU and the restatement's, so a differing count is a bug and not a tie.
Heading accuracy: the device adds, per TP pair, 1 - |d| / pi evaluated in double from the same float32 headings the restatement
reads, rounded to nearest at 2^-32.  The rounding is at most 2^-33 per pair and two double evaluations of the expression differ by a
few 2^-53, so |HA_device - HA_reference| <= TP * 2^-32 for every (shard, level, cutoff); the bound is computed from the TP count of
that entry, nothing is tuned.
"""
import numpy as np
import pytest
import torch

from tests import waymo_eval_cases as cases
from tests import waymo_eval_ref as ref

pytestmark = pytest.mark.gpu

_REF = {}


def _reference(name, config_type, box_type, scene):
    key = (name, tuple(config_type), box_type)
    if key not in _REF:
        _REF[key] = ref.counts(config_type, box_type, *cases.flat(scene))
    return _REF[key]


def _check(table, want_counts, want_ha, want_fixed=None):
    assert table.dtype == np.int64 and table.shape == want_counts.shape[:3] + (4,)
    assert np.array_equal(table[..., :3], want_counts)
    err = np.abs(table[..., 3] / 4294967296.0 - want_ha)
    bound = table[..., 0] * 2.0 ** -32
    assert (err <= bound).all(), (err.max(), bound[err > bound])


@pytest.fixture(scope='module')
def scenes():
    return {'scene%d' % i: cases.scene(seed, types) for i, (seed, types) in enumerate(cases.SCENES)}


@pytest.mark.parametrize('box_type', ['3d', 'bev'])
@pytest.mark.parametrize('config_type', [['object'], ['range']])
@pytest.mark.parametrize('name', ['scene0', 'scene1'])
def test_counts_equal_the_restatement(device, scenes, name, config_type, box_type):
    from detzero_amd import waymo_eval
    s = scenes[name]
    arrays = waymo_eval.problem_arrays(config_type, *cases.flat(s))
    table = waymo_eval.match_counts(config_type, s['n_frames'], *arrays, box_type=box_type, device=device)
    want_counts, want_ha, _ = _reference(name, config_type, box_type, s)
    assert want_counts[..., 0].sum() > 0 and want_counts[..., 1].sum() > 0 and want_counts[..., 2].sum() > 0
    _check(table, want_counts, want_ha)
    slots = waymo_eval.match_counts(config_type, s['n_frames'], *arrays, box_type=box_type, scheme='slots', device=device)
    assert np.array_equal(slots, table)                         # the two accumulation schemes give the same bits


def _host_problems(scene, config_type=('object',)):
    """Sorted device inputs and the host descriptor table (n,6) of a scene, in numpy: (problem, descending score, input index)."""
    from detzero_amd import waymo_eval
    pk, pb, ps, gk, gb, gd, n_shards = waymo_eval.problem_arrays(list(config_type), *cases.flat(scene))
    order = np.lexsort((np.arange(len(pk)), -ps.astype(np.float64), pk))
    g_order = np.argsort(gk, kind='stable')
    pk, pb, ps, gk, gb, gd = pk[order], pb[order], ps[order], gk[g_order], gb[g_order], gd[g_order]
    desc = []
    for key in sorted(set(pk.tolist()) | set(gk.tolist())):
        p, g = np.flatnonzero(pk == key), np.flatnonzero(gk == key)
        shard = key % n_shards
        desc.append((p[0] if len(p) else 0, len(p), g[0] if len(g) else 0, len(g), shard, int(waymo_eval.shard_type(list(config_type), shard))))
    return pb, ps, gb, gd, np.array(desc, dtype=np.int64), n_shards


def _dev(device, pb, ps, gb, gd):
    return (torch.from_numpy(pb).to(device), torch.from_numpy(ps).to(device), torch.from_numpy(gb).to(device), torch.from_numpy(gd).to(device))


@pytest.mark.parametrize('seed,n_pred,n_gt', cases.SINGLES)
def test_large_single_problems(device, seed, n_pred, n_gt):
    """280 x 20: more columns (300) than the workgroup has threads.  900 x 200: 1100 columns, the solver's vectors live in the
    workspace slice instead of LDS."""
    from detzero_amd import ops
    s = cases.single(seed, n_pred, n_gt)
    pb, ps, gb, gd, desc, n_shards = _host_problems(s)
    assert desc.shape == (1, 6) and desc[0, 1] == n_pred and desc[0, 3] == n_gt
    for box_type in ('3d', 'bev'):
        want_counts, want_ha, _ = _reference('single_%d_%d' % (n_pred, n_gt), ['object'], box_type, s)
        assert want_counts[0, 1, 0, 0] > n_gt // 2
        for scheme in ('atomic', 'slots'):
            _check(ops.eval_match_counts(*_dev(device, pb, ps, gb, gd), desc, n_shards, box_type, scheme=scheme), want_counts, want_ha)


def test_empty_problems_among_full_ones(device, scenes):
    from detzero_amd import ops
    s = scenes['scene0']
    pb, ps, gb, gd, desc, n_shards = _host_problems(s)
    plain = ops.eval_match_counts(*_dev(device, pb, ps, gb, gd), desc, n_shards)
    empty = np.array([(len(pb) if i % 2 else 0, 0, len(gb) if i % 3 else 0, 0, i % 4, i % 4 + 1) for i in range(64)], dtype=np.int64)
    mixed = np.concatenate([empty[:20], desc[:7], empty[20:50], desc[7:], empty[50:]])
    assert (mixed[:, 1] + mixed[:, 3] == 0).sum() >= 64
    for scheme in ('atomic', 'slots'):
        assert np.array_equal(ops.eval_match_counts(*_dev(device, pb, ps, gb, gd), mixed, n_shards, scheme=scheme), plain)
    _check(plain, *_reference('scene0', ['object'], '3d', s))


def test_same_input_twice_gives_the_same_bits(device, scenes):
    from detzero_amd import ops
    pb, ps, gb, gd, desc, n_shards = _host_problems(scenes['scene0'], ('object', 'range'))
    d = _dev(device, pb, ps, gb, gd)
    a, st_a = ops.eval_match_counts_nosync(*d, desc, n_shards)
    b, st_b = ops.eval_match_counts_nosync(*d, desc[::-1].copy(), n_shards)          # and in another problem order
    assert torch.equal(a, b) and int(st_a.item()) == 0 and int(st_b.item()) == 0
    assert int(a[..., 0].sum().item()) > 0


def test_descriptor_that_leaves_its_buffers_is_a_status(device, scenes):
    """Descriptors outside the predictions, the ground truths, the shards, the types, the size limit and the workspace: the status
    word says so, the table is as it was, and the good problems next to them are counted."""
    from detzero_amd import ops
    from detzero_amd import lib as L
    from detzero_amd.lib import DetZeroHipError
    pb, ps, gb, gd, desc, n_shards = _host_problems(scenes['scene0'])
    d = _dev(device, pb, ps, gb, gd)
    n_p, n_g = len(pb), len(gb)
    room = 1 << 20
    bad = np.array([
        (n_p - 2, 5, 0, 3, 0, 1, 0),                # predictions past the end
        (0, 3, n_g - 1, 4, 0, 1, 0),                # ground truths past the end
        (-1, 3, 0, 3, 0, 1, 0), (0, 3, 0, -2, 0, 1, 0),
        (0, 3, 0, 3, n_shards, 1, 0), (0, 3, 0, 3, -1, 1, 0),
        (0, 3, 0, 3, 0, 5, 0), (0, 3, 0, 3, 0, -1, 0),
        (0, 3000, 0, 2000, 0, 1, 0),                # P + G beyond DZ_LSA_MAX_DIM (and beyond the buffers)
        (0, 3, 0, 3, 0, 1, room - 16),              # the slice leaves the workspace
        (0, 3, 0, 3, 0, 1, 8), (0, 3, 0, 3, 0, 1, -256),
        (1 << 40, 3, 0, 3, 0, 1, 0), (0, 1 << 40, 0, 3, 0, 1, 0),
    ], dtype=np.int64)
    table = torch.full((n_shards, 2, 101, 4), 12345, dtype=torch.int64, device=device)
    out, status = ops.eval_match_counts_nosync(*d, torch.from_numpy(bad).to(device), n_shards, table=table, ws_bytes=room)
    torch.cuda.synchronize()
    assert int(status.item()) == 1 and out is table and bool((table == 12345).all())
    # among good ones: their counts, and the status
    good = np.zeros((len(desc), 7), dtype=np.int64)
    good[:, :6] = desc
    lib = L.load()
    need = np.array([lib.dz_eval_match_ws_bytes(int(p), int(g)) for p, g in desc[:, [1, 3]]], dtype=np.int64)
    good[:, 6] = np.cumsum(need) - need
    assert need.sum() <= room
    mixed = np.concatenate([bad[:5], good, bad[5:]])
    out, status = ops.eval_match_counts_nosync(*d, torch.from_numpy(mixed).to(device), n_shards, ws_bytes=room)
    assert int(status.item()) == 1
    assert np.array_equal(out.cpu().numpy(), ops.eval_match_counts(*d, desc, n_shards))
    with pytest.raises(DetZeroHipError):            # beyond the size limit, said by the host: refused before any launch
        ops.eval_match_counts(*d, np.array([(0, 3000, 0, 2000, 0, 1)]), n_shards)
