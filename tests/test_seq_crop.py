"""CPU: the sequence crop as built - the checked plan of ops.seq_crop_plan (chunks, count-table rows, refusals), the C entry points'
argument checks, the two kernels' resources from the compiler's report, the one shared inside test, and the orchestration of
object_crop.crop_sequence (frame groups, ranks) on the numpy ops of tests/crop_ref.py against the per-frame oracle."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from detzero_amd import object_crop, ops
from detzero_amd.lib import DetZeroHipError
from tests import seq_crop_cases as C
from tests.crop_ref import NumpyCropOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'detzero_amd', 'csrc')


@pytest.fixture(scope='module')
def lib():
    from detzero_amd import lib as L
    from detzero_amd.build import build
    build(verbose=False)
    return L.load()


def test_chunk_size_is_exported(lib):
    assert lib.dz_seq_crop_chunk_points() == ops.seq_crop_chunk_points() == C.CHUNK and C.CHUNK % 64 == 0


def test_plan_layout():
    """3 frames: 600 points x 2 boxes, 100 points x 0 boxes, 256 points x 3 boxes, chunk 256; reversed rank."""
    rank = np.arange(5)[::-1].copy()
    p = ops.seq_crop_plan([0, 600, 700, 956], [0, 2, 2, 5], rank, 956, 5, chunk=256)
    assert (p.n_frames, p.n_chunks, p.n_entries) == (3, 4, 2 * 3 + 3 * 1)
    np.testing.assert_array_equal(p.chunk_frame, [0, 0, 0, 2])                    # the frame without boxes has no chunk
    np.testing.assert_array_equal(p.chunk_first, [0, 3, 3, 4])
    np.testing.assert_array_equal(p.row_off, [0, 1, 2, 3, 6, 9])                 # segments 0..2 = frame 2's boxes (1 chunk), 3..4 = frame 0's (3)
    assert all(a.dtype == np.int32 for a in (p.pt_off, p.box_off, p.rank, p.row_off, p.chunk_frame, p.chunk_first))
    e = ops.seq_crop_plan([0], [0], None, 0, 0, chunk=256)                        # F = 0
    assert (e.n_frames, e.n_chunks, e.n_entries) == (0, 0, 0)
    z = ops.seq_crop_plan([0, 0, 10], [0, 3, 3], None, 10, 3, chunk=256)          # boxes only where there are no points, and the reverse
    assert (z.n_chunks, z.n_entries) == (0, 0)


@pytest.mark.parametrize('what,args', [
    ('rank repeats an index', ([0, 10], [0, 3], [0, 1, 1], 10, 3)),
    ('rank out of range', ([0, 10], [0, 3], [0, 1, 3], 10, 3)),
    ('rank negative', ([0, 10], [0, 3], [0, -1, 2], 10, 3)),
    ('rank too short', ([0, 10], [0, 3], [0, 1], 10, 3)),
    ('rank of floats', ([0, 10], [0, 3], [0.0, 1.0, 2.0], 10, 3)),
    ('pt_off descends', ([0, 8, 4, 10], [0, 1, 2, 3], None, 10, 3)),
    ('box_off descends', ([0, 4, 8, 10], [0, 2, 1, 3], None, 10, 3)),
    ('pt_off ends short of m', ([0, 4, 9], [0, 1, 3], None, 10, 3)),
    ('pt_off ends past m', ([0, 4, 11], [0, 1, 3], None, 10, 3)),
    ('box_off ends short of b', ([0, 4, 10], [0, 1, 2], None, 10, 3)),
    ('pt_off starts past 0', ([1, 4, 10], [0, 1, 3], None, 10, 3)),
    ('frame counts differ', ([0, 4, 10], [0, 3], None, 10, 3)),
    ('negative m', ([0], [0], None, -1, 0)),
    ('m = 2^31', ([0, 2 ** 31], [0, 1], None, 2 ** 31, 1)),
    ('table entries reach 2^31', ([0, 2 ** 31 - 1], [0, 300], None, 2 ** 31 - 1, 300)),
])
def test_plan_refusals(what, args):
    with pytest.raises(DetZeroHipError):
        ops.seq_crop_plan(*args, chunk=256)


def test_entry_points_refuse_bad_sizes(lib):
    """DZ_ERR_INVALID before anything is launched (no device here): negative sizes, sizes of 2^31, null pointers with chunks to work on."""
    from detzero_amd import lib as L
    nul = None
    geom = lambda m, nb, nf, nch: (nul, m, nul, nul, nb, nul, nul, nul, nf, nul, nul, nch)
    for m, nb, nf, nch, ne in ((-1, 0, 0, 0, 0), (0, -1, 0, 0, 0), (0, 0, -1, 0, 0), (0, 0, 0, -1, 0), (0, 0, 0, 0, -1), (2 ** 31, 1, 1, 0, 0),
                               (1, 2 ** 31, 1, 0, 0), (1, 1, 1, 2 ** 31, 1), (1, 1, 1, 0, 2 ** 31), (10, 3, 1, 1, 3), (0, 0, 0, 1, 1)):
        assert lib.dz_seq_crop_count(*geom(m, nb, nf, nch), nul, ne, nul) == L.ERR_INVALID, (m, nb, nf, nch, ne)
        assert lib.dz_last_error()
        assert lib.dz_seq_crop_fill(*geom(m, nb, nf, nch), nul, nul, ne, nul, 1, nul, nul, 0, nul) == L.ERR_INVALID, (m, nb, nf, nch, ne)
    for words, total in ((0, 0), (1, -1), (1, 2 ** 31)):
        assert lib.dz_seq_crop_fill(*geom(0, 0, 0, 0), nul, nul, 0, nul, words, nul, nul, total, nul) == L.ERR_INVALID, (words, total)
    # nothing to do is not an error: F = 0
    assert lib.dz_seq_crop_count(*geom(0, 0, 0, 0), nul, 0, nul) == 0
    assert lib.dz_seq_crop_fill(*geom(0, 0, 0, 0), nul, nul, 0, nul, 1, nul, nul, 0, nul) == 0


def test_kernels_have_no_scratch(tmp_path):
    """Both kernels: 0 bytes of scratch, no spilled register, a few KiB of static LDS (the compiler's resource report)."""
    src = os.path.join(CSRC, 'seq_crop.hip')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-c', src, '-o', str(tmp_path / 'sc.o'), '-Rpass-analysis=kernel-resource-usage']
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
    kernels = [k for k in kernels if 'k_seq_crop' in k['name']]
    assert sorted('count' in k['name'] for k in kernels) == [False, True], [k['name'] for k in kernels]
    for k in kernels:
        print(k)
        assert int(k['ScratchSize [bytes/lane]']) == 0 and int(k['VGPRs Spill']) == 0 and int(k['SGPRs Spill']) == 0, k
        assert int(k['LDS Size [bytes/block]']) <= 4096 and int(k['VGPRs']) <= 64, k


def test_one_body_for_the_inside_test():
    """The margins and the double comparison exist once, in pib_test.h; head_post.hip and seq_crop.hip include it; no atomics in the new file."""
    body = open(os.path.join(CSRC, 'pib_test.h')).read()
    assert body.count('1e-5f') >= 2 and 'cosf(-q[6])' in body and '(double)q[5] / 2.0' in body
    for f in ('head_post.hip', 'seq_crop.hip'):
        txt = open(os.path.join(CSRC, f)).read()
        assert '#include "pib_test.h"' in txt and 'pib_inside(' in txt and 'pib_stage_box(' in txt, f
        assert '1e-5f' not in txt, f
    assert 'atomic' not in re.sub(r'//.*', '', open(os.path.join(CSRC, 'seq_crop.hip')).read())


# ---------------------------------------------------------------------------------------------------------------- orchestration
def run_cpu(name, **kw):
    frames = [(object_crop.prepare_frame_points(raw, pose), boxes) for raw, pose, boxes in C.sequence(name)]
    return frames, object_crop.crop_sequence(frames, crop_ops=NumpyCropOps(), want_index=True, **kw)


@pytest.mark.parametrize('name', [n for n in C.SHAPES if n != '5x40x6000'])
def test_crop_sequence_orchestration_matches_the_oracle(name):
    frames, res = run_cpu(name)
    want = C.expected(name)
    got = res.to_lists()
    assert len(got) == len(want) == res.num_boxes and res.total == sum(w.shape[0] for w in want)
    for g, w in zip(got, want):
        assert C.same_bytes(g, w)
    allpts = np.concatenate([p for p, _ in frames]) if frames else np.zeros((0, 4))
    assert C.same_bytes(allpts[res.index.numpy()], res.rows.numpy())
    for idx in res.index_lists():
        assert (np.diff(idx) > 0).all()


def test_result_does_not_depend_on_the_frame_groups():
    name = 'tracks6'
    spec = C.SHAPES[name][0]
    rank, _ = C.object_major([t for t, _ in spec])
    for order in ('frame', rank, np.arange(len(rank))[::-1].copy()):
        _, one = run_cpu(name, order=order)
        _, cut = run_cpu(name, order=order, budget_bytes=1)
        assert one.n_groups == 1 and cut.n_groups == len(spec)
        assert C.same_bytes(one.rows.numpy(), cut.rows.numpy()) and C.same_bytes(one.offsets.numpy(), cut.offsets.numpy())
        assert np.array_equal(one.index.numpy(), cut.index.numpy())
        want = C.expected(name)
        got = one.to_lists()
        for b, w in enumerate(want):
            assert C.same_bytes(got[b if isinstance(order, str) else order[b]], w)


def test_frame_groups_respect_the_budget():
    g = object_crop.frame_groups([1000, 1000, 1000, 5000, 10], [2, 2, 2, 2, 2], 2 * (1000 * 44 + 2 * 4 * 16), 256)
    assert g == [(0, 2), (2, 3), (3, 4), (4, 5)]
    assert object_crop.frame_groups([], [], 100, 256) == []


def test_bad_order_is_refused():
    frames = [(object_crop.prepare_frame_points(raw, pose), boxes) for raw, pose, boxes in C.sequence('frame_without_boxes')]
    ops_ = NumpyCropOps()
    for order in (np.array([0, 1, 2, 3, 4, 5, 6, 6]), np.arange(7), np.arange(8) - 1):
        with pytest.raises(DetZeroHipError):
            object_crop.crop_sequence(frames, order=order, crop_ops=ops_)
    with pytest.raises(ValueError):
        object_crop.crop_sequence(frames, order='object', crop_ops=ops_)
    assert ops_.calls == 0
