"""CPU: csrc/lsa.h's prefix driver (lsa_assign_prefix), built for the host with one "thread", against scipy on every prefix.

The claim under test is the one csrc/eval_match.hip rests on: rows enter the shortest-augmenting-path solver one at a time, and after
row n - 1 its state is an optimal assignment of rows 0..n-1 - so one solve over G real columns (cost 1 - w) and P "unmatched"
columns (cost 1) passes through the maximum-weight matching of every leading row set.  tests/eval_match_host_main.cpp writes the valid
pairs (w > 0) after every row; each is compared with an independent scipy.optimize.linear_sum_assignment(maximize=True) of that
prefix.  Weights are uniform float32 draws, thresholded at 0.5 (w >= 0.5 ? w : 0) and thinned, so the optimum of a prefix is unique
(a tie needs two sums of distinct draws to coincide) and equal pair sets, not only equal totals, are asked for.

Shapes: 300 random problems with P <= 14, G <= 10 (P = 0 and G = 0 among them by construction), P = 0, G = 0, all weights zero, and
one 280 x 20 problem.  The last test checks that lsa_assign, whose loop body moved into a function of its own, still writes the bytes
it wrote before: tests/golden/lsa_assign_parent.bin holds the output of tests/lsa_host_main.cpp on tests/lsa_cases.SHAPES, recorded
at the commit before the move.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import lsa_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(src, exe):
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'detzero_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', src), '-o', exe])


def _weights(rng, p, g, keep=0.6):
    w = rng.rand(p, g).astype(np.float32)
    w[w < 0.5] = 0
    w[rng.rand(p, g) > keep] = 0
    return w


@pytest.fixture(scope='module')
def problems():
    rng = np.random.RandomState(20240)
    out = [('random_%d' % i, _weights(rng, rng.randint(0, 15), rng.randint(0, 11))) for i in range(300)]
    out.append(('no_predictions', np.zeros((0, 7), dtype=np.float32)))
    out.append(('no_ground_truth', np.zeros((9, 0), dtype=np.float32)))
    out.append(('all_zero', np.zeros((8, 6), dtype=np.float32)))
    out.append(('280x20', _weights(rng, 280, 20, keep=0.5)))
    return out


@pytest.fixture(scope='module')
def host_prefixes(problems, tmp_path_factory):
    work = tmp_path_factory.mktemp('eval_match_host')
    exe, inp, outp = str(work / 'eval_match_host_main'), str(work / 'problems.bin'), str(work / 'results.bin')
    _compile('eval_match_host_main.cpp', exe)
    with open(inp, 'wb') as f:
        f.write(np.int32(len(problems)).tobytes())
        for _, w in problems:
            f.write(np.array(w.shape, dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(w, dtype=np.float32).tobytes())
    subprocess.check_call([exe, inp, outp], timeout=120)
    raw = np.fromfile(outp, dtype=np.int32)
    out, at = [], 0
    for _, w in problems:
        status, at = raw[at], at + 1
        prefixes = []
        for n in range(1, w.shape[0] + 1):
            prefixes.append(raw[at:at + n])
            at += n
        out.append((status, prefixes))
    assert at == len(raw)
    return out


def _scipy_pairs(w):
    from scipy.optimize import linear_sum_assignment
    if 0 in w.shape:
        return set()
    rows, cols = linear_sum_assignment(w.astype(np.float64), maximize=True)
    return {(int(r), int(c)) for r, c in zip(rows, cols) if w[r, c] > 0}


def test_every_prefix_is_the_optimum_of_its_rows(problems, host_prefixes):
    checked = 0
    for (name, w), (status, prefixes) in zip(problems, host_prefixes):
        assert status == 0, name
        assert len(prefixes) == w.shape[0], name
        for n, cols in enumerate(prefixes, start=1):
            got = {(r, int(c)) for r, c in enumerate(cols) if c >= 0}
            assert got == _scipy_pairs(w[:n]), (name, n)
            checked += 1
    assert checked > 2000


def test_shapes_cover_the_edges(problems):
    shapes = [w.shape for _, w in problems]
    assert any(p == 0 and g > 0 for p, g in shapes) and any(g == 0 and p > 0 for p, g in shapes)
    assert any(p > g > 0 for p, g in shapes) and any(g > p > 0 for p, g in shapes) and (280, 20) in shapes
    assert any(not w.any() and w.size for _, w in problems)


def test_matching_changes_as_the_prefix_grows(problems, host_prefixes):
    """The prefixes are not nested: somewhere a row that was matched to one ground truth holds another after a later row entered."""
    moved = 0
    for (_, w), (_, prefixes) in zip(problems, host_prefixes):
        for a, b in zip(prefixes, prefixes[1:]):
            moved += int(((a >= 0) & (a != b[:len(a)])).any())
    assert moved > 50


def test_lsa_assign_writes_the_bytes_it_wrote_before(tmp_path):
    cases = lsa_cases.problems(lsa_cases.SHAPES)
    exe, inp, outp = str(tmp_path / 'lsa_host_main'), str(tmp_path / 'problems.bin'), str(tmp_path / 'results.bin')
    _compile('lsa_host_main.cpp', exe)
    with open(inp, 'wb') as f:
        f.write(np.int32(len(cases)).tobytes())
        for _, cost in cases:
            f.write(np.array(cost.shape, dtype=np.int32).tobytes())
            f.write(np.float64(lsa_cases.THRESHOLD).tobytes())
            f.write(np.ascontiguousarray(cost, dtype=np.float32).tobytes())
    subprocess.check_call([exe, inp, outp], timeout=120)
    with open(outp, 'rb') as f, open(os.path.join(ROOT, 'tests', 'golden', 'lsa_assign_parent.bin'), 'rb') as g:
        assert f.read() == g.read()
