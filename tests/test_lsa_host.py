"""CPU: the assignment core of csrc/lsa.h, built for the host with one "thread", against GNN_assignment (scipy).

The device runs the same header cooperatively across a workgroup (csrc/lsa.hip, tests/test_gpu_lsa.py); here a small stand-alone
program (tests/lsa_host_main.cpp) is compiled with the host compiler and run as a child process over a file of problems:
the shapes 0x5, 5x0, 1x1, 3x5, 5x3, 64x64, 65x130, 130x65 (a sparse and a dense matrix each), a matrix with every entry at or above
the threshold, one with a fully masked row and column, and ones where a masked pair lies on the unconstrained optimum.
Seeds: shape k of tests/lsa_cases.SHAPES uses seeds 2k (sparse) and 2k + 1 (dense); all of them pass the uniqueness pre-check.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import lsa_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def cases():
    return lsa_cases.problems(lsa_cases.SHAPES)


@pytest.fixture(scope='module')
def host_results(cases, tmp_path_factory):
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    work = tmp_path_factory.mktemp('lsa_host')
    exe, inp, outp = str(work / 'lsa_host_main'), str(work / 'problems.bin'), str(work / 'results.bin')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'detzero_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'lsa_host_main.cpp'), '-o', exe])
    with open(inp, 'wb') as f:
        f.write(np.int32(len(cases)).tobytes())
        for _, cost in cases:
            f.write(np.array(cost.shape, dtype=np.int32).tobytes())
            f.write(np.float64(lsa_cases.THRESHOLD).tobytes())
            f.write(np.ascontiguousarray(cost, dtype=np.float32).tobytes())
    subprocess.check_call([exe, inp, outp], timeout=120)
    raw = np.fromfile(outp, dtype=np.int32)
    out, at = [], 0
    for _, cost in cases:
        rows, cols = cost.shape
        counts = raw[at:at + 4]
        row_to_col = raw[at + 4:at + 4 + rows]
        rows_free = raw[at + 4 + rows:at + 4 + 2 * rows]
        cols_free = raw[at + 4 + 2 * rows:at + 4 + 2 * rows + cols]
        at += 4 + 2 * rows + cols
        out.append((counts, row_to_col, rows_free, cols_free))
    assert at == len(raw)
    return out


def test_cases_have_a_unique_optimum_by_a_margin(cases):
    """scipy alone: the matched set does not move when every cost moves by +-1e-6."""
    for name, cost in cases:
        assert lsa_cases.unique_by_margin(cost), name


def test_special_cases_are_what_they_claim(cases):
    by_name = dict(cases)
    assert (by_name['all_masked'] >= lsa_cases.THRESHOLD).all()
    m = by_name['masked_row_and_column']
    assert (m[4] >= 1).all() and (m[:, 6] >= 1).all() and (np.delete(np.delete(m, 4, 0), 6, 1) < 1).all()
    from scipy.optimize import linear_sum_assignment
    for name in ('masked_pair_on_raw_optimum', 'masked_pairs_in_blocks'):
        m = by_name[name]
        r, c = linear_sum_assignment(m.astype(np.float64))          # the raw matrix, no 5000
        assert (m[r, c][m[r, c] < 3.0] >= lsa_cases.THRESHOLD).any(), name


def test_host_build_matches_gnn_assignment(cases, host_results):
    for (name, cost), (counts, row_to_col, rows_free, cols_free) in zip(cases, host_results):
        want = lsa_cases.expected(cost)
        assert counts[3] == 0, (name, counts)
        at = np.flatnonzero(row_to_col >= 0)
        got = (np.stack([at, row_to_col[at]], axis=1), rows_free[:counts[1]], cols_free[:counts[2]])
        assert counts[0] == len(at) == len(want[0]), (name, counts, len(want[0]))
        assert lsa_cases.same_answer(got, want), name


def test_empty_sides_give_arange_lists(cases, host_results):
    """distance.py:18-19: a 0 x k or k x 0 problem has no matches and every row / column unmatched."""
    seen = 0
    for (name, cost), (counts, row_to_col, rows_free, cols_free) in zip(cases, host_results):
        if 0 in cost.shape:
            seen += 1
            assert counts.tolist() == [0, cost.shape[0], cost.shape[1], 0], name
            assert rows_free.tolist() == list(range(cost.shape[0])) and cols_free.tolist() == list(range(cost.shape[1])), name
    assert seen == 4
