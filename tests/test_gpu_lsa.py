"""GPU: ops.linear_assignment_batch (csrc/lsa.hip, one workgroup per problem) against GNN_assignment (scipy).

The problems are those of tests/test_lsa_host.py plus 257x63 and 63x257 (more columns than the workgroup has threads, both
orientations), all of them in ONE launch - problems of different shapes side by side - and the status word of every problem is
zero.  Each case first passes the uniqueness pre-check of tests/lsa_cases.py (seeds: shape k uses 2k and 2k + 1).
"""
import numpy as np
import pytest
import torch

from tests import lsa_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cases():
    cs = lsa_cases.problems(lsa_cases.GPU_SHAPES)
    for name, cost in cs:
        assert lsa_cases.unique_by_margin(cost), name
    return cs


def test_batch_of_mixed_shapes_matches_scipy(device, cases):
    from detzero_amd import ops
    costs = [torch.from_numpy(c).to(device) for _, c in cases]
    before = [c.clone() for c in costs]
    got = ops.linear_assignment_batch(costs, lsa_cases.THRESHOLD)
    assert len(got) == len(cases)
    for (name, cost), g, c, b in zip(cases, got, costs, before):
        assert torch.equal(c, b), name                                  # the input is not written
        assert lsa_cases.same_answer(g, lsa_cases.expected(cost)), name
        assert g[0].shape[1:] == (2,) and (np.diff(g[0][:, 0]) > 0).all(), name


def test_status_counts_and_offsets(device, cases):
    """The no-sync form: counts (P,4) with status 0 throughout, matched + unmatched = rows, lists at the problems' offsets."""
    from detzero_amd import ops
    flat = torch.from_numpy(np.concatenate([c.reshape(-1) for _, c in cases])).to(device)
    shapes = [c.shape for _, c in cases]
    row_to_col, rows_free, cols_free, counts, row_off, col_off = ops.linear_assignment_batch_nosync(flat, shapes, lsa_cases.THRESHOLD)
    counts, row_to_col, rows_free, cols_free = counts.cpu().numpy(), row_to_col.cpu().numpy(), rows_free.cpu().numpy(), cols_free.cpu().numpy()
    assert counts.shape == (len(cases), 4) and (counts[:, 3] == 0).all()
    for p, (name, cost) in enumerate(cases):
        r, c = cost.shape
        matched, want_rows, want_cols = lsa_cases.expected(cost)
        assert counts[p].tolist() == [len(matched), len(want_rows), len(want_cols), 0], name
        assert rows_free[row_off[p]:row_off[p] + counts[p, 1]].tolist() == want_rows.tolist(), name
        assert cols_free[col_off[p]:col_off[p] + counts[p, 2]].tolist() == want_cols.tolist(), name
        r2c = row_to_col[row_off[p]:row_off[p] + r]
        assert (r2c >= 0).sum() == len(matched) and r2c[matched[:, 0]].tolist() == matched[:, 1].tolist(), name


def test_single_problem_and_repeat(device, cases):
    """One problem per launch gives what the batch gave; a second call gives the same bytes."""
    from detzero_amd import ops
    name, cost = [c for c in cases if c[0].startswith('sparse_65x130')][0]
    a = ops.linear_assignment_batch([torch.from_numpy(cost).to(device)], lsa_cases.THRESHOLD)[0]
    b = ops.linear_assignment_batch([torch.from_numpy(cost).to(device)], lsa_cases.THRESHOLD)[0]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert lsa_cases.same_answer(a, lsa_cases.expected(cost))
    assert ops.linear_assignment_batch([]) == []


def test_vectors_in_the_workspace(device):
    """max(rows, cols) > 1024: the per-column vectors live in the problem's workspace slice, next to a small problem in LDS."""
    from detzero_amd import ops
    from detzero_amd import lib as L
    lib = L.load()
    assert lib.dz_lsa_ws_bytes(1024, 1024) == 0 and lib.dz_lsa_ws_bytes(0, 5000) == 0
    need = lib.dz_lsa_ws_bytes(40, 1030)          # 2 * 1030 + 40 doubles, 3 * 1030 + 40 ints
    assert need >= (2 * 1030 + 40) * 8 + (3 * 1030 + 40) * 4 and need % 256 == 0 and need == lib.dz_lsa_ws_bytes(1030, 40)
    big, small = lsa_cases.sparse(40, 1030, 40, keep=0.01), lsa_cases.dense(5, 3, 41)
    assert lsa_cases.unique_by_margin(big) and lsa_cases.unique_by_margin(small)
    tall = np.ascontiguousarray(big.T)
    got = ops.linear_assignment_batch([torch.from_numpy(m).to(device) for m in (big, small, tall)], lsa_cases.THRESHOLD)
    for g, m in zip(got, (big, small, tall)):
        assert lsa_cases.same_answer(g, lsa_cases.expected(m))


@pytest.mark.parametrize('shapes,sum_is_less', [([(1100, 50), (300, 300)], True), ([(2000, 1), (1, 1000)], True),
                                                ([(300, 300), (40, 1100), (1100, 50), (5, 3)], False)],
                         ids=['1100x50+300x300', '2000x1+1x1000', 'two-slices-between-lds-problems'])
def test_largest_rows_and_columns_from_different_problems(device, shapes, sum_is_less):
    """The batch's largest row count and largest column count come from different problems.  In the first two batches a workspace
    for one (max rows) x (max cols) problem would be larger than the sum of the slices; in the third (two slices) smaller.  The sum
    is what the call needs either way: one slice per problem with a side > 1024, none for the others, every status 0."""
    from detzero_amd import ops
    from detzero_amd import lib as L
    lib = L.load()
    total = sum(lib.dz_lsa_ws_bytes(r, c) for r, c in shapes)
    assert total > 0 and (total < lib.dz_lsa_ws_bytes(max(r for r, _ in shapes), max(c for _, c in shapes))) == sum_is_less
    mats = [lsa_cases.dense(r, c, 50 + k) if min(r, c) == 1 else lsa_cases.sparse(r, c, 50 + k) for k, (r, c) in enumerate(shapes)]
    for m in mats:
        assert lsa_cases.unique_by_margin(m), m.shape
    flat = torch.from_numpy(np.concatenate([m.reshape(-1) for m in mats])).to(device)
    counts = ops.linear_assignment_batch_nosync(flat, shapes, lsa_cases.THRESHOLD)[3].cpu().numpy()
    assert (counts[:, 3] == 0).all(), counts
    got = ops.linear_assignment_batch([torch.from_numpy(m).to(device) for m in mats], lsa_cases.THRESHOLD)
    for g, m in zip(got, mats):
        assert lsa_cases.same_answer(g, lsa_cases.expected(m)), m.shape


def test_slice_outside_the_workspace_is_a_status_not_a_write(device):
    """The library call itself with a workspace one slice short: the problem whose slice leaves it gets status 3 and writes its
    counts only, the problem whose slice fits and the one in LDS are solved."""
    from detzero_amd import ops
    from detzero_amd import lib as L
    lib = L.load()
    shapes = [(40, 1030), (5, 3), (1030, 40)]
    mats = [lsa_cases.sparse(40, 1030, 40, keep=0.01), lsa_cases.dense(5, 3, 41)]
    mats.append(np.ascontiguousarray(mats[0].T))
    one = lib.dz_lsa_ws_bytes(40, 1030)
    desc, cost_at, row_at, col_at = np.zeros((3, 6), dtype=np.int64), 0, 0, 0
    for p, (r, c) in enumerate(shapes):
        desc[p] = (r, c, cost_at, row_at, col_at, 0 if p < 2 else one)
        cost_at, row_at, col_at = cost_at + r * c, row_at + r, col_at + c
    flat = torch.from_numpy(np.concatenate([m.reshape(-1) for m in mats])).to(device)
    row_to_col = torch.full((row_at,), -7, dtype=torch.int32, device=device)
    rows_free, cols_free = torch.empty((row_at,), dtype=torch.int32, device=device), torch.empty((col_at,), dtype=torch.int32, device=device)
    counts = torch.zeros((3, 4), dtype=torch.int32, device=device)
    ws = torch.zeros((one,), dtype=torch.uint8, device=device)             # room for the first slice only
    d_desc = torch.from_numpy(desc).to(device)
    rc = lib.dz_lsa_batch(L.ptr(flat), cost_at, L.ptr(d_desc), 3, 1030, 1030, lsa_cases.THRESHOLD, L.ptr(row_to_col), L.ptr(rows_free), row_at,
                          L.ptr(cols_free), col_at, L.ptr(counts), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, 'dz_lsa_batch')
    counts, row_to_col = counts.cpu().numpy(), row_to_col.cpu().numpy()
    assert counts[:, 3].tolist() == [0, 0, 3] and counts[2, :3].tolist() == [0, 0, 0]
    assert (row_to_col[45:] == -7).all()                                    # the refused problem wrote no row
    for p in range(2):
        matched = lsa_cases.expected(mats[p])[0]
        r2c = row_to_col[desc[p, 3]:desc[p, 3] + shapes[p][0]]
        assert (r2c >= 0).sum() == len(matched) and r2c[matched[:, 0]].tolist() == matched[:, 1].tolist()


def test_nan_costs_stop_with_a_status(device):
    """A matrix of NaN has no finite column: status 1, nothing matched, and the problem next to it is solved."""
    from detzero_amd import ops
    bad = np.full((4, 6), np.nan, dtype=np.float32)
    good = lsa_cases.dense(3, 5, 6)
    flat = torch.from_numpy(np.concatenate([bad.reshape(-1), good.reshape(-1)])).to(device)
    row_to_col, rows_free, cols_free, counts, row_off, col_off = ops.linear_assignment_batch_nosync(flat, [bad.shape, good.shape], 1.0)
    counts = counts.cpu().numpy()
    assert counts[0].tolist() == [0, 4, 6, 1] and counts[1, 3] == 0 and counts[1, 0] == 3
    assert (row_to_col.cpu().numpy()[:4] == -1).all()


def test_sizes_beyond_the_limits_are_refused(device):
    from detzero_amd import ops
    from detzero_amd.lib import DetZeroHipError
    with pytest.raises(DetZeroHipError):
        ops.linear_assignment_batch_nosync(torch.zeros(0, device=device), [(ops.LSA_MAX_DIM + 1, 0)], 1.0)
    with pytest.raises(DetZeroHipError):
        ops.linear_assignment_batch_nosync(torch.zeros(5, device=device), [(2, 3)], 1.0)            # 5 costs for a 2 x 3 matrix
    with pytest.raises(DetZeroHipError):
        ops.linear_assignment_batch([torch.zeros((2, 2), dtype=torch.float64, device=device)])
