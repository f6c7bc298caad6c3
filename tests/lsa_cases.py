"""Test helper: the assignment problems shared by tests/test_lsa_host.py (CPU) and tests/test_gpu_lsa.py, and their scipy answers.

Every problem is float32, threshold 1.0 (what the tracker passes).  ``sparse`` matrices have about 5 % of their entries below the
threshold - the shape of a tracker cost matrix, where most pairs are masked to 5000 - ``dense`` ones are uniform in [0, 1).
``unique_by_margin`` is the pre-check of both tests: with scipy alone, the matched set must not change when every cost moves by
+-1e-6, so the optimum is unique by a margin far above double rounding and a differing answer is a bug, not a tie.
"""
import numpy as np

THRESHOLD = 1.0
SHAPES = [(0, 5), (5, 0), (1, 1), (3, 5), (5, 3), (64, 64), (65, 130), (130, 65)]
GPU_SHAPES = SHAPES + [(257, 63), (63, 257)]


def sparse(rows, cols, seed, keep=0.05):
    rng = np.random.RandomState(seed)
    cost = (1.0 + rng.rand(rows, cols)).astype(np.float32)              # masked: anything >= threshold
    cost[rng.rand(rows, cols) < 0.5] = 5000.                            # (some already carry the tracker's 5000)
    live = rng.rand(rows, cols) < keep
    cost[live] = rng.rand(int(live.sum())).astype(np.float32)
    return cost


def dense(rows, cols, seed):
    return np.random.RandomState(seed).rand(rows, cols).astype(np.float32)


def special_cases():
    """(name, matrix): the edge cases named by the tests."""
    out = []
    out.append(('all_masked', (1.0 + np.random.RandomState(100).rand(7, 9)).astype(np.float32)))
    m = dense(9, 11, 101)
    m[4, :] = 5000.
    m[:, 6] = 1.5
    out.append(('masked_row_and_column', m))
    # raw optimum (0,1) + (1,0) = 1.15 uses the masked 1.05; with the 5000 in its place the diagonal (1.8) wins
    out.append(('masked_pair_on_raw_optimum', np.array([[0.9, 0.1], [1.05, 0.9]], dtype=np.float32)))
    m = np.full((6, 7), 3.0, dtype=np.float32)
    for k in range(3):
        m[2 * k:2 * k + 2, 2 * k:2 * k + 2] = np.array([[0.9, 0.1], [1.05, 0.9]], dtype=np.float32) - np.float32(0.01 * k)
    m[4, 4] = 0.85
    out.append(('masked_pairs_in_blocks', m))
    return out


def problems(shapes, first_seed=0):
    """[(name, matrix)]: a sparse and a dense matrix per shape (seeds first_seed, first_seed + 1, ...), then the special cases."""
    out, seed = [], first_seed
    for rows, cols in shapes:
        out.append(('sparse_%dx%d_seed%d' % (rows, cols, seed), sparse(rows, cols, seed)))
        out.append(('dense_%dx%d_seed%d' % (rows, cols, seed + 1), dense(rows, cols, seed + 1)))
        seed += 2
    return out + special_cases()


def scipy_matched(masked64, live):
    """Matched (row, col) set of a float64 matrix that already carries the 5000; live = the pairs below the threshold."""
    from scipy.optimize import linear_sum_assignment
    if masked64.shape[0] == 0 or masked64.shape[1] == 0:
        return set()
    rows, cols = linear_sum_assignment(masked64)
    return {(int(r), int(c)) for r, c in zip(rows, cols) if live[r, c]}


def unique_by_margin(cost, trials=4, eps=1e-6):
    m = cost.astype(np.float64)
    live = m < THRESHOLD
    m[~live] = 5000.
    base = scipy_matched(m, live)
    rng = np.random.RandomState(12345)
    for _ in range(trials):
        moved = m + eps * np.where(rng.rand(*m.shape) < 0.5, -1.0, 1.0)
        if scipy_matched(moved, live) != base:
            return False
    return True


def expected(cost):
    """GNN_assignment's answer (the product's scipy path) on a copy: (matched (K,2), unmatched rows, unmatched columns)."""
    from detzero_amd.track_models import GNN_assignment
    return GNN_assignment(cost.copy(), THRESHOLD)


def same_answer(got, want):
    """got / want: (matched, rows_free, cols_free); matched compared as a set of pairs, the lists exactly."""
    gm = {(int(r), int(c)) for r, c in np.asarray(got[0]).reshape(-1, 2)}
    wm = {(int(r), int(c)) for r, c in np.asarray(want[0]).reshape(-1, 2)}
    return gm == wm and list(got[1]) == list(want[1]) and list(got[2]) == list(want[2])
