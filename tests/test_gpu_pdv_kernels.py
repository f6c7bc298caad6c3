"""The kernels of the PDV second stage (csrc/pdv.hip, csrc/pdv_sa.hip) one by one against the float64 references of oracle/pdv.py,
the PDV counterpart of tests/test_gpu_dense_conv.py / test_gpu_sparse_conv.py / test_gpu_head_post.py.  tests/test_pdv.py holds the
stage together on a recorded scene; here every input is made by hand so that a wrong lane, word, batch offset or tile shows:

  voxel centroids   point ORDER chosen for the segmented scan of k_cen_accumulate (runs of 1 .. 300 equal keys, a run starting at lane
                    40, one filling a wave, one across a 256-thread block, two cells alternating), odd grids whose level-2 grid is a
                    ceiling, NaN / boundary / out-of-batch points, an empty frame between two populated ones, n = 0 / 1 / 65;
  ball query        rows shorter than a bitmap word, rows over three words, a 33-cell row in three frames; full and sparse levels, an
                    empty frame next to a populated one, radii below a cell / 2.5 cells / beyond the grid, queries on centroids, outside
                    every face near and 1e6 away, on another frame's centroid, centroids exactly ON the ball surface;
  grouping          offsets and features exact, density within a measured tolerance, padding zero, poisoned unreferenced rows;
  fused pooling     every instance of dz_pdv_sa_pool / dz_pdv_sa_pool_split against float64 within the project's per-layer BOUND, odd
                    mq, a tile across two frames, empty / full tile pairs, persistent waves at three iterations, a column block of a
                    wider output, refusals that write nothing;
  part counts       both kernels against the reference: an exact group on cell and box faces, the random inputs of tests/test_pdv.py
                    for every point that is not within 1e-4 of a decision;
  index lookup      ranks, inactive and out-of-grid cells, rows behind a device count.

Numbers in this file: BOUND is the project's (tests/test_gpu_dense_conv.py); the summation bounds are derived in the docstrings; the
density tolerance and the sub-margin share are measured on the references alone (CPU tests below print them).
"""
import functools

import numpy as np
import pytest
import torch

from detzero_amd import lib as L
from detzero_amd import ops
from oracle import pdv as opdv
from tests.test_gpu_dense_conv import BOUND

U32 = 2.0 ** -24                     # unit roundoff of float32
SENT_I, SENT_F = -77777, -12345.5    # what the tests fill output buffers with
TAIL = 8                             # sentinel rows behind every output
LO = np.array([-0.7, -0.5, -0.3], np.float32)          # x, y, z of the hand-made levels
VS = np.array([0.2, 0.25, 0.3], np.float32)
MARGIN, MARGIN_SHARE_CAP = 1e-4, 0.02                   # part counts, random group: a condition on the inputs, not a tolerance


# ------------------------------------------------------------------------------------------------------------------------
# hand-made levels (numpy; shared by the CPU and the GPU tests)
# ------------------------------------------------------------------------------------------------------------------------
def make_cells(rng, batch, dims, occupancy, empty_frames=()):
    """(m, 4) int64 (b, z, y, x) in ascending key order: every cell of the populated frames with probability `occupancy`."""
    d, h, w = dims
    out = []
    for b in range(batch):
        if b in empty_frames:
            continue
        keep = np.nonzero(rng.random(d * h * w) < occupancy)[0] if occupancy < 1.0 else np.arange(d * h * w)
        if keep.size == 0:
            keep = np.array([d * h * w // 2])
        out.append(np.stack([np.full(keep.size, b), keep // (h * w), keep // w % h, keep % w], axis=1))
    return np.concatenate(out).astype(np.int64)


def cell_positions(rng, cells, lo=LO, vs=VS):
    """One float32 position strictly inside every cell (the precondition of the cell walk: a centroid lies in its cell)."""
    u = rng.uniform(0.1, 0.9, (cells.shape[0], 3))
    p = (lo.astype(np.float64) + (cells[:, [3, 2, 1]] + u) * vs.astype(np.float64)).astype(np.float32)
    assert np.array_equal(((p - lo) / vs).astype(np.float32).astype(np.int64), cells[:, [3, 2, 1]])
    return p


def frame_counts(cells, batch):
    return np.bincount(cells[:, 0], minlength=batch).astype(np.int64)


def make_queries(rng, cells, xyz, batch, dims, per_batch):
    """per_batch queries for every frame: on centroids of the frame, outside each of the six faces (0.4 cell and 1e6 away), on
    centroids of the OTHER frames, the rest anywhere in the grid."""
    d, h, w = dims
    ext = np.array([w, h, d]) * VS.astype(np.float64)
    mid = LO + ext / 2
    out = []
    for b in range(batch):
        q = []
        own, other = xyz[cells[:, 0] == b], xyz[cells[:, 0] != b]
        q += [own[i] for i in rng.permutation(own.shape[0])[:6]]
        for a in range(3):
            for side in (0, 1):
                for dist in (0.4 * VS[a], 1e6):
                    p = mid.copy()
                    p[a] = LO[a] - dist if side == 0 else LO[a] + ext[a] + dist
                    q.append(p)
        q += [other[i] for i in rng.permutation(other.shape[0])[:4]]
        while len(q) < per_batch:
            q.append(LO + rng.random(3) * ext)
        out.append(np.asarray(q[:per_batch], np.float32))
    return np.concatenate(out)


def ball_reference(radius, ns, xyz, cells, batch, new_xyz, per_batch):
    mq = new_xyz.shape[0]
    qcnt = np.array([min(max(mq - b * per_batch, 0), per_batch) for b in range(batch)])
    raw = opdv.ball_query_count(radius, ns, xyz, frame_counts(cells, batch), new_xyz, qcnt)
    return opdv.pad_ball_indices(raw)


def batch_starts(cells, batch, mq, per_batch):
    start = np.concatenate([[0], np.cumsum(frame_counts(cells, batch))])
    return start[np.arange(mq) // per_batch]


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the references on hand-computed cases, against differently written code, and on planted faults
# ------------------------------------------------------------------------------------------------------------------------
def test_ball_query_and_density_by_hand():
    xyz = np.array([[0, 0, 0], [0.5, 0, 0], [0.25, 0, 0], [0, 0.5 - 2.0 ** -10, 0], [9, 9, 9], [0.1, 0, 0]], np.float32)
    raw = opdv.ball_query_count(0.5, 4, xyz, np.array([5, 1]), np.array([[0, 0, 0], [0, 0, 0], [7, 7, 7]], np.float32), np.array([1, 2]))
    # frame 0: point 1 is ON the surface (d2 == r2: out), point 3 is 2^-10 inside; frame 1 sees only its own point, index 0
    assert raw.tolist() == [[0, 2, 3, -1], [0, -1, -1, -1], [-1, -1, -1, -1]]
    idx, cnt = opdv.pad_ball_indices(raw)
    assert idx.tolist() == [[0, 2, 3, 0], [0, 0, 0, 0], [0, 0, 0, 0]] and cnt.tolist() == [3, 1, 0]
    # density: one sample -> (2 pi)^-3/2 / h^3; two samples one bandwidth apart -> (1 + e^-1/2) / 2 of it; padded rows repeat their source
    one = (2 * np.pi) ** -1.5 / 0.25 ** 3
    off = np.zeros((3, 4, 3), np.float32)
    off[1, 1, 0] = 0.25
    off[1, 2:] = off[1, 0]
    dens = opdv.kde_density_f64(off, np.array([1, 2, 0]))
    assert np.allclose(dens[0], one, rtol=1e-14) and np.allclose(dens[1], one * (1 + np.exp(-0.5)) / 2, rtol=1e-14) and not dens[2].any()
    d32 = opdv.kde_density_f32(off, np.array([1, 2, 0]))
    assert d32.dtype == np.float32 and np.allclose(d32, dens, rtol=2e-6) and not d32[2].any()


def test_centroids_reference_against_unique_and_scatter_mean():
    rng = np.random.default_rng(3)
    n, c, batch, grid, s = 4000, 4, 3, (7, 5, 3), 2
    lo, vs = np.array([-2.0, -1.0, -0.5], np.float32), np.array([0.6, 0.4, 0.35], np.float32)
    pts = np.zeros((n, 1 + c), np.float32)
    pts[:, 0] = rng.integers(-1, batch + 1, n)
    pts[:, 1:4] = lo + rng.uniform(-0.1, 1.1, (n, 3)) * (np.array(grid) * vs)
    pts[:, 4:] = rng.standard_normal((n, c - 3))
    pts[5, 2] = np.nan
    l1, l2 = opdv.centroids_f64(pts, np.concatenate([lo, lo + np.array(grid) * vs]), vs, grid, batch, s)
    t = torch.from_numpy(pts)
    q = (t[:, 1:4] - torch.from_numpy(lo)) / torch.from_numpy(vs)
    ok = ((q >= 0) & (q < torch.tensor(grid).float())).all(-1) & (t[:, 0] >= 0) & (t[:, 0] < batch)
    vox = torch.cat([t[ok, 0:1].long(), q[ok].long()[:, [2, 1, 0]]], dim=1)
    uniq, inv, counts = vox.unique(dim=0, return_inverse=True, return_counts=True)
    mean = torch.zeros((uniq.shape[0], 1 + c), dtype=torch.float64).index_add_(0, inv, t[ok].double()) / counts[:, None]
    assert 0.2 < float(ok.float().mean()) < 0.9 and not bool(ok[5])
    assert np.array_equal(l1['coords'], uniq.numpy()) and np.array_equal(l1['counts'], counts.numpy())
    assert np.allclose(l1['mean'], mean.numpy(), rtol=1e-13, atol=1e-13) and np.array_equal(l1['inside'], ok.numpy())
    vox2 = uniq.clone()
    vox2[:, 1:] = torch.div(uniq[:, 1:], s, rounding_mode='trunc')
    uniq2, inv2 = vox2.unique(dim=0, return_inverse=True)
    n2 = torch.zeros(uniq2.shape[0], dtype=torch.int64).index_add_(0, inv2, counts)
    mean2 = torch.zeros((uniq2.shape[0], 1 + c), dtype=torch.float64).index_add_(0, inv2, mean * counts[:, None]) / n2[:, None]
    assert np.array_equal(l2['coords'], uniq2.numpy()) and np.array_equal(l2['counts'], n2.numpy())
    assert np.allclose(l2['mean'], mean2.numpy(), rtol=1e-13, atol=1e-13)
    assert int(l2['coords'][:, 3].max()) == 3 and int(l2['coords'][:, 1].max()) == 1         # the ceiling cells of the odd grid exist


def test_part_counts_reference_on_two_boxes_by_hand():
    rois = np.array([[[0, 0, 0, 6, 6, 3, 0], [2, 0, 0, 6, 3, 3, np.pi / 2]]], np.float32)      # box 1 stands upright: its long side along y
    pts = np.array([[0, -2.5, -2.5, -1.0],       # box 0 only (x - 2 = -4.5 is outside box 1): cell (0, 0, 1)
                    [0, 1.25, 0.25, 0.0],        # both; box 0: cell (4, 3, 3); box 1: local x = y = 0.25, local y = -(x - 2) = 0.75 -> cell (3, 4, 3)
                    [0, 1.25, 0.25, 0.0],
                    [0, 9.0, 9.0, 0.0],          # neither
                    [1, 0.0, 0.0, 0.0]], np.float32)   # a frame without boxes
    counts, margin = opdv.part_counts_ref(pts, rois, 6, 2)
    assert counts.shape == (1, 2, 6, 6, 6) and int(counts.sum()) == 5
    assert counts[0, 0, 0, 0, 1] == 1 and counts[0, 0, 4, 3, 3] == 2 and counts[0, 1, 3, 4, 3] == 2
    assert np.isinf(margin[4]) and margin[3] > 1.0 and margin[0] < 1e-9            # (point 0 sits on a cell face in z: (-1 + 1.5) / 0.5 = 1)
    one, _ = opdv.part_counts_ref(pts, rois, 6, 1)
    assert int(one[0, 1].sum()) == 0 and int(one[0, 0].sum()) == 3                 # max_boxes = 1: the first box in box order takes the point


def random_part_inputs(o, n):
    """The inputs of tests/test_pdv.py::test_part_counts_binned_equals_every_box, statement for statement (same seed, same draws)."""
    g = torch.Generator().manual_seed(o)
    b = 3
    rois = torch.zeros(b, o, 7)
    rois[..., 0:2] = (torch.rand(b, o, 2, generator=g) - 0.5) * 150
    rois[..., 2] = torch.rand(b, o, generator=g) * 4 - 2
    rois[..., 3:6] = torch.rand(b, o, 3, generator=g) * torch.tensor([8., 3., 3.]) + 0.3
    rois[..., 6] = (torch.rand(b, o, generator=g) - 0.5) * 6.3
    crowd = min(o, 40)
    rois[1, :crowd, 0:2] = torch.tensor([10., -5.]) + torch.rand(crowd, 2, generator=g)
    if o > 5:
        rois[0, 3, 3:6] = 0
        rois[0, 4, 0] = float('nan')
        rois[2, 5, 0] = 1e6
    pts = torch.zeros(n, 5)
    pts[:, 0] = torch.randint(0, b, (n,), generator=g).float()
    k = torch.randint(0, o, (n,), generator=g)
    centre = rois[pts[:, 0].long(), k, :3]
    near = centre + (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([6., 3., 3.])
    far = (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([400., 400., 10.])
    pts[:, 1:4] = torch.where((torch.rand(n, generator=g) < 0.6)[:, None], near, far)
    pts[0, 1] = float('nan')
    pts[1, 2] = float('inf')
    pts[2, 0] = 7
    pts[3, 0] = -1
    return pts, rois


RANDOM_PART_CASES = [(37, 5000, 2), (600, 30000, 3)]


@functools.lru_cache(maxsize=None)
def random_part_reference(o, n, max_boxes):
    """Per point its own (B, O, G, G, G) contribution is too large to keep; what is kept: the points, the boxes, the margin, and
    the reference counts of the points AT OR ABOVE the margin (the GPU tests count exactly those points)."""
    pts, rois = random_part_inputs(o, n)
    _, margin = opdv.part_counts_ref(pts.numpy(), rois.numpy(), 6, max_boxes)
    sure = margin >= MARGIN
    counts, _ = opdv.part_counts_ref(pts.numpy()[sure], rois.numpy(), 6, max_boxes, want_margin=False)
    return pts, rois, margin, sure, counts


@pytest.mark.parametrize('o, n, max_boxes', RANDOM_PART_CASES)
def test_random_part_inputs_keep_the_margin_cap(o, n, max_boxes):
    """The condition of the random part-count group, kept by the reference alone: fewer than 2 % of the points take a decision
    (box face, cell face) within 1e-4 of its boundary.  Measured: 0.04 % at (37, 5000), 0.02 % at (600, 30000) - see the printed line."""
    pts, rois, margin, sure, counts = random_part_reference(o, n, max_boxes)
    share = 1.0 - float(sure.mean())
    print('  part counts (o %d, n %d): %.3f %% of the points are within %.0e of a decision (cap %.0f %%); %d counted' % (
        o, n, 100 * share, MARGIN, 100 * MARGIN_SHARE_CAP, int(counts.sum())))
    assert share < MARGIN_SHARE_CAP and int(counts.sum()) > n // 50


# ---- fused pooling: instances, stacks, bounds ----------------------------------------------------------------------------------
# (mode, cin_pad, c, h): the fp32 kernel takes any c % 4 == 0 with c + 4 <= cin_pad, the split kernel c = cin_pad - 16 only
POOL_CASES = [('f32', 80, 64, 32), ('f32', 144, 128, 64), ('f32', 80, 32, 32),
              ('f16x2', 80, 64, 32), ('bf16x2', 80, 64, 32), ('f16x2', 144, 128, 64), ('bf16x2', 144, 128, 64)]
MATH = {'f32': 0, 'f16x2': 1, 'bf16x2': 2}
# Per element |got - ref| <= K * D + DT * dens + FLOOR * ones (oracle.pdv.sa_pool_f64 returns D, dens, ones):
#   K      one BOUND per layer: layer 1 errs by BOUND * den1_j per hidden channel, which layer 2 passes on through |w2| |s2| (that sum is
#          <= D, as |h_j| <= den1_j), layer 2 adds BOUND * D: 2 * BOUND.  The split kernel also SPLITS fp32 values that no pair16 tensor
#          held before - the gathered row (layer 1) and the hidden activations (layer 2): v - hi - lo is at most u16^2 |v| with u16 the
#          unit roundoff of the 16-bit format (hi = round(v), lo = round(v - hi)): 2^-11 for fp16, 2^-8 for bf16.  Each operand error goes
#          through the same sums as above: 2 * u16^2 more.
#   FLOOR  an fp16 lo half below 2^-14 is subnormal (quantum 2^-24): its rounding error is 2^-25 ABSOLUTE per element instead of
#          u16^2 |v|; an absolute error e on every element of x gives e * |s1_j| sum_k |w1_kj| in layer 1 and e on every hidden value,
#          through |w2| |s2|: e * ones.  bf16 has float32's exponent range: no floor.
#   DT     the density column is computed on the device: its relative tolerance (density_tolerance() below) times what it is multiplied by.
POOL_K = {'f32': 2 * BOUND['f32'], 'f16x2': 2 * BOUND['f16x2'] + 2 * 2.0 ** -22, 'bf16x2': 2 * BOUND['bf16x2'] + 2 * 2.0 ** -16}
POOL_FLOOR = {'f32': 0.0, 'f16x2': 2.0 ** -25, 'bf16x2': 0.0}
POOL_DIMS = (3, 5, 7)                # 105 cells per frame: not a multiple of 32, so frame 1 starts in the middle of a bitmap word


def make_stack_np(seed, cin_pad, c, h):
    """Two layers with BatchNorm-like scales of both signs; the weight rows of the PADDING columns are random too (the kernels must
    feed zeros there, whatever the weights hold)."""
    rng = np.random.default_rng(seed)
    f = np.float32
    return {'w1': (rng.standard_normal((cin_pad, h)) / np.sqrt(c + 4)).astype(f), 's1': (rng.uniform(0.5, 1.5, h) * rng.choice([-1, 1], h)).astype(f),
            'b1': (rng.standard_normal(h) * 0.3).astype(f), 'w2': (rng.standard_normal((h, h)) / np.sqrt(h)).astype(f),
            's2': (rng.uniform(0.5, 1.5, h) * rng.choice([-1, 1], h)).astype(f), 'b2': (rng.standard_normal(h) * 0.3).astype(f)}


def pool_world(seed, c, batch=2, dims=POOL_DIMS, occupancy=1.0):
    rng = np.random.default_rng(seed)
    cells = make_cells(rng, batch, dims, occupancy)
    xyz = cell_positions(rng, cells)
    feats = rng.standard_normal((cells.shape[0], c)).astype(np.float32)
    return {'rng': rng, 'cells': cells, 'xyz': xyz, 'feats': feats, 'batch': batch, 'dims': dims}


PAIR_PATTERN = [0, 0, 0, 16, 16, 0, 1, 15, 2, 16, 0, 0, 15, 1, 16, 16, 2]       # tiles (2t, 2t + 1): (empty, empty), (empty, full), (full, empty), (1, 15), ...


def hand_balls(world, cnts, per_batch):
    """idx / cnt as the ball query would write them (ascending, padded with the first hit, zeros for an empty ball) with the counts
    given; row 0 of every frame is in no ball.  Query positions anywhere in the grid."""
    rng, cells, batch = world['rng'], world['cells'], world['batch']
    per_frame = frame_counts(cells, batch)
    mq = len(cnts)
    idx = np.zeros((mq, 16), np.int32)
    for q, k in enumerate(cnts):
        if k:
            hit = np.sort(rng.choice(np.arange(1, per_frame[q // per_batch]), size=k, replace=False))
            idx[q] = np.concatenate([hit, np.full(16 - k, hit[0])])
    d, h, w = world['dims']
    new_xyz = (LO + rng.random((mq, 3)) * (np.array([w, h, d]) * VS)).astype(np.float32)
    return new_xyz, idx, np.asarray(cnts, np.int32)


def poison_unreferenced(world, idx, cnt, per_batch):
    """Copies of xyz / feats with NaN in every row no non-empty ball references."""
    starts = batch_starts(world['cells'], world['batch'], idx.shape[0], per_batch)
    used = np.zeros(world['xyz'].shape[0], bool)
    live = cnt > 0
    used[(idx[live].astype(np.int64) + starts[live, None]).reshape(-1)] = True
    xyz, feats = world['xyz'].copy(), world['feats'].copy()
    xyz[~used] = np.nan
    feats[~used] = np.nan
    return xyz, feats, starts, used


def pool_reference(stack, cin_pad, new_xyz, xyz, feats, starts, idx, cnt, w1=None, w2=None, drop=None):
    rows = opdv.group_rows_f64(new_xyz, xyz, feats, starts, idx, cnt, cin_pad)
    return opdv.sa_pool_f64(rows, stack['w1'] if w1 is None else w1, stack['s1'], stack['b1'], stack['w2'] if w2 is None else w2,
                            stack['s2'], stack['b2'], drop=drop), rows


def pool_allowance(mode, res, dt):
    return POOL_K[mode] * res['D'] + dt * res['dens'] + POOL_FLOOR[mode] * res['ones'][None, :]


@functools.lru_cache(maxsize=None)
def group_cases():
    """The grouping cases (all numpy): level, queries, reference balls and reference rows for nsample 1 / 16 / 32, c 1 / 64 / 130, both
    row strides, mq 1 / 5.  Row 0 of each frame lies outside every ball (queries whose ball holds it are not used)."""
    rng = np.random.default_rng(11)
    batch, dims = 2, (3, 5, 7)
    cells = make_cells(rng, batch, dims, 0.6)
    xyz = cell_positions(rng, cells)
    per_frame = frame_counts(cells, batch)
    cases = []
    for ns in (1, 16, 32):
        radius = np.float32(0.45)
        # three queries of frame 0, two of frame 1 (per_batch = 3): candidates per frame, the first whose ball avoids row 0; one far away
        cand = make_queries(rng, cells, xyz, batch, dims, 60).reshape(batch, 60, 3)
        chosen = []
        for b, want in ((0, 3), (1, 2)):
            raw = opdv.ball_query_count(radius, ns, xyz, per_frame, cand[b], np.array([60, 0] if b == 0 else [0, 60]))
            okq = [i for i in range(60) if not (raw[i] == 0).any()]
            full = [i for i in okq if (raw[i] >= 0).sum() >= min(ns, 3)]
            empty = [i for i in okq if raw[i, 0] < 0]
            pick = full[:want - 1] + empty[:1] if b == 0 else full[:want]
            assert len(pick) == want
            chosen.append(cand[b][pick])
        for mq in (1, 5):
            new_xyz = np.concatenate(chosen)[:mq]
            idx, cnt = ball_reference(radius, ns, xyz, cells, batch, new_xyz, 3)
            assert mq == 1 or (0 in cnt.tolist() and max(cnt.tolist()) >= min(ns, 3))
            for c in (1, 64, 130):
                feats = rng.standard_normal((cells.shape[0], c)).astype(np.float32)
                w = {'rng': rng, 'cells': cells, 'xyz': xyz, 'feats': feats, 'batch': batch, 'dims': dims}
                pxyz, pfeats, starts, used = poison_unreferenced(w, idx, cnt, 3)
                assert not used[0] and not used[per_frame[0]]
                for stride in (c + 4, c + 12):
                    rows = opdv.group_rows_f64(new_xyz, pxyz, pfeats, starts, idx, cnt, stride)
                    assert not np.isnan(rows).any()
                    cases.append({'ns': ns, 'mq': mq, 'c': c, 'stride': stride, 'cells': cells, 'xyz': pxyz, 'feats': pfeats, 'new_xyz': new_xyz,
                                  'idx': idx, 'cnt': cnt, 'rows': rows, 'batch': batch, 'dims': dims})
    return cases


@functools.lru_cache(maxsize=None)
def density_tolerance():
    """Relative tolerance of a device density against kde_density_f64.  Nothing in the project fixes one, so it is measured on the
    references: the worst relative error of the float32 numpy restatement of the same loop (kde_density_f32) over the balls of
    group_cases(), times 4 - the device's expf and division differ from numpy's by a few ulp.  Measured: 2.4e-07 -> tolerance 9.6e-07."""
    worst = 0.0
    for case in group_cases():
        off = case['rows'][..., 0:3].astype(np.float32)
        d64, d32 = opdv.kde_density_f64(off, case['cnt']), opdv.kde_density_f32(off, case['cnt'])
        live = d64 > 0
        if live.any():
            worst = max(worst, float((np.abs(d32[live] - d64[live]) / d64[live]).max()))
    return worst, 4 * worst


def test_density_tolerance_is_measured_on_the_references():
    worst, tol = density_tolerance()
    print('  density: float32 restatement vs float64 worst relative error %.2e -> device tolerance %.2e' % (worst, tol))
    assert 2.0 ** -26 < worst < 2.0 ** -18          # a float32 evaluation of a dozen operations: a few units of 2^-24, not zero, not a different formula


def test_references_report_planted_faults():
    """What the comparisons of this file would say about the smallest faults a kernel could have, shown on the references themselves:
    a sample dropped from the max of one ball, a ball shifted by one centroid row, one cell's count off by one point."""
    # ---- a dropped sample in the max: beyond the allowance of every mode
    _, tol = density_tolerance()
    for mode, cin_pad, c, h in POOL_CASES:
        world = pool_world(5, c)
        stack = make_stack_np(cin_pad + c, cin_pad, c, h)
        new_xyz, idx, cnt = hand_balls(world, [16, 16, 16], 2)
        xyz, feats, starts, _ = poison_unreferenced(world, idx, cnt, 2)
        ref, rows = pool_reference(stack, cin_pad, new_xyz, xyz, feats, starts, idx, cnt)
        x = torch.from_numpy(rows)
        k = {n: torch.from_numpy(v.astype(np.float64)) for n, v in stack.items()}
        act = torch.relu((torch.relu((x @ k['w1']) * k['s1'] + k['b1']) @ k['w2']) * k['s2'] + k['b2'])
        ch = int(act[1].amax(dim=0).argmax())
        bad, _ = pool_reference(stack, cin_pad, new_xyz, xyz, feats, starts, idx, cnt, drop=(1, int(act[1, :, ch].argmax())))
        excess = np.abs(bad['out'] - ref['out']) / pool_allowance(mode, ref, tol)
        print('  %-7s cin_pad %3d c %3d: a dropped sample is %.1e allowances away' % (mode, cin_pad, c, float(excess.max())))
        assert float(excess.max()) > 10.0 and float(excess[0].max()) == 0.0 and float(excess[2].max()) == 0.0
        # ---- a ball shifted by one row: the grouped rows are compared exactly, the pooled output is beyond the allowance
        shifted = idx.copy()
        shifted[1] += 1
        bad, bad_rows = pool_reference(stack, cin_pad, new_xyz, world['xyz'], world['feats'], starts, shifted, cnt)
        assert not np.array_equal(bad_rows[1], rows[1]) and np.array_equal(bad_rows[0], rows[0])
        assert float((np.abs(bad['out'] - ref['out']) / pool_allowance(mode, ref, tol))[1].max()) > 10.0
    # ---- ball query: the same shift is an index mismatch
    cells = make_cells(np.random.default_rng(1), 2, (3, 5, 7), 1.0)
    xyz = cell_positions(np.random.default_rng(1), cells)
    q = xyz[[40, 150]]
    idx, cnt = ball_reference(np.float32(0.5), 16, xyz, cells, 2, q, 1)
    moved = xyz.copy()
    moved[7:] = xyz[:-7]                          # every centroid one (z, y) row further
    idx2, cnt2 = ball_reference(np.float32(0.5), 16, moved, cells, 2, q, 1)
    assert cnt.min() > 3 and not np.array_equal(idx, idx2)
    # ---- one cell's count off by one: counts are compared exactly; the mean moves by more than the bound of even the longest run
    pts, meta = centroid_points(3, (7, 5, 3), 2, 5)
    l1 = opdv.centroids_f64(pts, meta['range'], meta['vs'], (7, 5, 3), 2)[0]
    big = int(l1['counts'].argmax())
    members = np.nonzero(l1['inside'])[0][l1['inverse'] == big]
    far = members[np.abs(pts[members, 1] - l1['mean'][big, 1]).argmax()]
    l1b = opdv.centroids_f64(np.delete(pts, far, axis=0), meta['range'], meta['vs'], (7, 5, 3), 2)[0]
    assert l1b['counts'][big] == l1['counts'][big] - 1 and l1['counts'][big] > 300
    moved_by = abs(l1b['mean'][big, 1] - l1['mean'][big, 1])
    bound = (l1['counts'][big] + 2) * U32 * l1['amax'][big, 1]
    print('  centroid of %d points: one point less moves the mean by %.2e, the bound is %.2e' % (l1['counts'][big], moved_by, bound))
    assert moved_by > bound
    pc, _ = opdv.part_counts_ref(np.array([[0, 0.1, 0.1, 0.1]] * 3, np.float32), np.array([[[0, 0, 0, 6, 6, 3, 0]]], np.float32), 6, 1)
    pc1, _ = opdv.part_counts_ref(np.array([[0, 0.1, 0.1, 0.1]] * 2, np.float32), np.array([[[0, 0, 0, 6, 6, 3, 0]]], np.float32), 6, 1)
    assert int(np.abs(pc - pc1).sum()) == 1


def test_case_table_covers_every_pool_instance():
    """Every (cin_pad, widths) the two `_supported` predicates accept, found by sweeping them, has a case in POOL_CASES - in every
    split mode for the split entry; an instance added to csrc/pdv_sa.hip without a case here fails this test."""
    lib = L.load()
    widths = (16, 32, 48, 64, 96, 128, 256)
    pads = range(16, 321, 16)
    plain = {(p, a, b) for p in pads for a in widths for b in widths if lib.dz_pdv_sa_pool_supported(p - 16, p, a, b, 16, 1, 1)}
    split = {(p, c, a, b) for p in pads for c in range(0, 321, 4) for a in widths for b in widths if lib.dz_pdv_sa_pool_split_supported(c, p, a, b, 16, 1, 1)}
    assert plain == {(p, h, h) for m, p, c, h in POOL_CASES if m == 'f32'}, sorted(plain)
    for mode in ('f16x2', 'bf16x2'):
        assert split == {(p, c, h, h) for m, p, c, h in POOL_CASES if m == mode}, (mode, sorted(split))
    for mode, p, c, h in POOL_CASES:
        assert lib.dz_pdv_sa_pool_supported(c, p, h, h, 16, 1, 1)
        assert bool(lib.dz_pdv_sa_pool_split_supported(c, p, h, h, 16, 1, 1)) == (c == p - 16)
    # the fp32 kernel's free parameter c: a multiple of 4 that leaves room for the four leading columns - and a case that is NOT c = cin_pad - 16
    assert [c for c in range(0, 100) if lib.dz_pdv_sa_pool_supported(c, 80, 32, 32, 16, 1, 1)] == list(range(0, 77, 4))
    assert any(m == 'f32' and c != p - 16 for m, p, c, h in POOL_CASES)
    for bad in ((64, 80, 32, 32, 8, 1, 1), (66, 80, 32, 32, 16, 1, 1), (64, 80, 32, 32, 16, 0, 1), (64, 80, 32, 32, 16, 1, 0)):
        assert not lib.dz_pdv_sa_pool_supported(*bad) and not lib.dz_pdv_sa_pool_split_supported(*bad)
    assert not lib.dz_pdv_sa_pool_split_supported(32, 80, 32, 32, 16, 1, 1)


# ------------------------------------------------------------------------------------------------------------------------
# voxel centroids
# ------------------------------------------------------------------------------------------------------------------------
def centroid_points(seed, grid, batch, c, empty_frame=None):
    """Points (n, 1 + c) in an ORDER that walks k_cen_accumulate's segmented scan (one thread per point, 64 lanes, 256-thread blocks;
    lane = position % 64) through its edges; meta records where the runs start.  Geometry: dyadic cell size 0.5 for the 7 x 5 x 3 grid (the
    point ON hi is exactly outside, the one an ulp below exactly inside), 0.6 / 0.4 / 0.15 for the 9 x 1 x 2 one (quotients round)."""
    rng = np.random.default_rng(seed)
    gx, gy, gz = grid
    vs = np.array([0.5, 0.5, 0.5] if grid == (7, 5, 3) else [0.6, 0.4, 0.15], np.float32)
    lo = np.array([-0.5, -1.0, -0.5], np.float32)           # (hi - ulp) - lo is exact for the dyadic grid: 3 - 2^-22 + 0.5
    hi = (lo + np.array(grid, np.float32) * vs).astype(np.float32)
    frames = [b for b in range(batch) if b != empty_frame]
    cells = [(b, x, y, z) for b in frames for z in range(gz) for y in range(gy) for x in range(gx)]
    cell_a, cell_b, cell_c = cells[5], cells[-3], cells[len(cells) // 2]
    others = [cl for cl in cells if cl not in (cell_a, cell_b, cell_c)]
    seq, meta, nxt = [], {}, [0]

    def filler():
        nxt[0] += 1
        return others[(nxt[0] * 7) % len(others)]                   # (7 is coprime to both cell counts: consecutive fillers differ)
    special = 7
    for run in (1, 2, 63, 64, 65, 300):
        seq += [cell_a] * run + [filler()]
    for name, mod, at, cell, run in (('lane40', 64, 40, cell_b, 50), ('wave', 64, 0, cell_c, 64), ('block', 256, 250, cell_a, 12)):
        while (special + len(seq)) % mod != at:
            seq.append(filler())
        meta[name] = special + len(seq)
        seq += [cell] * run
    seq.append(filler())
    meta['alternate'] = special + len(seq)
    seq += [cell_a, cell_b] * 65
    seq += [cells[i] for i in rng.integers(0, len(cells), 100)]
    arr = np.asarray(seq, np.float64)
    n = special + len(seq)
    pts = np.zeros((n, 1 + c), np.float32)
    pts[special:, 0] = arr[:, 0]
    pts[special:, 1:4] = (lo + (arr[:, 1:4] + rng.uniform(0.05, 0.95, (len(seq), 3))) * vs).astype(np.float32)
    pts[:, 4:] = rng.standard_normal((n, c - 3)) * 3
    inside = (lo + (np.array(cell_a[1:]) + 0.5) * vs).astype(np.float32)
    pts[:special, 0] = frames[0]
    pts[:special, 1:4] = inside
    pts[0, 1] = np.nan                                    # NaN x
    pts[1, 3] = np.nan                                    # NaN z
    pts[2, 1] = hi[0]                                     # exactly on hi
    pts[3, 1] = np.nextafter(hi[0], np.float32(-np.inf))  # one ulp below hi
    pts[4, 2] = lo[1] - np.float32(1e-3)                  # below lo
    pts[5, 0] = -1
    pts[6, 0] = batch
    assert meta['lane40'] % 64 == 40 and meta['wave'] % 64 == 0 and meta['block'] % 256 == 250
    meta.update({'range': np.concatenate([lo, hi]), 'vs': vs, 'special': special})
    return pts, meta


def centroids_raw(dev, pts, meta, grid, batch, scaling, cap):
    """dz_pdv_voxel_centroids into buffers of cap + TAIL sentinel rows -> per level (m, cen, coords, counts) on the host."""
    lib = L.load()
    n, cols = pts.shape
    t = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
    lv = [[torch.full((cap + TAIL, cols), SENT_F, device=dev), torch.full((cap + TAIL, 4), SENT_I, dtype=torch.int32, device=dev),
           torch.full((cap + TAIL,), SENT_I, dtype=torch.int32, device=dev)] for _ in range(2)]
    dm = torch.full((2,), SENT_I, dtype=torch.int32, device=dev)
    gx, gy, gz = grid
    ws = torch.empty((lib.dz_pdv_centroids_workspace_bytes(n, batch, gx, gy, gz, scaling, cap),), dtype=torch.uint8, device=dev)
    rc = lib.dz_pdv_voxel_centroids(L.ptr(t) if n else None, n, cols - 1, L.f6(meta['range']), L.f3(meta['vs']), L.i3(grid), batch, scaling,
                                    L.ptr(lv[0][0]), L.ptr(lv[0][1]), L.ptr(lv[0][2]), L.ptr(dm[0:1]), cap,
                                    L.ptr(lv[1][0]), L.ptr(lv[1][1]), L.ptr(lv[1][2]), L.ptr(dm[1:2]), cap, L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, 'dz_pdv_voxel_centroids')
    torch.cuda.synchronize()
    m = dm.tolist()
    return [(m[k], lv[k][0].cpu().numpy(), lv[k][1].cpu().numpy(), lv[k][2].cpu().numpy()) for k in range(2)]


@pytest.mark.gpu
@pytest.mark.parametrize('c', [3, 5])
@pytest.mark.parametrize('grid, batch, empty_frame', [((7, 5, 3), 2, None), ((9, 1, 2), 3, 1)], ids=['7x5x3_b2', '9x1x2_b3_frame1_empty'])
def test_voxel_centroids(device, grid, batch, empty_frame, c):
    """dz_pdv_voxel_centroids, both levels (scaling 2 on odd extents: the level-2 grid is a ceiling; 105 / 18 cells per frame, no multiple
    of 32), against oracle.pdv.centroids_f64.  Rows, coordinates, their ascending (b, z, y, x) order, counts and the batch column: exact.
    Means, per cell and column, with u = 2^-24 and max|x| over the cell's points:
      level 1   |mean - ref| <= (count + 2) u max|x|: a float32 sum of `count` terms in ANY order (the run's tree, then atomics) is off by
                at most (count - 1) u sum|x| <= (count - 1) u count max|x| to first order, the division by count brings it to
                (count - 1) u max|x| and adds one rounding u |mean|; the remaining 2 u max|x| hold the second-order terms.
      level 2   the mean of k children weighted by their counts w_i (N = sum w_i) from the DEVICE's level-1 means: each child is off by its
                level-1 bound (w_i + 2) u max_i, its product with w_i by one more rounding u w_i max_i, the sum of the k products (each at
                most w_i max|x|, together N max|x|) by (k - 1) u N max|x|, the division adds u max|x|:
                |mean2 - ref2| <= u (sum_i w_i (w_i + 3) max_i / N + (k + 2) max|x|)   (the + 2 as in level 1).
    Rows m .. cap of the means and counts are the zeros the entry point fills them with, rows m .. cap of the coordinates and every row
    behind cap keep the caller's sentinel.  The point order (centroid_points) puts runs of 1, 2, 63, 64, 65 and 300 equal keys, a run
    from lane 40 across a wave, a run filling a wave, a run across a 256-thread block and two alternating cells in front of the scan -
    asserted there from the positions; n = 0, 1, 65 are the tail of the same list."""
    pts_all, meta = centroid_points(grid[0] + c, grid, batch, c, empty_frame)
    gx, gy, gz = grid
    cap = batch * gx * gy * gz + 3
    for n in (pts_all.shape[0], 65, 1, 0):
        pts = pts_all[pts_all.shape[0] - n:]
        ref = opdv.centroids_f64(pts, meta['range'], meta['vs'], grid, batch, 2)
        got = centroids_raw(device, pts, meta, grid, batch, 2, cap)
        if n == pts_all.shape[0]:
            ins = ref[0]['inside']
            assert not ins[[0, 1, 4, 5, 6]].any() and (grid != (7, 5, 3) or (ins[3] and not ins[2]))     # NaN, below lo, batch out: outside; dyadic cells: ON hi outside, an ulp below inside
            assert int(ref[0]['counts'].max()) >= 495 and (empty_frame is None or not (ref[0]['coords'][:, 0] == empty_frame).any())
            assert len(set(ref[0]['coords'][:, 0].tolist())) == batch - (empty_frame is not None)
        worst = [0.0, 0.0]
        for k, (r, (m, cen, coords, counts)) in enumerate(zip(ref, got)):
            assert m == r['coords'].shape[0], (n, k, m, r['coords'].shape[0])
            assert np.array_equal(coords[:m], r['coords']) and np.array_equal(counts[:m], r['counts']), (n, k)
            assert np.array_equal(cen[:m, 0], r['mean'][:, 0]), (n, k)
            if k == 0:
                bound = (r['counts'][:, None] + 2) * U32 * r['amax']
            else:
                bound = U32 * (r['child_bound_sum'] / np.maximum(r['counts'], 1)[:, None] + (r['members'][:, None] + 2) * r['amax'])
            err = np.abs(cen[:m, 1:].astype(np.float64) - r['mean'][:, 1:])
            assert (err <= bound[:, 1:]).all(), (n, k, float((err / np.maximum(bound[:, 1:], 1e-300)).max()))
            if m:
                worst[k] = float((err / np.maximum(bound[:, 1:], 1e-300)).max())
            assert not cen[m:cap].any() and not counts[m:cap].any() and (coords[m:cap] == SENT_I).all(), (n, k)
            assert (cen[cap:] == SENT_F).all() and (counts[cap:] == SENT_I).all() and (coords[cap:] == SENT_I).all(), (n, k)
        print('  centroids grid %s c %d n %4d: %3d / %3d cells, worst error / bound %.2f (level 1) %.2f (level 2)' % (
            grid, c, n, got[0][0], got[1][0], worst[0], worst[1]))


# ------------------------------------------------------------------------------------------------------------------------
# ball query, grouping
# ------------------------------------------------------------------------------------------------------------------------
def make_level(dev, batch, dims, cells):
    lvl = ops.SparseLevel(batch, dims, max(cells.shape[0], 1), dev)
    lvl.build_from_coords(torch.from_numpy(cells.astype(np.int32)).to(dev).contiguous(), want_rank=False)
    return lvl


def ball_query_raw(dev, lvl, new_xyz, per_batch, xyz, radius, ns):
    """dz_pdv_ball_query into buffers with TAIL sentinel rows behind mq -> idx, cnt (device, whole buffers)."""
    mq = new_xyz.shape[0]
    idx = torch.full((mq + TAIL, ns), SENT_I, dtype=torch.int32, device=dev)
    cnt = torch.full((mq + TAIL,), SENT_I, dtype=torch.int32, device=dev)
    q, p = torch.from_numpy(new_xyz).to(dev).contiguous(), torch.from_numpy(xyz).to(dev).contiguous()
    rc = L.load().dz_pdv_ball_query(L.ptr(q), mq, per_batch, L.ptr(p), L.ptr(lvl.bitmap), L.ptr(lvl.prefix), lvl.batch, *lvl.shape, L.f3(LO), L.f3(VS),
                                    float(radius), ns, L.ptr(idx), L.ptr(cnt), L.stream())
    L.check(rc, 'dz_pdv_ball_query')
    return idx, cnt


def check_balls(dev, lvl, cells, xyz, batch, new_xyz, per_batch, radius, ns, what):
    idx, cnt = ball_query_raw(dev, lvl, new_xyz, per_batch, xyz, radius, ns)
    ridx, rcnt = ball_reference(radius, ns, xyz, cells, batch, new_xyz, per_batch)
    mq = new_xyz.shape[0]
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    assert np.array_equal(cnt[:mq], rcnt), (what, np.nonzero(cnt[:mq] != rcnt)[0][:5])
    assert np.array_equal(idx[:mq], ridx), (what, np.nonzero((idx[:mq] != ridx).any(axis=1))[0][:5])
    assert not idx[:mq][rcnt == 0].any()
    assert (idx[mq:] == SENT_I).all() and (cnt[mq:] == SENT_I).all(), what
    return rcnt


@pytest.mark.gpu
@pytest.mark.parametrize('dims, batch', [((3, 5, 7), 2), ((2, 3, 70), 2), ((1, 1, 33), 3)], ids=['3x5x7_b2', '2x3x70_b2', '1x1x33_b3'])
def test_ball_query_equals_the_scan_over_all_points(device, dims, batch):
    """dz_pdv_ball_query against oracle.pdv.ball_query_count (every point of the frame tested, float32 operation for operation) after the
    padding rule, index for index.  (3, 5, 7): rows of 7 cells start at any bit of a word; (2, 3, 70): a row covers a whole middle
    word; (1, 1, 33) x 3 frames: every frame starts inside a word.  Each grid full, 30 % occupied, with frame 0 empty and with the last
    frame empty; nsample 1 / 16 / 32; radii below a cell, 2.5 cells, beyond the grid (the count saturates: the first nsample centroids
    in index order); queries per frame on its centroids, outside each face (near and 1e6 away), on other frames' centroids; mq = 257
    in groups of 129 (a second, partial block of 256 threads and a partial last frame)."""
    rng = np.random.default_rng(dims[2])
    seen = {'empty': 0, 'short': 0, 'full': 0}
    for occ, empty_frames in ((1.0, ()), (0.3, ()), (0.5, (0,)), (0.5, (batch - 1,))):
        cells = make_cells(rng, batch, dims, occ, empty_frames)
        xyz = cell_positions(rng, cells)
        lvl = make_level(device, batch, dims, cells)
        new_xyz = make_queries(rng, cells, xyz, batch, dims, 40)
        for ns in (1, 16, 32):
            for radius in (np.float32(0.9 * VS.min()), np.float32(2.5 * VS.max()), np.float32(1e3)):
                rcnt = check_balls(device, lvl, cells, xyz, batch, new_xyz, 40, radius, ns, (dims, occ, empty_frames, ns, float(radius)))
                seen['empty'] += int((rcnt == 0).sum()); seen['short'] += int(((rcnt > 0) & (rcnt < ns)).sum()); seen['full'] += int((rcnt == ns).sum())
        if batch == 2:
            big = make_queries(rng, cells, xyz, batch, dims, 129)[:257]
            check_balls(device, lvl, cells, xyz, batch, big, 129, np.float32(2.5 * VS.max()), 16, (dims, occ, empty_frames, 'mq 257'))
    print('  ball query %s: %d empty, %d short, %d saturated balls' % (dims, seen['empty'], seen['short'], seen['full']))
    assert min(seen.values()) > 50


@pytest.mark.gpu
def test_ball_query_on_the_ball_surface(device):
    """Centroids exactly ON the surface (d2 == r2, dyadic coordinates, r = 0.5: out, the comparison is strict) and 2^-10 inside it."""
    lo, vs = np.zeros(3, np.float32), np.full(3, 0.5, np.float32)
    cells = np.array([[0, 0, 1, 2], [0, 1, 1, 1], [0, 1, 1, 2], [0, 1, 1, 3], [0, 1, 2, 2]], np.int64)          # (b, z, y, x), key order
    e = 2.0 ** -10
    xyz = np.array([[1.0, 0.75, 0.25 + e], [0.5 + e, 0.75, 0.75], [1.0, 0.75, 0.75], [1.5, 0.75, 0.75], [1.0, 1.25, 0.75]], np.float32)
    assert np.array_equal((xyz / vs).astype(np.int64), cells[:, [3, 2, 1]])
    lvl = make_level(device, 1, (3, 3, 4), cells)
    q = torch.tensor([[1.0, 0.75, 0.75]], device=device)
    idx = torch.full((1 + TAIL, 4), SENT_I, dtype=torch.int32, device=device)
    cnt = torch.full((1 + TAIL,), SENT_I, dtype=torch.int32, device=device)
    p = torch.from_numpy(xyz).to(device)
    rc = L.load().dz_pdv_ball_query(L.ptr(q), 1, 1, L.ptr(p), L.ptr(lvl.bitmap), L.ptr(lvl.prefix), 1, 3, 3, 4, L.f3(lo), L.f3(vs), 0.5, 4, L.ptr(idx), L.ptr(cnt), L.stream())
    L.check(rc, 'dz_pdv_ball_query')
    ridx, rcnt = opdv.pad_ball_indices(opdv.ball_query_count(0.5, 4, xyz, np.array([5]), q.cpu().numpy(), np.array([1])))
    assert ridx.tolist() == [[0, 1, 2, 0]] and rcnt.tolist() == [3]
    assert idx[:1].cpu().tolist() == [[0, 1, 2, 0]] and cnt[:1].cpu().tolist() == [3] and bool((idx[1:] == SENT_I).all())


@pytest.mark.gpu
def test_group_features(device):
    """dz_pdv_group_features on the reference's balls (oracle.pdv.ball_query_count, no kernel in front): offsets and gathered features
    exact, padding columns zero, an empty ball all zero, rows behind mq untouched; nsample 1 / 16 / 32, c 1 / 64 / 130 (the lane loop over
    the columns wraps once and twice), row strides c + 4 and c + 12, mq 1 and 5 (a partial block of four waves).  Every feature and
    centroid row no ball references is NaN, row 0 of each frame among them (an empty ball's indices point at it: it must not be read
    into the result).  Density: relative error against kde_density_f64 within density_tolerance() - measured there on the float32
    numpy restatement over these very balls: worst 2.4e-07, times 4 = 9.6e-07 for the device."""
    worst_np, tol = density_tolerance()
    worst = 0.0
    for case in group_cases():
        lvl = make_level(device, case['batch'], case['dims'], case['cells'])
        mq, ns, stride, c = case['mq'], case['ns'], case['stride'], case['c']
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)        # noqa: E731
        rows = torch.full((mq * ns + TAIL, stride), SENT_F, device=device)
        q, p, f, idx, cnt = t(case['new_xyz']), t(case['xyz']), t(case['feats']), t(case['idx']), t(case['cnt'])
        d, h, w = case['dims']
        rc = L.load().dz_pdv_group_features(L.ptr(q), mq, 3, L.ptr(p), L.ptr(f), c, L.ptr(lvl.bitmap), L.ptr(lvl.prefix), d * h * w, L.ptr(idx), L.ptr(cnt),
                                            ns, L.ptr(rows), stride, L.stream())
        L.check(rc, 'dz_pdv_group_features')
        got = rows.cpu().numpy().astype(np.float64)
        ref = case['rows'].reshape(mq * ns, stride)
        what = (ns, mq, c, stride)
        assert np.array_equal(got[:mq * ns, 0:3], ref[:, 0:3]), what
        assert np.array_equal(got[:mq * ns, 4:], ref[:, 4:]), what
        assert not got[:mq * ns, 4 + c:].any() and not got[:mq * ns][np.repeat(case['cnt'] == 0, ns)].any(), what
        assert (got[mq * ns:] == SENT_F).all(), what
        live = ref[:, 3] > 0
        if live.any():
            rel = float((np.abs(got[:mq * ns, 3][live] - ref[live, 3]) / ref[live, 3]).max())
            worst = max(worst, rel)
            assert rel <= tol, (what, rel, tol)
    print('  density: device vs float64 worst relative error %.2e; float32 numpy restatement %.2e; tolerance %.2e' % (worst, worst_np, tol))


# ------------------------------------------------------------------------------------------------------------------------
# fused pooling
# ------------------------------------------------------------------------------------------------------------------------
def device_stack(stack, dev):
    t = lambda a: torch.from_numpy(a).to(dev).contiguous()        # noqa: E731
    return [{'w': t(stack['w1']), 'scale': t(stack['s1']), 'shift': t(stack['b1']), 'relu': True, 'cout': stack['w1'].shape[1]},
            {'w': t(stack['w2']), 'scale': t(stack['s2']), 'shift': t(stack['b2']), 'relu': True, 'cout': stack['w2'].shape[1]}]


def split_weights_held(dstack, math, cin_pad, h):
    """The values the pair16 weights of the split kernel actually hold (decoded on the host), as (cin, cout) float64."""
    from detzero_amd.refine_modules import _split_w
    out = []
    for layer, ci in zip(dstack, (cin_pad, h)):
        packed = _split_w(layer, math)
        out.append(ops.pair16_unpack(packed.cpu(), math).double().t()[:ci, :h].contiguous().numpy())
    return out


def run_pool(dev, mode, cin_pad, c, h, world, stack, dstack, lvl, new_xyz, idx, cnt, per_batch, label):
    """One launch (twice: bit-identical) of the instance against sa_pool_f64 -> worst error / allowance, worst error / D."""
    from detzero_amd import pdv_modules as pm
    mq = idx.shape[0]
    xyz, feats, starts, _ = poison_unreferenced(world, idx, cnt, per_batch)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    q, p, f, ti, tc = t(new_xyz), t(xyz), t(feats), t(idx), t(cnt)
    _, tol = density_tolerance()
    outs = []
    for _ in range(2):
        if mode == 'f32':
            assert pm.sa_pool_supported(c, dstack, 16)
            outs.append(pm.sa_pool(q, per_batch, p, f, lvl, ti, tc, dstack))
        else:
            assert pm.sa_pool_split_supported(c, dstack, 16, MATH[mode])
            wide = torch.full((mq + TAIL, h + 24), SENT_F, device=dev)
            pm.sa_pool_split(q, per_batch, p, f, lvl, ti, tc, dstack, MATH[mode], out=wide[:mq, 8:8 + h])
            assert bool((wide[:, :8] == SENT_F).all()) and bool((wide[:, 8 + h:] == SENT_F).all()) and bool((wide[mq:] == SENT_F).all()), label
            outs.append(wide[:mq, 8:8 + h].clone())
    assert torch.equal(outs[0], outs[1]), (label, 'two launches differ')
    if not cnt.any():
        assert bool((outs[0] == outs[0][0:1]).all()), (label, 'empty balls: every row is the stack on a zero row')
    w1, w2 = (None, None) if mode == 'f32' else split_weights_held(dstack, MATH[mode], cin_pad, h)
    ref, _ = pool_reference(stack, cin_pad, new_xyz, xyz, feats, starts, idx, cnt, w1=w1, w2=w2)
    got = outs[0].cpu().numpy().astype(np.float64)
    assert got.shape == ref['out'].shape and not np.isnan(got).any(), label
    err = np.abs(got - ref['out'])
    ratio, plain = float((err / pool_allowance(mode, ref, tol)).max()), float((err / ref['D']).max())
    assert ratio <= 1.0, (label, ratio, plain, POOL_K[mode])
    return ratio, plain


@pytest.mark.gpu
@pytest.mark.parametrize('mode, cin_pad, c, h', POOL_CASES, ids=['%s-%d-%d-%d' % k for k in POOL_CASES])
def test_fused_pooling_vs_float64(device, mode, cin_pad, c, h):
    """Every instance of dz_pdv_sa_pool (exact fp32) and dz_pdv_sa_pool_split (pair16 operands, two balls per wave) against
    oracle.pdv.sa_pool_f64 on the grouped rows of oracle.pdv.group_rows_f64 - for the split modes on the weights the pair16 tensors
    hold.  Bound: POOL_K / POOL_FLOOR above (the project's BOUND once per layer) plus the density tolerance through the layers.
    Launches: mq 1, 2, 3, 17 with the tile pairs of PAIR_PATTERN ((empty, empty), (empty, full), (full, empty), (1, 15) ...; with 17
    balls there are 9 tiles, one per wave: tiles 0 and 5 are empty pairs - the first real tile of their waves - the other waves start on
    a non-empty tile, tile 8 holds one ball); mq 6 in frames of 3 (tile (2, 3) holds
    a ball of each frame, frame 1 starts at centroid 105, inside a bitmap word); every ball empty (each row = the stack on zero rows);
    and the balls dz_pdv_ball_query itself finds on a 40 % level.  The split kernel writes a column block of a wider tensor (ldo > h):
    the columns beside it and the rows behind mq keep their sentinel; unreferenced centroid and feature rows are NaN; two launches
    are bit-identical."""
    from detzero_amd import pdv_modules as pm
    world = pool_world(cin_pad + c, c)
    stack = make_stack_np(cin_pad + c, cin_pad, c, h)
    dstack = device_stack(stack, device)
    lvl = make_level(device, world['batch'], world['dims'], world['cells'])
    worst = (0.0, 0.0)
    launches = [('mq1', [16], 1), ('mq2', [0, 16], 1), ('mq3', [16, 0, 2], 2), ('mq17', PAIR_PATTERN, 9), ('straddle', [16, 1, 0, 16, 0, 15], 3),
                ('all-empty', [0] * 5, 3)]
    for label, cnts, per_batch in launches:
        new_xyz, idx, cnt = hand_balls(world, cnts, per_batch)
        worst = max(worst, run_pool(device, mode, cin_pad, c, h, world, stack, dstack, lvl, new_xyz, idx, cnt, per_batch, (mode, cin_pad, c, label)))
    # balls from the ball query itself (the one place where a kernel under test feeds another)
    sparse = pool_world(cin_pad + c + 1, c, occupancy=0.4)
    lvl2 = make_level(device, sparse['batch'], sparse['dims'], sparse['cells'])
    new_xyz = make_queries(sparse['rng'], sparse['cells'], sparse['xyz'], 2, sparse['dims'], 9)[:17]
    idx, cnt = pm.ball_query(torch.from_numpy(new_xyz).to(device), 9, torch.from_numpy(sparse['xyz']).to(device), lvl2, LO, VS, 0.6, 16)
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    assert 0 in cnt.tolist() and int(cnt.max()) > 4
    worst = max(worst, run_pool(device, mode, cin_pad, c, h, sparse, stack, dstack, lvl2, new_xyz, idx, cnt, 9, (mode, cin_pad, c, 'query')))
    print('  pooling %-7s cin_pad %3d c %3d h %2d: worst error / allowance %.3f; worst |err| / D %.2e (K = %.2e, density tolerance %.1e)' % (
        mode, cin_pad, c, h, worst[0], worst[1], POOL_K[mode], density_tolerance()[1]))


@pytest.mark.gpu
@pytest.mark.parametrize('mode, cin_pad, c, h, empty_share', [('f32', 80, 64, 32, 0.2), ('f16x2', 144, 128, 64, 0.7)], ids=['f32-80', 'f16x2-144-70pct-empty'])
def test_fused_pooling_persistent_loop(device, mode, cin_pad, c, h, empty_share):
    """Enough balls for every persistent wave to run three iterations: the fp32 kernel launches at most CUs blocks of 8 waves, a
    ball each (mq = 3 * 8 CUs + 1), the split kernel CUs blocks of 8 waves, a TILE of two balls each (mq = 3 * 16 CUs + 1: 3 * 8 CUs
    tiles and a last tile of one ball) - so the prefetch two strides ahead, the hand-over after the virtual first tile and the last,
    odd tile all run.  With 70 % of the balls empty most tiles of the split launch take the both-empty shortcut and the prefetch past it."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    assert L.load().dz_device_cu_count() == cus
    mq = 3 * cus * (8 if mode == 'f32' else 16) + 1
    world = pool_world(cin_pad, c)
    stack = make_stack_np(cin_pad, cin_pad, c, h)
    dstack = device_stack(stack, device)
    lvl = make_level(device, world['batch'], world['dims'], world['cells'])
    rest = (1.0 - empty_share) / 4
    cnts = world['rng'].choice([0, 1, 2, 15, 16], size=mq, p=[empty_share, rest, rest, rest, rest]).tolist()
    cnts[-1] = 16
    per_batch = (mq + 1) // 2
    new_xyz, idx, cnt = hand_balls(world, cnts, per_batch)
    if mode != 'f32':
        both_empty = int(((cnt[0:mq - 1:2] == 0) & (cnt[1:mq:2] == 0)).sum())
        assert both_empty > 0.3 * (mq // 2)
    ratio, plain = run_pool(device, mode, cin_pad, c, h, world, stack, dstack, lvl, new_xyz, idx, cnt, per_batch, (mode, cin_pad, 'persistent'))
    print('  pooling %-7s persistent, %d CUs, mq %d: worst error / allowance %.3f; worst |err| / D %.2e (K = %.2e)' % (mode, cus, mq, ratio, plain, POOL_K[mode]))


@pytest.mark.gpu
def test_fused_pooling_refusals_write_nothing(device):
    """nsample 8, c 66, the split entry with c 32, and math 0 on the split entry: the error code, and not one element written."""
    lib = L.load()
    c = 64
    world = pool_world(1, c)
    lvl = make_level(device, 2, POOL_DIMS, world['cells'])
    new_xyz, idx, cnt = hand_balls(world, [16, 2, 0], 2)
    stack = device_stack(make_stack_np(1, 80, c, 32), device)
    from detzero_amd.refine_modules import _split_w
    w1p, w2p = _split_w(stack[0], 1), _split_w(stack[1], 1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)        # noqa: E731
    q, p, f, ti, tc = t(new_xyz), t(world['xyz']), t(np.concatenate([world['feats'], world['feats'][:, :2]], axis=1)), t(idx), t(cnt)
    out = torch.full((3 + TAIL, 32), SENT_F, device=device)
    l1, l2 = stack

    def plain(cc, ns):
        return lib.dz_pdv_sa_pool(L.ptr(q), 3, 2, L.ptr(p), L.ptr(f), cc, L.ptr(lvl.bitmap), L.ptr(lvl.prefix), 105, L.ptr(ti), L.ptr(tc), ns, L.ptr(l1['w']), 32,
                                  L.ptr(l1['scale']), L.ptr(l1['shift']), 32, L.ptr(l2['w']), 32, L.ptr(l2['scale']), L.ptr(l2['shift']), 32, 80, L.ptr(out), L.stream())

    def split(cc, ns, math):
        return lib.dz_pdv_sa_pool_split(L.ptr(q), 3, 2, L.ptr(p), L.ptr(f), f.shape[0], cc, L.ptr(lvl.bitmap), L.ptr(lvl.prefix), 105, L.ptr(ti), L.ptr(tc), ns,
                                        L.ptr(w1p), w1p.shape[1], L.ptr(l1['scale32']), L.ptr(l1['shift32']), 32, L.ptr(w2p), w2p.shape[1], L.ptr(l2['scale32']),
                                        L.ptr(l2['shift32']), 32, 80, math, L.ptr(out), 32, L.stream())
    assert plain(64, 8) == L.ERR_UNSUPPORTED and plain(66, 16) == L.ERR_UNSUPPORTED
    assert split(64, 8, 1) == L.ERR_UNSUPPORTED and split(66, 16, 1) == L.ERR_UNSUPPORTED and split(32, 16, 1) == L.ERR_UNSUPPORTED
    assert split(64, 16, 0) == L.ERR_INVALID and b'not a split mode' in lib.dz_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENT_F).all())


# ------------------------------------------------------------------------------------------------------------------------
# part counts
# ------------------------------------------------------------------------------------------------------------------------
def both_part_kernels(points, rois, grid, max_boxes):
    from detzero_amd import pdv_modules as pm
    saved = pm.PART_COUNTS_BINNED
    try:
        pm.PART_COUNTS_BINNED = False
        every = pm.part_counts(points, rois, grid, max_boxes)
        pm.PART_COUNTS_BINNED = True
        binned = pm.part_counts(points, rois, grid, max_boxes)
    finally:
        pm.PART_COUNTS_BINNED = saved
    return every.cpu().numpy(), binned.cpu().numpy()


def exact_part_inputs(o, n):
    """Heading-0 boxes whose cell size (size / 6) is dyadic, points on multiples of 1/8: every subtraction, sum and quotient is exact."""
    rng = np.random.default_rng(o + n)
    rois = np.zeros((2, o, 7), np.float32)
    rois[:, 0] = [0, 0, 0, 3, 6, 1.5, 0]
    if o > 1:
        rois[:, 1] = [0.5, 0, 0, 3, 6, 1.5, 0]
        rois[:, 2] = [0, 0.5, 0, 6, 3, 3, 0]
        rois[:, 3] = [10, 10, 0, 0, 0, 0, 0]                       # zero size
        rois[:, 4] = [np.nan, 10, 0, 3, 3, 3, 0]
        for k in range(5, o - 1):
            rois[:, k] = [20 + 4 * k, 0, 0, 3, 1.5, 1.5, 0]
        rois[:, o - 1] = [0, -20, 0, 3, 3, 3, 0]                   # the only box of the second staged chunk of 64
    rois[1, :, 0] += 128                                           # frame 1: the same boxes elsewhere
    special = [[-1.5 + 0.5 * k, 0.25, 0.125] for k in range(1, 6)]                    # inner cell faces in x: the upper cell
    special += [[0.25, -3 + k, 0.125] for k in range(1, 6)] + [[0.25, 0.25, -0.75 + 0.25 * k] for k in range(1, 6)]
    special += [[-1.5, -3, -0.75],                                                   # lower faces: inside, cell (0, 0, 0)
                [1.5, 0.25, 0.125], [0.25, 3, 0.125],                                # upper faces in x / y: in the box (takes a slot of max_boxes), no cell
                [0.25, 0.25, 0.75], [0.25, 0.25, -0.75],                             # |dz| == h / 2: in; the upper one lands in no cell
                [0.25, 0.25, 0.125],                                                 # in boxes 0, 1, 2: counted in the first two
                [10, 10, 0], [0, 10, 0],                                             # the zero-size box's centre; the NaN box's y, z
                [0, -20, 0], [-1.5, -21.5, -1.5], [1.5, -20, 0]]                     # the last box: centre, lower corner, upper x face
    special = np.asarray(special, np.float32)
    m = max(n - special.shape[0], 0)
    rnd = np.stack([rng.integers(-24, 25, m) / 8.0, rng.integers(-32, 33, m) / 8.0, rng.integers(-8, 9, m) / 8.0], axis=1).astype(np.float32)
    xyz = np.concatenate([special, rnd])[:n]
    pts = np.zeros((n, 5), np.float32)
    pts[:, 1:4] = xyz
    pts[n // 2:, 0] = 1
    pts[n // 2:, 1] += 128
    return pts, rois


@pytest.mark.gpu
@pytest.mark.parametrize('n', [0, 1, 257])
@pytest.mark.parametrize('o', [1, 65])
def test_part_counts_exact_group(device, o, n):
    """dz_pdv_part_counts and dz_pdv_part_counts_binned against oracle.pdv.part_counts_ref, every count equal, on inputs where all
    arithmetic is exact: points ON inner cell faces (the upper cell), on the lower box faces (in), on the upper faces (quotient == G:
    inside the box, one of max_boxes used up, no cell), |dz| == h / 2 (in), a point in three overlapping boxes with max_boxes = 2, a
    zero-size and a NaN box (nothing), 65 boxes (the second staged chunk of 64 holds one box, with points in it), n = 0 / 1 / 257."""
    pts, rois = exact_part_inputs(o, n)
    ref, _ = opdv.part_counts_ref(pts, rois, 6, 2)
    every, binned = both_part_kernels(torch.from_numpy(pts).to(device), torch.from_numpy(rois).to(device), 6, 2)
    if n == 257:
        assert int(ref[0, 0].sum()) > 30 and int(ref[1, 0].sum()) > 10 and (o == 1 or (int(ref[0, o - 1].sum()) == 2 and not ref[:, 3:5].any()))
        if o > 1:          # the three-box point and the upper-x-face point, by hand: boxes 0 and 1 only / box 1 only
            only, _ = opdv.part_counts_ref(np.array([[0, 0.25, 0.25, 0.125], [0, 1.5, 0.25, 0.125]], np.float32), rois, 6, 2)
            assert only[0, 0].sum() == 1 and only[0, 1].sum() == 2 and only[0, 2].sum() == 0
    assert np.array_equal(every, ref), ('every box', o, n, int(np.abs(every - ref).sum()))
    assert np.array_equal(binned, ref), ('binned', o, n, int(np.abs(binned - ref).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize('o, n, max_boxes', RANDOM_PART_CASES)
def test_part_counts_random_group(device, o, n, max_boxes):
    """The random inputs of tests/test_pdv.py::test_part_counts_binned_equals_every_box: every point whose reference margin is at
    least 1e-4 (no box face, no cell face closer than that in float64, over every box it was tested against) is counted identically by
    both kernels; the points below the margin are left out of the launch.  Their share is below 2 % - a condition the reference
    keeps on its own (test_random_part_inputs_keep_the_margin_cap), not a tolerance."""
    pts, rois, margin, sure, ref = random_part_reference(o, n, max_boxes)
    assert 1.0 - float(sure.mean()) < MARGIN_SHARE_CAP
    kept = pts[torch.from_numpy(sure)].contiguous()
    every, binned = both_part_kernels(kept.to(device), rois.to(device), 6, max_boxes)
    assert int(ref.sum()) > n // 50
    assert np.array_equal(every, ref), ('every box', int(np.abs(every - ref).sum()))
    assert np.array_equal(binned, ref), ('binned', int(np.abs(binned - ref).sum()))


# ------------------------------------------------------------------------------------------------------------------------
# index lookup
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_index_lookup(device):
    """dz_index_lookup on a (3, 5, 7) level of two frames: active cells give their rank (= row in key order), inactive cells and
    coordinates outside the grid on every side give -1, rows behind a device count d_n give -1, rows behind n are not written."""
    rng = np.random.default_rng(9)
    batch, dims = 2, (3, 5, 7)
    cells = make_cells(rng, batch, dims, 0.4)
    lvl = make_level(device, batch, dims, cells)
    every = make_cells(rng, batch, dims, 1.0)
    outside = np.array([[2, 0, 0, 0], [-1, 0, 0, 0], [0, -1, 0, 0], [0, 3, 0, 0], [1, 0, 5, 0], [1, 0, -1, 0], [0, 0, 0, 7], [1, 2, 4, -1]], np.int64)
    query = np.concatenate([every, outside, every[:11]])
    key = lambda a: ((a[:, 0] * 3 + a[:, 1]) * 5 + a[:, 2]) * 7 + a[:, 3]        # noqa: E731
    rank = {int(k): i for i, k in enumerate(key(cells))}
    ok = (query[:, 0] >= 0) & (query[:, 0] < 2) & (query[:, 1] >= 0) & (query[:, 1] < 3) & (query[:, 2] >= 0) & (query[:, 2] < 5) & (query[:, 3] >= 0) & (query[:, 3] < 7)
    ref = np.array([rank.get(int(k), -1) if good else -1 for k, good in zip(key(query), ok)])
    assert (ref >= 0).sum() > 60 and (ref < 0).sum() > 100
    n = query.shape[0]
    tq = torch.from_numpy(query.astype(np.int32)).to(device).contiguous()
    for d_n in (None, n - 5, 0):
        out = torch.full((n + TAIL,), SENT_I, dtype=torch.int32, device=device)
        dn = None if d_n is None else torch.tensor([d_n], dtype=torch.int32, device=device)
        rc = L.load().dz_index_lookup(L.ptr(tq), L.ptr(dn), n, L.ptr(lvl.bitmap), L.ptr(lvl.prefix), batch, *dims, ops.LAYOUT_LINEAR, L.ptr(out), L.stream())
        L.check(rc, 'dz_index_lookup')
        want = ref.copy()
        if d_n is not None:
            want[d_n:] = -1
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], want) and (got[n:] == SENT_I).all(), d_n
