"""ORACLE (test infrastructure only): the three CUDA kernels under the PDV second stage, restated in numpy.

The reference's PDV head (detection/detzero_det/models/centerpoint_modules/pdv_head.py) is Python on top of three compiled
CUDA extensions that cannot be built here (CUDAExtension, <cuda.h>).  Their kernels are short and read literally:
  * ball_query_count_kernel_stack   utils/detzero_utils/ops/pointnet2/pointnet2_stack/src/ball_query_count_gpu.cu:16-62
  * group_points_kernel_stack       .../src/group_points_gpu.cu:71-102
  * points_in_multi_boxes_kernel    utils/detzero_utils/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu:16-36,377-404
tests/golden/gen_pdv_golden.py installs these functions in place of the extension modules and then runs the reference's OWN
Python classes (PDVHead, StackSAModuleMSGAttention, QueryAndGroup, the KDE, TransformerEncoder, density / voxel aggregation
utilities) on the CPU; everything above the three kernels in the fixture is therefore the reference itself.
All arithmetic float32, one rounding per operation (nvcc may contract a*a + b*b into an FMA; a point exactly on a ball or
box boundary could differ - the synthetic inputs keep clear of that, see the margin checks in the generator).
"""
import numpy as np


def ball_query_count(radius, nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt):
    """-> idx (M, nsample) int32, -1 filled: for every query the first `nsample` points of ITS batch item, in index order,
    with squared distance < radius^2; indices are relative to the batch item's first point; a ball without any point has
    idx[0] = -1 (all of its row stays -1)."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    new_xyz = np.ascontiguousarray(new_xyz, np.float32)
    m = new_xyz.shape[0]
    idx = np.full((m, nsample), -1, np.int32)
    r2 = np.float32(radius) * np.float32(radius)
    p_start = np.concatenate([[0], np.cumsum(xyz_batch_cnt)]).astype(np.int64)
    q_start = np.concatenate([[0], np.cumsum(new_xyz_batch_cnt)]).astype(np.int64)
    for b in range(len(xyz_batch_cnt)):
        pts = xyz[p_start[b]:p_start[b + 1]]
        for q in range(q_start[b], q_start[b + 1]):
            d = new_xyz[q][None, :] - pts
            sq = (d * d).astype(np.float32)
            d2 = ((sq[:, 0] + sq[:, 1]).astype(np.float32) + sq[:, 2]).astype(np.float32)
            hit = np.nonzero(d2 < r2)[0][:nsample]
            idx[q, :hit.size] = hit
    return idx


def group_points(features, features_batch_cnt, idx, idx_batch_cnt):
    """-> (M, C, nsample): features[batch start + idx[m, s], c]."""
    features = np.ascontiguousarray(features, np.float32)
    m, ns = idx.shape
    out = np.zeros((m, features.shape[1], ns), np.float32)
    p_start = np.concatenate([[0], np.cumsum(features_batch_cnt)]).astype(np.int64)
    q_start = np.concatenate([[0], np.cumsum(idx_batch_cnt)]).astype(np.int64)
    for b in range(len(idx_batch_cnt)):
        rows = idx[q_start[b]:q_start[b + 1]].astype(np.int64) + p_start[b]
        out[q_start[b]:q_start[b + 1]] = np.transpose(features[rows], (0, 2, 1))
    return out


def point_in_box(pts, box):
    """check_pt_in_box3d: |z - cz| <= dz/2, then the rotated xy test with margin 1e-5 (float32 cos / sin of -heading)."""
    pts = pts.astype(np.float32)
    cx, cy, cz, dx, dy, dz, rz = (np.float32(v) for v in box[:7])
    zok = ~(np.abs(pts[:, 2] - cz).astype(np.float64) > np.float64(dz) / 2.0)
    cosa, sina = np.float32(np.cos(np.float32(-rz))), np.float32(np.sin(np.float32(-rz)))
    sx, sy = pts[:, 0] - cx, pts[:, 1] - cy
    lx = (sx * cosa).astype(np.float32) + (sy * (-sina)).astype(np.float32)
    ly = (sx * sina).astype(np.float32) + (sy * cosa).astype(np.float32)
    inx = np.abs(lx).astype(np.float64) < np.float64(dx) / 2.0 + np.float64(np.float32(1e-5))
    iny = np.abs(ly).astype(np.float64) < np.float64(dy) / 2.0 + np.float64(np.float32(1e-5))
    return zok & inx & iny


def points_in_multi_boxes(points, boxes, max_num_boxes):
    """points (B, M, 3), boxes (B, T, 7) -> (B, M, max_num_boxes) int32: per point the first max_num_boxes boxes (in box order)
    that contain it, -1 filled."""
    bsz, m, _ = points.shape
    out = np.full((bsz, m, max_num_boxes), -1, np.int32)
    for b in range(bsz):
        fill = np.zeros(m, np.int64)
        for k in range(boxes.shape[1]):
            inside = point_in_box(points[b], boxes[b, k]) & (fill < max_num_boxes)
            sel = np.nonzero(inside)[0]
            out[b, sel, fill[sel]] = k
            fill[sel] += 1
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# float64 references of the project's own PDV kernels (tests/test_gpu_pdv_kernels.py).  Decisions (which cell, which ball, which box)
# follow the float32 arithmetic of the reference's Python; everything that is summed or multiplied afterwards is float64.
# ----------------------------------------------------------------------------------------------------------------------------------
def _level_from_keys(key, rows, weights, dims, batch_col):
    """Unique keys ascending, weights summed, weighted mean and per-column max |x| of the member rows (float64)."""
    d, h, w = dims
    uk, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    cols = rows.shape[1]
    sums, amax = np.zeros((uk.size, cols)), np.zeros((uk.size, cols))
    counts = np.zeros(uk.size, np.int64)
    np.add.at(sums, inv, rows * weights[:, None])
    np.add.at(counts, inv, weights)
    np.maximum.at(amax, inv, np.abs(rows))
    mean = sums / np.maximum(counts, 1)[:, None]
    members = np.zeros(uk.size, np.int64)
    np.add.at(members, inv, 1)
    coords = np.stack([uk // (d * h * w), uk // (h * w) % d, uk // w % h, uk % w], axis=1).astype(np.int64)
    if uk.size:
        first = np.zeros(uk.size, np.int64)
        first[inv[::-1]] = np.arange(key.size)[::-1]
        mean[:, 0] = batch_col[first]
    return {'coords': coords, 'counts': counts, 'mean': mean, 'amax': amax, 'members': members, 'inverse': inv}


def centroids_f64(points_b, pc_range, vs, grid, batch, scaling=None):
    """Voxel centroids of points (n, 1 + c) [b, x, y, z, ...] (voxel_aggregation_utils.py:7-159).
    Cell of a point: (p - lo) / vs in float32; outside iff < 0 or >= grid on any axis, or its batch index is not in [0, batch); then
    truncation.  A NaN quotient is outside as well: the reference compares (both comparisons false) and then converts NaN to an
    integer, which has no defined value - no cell can be meant.
    -> [level 1, level 2 (if scaling)]: dicts with coords (m, 4) int64 (b, z, y, x) in ascending key order, counts (m,), mean
    (m, 1 + c) float64 (column 0 = the batch index), amax = max |x| over the cell's members per column (what the error bounds of the
    float32 sums scale with), members = rows summed (points / level-1 cells); level 2: parents = coords // scaling, means weighted by
    the level-1 counts, `child_bound_sum` = sum over the children of count * (count + 3) * amax (test_voxel_centroids' level-2 bound)."""
    p = np.ascontiguousarray(points_b, np.float32).reshape(-1, np.shape(points_b)[1])
    lo, vs = np.asarray(pc_range[:3], np.float32), np.asarray(vs, np.float32)
    gx, gy, gz = (int(v) for v in grid)
    with np.errstate(invalid='ignore', over='ignore'):
        q = ((p[:, 1:4] - lo) / vs).astype(np.float32)
        bf = np.trunc(p[:, 0])
        inside = np.all((q >= 0) & (q < np.array([gx, gy, gz], np.float32)), axis=1) & (bf >= 0) & (bf < batch)
    q, pv, bi = q[inside], p[inside].astype(np.float64), bf[inside].astype(np.int64)
    c = q.astype(np.int64)
    key = ((bi * gz + c[:, 2]) * gy + c[:, 1]) * gx + c[:, 0]
    l1 = _level_from_keys(key, pv, np.ones(key.size, np.int64), (gz, gy, gx), bi.astype(np.float64))
    l1['inside'] = inside
    if scaling is None:
        return [l1]
    s = int(scaling)
    d2, h2, w2 = -(-gz // s), -(-gy // s), -(-gx // s)
    c1 = l1['coords']
    key2 = ((c1[:, 0] * d2 + c1[:, 1] // s) * h2 + c1[:, 2] // s) * w2 + c1[:, 3] // s
    l2 = _level_from_keys(key2, l1['mean'], l1['counts'], (d2, h2, w2), c1[:, 0].astype(np.float64))
    # amax of a parent = over its points = over its children's amax
    amax2 = np.zeros_like(l2['amax'])
    np.maximum.at(amax2, l2['inverse'], l1['amax'])
    l2['amax'] = amax2
    cb = np.zeros_like(amax2)
    np.add.at(cb, l2['inverse'], (l1['counts'] * (l1['counts'] + 3))[:, None] * l1['amax'])
    l2['child_bound_sum'] = cb
    return [l1, l2]


KDE_BANDWIDTH = 0.25
_LOG_SQRT_2PI = 0.91893853320467274178


def kde_density_f64(offsets, cnt):
    """Gaussian kernel density of every sample of a ball at its own position (kde_utils.py:17-64, bandwidth 0.25):
    offsets (..., ns, 3) float32, cnt (...) -> (..., ns) float64: mean over the first cnt samples s of prod_d N((o_e - o_s)_d / h) / h^3.
    Balls with cnt == 0 give 0."""
    o = np.asarray(offsets, np.float32).astype(np.float64)
    cnt = np.asarray(cnt, np.int64)
    ns = o.shape[-2]
    u = (o[..., :, None, :] - o[..., None, :, :]) / KDE_BANDWIDTH                     # [e, s, d]
    k = np.exp(np.sum(-(u * u) / 2.0 - _LOG_SQRT_2PI, axis=-1))
    k = k * (np.arange(ns) < cnt[..., None, None])
    return k.sum(axis=-1) / (KDE_BANDWIDTH ** 3 * np.maximum(cnt, 1)[..., None])


def kde_density_f32(offsets, cnt):
    """The same loop with every operation rounded to float32 (the arithmetic of the device kernels up to their expf and division):
    used only to SIZE the tolerance of the device density against kde_density_f64."""
    o = np.asarray(offsets, np.float32)
    cnt = np.asarray(cnt, np.int64)
    ns = o.shape[-2]
    f = np.float32
    acc = np.zeros(o.shape[:-1], f)
    for s in range(ns):
        lp = np.zeros(o.shape[:-1], f)
        for d in range(3):
            u = ((o[..., :, d] - o[..., s:s + 1, d]).astype(f) / f(KDE_BANDWIDTH)).astype(f)
            lp = (lp + ((-(u * u).astype(f) / f(2.0)).astype(f) - f(_LOG_SQRT_2PI)).astype(f)).astype(f)
        acc = (acc + np.where((s < cnt)[..., None], np.exp(lp).astype(f), f(0))).astype(f)
    h3 = f(f(f(KDE_BANDWIDTH) * f(KDE_BANDWIDTH)) * f(KDE_BANDWIDTH))
    den = (h3 * np.maximum(cnt, 1).astype(f)).astype(f)
    return np.where((cnt > 0)[..., None], (acc / den[..., None]).astype(f), f(0))


def pad_ball_indices(raw):
    """ball_query_count's -1 filled rows -> the kernels' rows: short balls padded with their first hit, empty balls all zero; cnt."""
    raw = np.asarray(raw)
    cnt = (raw >= 0).sum(axis=1).astype(np.int32)
    first = np.where(cnt > 0, raw[:, 0], 0)
    return np.where(raw >= 0, raw, first[:, None]).astype(np.int32), cnt


def group_rows_f64(new_xyz, xyz, feats, batch_start, idx, cnt, row_stride):
    """Rows the pooling MLP consumes (pointnet2_utils.py:192-211): (M, ns, row_stride) float64 =
    [dx, dy, dz (float32 differences), density, the c features of the sample, zero padding]; an empty ball: all zero."""
    new_xyz, xyz, feats = np.asarray(new_xyz, np.float32), np.asarray(xyz, np.float32), np.asarray(feats, np.float32)
    idx, cnt = np.asarray(idx, np.int64), np.asarray(cnt, np.int64)
    m, ns = idx.shape
    c = feats.shape[1]
    v = idx + np.asarray(batch_start, np.int64)[:, None]
    live = cnt > 0
    v = np.where(live[:, None], v, 0)
    with np.errstate(invalid='ignore'):
        off = (xyz[v] - new_xyz[:, None, :]).astype(np.float32)
    off = np.where(live[:, None, None], off, np.float32(0))
    rows = np.zeros((m, ns, row_stride))
    rows[..., 0:3] = off
    rows[..., 3] = kde_density_f64(off, cnt)
    rows[..., 4:4 + c] = np.where(live[:, None, None], feats[v].astype(np.float64), 0.0)
    return rows


def sa_pool_f64(rows, w1, s1, b1, w2, s2, b2, drop=None):
    """One set-abstraction branch (pointnet2_modules.py:31-158) on grouped rows (M, ns, cin): two point-wise layers
    relu(scale * (x W) + shift), max over the ns samples -> (M, h2) float64.
    Also per ball and output channel, maximised over the samples (max and ReLU are 1-Lipschitz):
      D      = |s2| sum_j |w2_j| den1_j + |b2| with den1_j = |s1_j| sum_k |x_k| |w1_kj| + |b1_j|   (the per-layer error bounds scale with it)
      dens   = |s2| sum_j |w2_j| |s1_j| |w1[3, j]| |x_3|     (what a relative error of the density column is multiplied by)
      ones   = |s2| sum_j |w2_j| (|s1_j| sum_k |w1_kj| + 1)  (what an ABSOLUTE error per operand element is multiplied by)
    drop = (ball, sample): that sample is left out of the ball's max (a planted fault for the tests)."""
    import torch
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))      # noqa: E731
    x, w1, s1, b1, w2, s2, b2 = (t(a) for a in (rows, w1, s1, b1, w2, s2, b2))
    hid = torch.relu((x @ w1) * s1 + b1)
    out = torch.relu((hid @ w2) * s2 + b2)
    if drop is not None:
        out[drop[0], drop[1]] = 0.0
    den1 = (x.abs() @ w1.abs()) * s1.abs() + b1.abs()
    d = (den1 @ w2.abs()) * s2.abs() + b2.abs()
    dens = ((x[..., 3:4].abs() * (w1[3].abs() * s1.abs())) @ w2.abs()) * s2.abs()
    ones = ((w1.abs().sum(dim=0) * s1.abs() + 1.0) @ w2.abs()) * s2.abs()
    return {'out': out.amax(dim=1).numpy(), 'D': d.amax(dim=1).numpy(), 'dens': dens.amax(dim=1).numpy(), 'ones': ones.numpy()}


def part_counts_ref(points_b, rois, grid, max_boxes, want_margin=True):
    """Points per box part (density_utils.py:48-109): per point the first max_boxes boxes containing it in box order
    (points_in_multi_boxes above), its cell in each = rotate by -heading, shift to the corner, divide by size / grid in float32;
    a quotient < 0, >= grid or NaN lands in no cell.  points (n, 1 + 3 + ...) [b, x, y, z], rois (B, O, 7).
    -> counts (B, O, G, G, G) int64, margin (n,) float64: the smallest distance of any decision taken for the point from its boundary,
    over every box the point was tested against (boxes up to the one that filled max_boxes).  Membership of one box: inside = the
    nearest of its three face tests (metres), outside = the farthest of the tests that fail (all of them would have to flip); cell: the
    distance of the float64 quotient from the nearest integer (cells).  inf for a point no decision was taken for
    (and for every point with want_margin=False: counts only)."""
    pts = np.asarray(points_b, np.float32)
    rois = np.asarray(rois, np.float32)[..., :7]
    bsz, o = rois.shape[0], rois.shape[1]
    g = int(grid)
    counts = np.zeros((bsz, o, g, g, g), np.int64)
    margin = np.full(pts.shape[0], np.inf)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        bf = np.trunc(pts[:, 0])
        for b in range(bsz):
            sel = np.nonzero(bf == b)[0]
            if sel.size == 0 or o == 0:
                continue
            xyz = pts[sel, 1:4]
            member = points_in_multi_boxes(xyz[None], rois[b][None], max_boxes)[0]              # (m, max_boxes)
            found = np.zeros(sel.size, np.int64)
            mg = np.full(sel.size, np.inf)
            x64 = xyz.astype(np.float64)
            for k in range(o):
                box = rois[b, k]
                tested = found < max_boxes
                isin = (member == k).any(axis=1)
                if want_margin:
                    # ---- margins (float64)
                    cx, cy, cz, dx, dy, dz, rz = (np.float64(v) for v in box)
                    ca, sa = np.cos(-rz), np.sin(-rz)
                    sx, sy = x64[:, 0] - cx, x64[:, 1] - cy
                    lx, ly, lz = sx * ca - sy * sa, sx * sa + sy * ca, x64[:, 2] - cz
                    tz, tx, ty = dz / 2.0 - np.abs(lz), dx / 2.0 + 1e-5 - np.abs(lx), dy / 2.0 + 1e-5 - np.abs(ly)      # >= 0 / > 0: passes
                    t = np.stack([tz, tx, ty], axis=1)
                    ok = np.stack([tz >= 0, tx > 0, ty > 0], axis=1)
                    inside64 = ok.all(axis=1)
                    m_box = np.where(inside64, np.abs(t).min(axis=1), np.where(ok, 0.0, np.abs(t)).max(axis=1))
                    m_box = np.where(np.isnan(m_box), np.inf, m_box)                              # a NaN box: no test can pass, nothing to flip
                    quot = np.stack([(lx + dx / 2.0) / (dx / g), (ly + dy / 2.0) / (dy / g), (lz + dz / 2.0) / (dz / g)], axis=1)
                    m_cell = np.abs(quot - np.clip(np.round(quot), 0, g)).min(axis=1)
                    m_cell = np.where(np.isnan(m_cell), np.inf, m_cell)
                    m_here = np.where(isin | inside64, np.minimum(m_box, m_cell), m_box)
                    mg = np.where(tested, np.minimum(mg, m_here), mg)
                # ---- the cell (float32, the reference's operations)
                idxs = np.nonzero(isin)[0]
                if idxs.size:
                    f = np.float32
                    cosa, sina = f(np.cos(f(-box[6]))), f(np.sin(f(-box[6])))
                    s_x, s_y = xyz[idxs, 0] - box[0], xyz[idxs, 1] - box[1]
                    loc = np.stack([(s_x * cosa).astype(f) + (s_y * (-sina)).astype(f), (s_x * sina).astype(f) + (s_y * cosa).astype(f),
                                    xyz[idxs, 2] - box[2]], axis=1).astype(f)
                    gq = ((loc + (box[3:6] / f(2.0)).astype(f)).astype(f) / (box[3:6] / f(g)).astype(f)).astype(f)
                    good = np.all((gq >= 0) & (gq < f(g)), axis=1)
                    cell = gq[good].astype(np.int64)
                    np.add.at(counts[b, k], (cell[:, 0], cell[:, 1], cell[:, 2]), 1)
                found += isin
            margin[sel] = mg
    return counts, margin
