"""Box ops (csrc/box_ops.hip, box_geom.h:rect_hull_area): the references of tests/test_gpu_box_ops.py, checked on the CPU, and
everything about the feature that answers without a GPU.

References (all in this file; oracle/ has no hull routine):

  * hull area: a float64 monotone chain over corners computed in float64 from the float32 box values (`hull_ref`), self-checked
    against closed forms.  Per-pair bound of an fp32 implementation: 4 * 2^-23 * max(|x|, |y|, 1) * hull perimeter - corner
    rounding times the length it sweeps (`x`, `y`: the corner coordinates of the pair).  `hull_area_f32` restates
    rect_hull_area operation for operation in numpy float32; over the regimes below its worst error is printed as a fraction of
    the bound.
  * GIoU: the float64 formula (`giou_ref`) fed with a BEV overlap matrix (on the device: dz_boxes_overlap_bev's), the float64
    hull and float64 heights; per-pair tolerance (hull bound / hull area) + 16 * 2^-24 (`giou_tol`).
  * axis-aligned NMS: a greedy sweep with iou_normal evaluated in np.float32 operation for operation (`nms_normal_ref`); keep
    lists must be equal.
"""
import ctypes
import importlib.util
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_TRACKING = '/root/reference/tracking'

F32_EPS = 2.0 ** -23
HEADINGS = [0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi, 1e-7]
REGIMES = ['random', 'identical', 'inside', 'edges', 'headings', 'far', 'tiny']
SHAPES = [(0, 5), (5, 0), (1, 1), (7, 3), (129, 65)]


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
def _heights(rng, n, kind):
    """z, dz with tops / bottoms on a 0.25 m lattice, so that touching pairs overlap by exactly 0 and equal tops are bit-equal."""
    dz = 0.5 + 0.25 * rng.integers(0, 9, n)                  # 0.5 .. 2.5
    bottom = 0.25 * rng.integers(-8, 9, n) if kind == 'mixed' else np.zeros(n)
    return (bottom + dz / 2).astype(np.float32), dz.astype(np.float32)


def random_boxes(n, seed, spread=15.0, centre=(0.0, 0.0)):
    rng = np.random.default_rng(seed)
    b = np.zeros((n, 7), np.float32)
    b[:, 0] = centre[0] + rng.uniform(-spread, spread, n)
    b[:, 1] = centre[1] + rng.uniform(-spread, spread, n)
    b[:, 3] = rng.uniform(0.3, 12.0, n)
    b[:, 4] = rng.uniform(0.3, 12.0, n)
    b[:, 2], b[:, 5] = _heights(rng, n, 'mixed')
    b[:, 6] = rng.uniform(-math.pi, math.pi, n)
    return b


def pair_boxes(regime, na, nb, seed=0):
    """(a (na,7), b (nb,7)) float32.  Row j of b is derived from row j % na of a where the regime is about pairs."""
    rng = np.random.default_rng(1000 + seed)
    a = random_boxes(na, seed)
    b = random_boxes(nb, seed + 1)
    src = a[np.arange(nb) % max(na, 1)] if na else b
    if regime == 'identical':
        b = src.copy()
    elif regime == 'inside':                                  # b strictly inside a's footprint, any heading; heights nested
        b = src.copy()
        b[:, 3:5] = src[:, 3:5].min(axis=1, keepdims=True) * 0.3      # circumradius 0.21 * min side < half min side
        b[:, 6] = rng.uniform(-math.pi, math.pi, nb)
        b[:, 5] = src[:, 5] / 2                                        # same centre, half the height: nested
    elif regime == 'edges':                                   # integer lattice, integer sizes, axis-aligned: shared edges, collinear sides
        for x in (a, b):
            x[:, 0:2] = np.random.default_rng(seed + len(x)).integers(-6, 7, (len(x), 2))
            x[:, 3:5] = np.random.default_rng(seed + 7 + len(x)).integers(1, 5, (len(x), 2))
            x[:, 6] = 0.0
        if na:
            k = np.arange(nb) % na
            b[:, :] = a[k]
            b[:, 0] = a[k, 0] + a[k, 3]                       # b = a moved by its own length: one full shared edge
            b[:, 2] = a[k, 2] + a[k, 5]                       # and heights that touch: overlap exactly 0
    elif regime == 'headings':
        a[:, 6] = np.array(HEADINGS, np.float32)[np.arange(na) % len(HEADINGS)]
        b[:, 6] = np.array(HEADINGS, np.float32)[(np.arange(nb) // 2) % len(HEADINGS)]
        b[:, 0:2] = src[:, 0:2] + rng.uniform(-1, 1, (nb, 2)).astype(np.float32)
    elif regime == 'far':                                     # overlapping neighbours at |x|, |y| ~ 75 m, and pairs 75 m and more apart
        a = random_boxes(na, seed, spread=4.0, centre=(75.0, -75.0))
        b = random_boxes(nb, seed + 1, spread=4.0, centre=(75.0, -75.0))
        b[1::2, 0] -= 75.0
        b[3::4, 1] += 150.0
    elif regime == 'tiny':                                    # a 0.05 m box, a zero-size box, among ordinary ones
        b = src.copy()
        b[0::3, 3:5] = 0.05
        b[1::3, 3:6] = 0.0
        a[2::5, 3:5] = 0.05
        a[4::5, 3:6] = 0.0
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


def nms_boxes(n, seed=0):
    """n boxes in descending score order: tight clusters of near-duplicates scattered over the order, so that suppression chains
    cross 64-column blocks, and some loners."""
    rng = np.random.default_rng(seed)
    n_cl = max(1, n // 12)
    centres = rng.uniform(-40, 40, (n_cl, 2))
    sizes = rng.uniform(1.0, 5.0, (n_cl, 2))
    which = rng.integers(0, n_cl, n)
    b = np.zeros((n, 7), np.float32)
    b[:, 0:2] = centres[which] + rng.normal(0, 0.25, (n, 2)) * sizes[which]
    b[:, 3:5] = sizes[which] * rng.uniform(0.85, 1.15, (n, 2))
    b[:, 2], b[:, 5] = 0.0, 1.5
    b[:, 6] = rng.uniform(-math.pi, math.pi, n)
    return b


# ------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------
def corners64(boxes):
    """(N,7) float32 -> (N,4,2) float64 footprint corners."""
    b = np.asarray(boxes, np.float32).astype(np.float64)
    t = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], np.float64) * 0.5
    loc = t[None] * b[:, None, 3:5]
    c, s = np.cos(b[:, 6])[:, None], np.sin(b[:, 6])[:, None]
    return np.stack([loc[..., 0] * c - loc[..., 1] * s + b[:, None, 0], loc[..., 0] * s + loc[..., 1] * c + b[:, None, 1]], axis=-1)


def _chain64(pts):
    """float64 monotone chain -> hull vertices (counter-clockwise)."""
    P = sorted(set((float(x), float(y)) for x, y in pts))
    if len(P) <= 2:
        return P
    cross = lambda o, p, q: (p[0] - o[0]) * (q[1] - o[1]) - (p[1] - o[1]) * (q[0] - o[0])      # noqa: E731
    lower, upper = [], []
    for p in P:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(P):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def hull_ref(a, b):
    """-> (area, bound) float64 (N,M): convex hull area of the 8 corners of each pair and the fp32 error bound
    4 * 2^-23 * max(|x|, |y|, 1) * perimeter."""
    ca, cb = corners64(a), corners64(b)
    area = np.zeros((len(a), len(b)))
    bound = np.zeros((len(a), len(b)))
    for i in range(len(a)):
        for j in range(len(b)):
            pts = np.concatenate([ca[i], cb[j]])
            H = _chain64(pts)
            m = len(H)
            ar = 0.5 * abs(sum(H[k][0] * H[(k + 1) % m][1] - H[(k + 1) % m][0] * H[k][1] for k in range(m))) if m >= 3 else 0.0
            per = sum(math.hypot(H[k][0] - H[(k + 1) % m][0], H[k][1] - H[(k + 1) % m][1]) for k in range(m)) if m >= 2 else 0.0
            area[i, j] = ar
            bound[i, j] = 4 * F32_EPS * max(float(np.abs(pts).max()), 1.0) * per
    return area, bound


_REF_CACHE = {}


def pair_case(regime, shape):
    """Inputs and float64 hull reference of one (regime, shape), computed once and shared by the tests that need them."""
    key = (regime, shape)
    if key not in _REF_CACHE:
        a, b = pair_boxes(regime, shape[0], shape[1])
        area, bound = hull_ref(a, b)
        for x in (a, b, area, bound):
            x.setflags(write=False)
        _REF_CACHE[key] = (a, b, area, bound)
    return _REF_CACHE[key]


def heights64(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    a_max, a_min = (a[:, 2] + a[:, 5] / 2)[:, None], (a[:, 2] - a[:, 5] / 2)[:, None]
    b_max, b_min = (b[:, 2] + b[:, 5] / 2)[None, :], (b[:, 2] - b[:, 5] / 2)[None, :]
    return a_max, a_min, b_max, b_min


def giou_ref(a, b, overlap_bev, hull_area, exact, with_ratio=False):
    """iou3d_nms_utils.py:110-151 in float64; exact=False keeps its enclosing height min(tops) - min(bottoms).
    with_ratio: also U / C, the term through which the hull enters (<= 1 for a true enclosing volume)."""
    a_max, a_min, b_max, b_min = heights64(a, b)
    oh = np.maximum(np.minimum(a_max, b_max) - np.maximum(a_min, b_min), 0)
    top = np.maximum(a_max, b_max) if exact else np.minimum(a_max, b_max)
    uh = np.maximum(top - np.minimum(a_min, b_min), 0)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    o3 = np.asarray(overlap_bev, np.float64) * oh
    c3 = np.maximum(hull_area * uh, 1e-6)
    u3 = np.maximum((a64[:, 3] * a64[:, 4] * a64[:, 5])[:, None] + (b64[:, 3] * b64[:, 4] * b64[:, 5])[None, :] - o3, 1e-6)
    g = o3 / u3 - (c3 - u3) / c3
    return (g, u3 / c3) if with_ratio else g


def giou_tol(hull_area, hull_bound, ratio=None):
    """(hull bound / hull area) + 16 * 2^-24 per pair: the hull is the only non-rounding error source and enters through U/C;
    the second term covers the half-dozen fp32 operations on values of magnitude <= 1.  A hull of area 0 (coincident or
    collinear points) has its C clamped to 1e-6 on both sides: no hull term where the bound is 0 too, none needed (inf) otherwise.

    Both terms presuppose U / C <= 1, which holds for a true enclosing volume: always with the exact height, and with the
    reference's height term where the tops are equal.  Where one top is above the other the reference's C can be smaller than
    U without limit (C is clamped at 1e-6: a zero-height box under a 100 m^3 one gives -(C - U) / C = 1e8), the error of U / C
    is (U / C) * (hull bound / hull area) and an fp32 rounding is 2^-24 of a value of magnitude U / C.  `ratio` = U / C of the
    float64 reference scales the tolerance by max(1, U / C) for those pairs: the same derivation without its premise, and
    the same number wherever the premise holds."""
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(hull_area > 0, hull_bound / hull_area, np.where(hull_bound > 0, np.inf, 0.0))
    tol = rel + 16 * 2.0 ** -24
    return tol if ratio is None else tol * np.maximum(1.0, ratio)


def iou_normal32(box, others):
    """iou3d_nms_kernel.cu:433-444 in np.float32, operation for operation: one box against (K,7)."""
    f = np.float32
    a, b = np.asarray(box, f), np.asarray(others, f)
    two = f(2)
    left = np.maximum(a[0] - a[3] / two, b[:, 0] - b[:, 3] / two)
    right = np.minimum(a[0] + a[3] / two, b[:, 0] + b[:, 3] / two)
    top = np.maximum(a[1] - a[4] / two, b[:, 1] - b[:, 4] / two)
    bottom = np.minimum(a[1] + a[4] / two, b[:, 1] + b[:, 4] / two)
    width, height = np.maximum(right - left, f(0)), np.maximum(bottom - top, f(0))
    inter = width * height
    sa, sb = a[3] * a[4], b[:, 3] * b[:, 4]
    out = inter / np.maximum(sa + sb - inter, f(1e-8))
    assert out.dtype == np.float32
    return out


def nms_normal_ref(boxes, thresh, post_max):
    """Greedy by order: keep box i unless a kept earlier box has iou_normal > thresh with it; at most post_max."""
    n = len(boxes)
    thr = np.float32(thresh)
    gone = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if gone[i] or len(keep) >= post_max:
            continue
        keep.append(i)
        if i + 1 < n:
            gone[i + 1:] |= iou_normal32(boxes[i], boxes[i + 1:]) > thr
    return np.array(keep, np.int64)


def on_threshold_pair():
    """Unit squares offset 0.5: IoU = 0.5 / 1.5 = np.float32(1/3) exactly."""
    b = np.zeros((2, 7), np.float32)
    b[:, 3:6] = 1.0
    b[1, 0] = 0.5
    return b


# ---- rect_hull_area restated in float32 (CPU check of the algorithm: the 19-exchange network, the chain, the shoelace)
_NETWORK = [(0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7), (0, 1), (2, 3), (4, 5), (6, 7), (2, 4), (3, 5), (1, 4), (3, 6),
            (1, 2), (3, 4), (5, 6)]


def hull_area_f32(A, B):
    f = np.float32

    def corners(X):
        hx, hy = X[3] / f(2), X[4] / f(2)
        c, s = f(np.cos(X[6])), f(np.sin(X[6]))
        out = []
        for px, py in ((X[0] - hx, X[1] - hy), (X[0] + hx, X[1] - hy), (X[0] + hx, X[1] + hy), (X[0] - hx, X[1] + hy)):
            out.append(((px - X[0]) * c + (py - X[1]) * (-s) + X[0], (px - X[0]) * s + (py - X[1]) * c + X[1]))
        return out
    A, B = np.asarray(A, f), np.asarray(B, f)
    p = corners(A) + corners(B)
    for i, j in _NETWORK:
        if p[j][0] < p[i][0] or (p[j][0] == p[i][0] and p[j][1] < p[i][1]):
            p[i], p[j] = p[j], p[i]
    cr3 = lambda p1, p2, p0: (p1[0] - p0[0]) * (p2[1] - p0[1]) - (p2[0] - p0[0]) * (p1[1] - p0[1])      # noqa: E731
    stk = []
    for i in range(8):
        while len(stk) >= 2 and cr3(stk[-1], p[i], stk[-2]) <= 0:
            stk.pop()
        stk.append(p[i])
    floor_k = len(stk) + 1
    for i in range(6, -1, -1):
        while len(stk) >= floor_k and cr3(stk[-1], p[i], stk[-2]) <= 0:
            stk.pop()
        if len(stk) < 9:
            stk.append(p[i])
    area = f(0)
    for j in range(1, len(stk) - 2):
        u = (stk[j][0] - stk[0][0], stk[j][1] - stk[0][1])
        v = (stk[j + 1][0] - stk[0][0], stk[j + 1][1] - stk[0][1])
        area = area + (u[0] * v[1] - u[1] * v[0])
    assert isinstance(area, np.float32)
    return abs(area) / f(2)


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the references themselves
# ------------------------------------------------------------------------------------------------------------------------
def _box(x, y, dx, dy, heading=0.0):
    return np.array([[x, y, 0, dx, dy, 1, heading]], np.float32)


def test_hull_ref_closed_forms():
    a = _box(3.0, -2.0, 4.0, 1.5, 0.7)
    assert abs(hull_ref(a, a)[0][0, 0] - 6.0) < 1e-6                                      # identical boxes -> dx * dy
    assert abs(hull_ref(_box(0, 0, 1, 1), _box(2, 0, 1, 1))[0][0, 0] - 3.0) < 1e-12         # unit squares offset (2, 0) -> 3
    got = hull_ref(_box(0, 0, 1, 1), _box(0, 0, 1, 1, math.pi / 4))[0][0, 0]               # plus itself turned 45 deg -> sqrt 2
    assert abs(got - math.sqrt(2)) < 1e-6            # (the float32 heading is pi/4 to 2e-8 only)
    area, bound = hull_ref(_box(0, 0, 0, 0), _box(0, 0, 0, 0))
    assert area[0, 0] == 0 and bound[0, 0] == 0


def test_sorting_network_sorts_every_zero_one_input():
    for bits in range(256):
        v = [(bits >> k) & 1 for k in range(8)]
        for i, j in _NETWORK:
            if v[j] < v[i]:
                v[i], v[j] = v[j], v[i]
        assert v == sorted(v)


@pytest.mark.parametrize('regime', REGIMES)
def test_hull_f32_restatement_within_bound(regime):
    """The algorithm of rect_hull_area in numpy float32 against the float64 chain, on the (7, 3) and part of the (129, 65) case."""
    worst = 0.0
    for shape, rows in (((7, 3), 7), ((129, 65), 12)):
        a, b, area, bound = pair_case(regime, shape)
        for i in range(rows):
            for j in range(b.shape[0]):
                err = abs(float(hull_area_f32(a[i], b[j])) - area[i, j])
                assert err <= bound[i, j], (regime, i, j, err, bound[i, j])
                if bound[i, j] > 0:
                    worst = max(worst, err / bound[i, j])
    print('\n[box_ops] hull fp32 restatement %-10s worst error / bound %.3f' % (regime, worst))


def test_inputs_reach_the_height_cases():
    """The 3-D regimes hold disjoint, touching (overlap exactly 0) and nested heights, and pairs with equal and unequal tops."""
    seen = set()
    for regime in REGIMES:
        a, b, _, _ = pair_case(regime, (129, 65))
        a_max, a_min, b_max, b_min = heights64(a, b)
        d = np.minimum(a_max, b_max) - np.maximum(a_min, b_min)
        if np.any(d < 0):
            seen.add('disjoint')
        if np.any((d == 0) & (a_max > a_min) & (b_max > b_min)):
            seen.add('touching')
        if np.any((a_min < b_min) & (b_max < a_max)):
            seen.add('nested')
        if np.any(a_max == b_max):
            seen.add('equal tops')
    assert seen == {'disjoint', 'touching', 'nested', 'equal tops'}


def test_giou_ref_values():
    a = _box(0, 0, 2, 2)
    ov = lambda x, y: np.array([[1.0 * max(0.0, 2 - abs(float(x[0, 0] - y[0, 0]))) * 2]])      # noqa: E731  axis-aligned 2 x 2 squares
    area = hull_ref(a, a)[0]
    assert abs(giou_ref(a, a, ov(a, a), area, True)[0, 0] - 1.0) < 1e-12 and abs(giou_ref(a, a, ov(a, a), area, False)[0, 0] - 1.0) < 1e-12
    far = _box(6, 0, 2, 2)
    g = giou_ref(a, far, ov(a, far), hull_ref(a, far)[0], True)[0, 0]            # IoU 0, U = 8, C = 16 -> -0.5
    assert abs(g + 0.5) < 1e-12
    # the reference's height term: same footprint and bottom, heights 1 and 10 -> O = 4, U = 40, C = 4 * 1: 0.1 - (4 - 40) / 4 = 9.1;
    # the quantity the tracker uses is NOT confined to [-1, 1] where one box's top is above the other's
    lo, hi = _box(0, 0, 2, 2), _box(0, 0, 2, 2)
    lo[0, 2], lo[0, 5], hi[0, 2], hi[0, 5] = 0.5, 1.0, 5.0, 10.0
    assert abs(giou_ref(lo, hi, ov(lo, hi), hull_ref(lo, hi)[0], False)[0, 0] - 9.1) < 1e-12
    assert abs(giou_ref(lo, hi, ov(lo, hi), hull_ref(lo, hi)[0], True)[0, 0] - 0.1) < 1e-12


def test_on_threshold_pair_is_one_third_in_float32():
    b = on_threshold_pair()
    iou = iou_normal32(b[0], b[1:])[0]
    assert iou == np.float32(1 / 3)
    thr = float(np.float32(1 / 3))
    assert nms_normal_ref(b, thr, 2).tolist() == [0, 1]                                       # '>' : on the threshold survives
    assert nms_normal_ref(b, float(np.nextafter(np.float32(1 / 3), np.float32(0))), 2).tolist() == [0]


def test_nms_normal_ref_chains_and_post_max():
    b = np.zeros((4, 7), np.float32)
    b[:, 3:6] = 1.0
    b[:, 0] = [0.0, 0.3, 0.6, 5.0]            # 1 suppressed by 0; 2 overlaps 1 (gone) but not 0 enough: 0.4 / 1.6 = 0.25
    assert nms_normal_ref(b, 0.3, 4).tolist() == [0, 2, 3]
    assert nms_normal_ref(b, 0.3, 2).tolist() == [0, 2]
    turned = b.copy()
    turned[:, 6] = [0.3, -1.0, 2.0, 0.5]      # the heading is ignored
    assert nms_normal_ref(turned, 0.3, 4).tolist() == [0, 2, 3]
    big = nms_boxes(500, 3)
    keep = nms_normal_ref(big, 0.5, 500)
    assert 20 < len(keep) < 400 and keep.max() >= 448            # suppression happened, and decisions reach the last column block


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the C ABI and the Python surface
# ------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ['dz_boxes_pairwise_metric', 'dz_nms_normal', 'dz_nms_normal_batched']


def test_new_symbols_in_header_binding_and_library():
    from detzero_amd import lib as L
    from detzero_amd.build import build
    build(verbose=False)
    header = open(os.path.join(ROOT, 'include', 'detzero_hip.h')).read()
    cdll = ctypes.CDLL(L.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s + '(' in header and s in L.exported_symbols() and hasattr(cdll, s)
    for i, name in enumerate(['DZ_BOXM_UNION_BEV', 'DZ_BOXM_IOU3D', 'DZ_BOXM_GIOU3D', 'DZ_BOXM_GIOU3D_EXACT']):
        assert '#define %s %d' % (name, i) in header
    from detzero_amd import ops
    assert (ops.BOXM_UNION_BEV, ops.BOXM_IOU3D, ops.BOXM_GIOU3D, ops.BOXM_GIOU3D_EXACT) == (0, 1, 2, 3)


def test_host_side_argument_checks():
    """Refusals that are decided before any launch: they answer on a machine without a GPU (the pointers are host scratch, never read)."""
    from detzero_amd import lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    assert lib.dz_boxes_pairwise_metric(p, -1, p, 3, 1, p, None) == L.ERR_INVALID
    assert b'negative size' in lib.dz_last_error()
    assert lib.dz_boxes_pairwise_metric(p, 2, p, 3, 7, p, None) == L.ERR_UNSUPPORTED
    assert b'unknown metric 7' in lib.dz_last_error()
    assert lib.dz_boxes_pairwise_metric(p, 2, p, 3, -1, p, None) == L.ERR_UNSUPPORTED
    assert lib.dz_boxes_pairwise_metric(p, 0, p, 3, 1, p, None) == 0 and lib.dz_boxes_pairwise_metric(None, 3, None, 0, 3, None, None) == 0
    assert lib.dz_boxes_pairwise_metric(None, 2, p, 3, 1, p, None) == L.ERR_INVALID
    ws = lib.dz_nms_workspace_bytes(5000)
    assert lib.dz_nms_normal(p, None, 5000, 0.5, 10, p, p, p, ws, None) == L.ERR_INVALID
    assert b'4096' in lib.dz_last_error()
    assert lib.dz_nms_normal_batched(p, None, 2, 5000, 0.5, 10, p, p, p, 2 * ws, None) == L.ERR_INVALID
    assert lib.dz_nms_normal(p, None, -1, 0.5, 10, p, p, p, ws, None) == L.ERR_INVALID
    assert lib.dz_nms_normal(p, None, 8, 0.5, 10, None, p, p, ws, None) == L.ERR_INVALID            # keep
    assert lib.dz_nms_normal(None, None, 8, 0.5, 10, p, p, p, ws, None) == L.ERR_INVALID            # boxes
    assert lib.dz_nms_normal(p, None, 64, 0.5, 10, p, p, p, 8, None) == L.ERR_WORKSPACE
    assert lib.dz_nms_normal_batched(p, None, 0, 64, 0.5, 10, p, p, None, 0, None) == 0              # empty batch: no launch


def test_nms_normal_gpu_refuses_more_than_4096_boxes():
    import torch
    from detzero_amd import iou3d_nms_utils
    from detzero_amd.lib import DetZeroHipError
    with pytest.raises(DetZeroHipError, match='4096'):
        iou3d_nms_utils.nms_normal_gpu(torch.zeros(4097, 7), torch.zeros(4097), 0.5)


def test_shim_packages_expose_the_names():
    from detzero_amd import shim
    shim.install()
    from detzero_utils.ops.iou3d_nms import iou3d_nms_cuda, iou3d_nms_utils
    from detzero_utils.ops.roiaware_pool3d import roiaware_pool3d_utils
    import detzero_amd.iou3d_nms_utils as ours
    for name in ('boxes_iou_bev', 'boxes_iou3d_gpu', 'boxes_giou3d_gpu', 'boxes_union_bev_gpu', 'boxes_overlap_bev_gpu', 'nms_gpu', 'nms_normal_gpu'):
        assert getattr(iou3d_nms_utils, name) is getattr(ours, name)
    for name in ('boxes_overlap_bev_gpu', 'boxes_iou_bev_gpu', 'boxes_union_bev_gpu', 'nms_gpu', 'nms_normal_gpu'):
        assert callable(getattr(iou3d_nms_cuda, name))
    for name in ('points_in_boxes_gpu_v2', 'points_in_boxes_num_gpu'):
        assert callable(getattr(roiaware_pool3d_utils, name))


def test_reference_tracker_distance_module_loads_on_the_shim():
    path = os.path.join(REFERENCE_TRACKING, 'detzero_track', 'models', 'tracking_modules', 'data_association', 'distance.py')
    if not os.path.exists(path):
        pytest.skip('the reference tracker is not on this machine')
    pytest.importorskip('scipy')
    from detzero_amd import shim
    shim.install()
    spec = importlib.util.spec_from_file_location('_reference_distance', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    e7, b7 = np.zeros((0, 7), np.float32), np.zeros((3, 7), np.float32)
    for fn in (mod.bev_overlap_gpu, mod.IoUBEV_dis_mat, mod.IoU3D_dis_mat, mod.GIoU3D_dis_mat):
        out = fn(e7, b7)
        assert out.shape == (0, 3) and not out.any()
    out = mod.IoU2D_dis_mat(np.zeros((0, 4), np.float32), np.ones((3, 4), np.float32))
    assert out.shape == (0, 3) and not out.any()
    sys.modules.pop('_reference_distance', None)


def _head(nms_type):
    from detzero_amd.config import AttrDict
    from detzero_amd.det_modules import CenterHead
    from detzero_amd.synth import POINT_CLOUD_RANGE, VOXEL_SIZE_01
    from oracle import voxelize as ov
    names = ['Vehicle', 'Pedestrian', 'Cyclist']
    branch = lambda c: {'out_channels': c, 'num_conv': 2}      # noqa: E731
    hcfg = AttrDict({
        'CLASS_NAMES_EACH_HEAD': [names], 'SHARED_CONV_CHANNEL': 32, 'USE_BIAS_BEFORE_NORM': True, 'NUM_HM_CONV': 2, 'IOU_WEIGHT': 1,
        'SEPARATE_HEAD_CFG': {'HEAD_ORDER': ['center', 'center_z', 'dim', 'rot', 'iou'],
                              'HEAD_DICT': {'center': branch(2), 'center_z': branch(1), 'dim': branch(3), 'rot': branch(2), 'iou': branch(1)}},
        'TARGET_ASSIGNER_CONFIG': {'FEATURE_MAP_STRIDE': 8},
        'POST_PROCESSING': {'SCORE_THRESH': 0.03, 'POST_CENTER_LIMIT_RANGE': [-80, -80, -10.0, 80, 80, 10.0], 'MAX_OBJ_PER_SAMPLE': 128,
                            'NMS_CONFIG': {'NMS_TYPE': nms_type, 'NMS_THRESH': 0.3, 'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': 50}}})
    return CenterHead(hcfg, 64, 3, names, ov.grid_size_of(POINT_CLOUD_RANGE, VOXEL_SIZE_01), POINT_CLOUD_RANGE, VOXEL_SIZE_01).eval()


@pytest.mark.parametrize('nms_type', ['circle_nms', 'nms_cpu'])
def test_head_refuses_other_nms_types(nms_type):
    from detzero_amd.lib import DetZeroHipError
    with pytest.raises(DetZeroHipError, match='circle_nms'):
        _head(nms_type).decode_batched_nosync(None, 24, 24)


def test_proposal_layer_refuses_an_unknown_nms_type():
    import torch
    from detzero_amd.config import AttrDict
    from detzero_amd.lib import DetZeroHipError
    from detzero_amd.pdv_modules import PDVHead
    cfg = AttrDict({'NMS_TYPE': 'nms_cpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 64, 'NMS_POST_MAXSIZE': 16, 'NMS_THRESH': 0.7})
    batch = {'batch_size': 1, 'batch_box_preds': torch.zeros(1, 4, 7), 'batch_cls_preds': torch.zeros(1, 4, 1)}
    with pytest.raises(DetZeroHipError, match='nms_cpu'):
        PDVHead.proposal_layer(None, batch, cfg)
