"""ORACLE (test infrastructure only): plain float64 / longdouble references and deliberately WRONG variants for the kernels that
carry data between the stages - test-time augmentation and box fusion (oracle/wbf.py), sweep merge (oracle/waymo_io.py), object
crop (oracle/crop.py) - used by tests/test_gpu_sequence_kernels.py next to the restatements those modules hold."""
import numpy as np

from . import wbf as W

F64 = np.float64


# ------------------------------------------------------------------------------------------------ fusion, with planted faults
def fusion_variant(boxes, scores, labels, weights=None, iou_thr=W.IOU_THR, skip_box_thr=W.SKIP_THR, conf_type='avg',
                   allows_overflow=False, argmax='first', compare='gt', thr_f32=False, heading='best'):
    """oracle.wbf.weighted_boxes_fusion_3d (without object ids) with four switches; the defaults ARE that function (the test checks
    it), every other setting is a fault a kernel could have:
      argmax 'last'    the LAST cluster of the largest IoU instead of the first (torch.argmax takes the first)
      compare 'ge'     IoU >= threshold merges (the reference wants >)
      thr_f32          the threshold rounded to float32 before the comparison (the reference widens the float32 IoU to double)
      heading 'last'   the fused heading is the last member's (the reference takes the most confident, i.e. first, member's)"""
    boxes = np.asarray(boxes)
    t = boxes.shape[0]
    scores = np.asarray(scores).reshape(t, -1)
    labels = np.asarray(labels).reshape(t, -1)
    weights = np.ones(t) if weights is None else np.array(weights)
    per_label = {}
    for i in range(t):
        for j in range(boxes.shape[1]):
            lab = int(labels[i][j])
            if lab == 0:
                continue
            per_label.setdefault(lab, []).append([lab, float(scores[i][j]) * weights[i]] + [float(v) for v in boxes[i][j][:7]])
    overall = []
    for lab, rows in per_label.items():
        arr = np.array(rows)
        arr = arr[arr[:, 1].argsort()[::-1]]
        cand = arr[arr[:, 1] >= skip_box_thr[lab - 1]]
        thr = iou_thr[lab - 1]
        groups, fused = [], []
        for j in range(len(cand)):
            idx = -1
            if fused:
                ious = W.iou3d_one_to_many(cand[j][-7:], np.array(fused)[:, -7:])
                best = int(ious.argmax()) if argmax == 'first' else len(ious) - 1 - int(ious[::-1].argmax())
                v = float(ious[best])
                bound = float(np.float32(thr)) if thr_f32 else thr
                if (v >= bound) if compare == 'ge' else (v > bound):
                    idx = best
            if idx != -1:
                groups[idx].append(cand[j])
                fused[idx] = W._fused(groups[idx], conf_type)
                if heading == 'last':
                    fused[idx][-1] = groups[idx][-1][-1]
            else:
                groups.append([cand[j].copy()])
                fused.append(cand[j].copy())
        for i in range(len(groups)):
            n = len(groups[i])
            fused[i][1] = fused[i][1] * (n if allows_overflow else min(weights.sum(), n)) / weights.sum()
        if fused:
            overall.append(np.array(fused))
    if not overall:
        return np.zeros((0, 7)), np.zeros((0,)), np.zeros((0,), int)
    overall = np.concatenate(overall, axis=0)
    overall = overall[overall[:, 1].argsort()[::-1]]
    return overall[:, -7:], overall[:, 1], overall[:, 0].astype(int)


# ------------------------------------------------------------------------------------------------ rotation about z, float64
def rotate_xy_f64(xy, angle):
    """points @ [[c, s], [-s, c]] (common_utils.py:237-242) in float64; the angle is the float32 the reference holds it in."""
    a = F64(np.float32(angle))
    c, s = np.cos(a), np.sin(a)
    xy = np.asarray(xy, F64)
    return np.stack([xy[..., 0] * c - xy[..., 1] * s, xy[..., 0] * s + xy[..., 1] * c], axis=-1)


# ------------------------------------------------------------------------------------------------ sweep merge: the affine rows
def affine_rows(xyz, mat, dtype=F64):
    """x m0 + y m1 + z m2 + m3 for the three rows of mat (3, 4) in `dtype` (float64 or longdouble), left to right, xyz float32."""
    p = np.asarray(xyz, np.float32).astype(dtype)
    m = np.asarray(mat, F64).astype(dtype)
    val = np.empty((p.shape[0], 3), dtype)
    for r in range(3):
        val[:, r] = p[:, 0] * m[r, 0] + p[:, 1] * m[r, 1] + p[:, 2] * m[r, 2] + m[r, 3]
    return val


def near_f32_midpoint(val, rel=2.0 ** -50):
    """True where `val` (longdouble) lies within rel * |val| of the midpoint of its two float32 neighbours: there two float64
    evaluations of the same expression (another order, fused multiply-adds) may round to different float32 values."""
    val = np.asarray(val, np.longdouble)
    near = val.astype(np.float32)
    other = np.nextafter(near, np.where(val > near.astype(np.longdouble), np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    mid = (near.astype(np.longdouble) + other.astype(np.longdouble)) / 2
    return np.abs(val - mid) <= np.longdouble(rel) * np.abs(val)


def ulp_steps(a, b):
    """Distance of two float32 arrays in representable steps (both finite, same sign or zero)."""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


# ------------------------------------------------------------------------------------------------ crop: plain float64 inside test
def inside_f64(points, boxes):
    """(T, M) bool membership of roiaware_pool3d's test in exact float64 (|z| <= dz / 2, |x|, |y| < d / 2 in the box frame) and
    (T, M) float64 distance of every point to the nearest face plane of every box (NaN where a coordinate is NaN)."""
    p = np.asarray(points, F64)[None, :, :3]
    b = np.asarray(boxes, F64)[:, None, :]
    sx, sy, sz = p[..., 0] - b[..., 0], p[..., 1] - b[..., 1], p[..., 2] - b[..., 2]
    c, s = np.cos(b[..., 6]), np.sin(b[..., 6])
    lx, ly = sx * c + sy * s, -sx * s + sy * c
    with np.errstate(invalid='ignore'):
        inside = (np.abs(sz) <= b[..., 5] / 2) & (np.abs(lx) < b[..., 3] / 2) & (np.abs(ly) < b[..., 4] / 2)
        dist = np.minimum(np.minimum(np.abs(np.abs(lx) - b[..., 3] / 2), np.abs(np.abs(ly) - b[..., 4] / 2)), np.abs(np.abs(sz) - b[..., 5] / 2))
    return inside, dist


def crop_rows(mask, payload):
    """What the crop writes for a (T, M) membership: payload rows and point indices in (box, point) order, offsets (T + 1,)."""
    t_idx, p_idx = np.nonzero(mask)
    offsets = np.zeros(mask.shape[0] + 1, np.int64)
    np.cumsum(mask.sum(1), out=offsets[1:])
    return payload[p_idx], p_idx.astype(np.int32), offsets.astype(np.int32)
