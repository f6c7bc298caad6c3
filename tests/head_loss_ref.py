"""The tests' own numpy restatement of CenterHead's targets and losses (center_head.py:107-313, loss_utils.py:143-243,
centernet_utils.py:11-71): targets with the reference's float32 operation order, losses and gradients in float64.
tests/test_head_loss_cpu.py pins it to tests/golden/head_loss_golden.npz (the reference's own classes); the GPU tests use it
for inputs the fixture does not hold."""
import numpy as np

F = np.float32
LO, HI = float(F(1e-4)), float(F(1 - 1e-4))          # center_head.py:263 on a float32 tensor
REC_KEYS = ('hm', 'center_x', 'center_y', 'center_z', 'dim_x', 'dim_y', 'dim_z', 'rot_cos', 'rot_sin', 'loc', 'iou', 'total')


def ulps32(a, b):
    """|a - b| in units of float32 spacing at b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(b), np.finfo(F).tiny).astype(F)).astype(np.float64)


def gaussian_radius32(h, w, o):
    """centernet_utils.py:11-37, float32 arrays, python-float scalars rounded to float32 where torch rounds them."""
    om, op, om1, m2o, a16o = F(1 - o), F(1 + o), F(o - 1), F(-2 * o), F(4 * (4 * o))
    s = h + w
    with np.errstate(invalid='ignore'):
        r1 = (s + np.sqrt(s * s - F(4) * (w * h * om / op))) / F(2)
        b2 = F(2) * s
        r2 = (b2 + np.sqrt(b2 * b2 - F(16) * (om * w * h))) / F(2)
        b3 = m2o * s
        r3 = (b3 + np.sqrt(b3 * b3 - a16o * (om1 * w * h))) / F(2)
    return np.minimum(np.minimum(r1, r2), r3)


def gaussian2d(r):
    sigma = (2 * r + 1) / 6
    ax = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(ax[None, :] * ax[None, :] + ax[:, None] * ax[:, None]) / (2 * sigma * sigma))
    g[g < np.finfo(np.float64).eps * g.max()] = 0
    return g


def targets(gt, cls_table, ncls, h, w, stride, pc_range, voxel, nmax, overlap, min_radius):
    """gt (B, M, 8) f32 -> heat (B, ncls, H, W) f32, tb (B, nmax, 8) f64 (columns 3:8 unrounded), inds, masks (B, nmax) i64."""
    gt = np.asarray(gt, F)
    nb = gt.shape[0]
    heat = np.zeros((nb, ncls, h, w), F)
    tb = np.zeros((nb, nmax, 8), np.float64)
    inds = np.zeros((nb, nmax), np.int64)
    masks = np.zeros((nb, nmax), np.int64)
    r0, vs, st = np.asarray(pc_range, F), np.asarray(voxel, F), F(stride)
    table = np.concatenate([[0], np.asarray(cls_table, np.int64)])
    for b in range(nb):
        cls = gt[b, :, 7].astype(np.int64)
        hc = np.where((cls >= 1) & (cls < len(table)), table[np.clip(cls, 0, len(table) - 1)], 0)
        rows = np.nonzero(hc > 0)[0][:nmax]
        g = gt[b, rows]
        cx = np.clip((g[:, 0] - r0[0]) / vs[0] / st, F(0), F(w - 0.5))
        cy = np.clip((g[:, 1] - r0[1]) / vs[1] / st, F(0), F(h - 0.5))
        sx, sy = g[:, 3] / vs[0] / st, g[:, 4] / vs[1] / st
        rf = gaussian_radius32(sx, sy, overlap)
        rad = np.maximum(np.where(np.isfinite(rf), rf, 0).astype(np.int64), min_radius)      # (rows without a radius are skipped below)
        for k in range(len(rows)):
            if sx[k] <= 0 or sy[k] <= 0:
                continue
            x, y, r = int(cx[k]), int(cy[k]), int(rad[k])
            left, right, top, bottom = min(x, r), min(w - x, r + 1), min(y, r), min(h - y, r + 1)
            view = heat[b, hc[rows[k]] - 1, y - top:y + bottom, x - left:x + right]
            np.maximum(view, gaussian2d(r)[r - top:r + bottom, r - left:r + right].astype(F), out=view)
            inds[b, k], masks[b, k] = y * w + x, 1
            d = g[k].astype(np.float64)
            tb[b, k] = [cx[k] - F(x), cy[k] - F(y), d[2], np.log(d[3]), np.log(d[4]), np.log(d[5]), np.cos(d[6]), np.sin(d[6])]
    return heat, tb, inds, masks


# ---- rotated boxes in float64 (exact polygon clipping; the reference's kernel is float32 with its own margins) ----
def _corners(x, y, dx, dy, a):
    c, s = np.cos(a), np.sin(a)
    loc = np.array([[-dx, -dy], [dx, -dy], [dx, dy], [-dx, dy]], np.float64) / 2
    return loc @ np.array([[c, s], [-s, c]]) + [x, y]


def _clip(poly, p, q):
    out = []
    for i in range(len(poly)):
        a, b = poly[i], poly[(i + 1) % len(poly)]
        sa = (q[0] - p[0]) * (a[1] - p[1]) - (q[1] - p[1]) * (a[0] - p[0])
        sb = (q[0] - p[0]) * (b[1] - p[1]) - (q[1] - p[1]) * (b[0] - p[0])
        if sa >= 0:
            out.append(a)
        if (sa >= 0) != (sb >= 0):
            out.append(a + (b - a) * (sa / (sa - sb)))
    return out


def overlap_bev64(a, b):
    poly = list(_corners(a[0], a[1], a[3], a[4], a[6]))
    cb = _corners(b[0], b[1], b[3], b[4], b[6])
    for i in range(4):
        if not poly:
            return 0.0
        poly = _clip(poly, cb[i], cb[(i + 1) % 4])
    if len(poly) < 3:
        return 0.0
    p = np.array(poly)
    return 0.5 * abs(np.sum(p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1]))


def iou3d64(a, b):
    """iou3d_nms_utils.py:74-107 for one pair, float64."""
    oh = max(min(a[2] + a[5] / 2, b[2] + b[5] / 2) - max(a[2] - a[5] / 2, b[2] - b[5] / 2), 0.0)
    o3 = overlap_bev64(a, b) * oh
    return o3 / max(a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - o3, 1e-6)


def losses(head, heat, tb, inds, masks, weights, h, w, stride, pc_range, voxel, hm_mask=None):
    """float64: head (B, H*W, 12), heat (B, ncls, H, W), tb (B, nmax, 8), weights (cls, loc, code[8], iou)
    -> (record dict over REC_KEYS, grad (B, H*W, 12) of the total)."""
    head64 = np.asarray(head, np.float64)
    heat, tb = np.asarray(heat, np.float64), np.asarray(tb, np.float64)
    nb, ncls = heat.shape[0], heat.shape[1]
    cls_w, loc_w, code, iou_w = weights[0], weights[1], np.asarray(weights[2:10], np.float64), weights[10]
    grad = np.zeros(head64.shape, np.float64)
    # focal term
    x = head64[:, :, 9:9 + ncls].reshape(nb, h, w, ncls).transpose(0, 3, 1, 2)
    with np.errstate(over='ignore'):
        sg = 1 / (1 + np.exp(-x))
    free = (sg >= LO) & (sg <= HI)
    p = np.clip(sg, LO, HI)
    m = np.ones((nb, 1, h, w)) if hm_mask is None else np.asarray(hm_mask, np.float64)[:, None]
    pos_i, neg_i = heat == 1, heat < 1
    nw = (1 - heat) ** 4
    pos = np.where(pos_i, np.log(p) * (1 - p) ** 2, 0) * m
    neg = np.where(neg_i, np.log(1 - p) * p ** 2 * nw, 0) * m
    num_pos = float((pos_i * m).sum())
    hm = cls_w * (-neg.sum() if num_pos == 0 else -(pos.sum() + neg.sum()) / num_pos)
    dp = np.where(pos_i, (1 - p) ** 2 / p - 2 * (1 - p) * np.log(p), 0) + np.where(neg_i, (2 * p * np.log(1 - p) - p * p / (1 - p)) * nw, 0)
    gx = -cls_w / (num_pos if num_pos else 1) * m * dp * p * (1 - p) * free
    grad[:, :, 9:9 + ncls] = gx.transpose(0, 2, 3, 1).reshape(nb, h * w, ncls)
    # regression and IoU terms
    num = max(float(masks.sum()), 1.0)
    comp, iou_sum = np.zeros(8), 0.0
    r0, vs, st = np.asarray(pc_range, np.float64), np.asarray(voxel, np.float64), float(stride)
    for b in range(nb):
        for k in np.nonzero(masks[b])[0]:
            ind = int(inds[b, k])
            pr, t = head64[b, ind, :9], tb[b, k]
            d = pr[:8] - t
            comp += np.abs(d)
            grad[b, ind, :8] += loc_w * code * np.sign(d) / num
            if iou_w > 0:
                xs, ys = ind % w, ind // w
                box_p = [(xs + pr[0]) * st * vs[0] + r0[0], (ys + pr[1]) * st * vs[1] + r0[1], pr[2], *np.exp(pr[3:6]), np.arctan2(pr[6], pr[7])]
                box_t = [(xs + t[0]) * st * vs[0] + r0[0], (ys + t[1]) * st * vs[1] + r0[1], t[2], *np.exp(t[3:6]), np.arctan2(t[6], t[7])]
                di = pr[8] - iou3d64(box_p, box_t)
                iou_sum += abs(di)
                grad[b, ind, 8] += iou_w * np.sign(di) / num
    comp = comp / num * code
    loc = loc_w * comp.sum()
    iou = iou_sum / num if iou_w > 0 else 0.0
    rec = dict(zip(REC_KEYS, [hm, *comp, loc, iou, hm + loc + (iou_w * iou if iou_w > 0 else 0.0)]))
    return rec, grad


def tb_dict_of(recs, iou_weight):
    """The reference's tb_dict keys from one record per head."""
    out = {}
    for i, r in enumerate(recs):
        out['hm_loss_head_%d' % i] = r['hm']
        out['loc_loss_head_%d' % i] = r['loc']
        out['center_loss_head_%d' % i] = r['center_x'] + r['center_y']
        out['center_z_loss_head_%d' % i] = r['center_z']
        out['dim_loss_head_%d' % i] = r['dim_x'] + r['dim_y'] + r['dim_z']
        out['rot_loss_head_%d' % i] = r['rot_cos'] + r['rot_sin']
        if iou_weight > 0:
            out['iou_loss_head_%d' % i] = r['iou']
    out['rpn_loss'] = sum(r['total'] for r in recs)
    return out
