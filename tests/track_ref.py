"""Test helper: numpy restatement of the tracker's seven per-frame ops (predict, affinity, update, spawn, merge, compact, log).

A literal port of the per-track arithmetic of the reference's KalmanFilter (kalman_filter.py:10-146: the same 5x5 / 3x3 numpy
products in the same order), of one_stage's masking + GNN_assignment's 5000 (data_association.py:36-58, distance.py:22) and of
overlap_track_merge's sweep (track_manager.py:283-303), with the state in float32 (default, what the reference computes on float32
detections) or float64 (``dtype=np.float64``: the yardstick of the numeric tolerances).  The rotated-overlap geometry comes from
the oracle's C restatement (oracle/cref.py) in fp32 in both modes: it only feeds discrete decisions.

``NumpyTrackOps`` implements the ops interface of detzero_amd.track_models.HipTrackOps, so the product's TrackManager can be
driven without a GPU.
"""
import numpy as np

from oracle import cref

ROW_WORDS = 16
ROW_SCORE, ROW_HIT, ROW_NPTS, ROW_ID, ROW_CLS, ROW_FRAME = 9, 10, 11, 12, 13, 14
AFF_IOU_BEV, AFF_IOU3D, AFF_GIOU3D = 16, 1, 2


# ------------------------------------------------------------------------------------------------
# pair geometry (fp32)
# ------------------------------------------------------------------------------------------------
def iou3d(a, b):
    """iou3d_nms_utils.boxes_iou3d_gpu in float32 numpy around the oracle's BEV overlap."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    a_max, a_min = (a[:, 2] + a[:, 5] / 2)[:, None], (a[:, 2] - a[:, 5] / 2)[:, None]
    b_max, b_min = (b[:, 2] + b[:, 5] / 2)[None, :], (b[:, 2] - b[:, 5] / 2)[None, :]
    bev = cref.boxes_overlap_bev(a[:, :7], b[:, :7])
    oh = np.maximum(np.minimum(a_max, b_max) - np.maximum(a_min, b_min), np.float32(0))
    o3 = bev * oh
    va, vb = ((a[:, 3] * a[:, 4]) * a[:, 5])[:, None], ((b[:, 3] * b[:, 4]) * b[:, 5])[None, :]
    return (o3 / np.maximum((va + vb) - o3, np.float32(1e-6))).astype(np.float32)


def affinity(row_boxes, col_boxes, metric):
    if metric == AFF_IOU_BEV:
        return cref.boxes_iou_bev(row_boxes[:, :7], col_boxes[:, :7])
    if metric == AFF_IOU3D:
        return iou3d(row_boxes, col_boxes)
    raise NotImplementedError('GIoU3D: the convex hull has no CPU restatement in this helper')


def mask_affinity(aff, row_cls, col_cls, distinguish_class, thr):
    """one_stage's masking on an affinity matrix (in place), returns it."""
    thr = np.asarray(thr, dtype=np.float32)
    if aff.shape[0] and aff.shape[1]:
        for r, c in enumerate(row_cls):
            if distinguish_class:
                aff[r, col_cls != c] = 0.
            aff[r, aff[r, :] < thr[c]] = 0.
    return aff


def cost_of(aff):
    cost = np.float32(1.0) - aff
    cost[cost >= 1.] = 5000.
    return cost


def cost_matrix(row_boxes, row_cls, col_boxes, col_cls, metric, distinguish_class, thr, gaps=None):
    aff = affinity(np.asarray(row_boxes, np.float32), np.asarray(col_boxes, np.float32), metric)
    if gaps is not None and aff.size:
        t = np.asarray(thr, np.float32)[np.asarray(row_cls)][:, None]
        same = (np.asarray(row_cls)[:, None] == np.asarray(col_cls)[None, :]) | (not distinguish_class)
        live = same & (aff > 0)
        if live.any():
            gaps.append(float(np.min(np.abs(aff - t)[live])))
    return cost_of(mask_affinity(aff, np.asarray(row_cls), np.asarray(col_cls), distinguish_class, thr))


# ------------------------------------------------------------------------------------------------
# one track (kalman_filter.py)
# ------------------------------------------------------------------------------------------------
class Track:
    def __init__(self, box7, cls, score, num_points, track_id, p, q, dt, dtype=np.float32):
        box7 = np.asarray(box7, dtype=dtype)
        self.dtype = dtype
        self.size, self.heading = box7[3:6].copy(), box7[6].copy()
        self.cls, self.score, self.update_score, self.num_points, self.track_id = int(cls), score, score, int(num_points), int(track_id)
        self.x = np.zeros((5, 1), dtype=dtype)
        self.x[:3, :] = box7[:3].reshape(3, 1)
        self.bbox = np.zeros(9, dtype=dtype)
        self.bbox[:7] = box7[:7]
        self.F, self.P, self.Q = np.eye(5, dtype=dtype), np.eye(5, dtype=dtype), np.eye(5, dtype=dtype)
        self.H, self.R = np.eye(3, 5, dtype=dtype), np.eye(3, dtype=dtype)
        self.F[:2, 3:5] = np.eye(2, dtype=dtype) * dtype(dt)
        self.P[:3, :3] = self.P[:3, :3] * p[0]
        self.P[3:, 3:] = self.P[3:, 3:] * p[1]
        self.Q[:3, :3] = self.Q[:3, :3] * q[0]
        self.Q[3:, 3:] = self.Q[3:, 3:] * q[1]
        self.hit, self.miss = 1, 0

    def predict(self, gate_class, gaps=None):
        temp_x = self.x.copy()
        if self.cls == gate_class:
            speed, half = np.linalg.norm(temp_x[3:]), np.max(self.size) / 2.
            if gaps is not None and max(speed, half) > 0:
                gaps.append(float(abs(speed - half) / max(speed, half)))
            if speed <= half:
                temp_x[3:] = 0.
        self.x = self.F @ temp_x
        self.P = self.F @ self.P @ self.F.T + self.Q
        self.Q = self.Q * self.dtype(1.5)
        self.miss += 1
        self.hit = 0
        self.bbox = np.concatenate((self.x.reshape(-1)[:3], self.size, self.heading.reshape(-1), self.x.reshape(-1)[3:5]), axis=0)
        return self.bbox

    def update(self, box7, cls, score, num_points, stage, r):
        self.hit, self.miss = 1, 0
        self.score, self.num_points = score, int(num_points)
        if stage:
            self.hit = 2
            return
        box7 = np.asarray(box7, dtype=self.dtype)
        self.cls = int(cls)
        self.update_score = max(score, 0.03)
        z = box7[:3].reshape(3, 1)
        self.size, self.heading = box7[3:6].copy(), box7[6].copy()
        res_z = z - self.H @ self.x
        S = self.H @ self.P @ self.H.T + self.R * self.dtype(r)
        K = self.P @ self.H.T @ np.linalg.inv(S)
        self.x = self.x + K @ res_z
        self.P = self.P - K @ self.H @ self.P
        self.x[:3] = z
        self.bbox = np.concatenate((box7[0:3], self.size, self.heading.reshape(-1), self.x.reshape(-1)[3:5]), axis=0)


# ------------------------------------------------------------------------------------------------
# merge (track_manager.py:262-310)
# ------------------------------------------------------------------------------------------------
def merge_sweep(overlap, area, cls, ids, thr, gaps=None):
    """The reference's sweep on a given (T,T) float32 overlap-area matrix (modified in place): removed (T,) bool."""
    t = len(cls)
    cls, ids = np.asarray(cls), np.asarray(ids)
    thr = np.asarray(thr, dtype=np.float32)
    for i in range(t):
        overlap[i, cls != cls[i]] = 0.
    keep, dep = set(), set()
    for i in range(t):
        if i in dep or i in keep:
            continue
        ratio = overlap[i] / (area[i] + np.float32(1e-9))
        if gaps is not None:
            live = ratio > 0
            gaps.append(float(np.min(np.abs(ratio[live] - thr[cls[i]]))) if live.any() else 1.0)
        at = np.flatnonzero(ratio >= thr[cls[i]])
        if len(at) == 0:
            continue
        order = np.argsort(ids[at], kind='stable')
        best = at[order[0]]
        if best not in dep:
            keep.add(best)
            overlap[:, at] = 0.
            dep.update(at[order[1:]].tolist())
    removed = np.zeros(t, dtype=bool)
    removed[sorted(dep)] = True
    return removed


# ------------------------------------------------------------------------------------------------
# the ops object
# ------------------------------------------------------------------------------------------------
class NumpyTrackOps:
    """detzero_amd.track_models.HipTrackOps's interface on a Python list of ``Track``.  ``gaps`` (a dict of lists) collects the
    distances of every discrete comparison from its threshold; ``history`` keeps, per finished pass, the log rows and the logged
    boxes in the state's own precision."""

    def __init__(self, dtype=np.float32, gaps=None):
        self.dtype = dtype
        self.gaps = gaps
        self.history = []
        self.costs = []
        self.start_pass()

    def _gap(self, key):
        return None if self.gaps is None else self.gaps.setdefault(key, [])

    @property
    def n(self):
        return len(self.tracks)

    def start_pass(self, ext=None):
        self.tracks, self.rows, self.boxes, self.ext, self.det, self.removed = [], [], [], ext, None, None

    def set_detections(self, rows):
        self.det = np.asarray(rows, dtype=np.int32).reshape(-1, ROW_WORDS)

    def predict(self, gate_class):
        for t in self.tracks:
            t.predict(gate_class, self._gap('gate'))

    def _row_source(self, row_idx):
        boxes = np.zeros((len(row_idx), 7), dtype=np.float32)
        cls = np.zeros(len(row_idx), dtype=np.int64)
        for k, r in enumerate(row_idx):
            if r >= 0:
                boxes[k], cls[k] = self.tracks[r].bbox[:7].astype(np.float32), self.tracks[r].cls
            else:
                boxes[k], cls[k] = self.ext[-r - 1, :7].view(np.float32), self.ext[-r - 1, ROW_CLS]
        return boxes, cls

    def affinity(self, row_idx, col_idx, metric, distinguish_class, thr):
        boxes, cls = self._row_source(np.asarray(row_idx))
        d = self.det[np.asarray(col_idx, dtype=int)]
        cost = cost_matrix(boxes, cls, d[:, :7].copy().view(np.float32), d[:, ROW_CLS], metric, distinguish_class, thr, self._gap('affinity'))
        self.costs.append(cost.copy())
        return cost

    def update(self, match, r):
        for i, di, stage in np.asarray(match).reshape(-1, 3):
            d = self.det[di]
            self.tracks[i].update(d[:7].view(np.float32), d[ROW_CLS], d[ROW_SCORE:ROW_SCORE + 1].view(np.float32)[0], d[ROW_NPTS], stage, r)

    def spawn(self, source, idx, ids, p, q, dt):
        src = self.det if source == 'det' else self.ext
        for si, tid in zip(idx, ids):
            s = src[si]
            self.tracks.append(Track(s[:7].view(np.float32), s[ROW_CLS], s[ROW_SCORE:ROW_SCORE + 1].view(np.float32)[0], s[ROW_NPTS], tid,
                                     p, q, dt, self.dtype))

    def merge(self, thr):
        boxes = np.array([t.bbox[:7] for t in self.tracks], dtype=np.float32).reshape(-1, 7)
        overlap = cref.boxes_overlap_bev(boxes, boxes) if len(boxes) else np.zeros((0, 0), np.float32)
        self.removed = merge_sweep(overlap, boxes[:, 3] * boxes[:, 4], [t.cls for t in self.tracks], [t.track_id for t in self.tracks], thr,
                                   self._gap('merge'))

    def compact(self, merged, death_age):
        gone = self.removed if merged else np.zeros(len(self.tracks), dtype=bool)
        self.tracks = [t for t, g in zip(self.tracks, gone) if not g and not (death_age != -1 and t.miss >= death_age)]
        return len(self.tracks)

    def log(self, frame):
        for t in self.tracks:
            row = np.zeros(ROW_WORDS, dtype=np.int32)
            row[:9] = t.bbox.astype(np.float32).view(np.int32)
            row[ROW_SCORE] = np.float32(t.score).view(np.int32)
            row[ROW_HIT], row[ROW_NPTS], row[ROW_ID], row[ROW_CLS], row[ROW_FRAME] = t.hit, t.num_points, t.track_id, t.cls, frame
            self.rows.append(row)
            self.boxes.append(np.array(t.bbox, dtype=self.dtype))

    def fetch_log(self):
        rows = np.array(self.rows, dtype=np.int32).reshape(-1, ROW_WORDS)
        self.history.append((rows, np.array(self.boxes, dtype=self.dtype).reshape(-1, 9)))
        return rows, rows
