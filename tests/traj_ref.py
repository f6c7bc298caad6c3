"""Test helper: numpy restatement of the trajectory-pair ops (set_sides, table, rows) of detzero_amd.track_assign.HipTrajOps.

A literal port of the three loops of the reference the kernel replaces, on per-frame IoU matrices as get_iou_mat_dict builds them
(track_calculation.py:9-52), with the IoUs from the oracle's C restatement (oracle/cref.py) and tests/track_ref.iou3d:
  * assign_track_target's frame x ground-truth box x track loop (target_assign.py:55-75)       -> n_hit, sum_hit
  * get_trajectory_similarity's walk over the frames a pair shares (track_calculation.py:95-116) -> sum_all, n_same (and n_hit)
  * the matched pairs' per-frame read of iou_mat_dict (target_assign.py:104-111)                -> rows
Sums are float32, one add per frame in frame order, as the reference's ``+=`` on a float32 matrix / an np.float32 scalar.
"""
import numpy as np

from oracle import cref
from tests import track_ref

AFF_IOU_BEV, AFF_IOU3D = 16, 1


def frame_matrix(a_box, a_cls, b_box, b_cls, metric, distinguish_class, iou_fn=None):
    """One frame's class-masked IoU matrix, float32."""
    if metric not in (AFF_IOU_BEV, AFF_IOU3D):
        raise ValueError('metric %r' % (metric,))
    if iou_fn is not None:
        mat = iou_fn(a_box, b_box)
    else:
        mat = cref.boxes_iou_bev(a_box[:, :7], b_box[:, :7]) if metric == AFF_IOU_BEV else track_ref.iou3d(a_box, b_box)
    mat = np.array(mat, dtype=np.float32)
    if distinguish_class:
        for r, c in enumerate(a_cls):
            mat[r, b_cls != c] = 0.
    return mat


class NumpyTrajOps:
    """``iou_fn(metric)`` -> a function (a boxes, b boxes) -> matrix replaces the CPU IoUs (tools/bench_track_assign.py passes the
    device's per-frame box ops: the composition a user of the shim had before the kernel).  ``tables`` keeps what ``table`` returned."""

    def __init__(self, iou_fn=None):
        self.iou_fn = iou_fn
        self.sides = None
        self.tables = []

    def set_sides(self, a_box, a_cls, a_slot, b_box, b_cls, b_slot):
        self.sides = tuple(np.asarray(x) for x in (a_box, a_cls, a_slot, b_box, b_cls, b_slot))

    def _frames(self, metric, distinguish_class):
        """per frame: (a trajectories present, b trajectories present, matrix over them)"""
        a_box, a_cls, a_slot, b_box, b_cls, b_slot = self.sides
        fn = self.iou_fn(metric) if self.iou_fn is not None else None
        for f in range(a_slot.shape[0]):
            ia, ib = np.flatnonzero(a_slot[f] >= 0), np.flatnonzero(b_slot[f] >= 0)
            if len(ia) == 0 or len(ib) == 0:
                yield ia, ib, np.zeros((len(ia), len(ib)), np.float32), a_cls[a_slot[f, ia]]
                continue
            ra, rb = a_slot[f, ia], b_slot[f, ib]
            yield ia, ib, frame_matrix(a_box[ra], a_cls[ra], b_box[rb], b_cls[rb], metric, distinguish_class, fn), a_cls[ra]

    def table(self, metric, distinguish_class, thr):
        thr = np.asarray(thr, dtype=np.float32)
        assert np.all(thr > 0)
        n_a, n_b = self.sides[2].shape[1], self.sides[5].shape[1]
        sum_all, sum_hit = np.zeros((n_a, n_b), np.float32), np.zeros((n_a, n_b), np.float32)
        n_hit, n_same = np.zeros((n_a, n_b), np.int32), np.zeros((n_a, n_b), np.int32)
        for ia, ib, mat, cls in self._frames(metric, distinguish_class):
            for r, i in enumerate(ia):
                for c, j in enumerate(ib):
                    v = mat[r, c]
                    n_same[i, j] += 1
                    sum_all[i, j] += v
                    if v >= thr[cls[r]]:
                        n_hit[i, j] += 1
                        sum_hit[i, j] += v
        self.tables.append((sum_all, sum_hit, n_hit, n_same))
        return sum_all, sum_hit, n_hit, n_same

    def rows(self, metric, distinguish_class, pairs):
        pairs = np.asarray(pairs).reshape(-1, 2)
        out = np.zeros((len(pairs), self.sides[2].shape[0]), np.float32)
        for f, (ia, ib, mat, _) in enumerate(self._frames(metric, distinguish_class)):
            for p, (i, j) in enumerate(pairs):
                r, c = np.flatnonzero(ia == i), np.flatnonzero(ib == j)
                if len(r) and len(c):
                    out[p, f] = mat[r[0], c[0]]
        return out
