"""The DetZero tracker on a device-resident track table: TrackManager, PostProcessor, DetZeroTracker, build_model / run_model and
the dataset side (WaymoTrackDataset, build_dataloader).

Mirror of the reference's tracking package, same class names and config keys:
  * ``tracking/detzero_track/models/tracking_modules/track_manager.py:12-310``   TrackManager
  * ``.../data_association/data_association.py:9-155``, ``distance.py:9-41``     two_stage / one_stage / only_two_stage, GNN_assignment
  * ``.../kalman_filter/kalman_filter.py:6-146``                                 KalmanFilter (as kernels: csrc/track.hip)
  * ``.../kalman_filter/ab3dmot.py:9-149``                                       AB3DMOT (as kernels: csrc/track_ab3dmot.h)
  * ``.../post_process.py:10-138``                                               PostProcessor
  * ``tracking/detzero_track/models/{__init__,detzero_tracker}.py``              DetZeroTracker, build_model, run_model
  * ``tracking/detzero_track/datasets/{__init__,dataset,waymo_dataset}.py``      WaymoTrackDataset, build_dataloader

What is where.  The reference keeps a Python list of filter objects and walks it for every step; here the tracks of one sequence
are rows of a struct-of-arrays table on the device and the per-track / per-pair arithmetic (predict, the association cost
matrices with their masking, update, spawn, overlap_track_merge, the removal of merged and dead tracks, info()) are kernels.
The host keeps the reference's control flow: frames in order, the index bookkeeping of the association stages - including the
second stage's unmatched detections that never spawn and the num_points filter - and ``linear_sum_assignment``.  Per frame it
sees the cost matrices, sends the match lists back and reads one track count.  The ``info()`` rows of a pass are appended to a
device log that is read once when the pass ends (the reverse pass needs the forward results' ids and ``start`` flags, so a
sequence with REVERSE_TRACKING costs two reads); the forward rows that join the reverse pass, and the tracks it spawns from
them, are addressed as rows of that log on the device.

All per-frame arithmetic goes through one narrow ops object (``HipTrackOps`` is the only implementation in the product); the
tests drive the same orchestration with a numpy restatement of the seven ops.

Opt-in second way (``TrackManager.forward_batch``, ``DetZeroTracker.forward_batch``, ``run_model(..., batch=N)`` /
``DZ_TRACK_BATCH``): the whole frame loop of a pass on the device, one workgroup per sequence, the assignment included
(csrc/track_seq.hip, csrc/lsa.h), for a list of sequences at once.  The host packs all detections into one row buffer, reads the
forward logs once, regroups them per frame with the ``start`` flags exactly as ``forward`` does, uploads that and reads the reverse
logs: two launches per batch.  That host work goes through one sequence-ops object (``HipSeqTrackOps``; the tests have a stand-in
on the numpy ops).  The results are those of ``forward``.

Arithmetic is fp32, which is what the reference computes when its detections are float32; float64 ``boxes_global`` (what
transform_to_global produces) are rounded to fp32 when a frame is uploaded.  The size and heading of a track equal columns 3:7 of
its box wherever the reference reads them, so the table stores the box only.

Assign mode (every split but 'test') matches each sequence's tracks to the ground truth: track_assign.py, on the trajectory-pair
kernel (csrc/traj_pair.hip).

``FILTER.NAME: AB3DMOT`` (tools/cfgs/tk_model_cfgs/waymo_ab3dmot.yaml) is the reference's baseline filter: filterpy's
``KalmanFilter(dim_x=10, dim_z=7)`` over the state [x y z l w h theta vx vy vz], float64, with its own heading corrections, and with
it the BIRTH_AGE / DEATH_AGE output rule of track_manager.py:201-205.  On the device the filter's state lives in a float64
companion of the track table (``ops.TrackAb3dTable``, csrc/track_ab3dmot.h); the table's float32 box is the rounding of the float64
one, which is what the reference's association sees (track_manager.py:146-151).  A frame's detections then travel as the row buffer
plus a (D, 7) float64 array, the log as rows plus an (L, 9) float64 array; rows that fail the output rule are marked in the row's
word 15 on the device and dropped when the log is fetched.  The results are as the reference's: ``boxes_global`` float64 (n, 9) (a
track whose only row is its birth row keeps the reference's float32), ``num_points`` -1, ``hit`` in {0, 1}.  The config's P, Q, R and
DELTA_T are ignored as the reference's constructor ignores them, the stage flag of a match too (an update is always a full update).
Not mirrored: the reference wraps the matched detection's heading in place in the caller's array (ab3dmot.py:128); the caller's
detections are left alone here.  Refused: AB3DMOT with ``REVERSE_TRACKING.ENABLE: True`` - the filter ignores ``delta_t``, so a
reverse pass would run a forward-time motion model; no shipped config combines them.

Not covered (DetZeroHipError naming it): DISTANCE_METHOD IoU2D.  It is unusable in the reference itself: ``one_stage`` hands
``IoU2D_dis_mat`` seven columns and it asserts four (distance.py:76).
"""
import os
import pickle
from collections import defaultdict

import numpy as np
import torch

from . import ops, track_adapter
from .lib import DetZeroHipError

ROW_WORDS = ops.TRACK_ROW_WORDS
ROW_SCORE, ROW_HIT, ROW_NPTS, ROW_ID, ROW_CLS, ROW_FRAME = 9, 10, 11, 12, 13, 14      # include/detzero_hip.h: the row buffer's words
ROW_AB3D = 15                                            # AB3DMOT log rows: ops.TRACK_AB3D_ROW_DROP | ops.TRACK_AB3D_ROW_BIRTH
FILTERS = ('KalmanFilter', 'AB3DMOT')
AFF_IOU_BEV, AFF_IOU3D, AFF_GIOU3D = ops.TRACK_AFF_IOU_BEV, ops.BOXM_IOU3D, ops.BOXM_GIOU3D
# ('GIoU3D_dis_mat' is the key data_association/__init__.py:14 registers for GIoU3D_dis_mat)
METRICS = {'IoUBEV': AFF_IOU_BEV, 'IoU3D': AFF_IOU3D, 'GIoU3D': AFF_GIOU3D, 'GIoU3D_dis_mat': AFF_GIOU3D}
MAX_CLASSES = ops.TRACK_MAX_CLASSES
REVERSE_DELTA_T = -0.1                                  # track_manager.py:258


# ------------------------------------------------------------------------------------------------
# assignment (distance.py:9-41)
# ------------------------------------------------------------------------------------------------
def GNN_assignment(cost_matrix, threshold=1.):
    """Global nearest neighbour: costs >= threshold become 5000 (in place), Hungarian assignment, pairs at 5000 dropped.
    Returns (matched (K,2), unmatched rows, unmatched columns)."""
    from scipy.optimize import linear_sum_assignment
    n, m = cost_matrix.shape
    if n == 0 or m == 0:
        return np.zeros((0, 2), dtype=int), np.arange(n), np.arange(m)
    cost_matrix[cost_matrix >= threshold] = 5000.
    rows, cols = linear_sum_assignment(cost_matrix)
    ok = cost_matrix[rows, cols] < threshold
    matched = np.stack([rows[ok], cols[ok]], axis=1).astype(int) if ok.any() else np.empty((0, 2), dtype=int)
    row_free = np.setdiff1d(np.arange(n), matched[:, 0]).astype(int)
    col_free = np.setdiff1d(np.arange(m), matched[:, 1]).astype(int)
    return matched, row_free, col_free


# ------------------------------------------------------------------------------------------------
# ops: the per-frame arithmetic on the device table
# ------------------------------------------------------------------------------------------------
def det_rows(boxes, cls, score, num_points):
    """A frame's detections as a row buffer (include/detzero_hip.h): (D, 16) int32 host array."""
    d = len(cls)
    rows = np.zeros((d, ROW_WORDS), dtype=np.int32)
    if d == 0:
        return rows
    f = rows.view(np.float32)
    f[:, :7] = np.asarray(boxes, dtype=np.float32).reshape(d, -1)[:, :7]
    f[:, ROW_SCORE] = np.asarray(score, dtype=np.float32)
    rows[:, ROW_HIT] = 1
    rows[:, ROW_NPTS] = np.asarray(num_points).astype(np.int32)
    rows[:, ROW_ID] = -1
    rows[:, ROW_CLS] = cls
    return rows


class HipTrackOps:
    """The seven ops on csrc/track.hip.  One instance = one sequence at a time; ``start_pass`` empties the table.

    Interface (what a stand-in for tests implements):
      start_pass(ext=None)         empty table and log; ``ext`` = the log handle of an earlier pass whose rows can be addressed
      n                            live tracks
      set_detections(rows)         the frame's detections, a (D,16) int32 host row buffer
      predict(gate_class)
      affinity(row_idx, col_idx, metric, distinguish_class, thr) -> (R,C) float32 host cost matrix; row_idx < 0 = ext row -i-1
      update(match, r)             (M,3) [table row, detection row, stage]; r = the measurement noise
      spawn(source, idx, ids, p, q, dt)    source 'det' or 'ext'
      merge(thr)                   overlap_track_merge's verdicts, kept inside for compact
      compact(merged, death_age) -> new n
      log(frame)                   info() of every live track
      fetch_log() -> (rows (L,16) int32 host array, handle)

    ``filter='AB3DMOT'`` (csrc/track_ab3dmot.h; no ``ext``, no 'ext' spawn): the same calls, with
      set_detections(rows, boxes64)                 boxes64 = the (D,7) float64 measurements of the rows
      update(match, r) / spawn('det', idx, ids, p, q, dt)     r, p, q, dt and the stage column are ignored, as in the reference
      log(frame, frame_id, birth_age, death_age)    frame_id = the frame's key as an integer; the output rule marks word 15
      fetch_log()                                   the rows that passed the output rule only
      fetch_log_boxes() -> (L,9) float64            the boxes of the rows the last fetch_log returned
    """

    def __init__(self, device=None, init_cap=256, filter='KalmanFilter'):
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.init_cap = init_cap
        if filter not in FILTERS:
            raise DetZeroHipError('HipTrackOps: filter %s (%s)' % (filter, ', '.join(FILTERS)))
        self.ab3d = filter == 'AB3DMOT'
        self.start_pass()

    def _dev(self, a, dtype=np.int32):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.device)

    def start_pass(self, ext=None):
        self.table, self.spare = ops.TrackTable(self.init_cap, self.device), ops.TrackTable(self.init_cap, self.device)
        self.n = 0
        self.log_buf = torch.zeros((4 * self.init_cap, ROW_WORDS), dtype=torch.int32, device=self.device)
        self.log_n = 0
        self.ext = ext
        self.det = None
        self.removed = None
        if self.ab3d:
            if ext is not None:
                raise DetZeroHipError('HipTrackOps: the AB3DMOT filter has no reverse pass')
            self.ftable, self.fspare = ops.TrackAb3dTable(self.init_cap, self.device), ops.TrackAb3dTable(self.init_cap, self.device)
            self.log64 = torch.zeros((4 * self.init_cap, 9), dtype=torch.float64, device=self.device)
            self.det64 = None
            self.kept = None

    def set_detections(self, rows, boxes64=None):
        self.det = self._dev(rows) if len(rows) else torch.zeros((0, ROW_WORDS), dtype=torch.int32, device=self.device)
        if self.ab3d:
            if boxes64 is None or np.shape(boxes64) != (len(rows), 7):
                raise DetZeroHipError('track set_detections: the AB3DMOT filter takes the (D,7) float64 measurements beside the rows')
            self.det64 = self._dev(boxes64, np.float64).reshape(-1, 7)

    def predict(self, gate_class):
        if self.ab3d:
            return ops.track_ab3d_predict_nosync(self.table, self.ftable, self.n)
        ops.track_predict_nosync(self.table, self.n, gate_class)

    def affinity(self, row_idx, col_idx, metric, distinguish_class, thr):
        row_idx, col_idx = np.asarray(row_idx), np.asarray(col_idx)
        n_ext = 0 if self.ext is None else self.ext.shape[0]
        tab, fwd = row_idx[row_idx >= 0], -row_idx[row_idx < 0] - 1
        if (len(tab) and tab.max() >= self.n) or (len(fwd) and fwd.max() >= n_ext):
            raise DetZeroHipError('track affinity: row index outside the table (%d) / the forward rows (%d)' % (self.n, n_ext))
        if len(col_idx) and (col_idx.min() < 0 or col_idx.max() >= self.det.shape[0]):
            raise DetZeroHipError('track affinity: detection index outside the frame (%d)' % self.det.shape[0])
        out = ops.track_affinity_nosync(self.table, self.n, self.ext, self._dev(row_idx), self.det, self._dev(col_idx), metric,
                                        distinguish_class, thr)
        return out.cpu().numpy()

    def update(self, match, r):
        if len(match) and self.ab3d:
            if np.min(match[:, 1]) < 0 or np.max(match[:, 1]) >= self.det.shape[0] or np.min(match[:, 0]) < 0 or np.max(match[:, 0]) >= self.n:
                raise DetZeroHipError('track update: a match outside the table (%d) / the frame (%d)' % (self.n, self.det.shape[0]))
            ops.track_ab3d_update_nosync(self.table, self.ftable, self.n, self.det, self.det64, self._dev(match))
        elif len(match):
            ops.track_update_nosync(self.table, self.n, self.det, self._dev(match), r)

    def spawn(self, source, idx, ids, p, q, dt):
        m = len(idx)
        if m == 0:
            return
        if self.ab3d and source != 'det':
            raise DetZeroHipError('track spawn: the AB3DMOT filter spawns from detections only')
        src = self.det if source == 'det' else self.ext
        if src is None or np.min(idx) < 0 or np.max(idx) >= src.shape[0]:
            raise DetZeroHipError('track spawn: source row outside its buffer')
        grown = self.table.grown(self.n, self.n + m)
        if grown is not self.table:
            self.table, self.spare = grown, ops.TrackTable(grown.cap, self.device)
            if self.ab3d:
                self.ftable, self.fspare = self.ftable.grown(self.n, self.n + m), ops.TrackAb3dTable(grown.cap, self.device)
        if self.ab3d:
            ops.track_ab3d_spawn_nosync(self.table, self.ftable, self.n, src, self.det64, self._dev(idx), self._dev(ids))
        else:
            ops.track_spawn_nosync(self.table, self.n, src, self._dev(idx), self._dev(ids), p, q, dt)
        self.n += m

    def merge(self, thr):
        self.removed = ops.track_merge_nosync(self.table, self.n, thr)

    def compact(self, merged, death_age):
        if self.n == 0:
            return 0
        if self.ab3d:
            d_count = ops.track_ab3d_compact_nosync(self.table, self.ftable, self.n, self.removed if merged else None, death_age, self.spare,
                                                    self.fspare)
            self.ftable, self.fspare = self.fspare, self.ftable
        else:
            d_count = ops.track_compact_nosync(self.table, self.n, self.removed if merged else None, death_age, self.spare)
        self.table, self.spare = self.spare, self.table
        self.n = int(d_count.item())
        return self.n

    def log(self, frame, frame_id=None, birth_age=None, death_age=None):
        if self.log_n + self.n > self.log_buf.shape[0]:
            rows = self.log_buf.shape[0]
            while rows < self.log_n + self.n:
                rows *= 2
            new = torch.zeros((rows, ROW_WORDS), dtype=torch.int32, device=self.device)
            new[:self.log_n].copy_(self.log_buf[:self.log_n])
            self.log_buf = new
            if self.ab3d:
                new64 = torch.zeros((rows, 9), dtype=torch.float64, device=self.device)
                new64[:self.log_n].copy_(self.log64[:self.log_n])
                self.log64 = new64
        if self.ab3d:
            if frame_id is None or birth_age is None or death_age is None:
                raise DetZeroHipError('track log: the AB3DMOT filter takes the frame id and the BIRTH_AGE / DEATH_AGE of its output rule')
            ops.track_ab3d_log_nosync(self.table, self.ftable, self.n, frame, frame_id, birth_age, death_age, self.log_buf, self.log64,
                                      self.log_n)
        else:
            ops.track_log_nosync(self.table, self.n, frame, self.log_buf, self.log_n)
        self.log_n += self.n

    def fetch_log(self):
        handle = self.log_buf[:self.log_n]
        rows = handle.cpu().numpy()
        if self.ab3d:       # the rows that fail the output rule are dropped here: no extra read while the pass runs
            self.kept = (rows[:, ROW_AB3D] & ops.TRACK_AB3D_ROW_DROP) == 0
            return rows[self.kept], None
        return rows, handle

    def fetch_log_boxes(self):
        return self.log64[:self.log_n].cpu().numpy()[self.kept]


# ------------------------------------------------------------------------------------------------
# sequence ops: a pass of a batch of sequences in one launch
# ------------------------------------------------------------------------------------------------
class SeqPack:
    """The detections of a batch of sequences as ONE row buffer with per-frame offsets (what dz_track_seq_pass reads).

      frame_lists[s]   the sequence's frame ids in time order
      rows             (N,16) int32: every frame's row buffer (det_rows), sequences and frames back to back
      flags            (N,) int32: bit 0 = passes the first stage's score / point thresholds, bit 1 = enough points
                       (TrackManager._stage_masks on the frame's own arrays; 0 with the one_stage association)
      frame_row        (frames + 1,) first row of every frame, frames numbered through the batch
      seq_frame        (S + 1,) first frame of every sequence
      max_det[s]       the largest frame of the sequence
      dtypes[s]        the result dtypes of score / num_points (TrackManager._note_dtypes)
    With the AB3DMOT filter also
      boxes64          (N,7) float64: the measurements of the rows
      frame_ids        (frames,) int32: every frame's key as an integer (the output rule reads it, not the ordinal)
    """

    def __init__(self, mgr, data_dicts):
        self.data_dicts = data_dicts
        self.frame_lists = [sorted(list(dd.keys()), key=int) for dd in data_dicts]
        rows, flags, frame_row, seq_frame = [], [], [0], [0]
        boxes64, frame_ids = [], []
        self.max_det, self.dtypes = [], []
        for dd, frame_list in zip(data_dicts, self.frame_lists):
            dtypes = {'score': np.float32, 'num_points': np.int64}
            biggest = 0
            for frm_id in frame_list:
                det = dd[frm_id]
                cls, r = mgr._frame_rows(det)
                if mgr.stage == 'one_stage':
                    f = np.zeros(len(cls), dtype=np.int32)
                else:
                    first, enough = mgr._stage_masks(det, cls)
                    f = np.asarray(first).astype(np.int32).reshape(-1) | (np.asarray(enough).astype(np.int32).reshape(-1) << 1)
                rows.append(r)
                flags.append(f)
                if mgr.ab3dmot:
                    boxes64.append(mgr._frame_boxes64(det))
                    frame_ids.append(int(frm_id))
                frame_row.append(frame_row[-1] + len(cls))
                biggest = max(biggest, len(cls))
                mgr._note_dtypes(dtypes, det)
            seq_frame.append(len(frame_row) - 1)
            self.max_det.append(biggest)
            self.dtypes.append(dtypes)
        self.rows = np.concatenate(rows, axis=0) if rows else np.zeros((0, ROW_WORDS), dtype=np.int32)
        self.flags = np.concatenate(flags) if flags else np.zeros(0, dtype=np.int32)
        self.frame_row = np.array(frame_row, dtype=np.int64)
        self.seq_frame = np.array(seq_frame, dtype=np.int64)
        self.boxes64 = np.concatenate(boxes64, axis=0) if boxes64 else np.zeros((0, 7), dtype=np.float64)
        self.frame_ids = np.array(frame_ids, dtype=np.int32)

    def frames_of(self, s):
        return range(int(self.seq_frame[s]), int(self.seq_frame[s + 1]))

    def frame_rows(self, g):
        """(rows, flags) of frame g (numbered through the batch)."""
        return self.rows[self.frame_row[g]:self.frame_row[g + 1]], self.flags[self.frame_row[g]:self.frame_row[g + 1]]

    def subset(self, seqs):
        """The buffers of the listed sequences only, renumbered: (rows, flags, frame_row, seq_frame) as int32 arrays."""
        rows, flags, frame_row, seq_frame = [], [], [0], [0]
        for s in seqs:
            for g in self.frames_of(s):
                r, f = self.frame_rows(g)
                rows.append(r)
                flags.append(f)
                frame_row.append(frame_row[-1] + len(f))
            seq_frame.append(len(frame_row) - 1)
        return (np.concatenate(rows, axis=0) if rows else np.zeros((0, ROW_WORDS), dtype=np.int32),
                np.concatenate(flags) if flags else np.zeros(0, dtype=np.int32), np.array(frame_row, dtype=np.int32),
                np.array(seq_frame, dtype=np.int32))

    def subset64(self, seqs):
        """AB3DMOT: (boxes64, frame_ids) of the listed sequences, in the order of ``subset``."""
        boxes, ids = [np.zeros((0, 7), dtype=np.float64)], [np.zeros(0, dtype=np.int32)]
        for s in seqs:
            f0, f1 = int(self.seq_frame[s]), int(self.seq_frame[s + 1])
            boxes.append(self.boxes64[self.frame_row[f0]:self.frame_row[f1]])
            ids.append(self.frame_ids[f0:f1])
        return np.concatenate(boxes, axis=0), np.concatenate(ids)


class HipSeqTrackOps:
    """forward_batch's two passes on csrc/track_seq.hip.

    Interface (what a stand-in for tests implements):
      forward_pass(mgr, pack, seqs)               -> {s: (L,16) int32 host log rows, or None}
      reverse_pass(mgr, pack, seqs, fwd, groups)  -> {s: (L,16) int32 host log rows, or None}
                                                     fwd[s] = the forward rows, groups[s] = TrackManager._regroup(fwd[s])
    None = the sequence does not fit the batched path (the caller tracks it with TrackManager.forward).

    Capacities (tracks and log rows per sequence) start from the detections' counts, or from ``track_cap`` / ``log_cap``; a sequence
    that runs out of one sets its overflow word and is rerun, alone with the others that overflowed, with that capacity doubled
    (tracks: up to ops.TRACK_SEQ_MAX_TRACKS, which is tried before a sequence is given up; ``reruns`` counts the extra launches).
    Per pass and launch: one upload of the packed buffers, one read of the counts and overflow words, one read of the log rows.

    With the AB3DMOT filter (the manager's choice; forward pass only) the rows that fail the output rule are dropped from what
    forward_pass returns, and ``boxes64[s]`` holds the (L,9) float64 boxes of the rows returned for sequence s."""

    def __init__(self, device=None, track_cap=None, log_cap=None):
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.track_cap, self.log_cap = track_cap, log_cap
        self.reruns = 0
        self.boxes64 = {}

    def _dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)

    @staticmethod
    def _params(mgr):
        two = mgr.stage == 'two_stage'
        return ops.track_seq_params(mgr.metric, mgr.distinguish_class, mgr.gate_class, len(mgr.class_names), two, mgr.merge_enable,
                                    mgr.death_age, mgr.init_track_id, mgr.dist_thr, mgr.second_dist_thr if two else None,
                                    mgr.merge_thr if mgr.merge_enable else None, mgr.p, mgr.q, mgr.r, mgr.delta_t,
                                    ops.TRACK_FILTER_AB3DMOT if mgr.ab3dmot else ops.TRACK_FILTER_KALMAN, mgr.birth_age)

    def _run(self, mgr, pack, seqs, track_cap, log_cap, reverse_of=None):
        """Launch until no sequence overflows: {s: rows or None}.  reverse_of(sub) -> (the reverse pass's device lists, extra rows)."""
        out, todo = {}, list(seqs)
        params = self._params(mgr)
        first = True
        while todo:
            if not first:
                self.reruns += 1
            first = False
            rows, flags, frame_row, seq_frame = pack.subset(todo)
            det_cap = max([pack.max_det[s] for s in todo] + [1])
            reverse, extra = reverse_of(todo) if reverse_of is not None else (None, 0)
            log64 = None
            if mgr.ab3dmot:
                boxes64, frame_ids = pack.subset64(todo)
                ab3d = (torch.from_numpy(np.ascontiguousarray(boxes64)).to(self.device),
                        self._dev(frame_ids if len(frame_ids) else np.zeros(1, dtype=np.int32)))
                log, count, overflow, log64 = ops.track_seq_pass_nosync(params, self._dev(rows).reshape(-1, ROW_WORDS), self._dev(flags),
                                                                        self._dev(frame_row), self._dev(seq_frame), track_cap, track_cap + extra,
                                                                        det_cap, log_cap, reverse, ab3d)
            else:
                log, count, overflow = ops.track_seq_pass_nosync(params, self._dev(rows).reshape(-1, ROW_WORDS), self._dev(flags), self._dev(frame_row),
                                                                 self._dev(seq_frame), track_cap, track_cap + extra, det_cap, log_cap, reverse)
            state = torch.stack([count, overflow]).cpu().numpy()
            keep = torch.from_numpy((np.arange(log_cap)[None, :] < state[0][:, None]).reshape(-1)).to(self.device)
            got = log.reshape(-1, ROW_WORDS)[keep].cpu().numpy()
            got64 = log64.reshape(-1, 9)[keep].cpu().numpy() if log64 is not None else None
            at, again, grow_tracks, grow_log = 0, [], False, False
            for k, s in enumerate(todo):
                n, ovf = int(state[0, k]), int(state[1, k])
                if ovf == 0 and got64 is not None:
                    passed = (got[at:at + n, ROW_AB3D] & ops.TRACK_AB3D_ROW_DROP) == 0
                    out[s], self.boxes64[s] = got[at:at + n][passed], got64[at:at + n][passed]
                elif ovf == 0:
                    out[s] = got[at:at + n]
                elif ovf & (ops.TRACK_SEQ_OVF_LSA | ops.TRACK_SEQ_OVF_DESC):
                    out[s] = None
                else:
                    again.append(s)
                    grow_tracks, grow_log = grow_tracks or bool(ovf & ops.TRACK_SEQ_OVF_TRACKS), grow_log or bool(ovf & ops.TRACK_SEQ_OVF_LOG)
                at += n
            give_up = False
            if grow_tracks:                 # doubled, but tried at the limit itself before the sequences are given up
                give_up = track_cap >= ops.TRACK_SEQ_MAX_TRACKS
                track_cap = min(2 * track_cap, ops.TRACK_SEQ_MAX_TRACKS)
            if grow_log:
                log_cap *= 2
                give_up = give_up or log_cap * ROW_WORDS >= 2 ** 31
            if give_up:
                for s in again:
                    out[s] = None
                again = []
            todo = again
        return out

    def forward_pass(self, mgr, pack, seqs):
        self.boxes64 = {}
        if not seqs:
            return {}
        most = max([pack.max_det[s] for s in seqs] + [1])
        total = max([int(pack.frame_row[pack.seq_frame[s + 1]] - pack.frame_row[pack.seq_frame[s]]) for s in seqs] + [1])
        track_cap = self.track_cap if self.track_cap is not None else min(max(64, 2 * most), ops.TRACK_SEQ_MAX_TRACKS)
        log_cap = self.log_cap if self.log_cap is not None else max(256, 2 * total)
        return self._run(mgr, pack, seqs, track_cap, log_cap)

    def reverse_pass(self, mgr, pack, seqs, fwd, groups):
        if not seqs:
            return {}
        n_tracks = max([int(groups[s][1].sum()) for s in seqs] + [1])
        if n_tracks > ops.TRACK_SEQ_MAX_TRACKS:
            big = [s for s in seqs if int(groups[s][1].sum()) > ops.TRACK_SEQ_MAX_TRACKS]
            out = self.reverse_pass(mgr, pack, [s for s in seqs if s not in big], fwd, groups)
            out.update({s: None for s in big})
            return out
        track_cap = self.track_cap if self.track_cap is not None else n_tracks
        log_cap = self.log_cap if self.log_cap is not None else max([len(fwd[s]) for s in seqs] + [256])

        def reverse_of(todo):
            ext_cap = max([len(fwd[s]) for s in todo] + [1])
            ext = np.zeros((len(todo), ext_cap, ROW_WORDS), dtype=np.int32)
            going, start, going_at, start_at, most_going = [], [], [0], [0], 0
            for k, s in enumerate(todo):
                ext[k, :len(fwd[s])] = fwd[s]
                _, is_start, per_frame = groups[s]
                for at in per_frame:
                    going.append(at[~is_start[at]])
                    start.append(at[is_start[at]])
                    going_at.append(going_at[-1] + len(going[-1]))
                    start_at.append(start_at[-1] + len(start[-1]))
                    most_going = max(most_going, len(going[-1]))
            cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
            dev = (self._dev(ext), self._dev([len(fwd[s]) for s in todo]), self._dev(going_at), self._dev(cat(going)), self._dev(start_at),
                   self._dev(cat(start)))
            return dev, most_going

        return self._run(mgr, pack, seqs, track_cap, log_cap, reverse_of)


# ------------------------------------------------------------------------------------------------
# TrackManager
# ------------------------------------------------------------------------------------------------
def _lower(cfg):
    return {k.lower(): v for k, v in cfg.items()}


class TrackManager:
    """``forward({sample_idx: frame})`` -> ``{track_id: {boxes_global, name, score, sample_idx, hit, num_points, obj_ids, pose}}``
    (track_manager.py:85-143).  ``ops_factory`` builds the ops object of a sequence (default: HipTrackOps)."""

    def __init__(self, model_cfg, init_track_id=0, ops_factory=None, seq_ops_factory=None):
        self.model_cfg = model_cfg
        self.init_track_id = init_track_id
        self.ops_factory = ops_factory if ops_factory is not None else HipTrackOps
        self.ops = None
        self.seq_ops_factory = seq_ops_factory      # forward_batch's sequence-ops object (default: HipSeqTrackOps)
        self.seq_ops = None
        self.batched = 0            # sequences forward_batch tracked on the batched path ...
        self.fallbacks = 0          # ... and those it handed to forward (beyond a limit, or an assignment stopped with a status)

        flt = _lower(model_cfg.FILTER)
        if flt['name'] not in FILTERS:
            raise DetZeroHipError('FILTER.NAME %s is not provided by the HIP tracker (%s)' % (flt['name'], ', '.join(FILTERS)))
        self.filter_name = flt['name']
        self.ab3dmot = self.filter_name == 'AB3DMOT'
        # (AB3DMOT's own dimensions are 10 / 7 whatever the config says; the shipped waymo_ab3dmot.yaml carries 5 / 3 as the other one)
        if flt.get('x_dim', 5) != 5 or flt.get('z_dim', 3) != 3:
            raise DetZeroHipError('%s with X_DIM %s / Z_DIM %s (5 / 3 only)' % (self.filter_name, flt.get('x_dim'), flt.get('z_dim')))
        if self.ab3dmot and ops_factory is None:
            self.ops_factory = lambda: HipTrackOps(filter='AB3DMOT')
        self.p, self.q = tuple(flt.get('p', [1, 1])), tuple(flt.get('q', [1, 1]))
        self.r, self.delta_t = float(flt.get('r', 1)), float(flt.get('delta_t', 0.1))

        age = _lower(model_cfg.TRACK_AGE)
        self.birth_age, self.death_age = age.get('birth_age', 1), age.get('death_age', -1)

        da = _lower(model_cfg.DATA_ASSOCIATION)
        self.class_names = list(da['class_name'])
        if len(self.class_names) > MAX_CLASSES:
            raise DetZeroHipError('%d classes (at most %d)' % (len(self.class_names), MAX_CLASSES))
        self.class_code = {n: i for i, n in enumerate(self.class_names)}
        self.gate_class = self.class_code.get('Vehicle', -1)
        self.distinguish_class = bool(da['distinguish_class'])
        if da['distance_method'] not in METRICS:
            raise DetZeroHipError('DISTANCE_METHOD %s is not provided by the HIP tracker (%s)' % (da['distance_method'], ', '.join(METRICS)))
        self.metric = METRICS[da['distance_method']]
        if da['assignment_method'] != 'GNN':
            raise DetZeroHipError('ASSIGNMENT_METHOD %s (GNN only)' % da['assignment_method'])
        stage = da['stage']
        self.stage = stage['NAME']
        if self.stage not in ('one_stage', 'two_stage'):
            raise DetZeroHipError('association STAGE.NAME %s' % self.stage)
        self.dist_thr = [float(v) for v in stage['FIRST_STAGE']['DIST_THRESHOLD']][:len(self.class_names)]
        if self.stage == 'two_stage':
            second = stage['SECOND_STAGE']
            self.point_thr = np.array(second['POINT_THRESHOLD'])
            self.score_thr = np.array(second['SCORE_THRESHOLD'])
            self.second_dist_thr = [float(v) for v in second['DIST_THRESHOLD']][:len(self.class_names)]

        mg = _lower(model_cfg.TRACK_MERGE)
        self.merge_enable = bool(mg['enable'])
        if self.merge_enable:
            by_name = dict(zip(mg['class_name'], mg['class_threshold']))
            missing = [n for n in self.class_names if n not in by_name]
            if missing:
                raise DetZeroHipError('TRACK_MERGE has no threshold for %s' % ', '.join(missing))
            self.merge_thr = [float(by_name[n]) for n in self.class_names]
        self.reverse_enable = bool(_lower(model_cfg.REVERSE_TRACKING)['enable'])
        if self.ab3dmot and self.reverse_enable:
            raise DetZeroHipError('FILTER.NAME AB3DMOT with REVERSE_TRACKING.ENABLE: the filter ignores delta_t, so a reverse pass would '
                                  'run a forward-time motion model; the HIP tracker provides AB3DMOT on the forward pass only')

    # ---- a frame's detections ------------------------------------------------------------------
    def _codes(self, names):
        try:
            return np.array([self.class_code[n] for n in names], dtype=np.int32)
        except KeyError as e:
            raise DetZeroHipError('detection class %s is not in DATA_ASSOCIATION.CLASS_NAME %s' % (e, self.class_names))

    def _frame_rows(self, det_data):
        """-> (class codes, the frame's row buffer); the num_points default of track_manager.py:166-167 is written into det_data
        as the reference does."""
        one = self.stage == 'one_stage'
        if not one and 'num_points' not in det_data:
            det_data['num_points'] = np.zeros_like(det_data['score'])
        cls = self._codes(det_data['name'])
        npts = np.zeros(len(cls), dtype=np.int32) if one else det_data['num_points']
        return cls, det_rows(det_data['boxes_global'], cls, det_data['score'], npts)

    @staticmethod
    def _frame_boxes64(det_data):
        """AB3DMOT: the frame's measurements, (D,7) float64 (a copy: the caller's array is never written)."""
        d = len(det_data['name'])
        if d == 0:
            return np.zeros((0, 7), dtype=np.float64)
        return np.array(np.asarray(det_data['boxes_global'], dtype=np.float64).reshape(d, -1)[:, :7], dtype=np.float64)

    def _upload(self, ops, det_data):
        cls, rows = self._frame_rows(det_data)
        if self.ab3dmot:
            ops.set_detections(rows, self._frame_boxes64(det_data))
        else:
            ops.set_detections(rows)
        return cls

    # ---- association (data_association.py) -------------------------------------------------------
    def _one_stage(self, ops, row_idx, col_idx, thr):
        if len(row_idx) == 0 or len(col_idx) == 0:
            cost = np.ones((len(row_idx), len(col_idx)), dtype=np.float32)
        else:
            cost = ops.affinity(row_idx, col_idx, self.metric, self.distinguish_class, thr)
        return GNN_assignment(cost)

    def _stage_masks(self, det_data, cls):
        score_thr, point_thr = self.score_thr[cls], self.point_thr[cls]
        enough_points = np.greater_equal(det_data['num_points'], point_thr)
        return np.greater_equal(det_data['score'], score_thr) & enough_points, enough_points

    def _two_stage(self, ops, det_data, cls, row_idx):
        first_mask, enough_points = self._stage_masks(det_data, cls)
        if len(row_idx) == 0:
            det_unmatch = np.flatnonzero(enough_points)
            return np.zeros((0, 2), dtype=int), np.arange(0), det_unmatch, np.zeros(0, dtype=int)
        first_det = np.flatnonzero(first_mask)
        first, trk_free, det_free = self._one_stage(ops, row_idx, first_det, self.dist_thr)
        first[:, 1] = first_det[first[:, 1]]
        first_det_free = first_det[det_free]
        second_det = np.flatnonzero(~first_mask)
        second_trk = np.sort(np.asarray(trk_free, dtype=int))       # flatnonzero of the mask the reference builds
        second, trk_free, _ = self._one_stage(ops, row_idx[second_trk], second_det, self.second_dist_thr)
        second[:, 0] = second_trk[second[:, 0]]
        second[:, 1] = second_det[second[:, 1]]
        matched = np.concatenate((first, second), axis=0)
        stage = np.zeros(matched.shape[0], dtype=int)
        stage[first.shape[0]:] = 1
        # the second stage's unmatched detections never spawn (data_association.py:121-123)
        det_unmatch = first_det_free[enough_points[first_det_free]]
        return matched, second_trk[trk_free], det_unmatch, stage

    def _only_two_stage(self, ops, det_data, cls, row_idx):
        first_mask, enough_points = self._stage_masks(det_data, cls)
        if len(row_idx) == 0:
            return np.zeros((0, 2), dtype=int), np.arange(0), np.flatnonzero(enough_points)
        second_det = np.flatnonzero(~first_mask)
        second, trk_free, det_free = self._one_stage(ops, row_idx, second_det, self.second_dist_thr)
        second[:, 1] = second_det[second[:, 1]]
        return second, trk_free, second_det[det_free]

    # ---- the two per-frame modules ---------------------------------------------------------------
    def _merge_and_log(self, ops, ordinal, frm_id=None):
        if self.merge_enable and ops.n:
            ops.merge(self.merge_thr)
            ops.compact(True, -1)
        if self.ab3dmot:        # the BIRTH_AGE / DEATH_AGE output rule of track_manager.py:202-205 reads int(frame id), not the ordinal
            ops.log(ordinal, int(frm_id), self.birth_age, self.death_age)
        else:
            ops.log(ordinal)    # every live track

    def online_track_module(self, ops, ordinal, det_data, track_id_count, frm_id=None):
        """``frm_id``: the frame's key in the sequence dict (AB3DMOT's output rule needs it; the ordinal otherwise)."""
        if frm_id is None:
            frm_id = ordinal
        n = ops.n
        ops.predict(self.gate_class)
        cls = self._upload(ops, det_data)
        rows = np.arange(n)
        if self.stage == 'one_stage':
            matched, _, det_unmatch = self._one_stage(ops, rows, np.arange(len(cls)), self.dist_thr)
            stage = np.zeros(matched.shape[0], dtype=int)
        else:
            matched, _, det_unmatch, stage = self._two_stage(ops, det_data, cls, rows)
        ops.update(np.concatenate((matched, stage[:, None]), axis=1), self.r)
        ids = np.arange(track_id_count, track_id_count + len(det_unmatch))
        ops.spawn('det', det_unmatch, ids, self.p, self.q, self.delta_t)
        self._merge_and_log(ops, ordinal, frm_id)
        if self.death_age != -1:
            ops.compact(False, self.death_age)
        return track_id_count + len(det_unmatch)

    def reverse_tracking_module(self, ops, ordinal, det_data, fwd_rows, fwd_start, fwd_ids):
        """fwd_rows: rows of the forward log at this frame in track order; the ones that do not start here join the association as
        extra rows, the ones that start here become reverse tracks once the frame is done (track_manager.py:218-260)."""
        n = ops.n
        ops.predict(self.gate_class)
        cls = self._upload(ops, det_data)
        if self.stage != 'two_stage':
            raise DetZeroHipError('REVERSE_TRACKING needs the two_stage association (only_two_stage reads its SECOND_STAGE thresholds)')
        going = fwd_rows[~fwd_start]
        rows = np.concatenate((np.arange(n), -going - 1)).astype(int)
        matched, _, _ = self._only_two_stage(ops, det_data, cls, rows)
        matched = matched[matched[:, 0] < n]
        ops.update(np.concatenate((matched, np.ones((matched.shape[0], 1), dtype=int)), axis=1), self.r)
        self._merge_and_log(ops, ordinal)
        ops.spawn('ext', fwd_rows[fwd_start], fwd_ids[fwd_start], self.p, self.q, REVERSE_DELTA_T)

    # ---- log rows -> the reference's object-level structure -------------------------------------------
    def _tracks_of(self, rows, frame_list, data_dict, dtypes, boxes64=None):
        """{track id: dict} in the order in which the ids first appear in the log.  ``boxes64`` (AB3DMOT): the (L,9) float64 boxes of
        the rows - the results' boxes_global; num_points is then the reference's Python -1 (int64)."""
        out = {}
        if len(rows) == 0:
            return out
        ids = rows[:, ROW_ID]
        _, first = np.unique(ids, return_index=True)
        names = np.array(self.class_names)
        for at in np.sort(first):
            sel = np.flatnonzero(ids == ids[at])
            r = rows[sel]
            frames = [frame_list[o] for o in r[:, ROW_FRAME]]
            if boxes64 is None:
                boxes = r[:, :9].copy().view(np.float32)
            elif np.all(r[:, ROW_AB3D] & ops.TRACK_AB3D_ROW_BIRTH):       # np.array of the constructor's float32 bbox alone
                boxes = boxes64[sel].astype(np.float32)
            else:
                boxes = boxes64[sel].copy()
            out[int(ids[at])] = {
                'boxes_global': boxes,
                'name': np.array([names[c] for c in r[:, ROW_CLS]]),
                'score': r[:, ROW_SCORE].copy().view(np.float32).astype(dtypes['score']),
                'sample_idx': np.array(frames),
                'hit': r[:, ROW_HIT].astype(np.int64),
                'num_points': r[:, ROW_NPTS].astype(dtypes['num_points'] if boxes64 is None else np.int64),
                'obj_ids': r[:, ROW_ID].astype(np.int64),
                'pose': np.array([data_dict[f]['pose'] for f in frames]),
            }
        return out

    def _note_dtypes(self, dtypes, det_data):
        """The score / num_points dtypes of the results are those of the last frame that holds a detection."""
        if len(det_data['score']):
            dtypes['score'] = np.asarray(det_data['score']).dtype
            if self.stage != 'one_stage':
                dtypes['num_points'] = np.asarray(det_data['num_points']).dtype

    @staticmethod
    def _regroup(rows, n_frames):
        """Forward results per frame in track order, with the flag of each track's first frame (track_manager.py:117-128):
        -> (ids (L,), is_start (L,) bool, [rows of frame 0 in track order, rows of frame 1, ...])."""
        ids = rows[:, ROW_ID] if len(rows) else np.zeros(0, dtype=np.int32)
        _, first = np.unique(ids, return_index=True)
        is_start = np.zeros(len(rows), dtype=bool)
        is_start[first] = True
        rank = {int(ids[at]): k for k, at in enumerate(np.sort(first))}
        order = np.array([rank[int(i)] for i in ids], dtype=int)
        per_frame = []
        for ordinal in range(n_frames):
            at = np.flatnonzero(rows[:, ROW_FRAME] == ordinal) if len(rows) else np.zeros(0, dtype=int)
            per_frame.append(at[np.argsort(order[at], kind='stable')])
        return ids, is_start, per_frame

    @staticmethod
    def _prepend(tk_result, back_tracks):
        for tk_id, early in back_tracks.items():
            # the reverse pass inserts every row at the front (track_manager.py:134-141): the last one processed comes first
            for key, val in tk_result[tk_id].items():
                tk_result[tk_id][key] = np.concatenate((early[key][::-1].astype(val.dtype), val), axis=0)
        return tk_result

    def forward(self, data_dict):
        frame_list = sorted(list(data_dict.keys()), key=int)
        ops = self.ops if self.ops is not None else self.ops_factory()
        self.ops = ops
        ops.start_pass()
        track_id_count = self.init_track_id
        dtypes = {'score': np.float32, 'num_points': np.int64}
        for ordinal, frm_id in enumerate(frame_list):
            track_id_count = self.online_track_module(ops, ordinal, data_dict[frm_id], track_id_count, frm_id)
            self._note_dtypes(dtypes, data_dict[frm_id])
        rows, handle = ops.fetch_log()
        tk_result = self._tracks_of(rows, frame_list, data_dict, dtypes, ops.fetch_log_boxes() if self.ab3dmot else None)
        if not self.reverse_enable:
            return tk_result

        ids, is_start, per_frame = self._regroup(rows, len(frame_list))
        ops.start_pass(ext=handle)
        for ordinal in range(len(frame_list) - 1, -1, -1):
            at = per_frame[ordinal]
            self.reverse_tracking_module(ops, ordinal, data_dict[frame_list[ordinal]], at, is_start[at], ids[at].astype(np.int64))
        back, _ = ops.fetch_log()
        return self._prepend(tk_result, self._tracks_of(back, frame_list, data_dict, dtypes))

    # ---- a batch of sequences, a pass in one launch ------------------------------------------------------
    def forward_batch(self, data_dicts):
        """``forward`` for a list of sequences -> the list of their results, the same as ``forward`` gives one by one.
        The frame loop of a pass runs on the device for all sequences at once (csrc/track_seq.hip) through the sequence-ops object
        (``seq_ops_factory``, default HipSeqTrackOps).  A sequence the batched path cannot hold - a frame with more than
        ops.TRACK_SEQ_MAX_DET detections, more than ops.TRACK_SEQ_MAX_TRACKS tracks, an assignment that stops with a status - is
        tracked by ``forward`` inside the same call; ``batched`` / ``fallbacks`` count the sequences that went either way."""
        data_dicts = list(data_dicts)
        if self.seq_ops is None:
            self.seq_ops = self.seq_ops_factory() if self.seq_ops_factory is not None else HipSeqTrackOps()
        pack = SeqPack(self, data_dicts)
        if self.reverse_enable and self.stage != 'two_stage' and any(len(fl) for fl in pack.frame_lists):
            raise DetZeroHipError('REVERSE_TRACKING needs the two_stage association (only_two_stage reads its SECOND_STAGE thresholds)')
        seqs = [s for s in range(len(data_dicts)) if pack.max_det[s] <= ops.TRACK_SEQ_MAX_DET]
        fwd = self.seq_ops.forward_pass(self, pack, seqs)
        seqs = [s for s in seqs if fwd[s] is not None]
        results = {s: self._tracks_of(fwd[s], pack.frame_lists[s], data_dicts[s], pack.dtypes[s],
                                      self.seq_ops.boxes64[s] if self.ab3dmot else None) for s in seqs}
        if self.reverse_enable:
            groups = {s: self._regroup(fwd[s], len(pack.frame_lists[s])) for s in seqs}
            back = self.seq_ops.reverse_pass(self, pack, seqs, fwd, groups)
            for s in seqs:
                if back[s] is None:
                    del results[s]
                else:
                    self._prepend(results[s], self._tracks_of(back[s], pack.frame_lists[s], data_dicts[s], pack.dtypes[s]))
        self.batched += len(results)
        self.fallbacks += len(data_dicts) - len(results)
        return [results[s] if s in results else self.forward(dd) for s, dd in enumerate(data_dicts)]


# ------------------------------------------------------------------------------------------------
# PostProcessor (post_process.py), host numpy as in the reference
# ------------------------------------------------------------------------------------------------
def _trailing_misses(hit):
    """Indices from the end back to (not including) the last row with hit >= 1."""
    idx = []
    for i in range(len(hit) - 1, -1, -1):
        if hit[i] >= 1:
            break
        idx.append(i)
    return idx


class PostProcessor:
    """``processor_configs.CONFIG_LIST``: entries with ``.NAME`` in {empty_track_delete, velocity_optimize, motion_classify,
    static_drift_eliminate, box_size_update}, applied in order to the whole ``{track_id: track}`` dict, in place.  ``overlap_fn``
    = the all-pairs BEV overlap of motion_classify (default: the HIP kernel behind track_adapter.bev_overlap_gpu)."""

    def __init__(self, processor_configs, overlap_fn=None):
        self.overlap_fn = overlap_fn if overlap_fn is not None else track_adapter.bev_overlap_gpu
        self.post_process_queue = []
        for cfg in processor_configs.CONFIG_LIST:
            if not hasattr(self, cfg.NAME):
                raise DetZeroHipError('unknown post-processor %s' % cfg.NAME)
            self.post_process_queue.append((getattr(self, cfg.NAME), cfg))

    def forward(self, data_dict):
        for fn, cfg in self.post_process_queue:
            data_dict = fn(data_dict, cfg)
        return data_dict

    def empty_track_delete(self, data_dict, config):
        """Tracks with fewer than LEAST_AGE hit frames go; the others lose their leading and trailing missed frames (END_REMOVE)."""
        for tk_id in list(data_dict.keys()):
            tk = data_dict[tk_id]
            hit = tk['hit']
            hits = int(np.sum(hit > 0))
            if hits < config.LEAST_AGE:
                data_dict.pop(tk_id)
                continue
            if hits != len(hit) and config.END_REMOVE:
                lead = []
                for i in range(len(hit)):
                    if hit[i] >= 1:
                        break
                    lead.append(i)
                drop = lead + _trailing_misses(hit)
                for key in tk.keys():
                    tk[key] = np.delete(tk[key], drop, axis=0)
        return data_dict

    def velocity_optimize(self, data_dict, config):
        """The first HEADER_LENGTH velocities (all but the last of a shorter track) from the displacement to the next frame at 10 Hz."""
        for tk in data_dict.values():
            boxes = tk['boxes_global']
            n = len(boxes)
            if n < 2:
                continue
            for i in range(config.HEADER_LENGTH if n > config.HEADER_LENGTH else n - 1):
                boxes[i, 7:9] = (boxes[i + 1, :2] - boxes[i, :2]) * 10.
        return data_dict

    def motion_classify(self, data_dict, config):
        """'dynamic' when two of the track's updated boxes overlap by 1e-4 m^2 or less, else 'static'."""
        for tk in data_dict.values():
            at = np.flatnonzero(tk['hit'] == 1)
            state = 'static'
            if len(at) >= 2:
                boxes = np.ascontiguousarray(tk['boxes_global'][at, :7], dtype=np.float32)
                if np.any(self.overlap_fn(boxes, boxes) <= 1e-4):
                    state = 'dynamic'
            tk['state'] = state
        return data_dict

    def static_drift_eliminate(self, data_dict, config):
        """A static Vehicle's trailing missed frames take the box of its best-scored updated frame."""
        for tk in data_dict.values():
            if tk['state'] == 'static' and tk['name'][0] == 'Vehicle':
                at = np.flatnonzero(tk['hit'] == 1)
                best = at[np.argsort(tk['score'][at])[-1]]
                for i in _trailing_misses(tk['hit']):
                    tk['boxes_global'][i] = tk['boxes_global'][best].copy()
        return data_dict

    def box_size_update(self, data_dict, config):
        for tk in data_dict.values():
            scores, boxes = tk['score'], tk['boxes_global']
            if config.METHOD == 'max_score_box':
                at = np.where(scores == np.max(scores))[0]
                size = np.zeros(3, dtype=np.float32)
                for i in at:
                    size += boxes[i, 3:6]
                boxes[:, 3:6] = size / len(at)
            elif config.METHOD == 'score_weigthed_box':
                size = np.zeros(3, dtype=np.float32)
                for i in range(len(scores)):
                    size += scores[i] * boxes[i, 3:6]
                boxes[:, 3:6] = size / np.sum(scores)
            elif config.METHOD == 'largest_box':
                boxes[:, 3:6] = boxes[np.argsort(boxes[:, 3] * boxes[:, 4] * boxes[:, 5])[-1], 3:6].copy()
        return data_dict


TRACKING_MODULES = {'TrackManager': TrackManager, 'PostProcessor': PostProcessor}


# ------------------------------------------------------------------------------------------------
# model
# ------------------------------------------------------------------------------------------------
class DetZeroTracker:
    """TRACKING then POST_PROCESS over one sequence (detzero_tracker.py:4-46)."""

    def __init__(self, model_cfg, logger=None):
        self.model_cfg = model_cfg
        self.logger = logger
        self.module_list = []
        if model_cfg.get('TRACKING', None) is not None:
            self.module_list.append(TRACKING_MODULES[model_cfg.TRACKING.NAME](model_cfg=model_cfg.TRACKING))
        if model_cfg.get('POST_PROCESS', None) is not None:
            self.module_list.append(TRACKING_MODULES[model_cfg.POST_PROCESS.NAME](processor_configs=model_cfg.POST_PROCESS))

    def forward(self, data_dict):
        for module in self.module_list:
            data_dict = module.forward(data_dict=data_dict)
        return data_dict

    def forward_batch(self, data_dicts):
        """``forward`` for a list of sequences: TRACKING for all of them at once (TrackManager.forward_batch), then POST_PROCESS per
        sequence on the host as ``forward`` does."""
        outputs = list(data_dicts)
        for module in self.module_list:
            if hasattr(module, 'forward_batch'):
                outputs = module.forward_batch(outputs)
            else:
                outputs = [module.forward(data_dict=d) for d in outputs]
        return outputs


__all__ = {'DetZeroTracker': DetZeroTracker}


def build_model(model_cfg, logger=None):
    return __all__[model_cfg.NAME](model_cfg=model_cfg, logger=logger)


def _banner(text, total=100):
    return text.center(max(total, len(text)), '-')


def run_model(model, dataloader, dataset, workers, cfgs=None, logger=None, assign_ops=None, batch=None):
    """Tracks every sequence of every batch in this process and writes tracking-<split>-<time>.pkl and drop-<split>-<time>.pkl.
    ``workers`` is accepted for the reference's signature; no process pool ever opens the GPU - concurrency comes from ``batch``:
    None reads the environment variable DZ_TRACK_BATCH; unset or 0 tracks the sequences one after another (``model.forward``),
    N > 0 sends the sequences of each loader batch through ``model.forward_batch`` in groups of N, a pass of a group in one launch.  In assign
    mode (every split but 'test') each sequence's tracks are matched to the ground truth (track_assign.assign_track_target, with
    ``cfgs.REFINING.IOU_THRESHOLDS``) and the tracking pickle holds the ``{'label', 'unlabel'}`` dicts instead (models/__init__.py:26-56).
    ``assign_ops`` = the ops object of the assignment (default: track_assign.HipTrajOps)."""
    if dataset.assign_mode:
        from . import track_assign
        refining = cfgs.get('REFINING', None) if cfgs is not None else None
        iou_thresholds = refining.get('IOU_THRESHOLDS', None) if refining is not None else None
        if iou_thresholds is None:
            raise DetZeroHipError('assign mode (split %r): assign_track_target needs cfgs.REFINING.IOU_THRESHOLDS; pass the tracker '
                                  'config, or run with --split test' % getattr(dataset, 'split', None))
    if logger is not None:
        logger.info(_banner('Running Tracking Module!'))
    if batch is None:
        batch = int(os.environ.get('DZ_TRACK_BATCH', '0') or 0)
    batch = int(batch)
    if batch < 0:
        raise DetZeroHipError('run_model: batch %d (0 = one sequence after another, N > 0 = groups of N)' % batch)
    track_data, drop_data = {}, {}
    for seq_names, data_dicts in dataloader:
        seqs = data_dicts['detection']
        if batch > 0:
            outputs = []
            for i in range(0, len(seqs), batch):
                outputs += model.forward_batch(seqs[i:i + batch])
        else:
            outputs = [model.forward(seq) for seq in seqs]
        if dataset.assign_mode:
            outputs = [track_assign.assign_track_target(item, iou_thresholds=iou_thresholds, ops=assign_ops)
                       for item in zip(data_dicts['detection'], outputs, data_dicts['gt'])]
        track_data.update(dict(zip(seq_names, outputs)))
        drop_data.update(dict(zip(seq_names, data_dicts['det_drop'])))
    with open(dataset.get_track_path(), 'wb') as f:
        pickle.dump(track_data, f)
    with open(dataset.get_drop_path(), 'wb') as f:
        pickle.dump(drop_data, f)
    if logger is not None:
        logger.info(_banner('Tracking module running finished!'))


# ------------------------------------------------------------------------------------------------
# dataset
# ------------------------------------------------------------------------------------------------
class WaymoTrackDataset:
    """Detection results (a list of frame records or ``{sequence: {sample_idx: frame}}``) -> one item per sequence:
    ``(sequence_name, {'detection': processed frames, 'det_drop': removed boxes})`` (waymo_dataset.py:13-109)."""

    def __init__(self, dataset_cfg, data_path, log_time, split, root_path=None, logger=None, overlap_fn=None, count_fn=None):
        self.dataset_cfg = dataset_cfg
        self.det_path = data_path
        self.root_path = root_path if root_path is not None else dataset_cfg.DATA_PATH
        self.logger = logger
        self.split = split
        self.logtime = log_time
        self.data_processor = track_adapter.DataProcessor(dataset_cfg.DATA_PROCESSOR,
                                                          os.path.join(self.root_path, dataset_cfg.PROCESSED_DATA_TAG), overlap_fn, count_fn)
        if logger:
            logger.info(_banner('Initialize %s' % dataset_cfg.DATASET))
        track_path = os.path.join(self.root_path, 'tracking')
        os.makedirs(track_path, exist_ok=True)
        self.track_module_path = defaultdict(dict)
        self.track_module_path['tracking'] = os.path.join(track_path, '-'.join(['tracking', split, log_time]))
        self.track_module_path['det_drop'] = os.path.join(track_path, '-'.join(['drop', split, log_time]))
        self.track_module_path['detection'] = data_path
        self.gt_path = os.path.join(self.root_path, 'waymo_infos_%s.pkl' % split)
        self.gt_infos = None
        with open(data_path, 'rb') as f:
            raw = pickle.load(f)
        if isinstance(raw, list):
            raw = track_adapter.sequence_list_to_dict(raw)
        elif not isinstance(raw, dict):
            raise TypeError('The format of detection results must be List or Dict.')
        self.seq_name_list = list(raw.keys())
        self.seq_det_infos = [raw[s] for s in self.seq_name_list]

    @property
    def assign_mode(self):
        return self.split != 'test'

    def __len__(self):
        return len(self.seq_name_list)

    def _load_gt_infos(self):
        """waymo_infos_<split>.pkl, read at the first item of an assign-mode dataset rather than in the constructor (the
        reference's init_infos reads it there): building a dataset for its paths or its mode needs no ground truth."""
        with open(self.gt_path, 'rb') as f:
            gt_infos = track_adapter.sequence_list_to_dict(pickle.load(f))
        if len(gt_infos.keys()) != len(self.seq_name_list):
            raise ValueError('Ground-truth infomation loading falied.')
        self.gt_infos = [gt_infos[s] for s in self.seq_name_list]

    def __getitem__(self, idx):
        det, drop = self.data_processor.forward(data_dict=self.seq_det_infos[idx])
        data_dict = {'detection': det, 'det_drop': drop}
        if self.assign_mode:
            if self.gt_infos is None:
                self._load_gt_infos()
            data_dict['gt'] = self.gt_infos[idx]
        return self.seq_name_list[idx], data_dict

    @staticmethod
    def collate_batch(batch_list):
        names, dicts = [], defaultdict(list)
        for name, sample in batch_list:
            names.append(name)
            for k, v in sample.items():
                dicts[k].append(v)
        return names, dicts

    def get_track_path(self):
        return self.track_module_path['tracking'] + '.pkl'

    def get_drop_path(self):
        return self.track_module_path['det_drop'] + '.pkl'


class SequenceLoader:
    """In-process iterable over batches of sequences: no worker processes, no start method set."""

    def __init__(self, dataset, batch_size):
        self.dataset, self.batch_size = dataset, max(int(batch_size), 1)

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for i in range(0, len(self.dataset), self.batch_size):
            yield self.dataset.collate_batch([self.dataset[j] for j in range(i, min(i + self.batch_size, len(self.dataset)))])


DATASETS = {'WaymoTrackDataset': WaymoTrackDataset}


def build_dataloader(dataset_cfg, log_time, data_path, batch_size, workers, split, logger, root_path=None):
    dataset = DATASETS[dataset_cfg.DATASET](dataset_cfg=dataset_cfg, data_path=data_path, split=split, root_path=root_path,
                                            log_time=log_time, logger=logger)
    return dataset, SequenceLoader(dataset, batch_size)
