"""Per-object point crop of the refining data path on the GPU (first half).

Mirror of the crop step of ``daemon/prepare_object_data.py:241-273,310``: for every frame of a tracked sequence the
boxes (global frame) are enlarged, the frame's points are moved to the global frame (NLZ-flagged returns dropped,
intensity through tanh) and every object receives the points inside its enlarged box.  The reference computes a dense
(T, M) mask with ``points_in_boxes_gpu_v2``, copies it to the host and boolean-indexes once per object; here
``dz_crop_points_in_boxes`` compacts on the device (bitmap mask -> bitmap scan -> one gather) and only the kept rows and
T+1 offsets come back.  The host-side preparation of the points (float64 pose product exactly as numpy does it in the
reference) is unchanged on purpose: membership is decided on the same float32 coordinates as in the reference.

``crop_sequence`` is the same crop for a whole sequence at once: the frames' points back to back, every frame
with its own boxes, on the two-pass segmented kernels of csrc/seq_crop.hip - no (T, M) bitmap, no guessed capacity, one sync per frame
group - with the kept rows in (frame, box) order or, under a rank, in any segment order (object-major for object_features.PackedTracks).
"""
import numpy as np
import torch

from . import ops
from .lib import DetZeroHipError


def prepare_frame_points(pts, pose):
    """(N,6) [x,y,z,intensity,elongation,NLZ] lidar-frame points -> (N',4) float64 [x,y,z (global), tanh(intensity)]
    (prepare_object_data.py:262-267)."""
    pts = pts[pts[:, 5] == -1]
    homo = np.concatenate([pts[:, :3], np.ones((pts.shape[0], 1))], axis=-1) @ pose.T
    return np.concatenate([homo[:, :3], np.tanh(pts[:, 3:4])], axis=1)


def enlarge_boxes(boxes_global, enlarge_scale, crop_on_bev):
    """prepare_object_data.py:252-256"""
    b = boxes_global.copy()
    b[:, 3:6] *= enlarge_scale
    if crop_on_bev:
        b[:, 5] = 100
    return b


def crop_objects(pts_global, boxes_enlarged, device=None, cap=None):
    """pts_global (M,4) float64 (prepare_frame_points), boxes (T,7) -> list of T arrays: ``pts_global[mask[i]]`` of the
    reference, computed with one device compaction.  ``cap`` bounds the total number of kept rows (default 4 M: a point
    may fall into several overlapping boxes); a ValueError is raised when it is exceeded."""
    t, m = boxes_enlarged.shape[0], pts_global.shape[0]
    if t == 0:
        return []
    if m == 0:
        return [pts_global[:0] for _ in range(t)]
    dev = device if device is not None else torch.device('cuda', torch.cuda.current_device())
    cap = int(cap) if cap is not None else 4 * m
    xyz = torch.from_numpy(np.ascontiguousarray(pts_global[:, :3])).float().to(dev).contiguous()     # .float() as in the reference call
    payload = torch.from_numpy(np.ascontiguousarray(pts_global)).to(dev)
    boxes = torch.from_numpy(np.ascontiguousarray(boxes_enlarged[:, :7])).float().to(dev).contiguous()
    out, _, offsets, d_total = ops.crop_points_in_boxes_nosync(xyz, boxes, payload, cap)
    total = int(d_total.item())
    if total > cap:
        raise ValueError('crop_objects: %d kept points exceed the capacity %d' % (total, cap))
    rows = out[:total].cpu().numpy()
    off = offsets.cpu().numpy()
    return [rows[off[i]:off[i + 1]] for i in range(t)]


def crop_frame_objects(pts, pose, boxes_global, enlarge_scale=1.1, crop_on_bev=False, device=None):
    """One frame of prepare_object_data.py:250-273,310: raw (N,6) points + pose + (T,7) global boxes -> list of per-object points."""
    return crop_objects(prepare_frame_points(pts, pose), enlarge_boxes(np.asarray(boxes_global, dtype=np.float64), enlarge_scale, crop_on_bev),
                        device)


class SequenceCrop:
    """Device result of crop_sequence: ``rows`` (total,4) float64, the kept points segment after segment; ``offsets`` (B+1,) int32, the
    row range of every segment; ``index`` (total,) int64 or None, the source row of every kept point in the concatenation of the frames'
    points.  Segment s holds the points of the box whose rank is s (order='frame': box s of the frame-major list)."""

    def __init__(self, rows, offsets, index, n_groups):
        self.rows, self.offsets, self.index, self.n_groups = rows, offsets, index, n_groups
        self.total, self.num_boxes = int(rows.shape[0]), int(offsets.shape[0]) - 1

    def counts(self):
        """Points per segment, on the host (B,) int64."""
        return np.diff(self.offsets.cpu().numpy().astype(np.int64))

    def to_lists(self):
        """Host form: list of B (n_s,4) float64 arrays, ``pts[mask[i]]`` of the reference for the box of every segment."""
        rows, off = self.rows.cpu().numpy(), self.offsets.cpu().numpy()
        return [rows[off[i]:off[i + 1]] for i in range(self.num_boxes)]

    def index_lists(self):
        idx, off = self.index.cpu().numpy(), self.offsets.cpu().numpy()
        return [idx[off[i]:off[i + 1]] for i in range(self.num_boxes)]


class HipCropOps:
    """The per-frame point work of the object-data stage on the device: the only implementation in the product (the tests drive the
    same orchestration through a numpy one).  ``seq_crop`` is ops.seq_crop; ``chunk_points`` the chunk size its plan is laid out for."""

    def __init__(self, device=None):
        self.device = device if device is not None else torch.device('cuda', torch.cuda.current_device())

    def chunk_points(self):
        return ops.seq_crop_chunk_points()

    def seq_crop(self, xyz, boxes, payload, plan, want_index=False):
        return ops.seq_crop(xyz, boxes, payload, plan, want_index=want_index)


# device bytes one frame adds to a group: float32 xyz + float64 payload per point, counts + int64 scan + prefix per table entry
_POINT_BYTES, _ENTRY_BYTES = 12 + 32, 16


def frame_groups(n_pts, n_box, budget_bytes, chunk):
    """Consecutive frame ranges [(lo, hi), ...] whose staged points and count table stay within budget_bytes (a frame that exceeds
    it alone is a group of its own)."""
    groups, lo, used = [], 0, 0
    for f, (m, t) in enumerate(zip(n_pts, n_box)):
        need = int(m) * _POINT_BYTES + int(t) * (-(-int(m) // chunk)) * _ENTRY_BYTES
        if f > lo and used + need > budget_bytes:
            groups.append((lo, f))
            lo, used = f, 0
        used += need
    if len(n_pts) > lo:
        groups.append((lo, len(n_pts)))
    return groups


def crop_sequence(frames, enlarge_scale=1.1, crop_on_bev=False, order='frame', device=None, budget_bytes=256 << 20, want_index=False,
                  crop_ops=None):
    """The crop of a whole sequence: frames = [(pts_global (M_f,4) float64 from prepare_frame_points, boxes_global (T_f,7)), ...] ->
    SequenceCrop.  ``order`` is 'frame' (segments in (frame, box) order, the order of the reference's pickles) or a rank array: a
    permutation of 0..B-1 that names the segment of every box of the frame-major list (an object-major rank gives the order of
    object_features.PackedTracks).  The sequence is cut into frame groups within ``budget_bytes`` of device memory; every group is one
    upload, two launches and one sync (ops.seq_crop), and the result does not depend on the cut.  ``crop_ops`` (default HipCropOps on
    ``device``) does the device work."""
    crop_ops = crop_ops if crop_ops is not None else HipCropOps(device)
    dev = crop_ops.device
    n_pts = np.asarray([p.shape[0] for p, _ in frames], dtype=np.int64)
    # enlarged in the boxes' own dtype, as the reference does (float32 tracker boxes are scaled in float32)
    boxes = [enlarge_boxes(np.asarray(b)[:, :7], enlarge_scale, crop_on_bev) if np.size(b) else np.zeros((0, 7)) for _, b in frames]
    n_box = np.asarray([b.shape[0] for b in boxes], dtype=np.int64)
    nb = int(n_box.sum())
    p_start = np.concatenate([[0], np.cumsum(n_pts)])
    b_start = np.concatenate([[0], np.cumsum(n_box)])
    if isinstance(order, str):
        if order != 'frame':
            raise ValueError("crop_sequence: order is 'frame' or a rank array, not %r" % (order,))
        rank = None
    else:
        rank = ops.seq_crop_rank(order, nb)
    chunk = crop_ops.chunk_points()
    groups = frame_groups(n_pts, n_box, int(budget_bytes), chunk)
    parts = []                                 # per group: rows, seg_off of its local segments, index, the global segment of each local one
    for lo, hi in groups:
        b_lo, b_hi = int(b_start[lo]), int(b_start[hi])
        if rank is None:
            local_rank, seg_global = None, np.arange(b_lo, b_hi)
        else:
            seg_global = np.sort(rank[b_lo:b_hi])                 # the group's segments keep their global order
            local_rank = np.searchsorted(seg_global, rank[b_lo:b_hi])
        pts = np.concatenate([frames[f][0] for f in range(lo, hi)], axis=0) if hi > lo else np.zeros((0, 4))
        bx = np.concatenate(boxes[lo:hi], axis=0) if hi > lo else np.zeros((0, 7))
        plan = ops.seq_crop_plan(p_start[lo:hi + 1] - p_start[lo], b_start[lo:hi + 1] - b_lo, local_rank, pts.shape[0], b_hi - b_lo, chunk=chunk)
        xyz = torch.from_numpy(np.ascontiguousarray(pts[:, :3])).float().to(dev).contiguous()      # .float() as in the reference call
        payload = torch.from_numpy(np.ascontiguousarray(pts[:, :4])).to(dev)
        d_boxes = torch.from_numpy(np.ascontiguousarray(bx)).float().to(dev).contiguous()
        rows, index, seg_off, _ = crop_ops.seq_crop(xyz, d_boxes, payload, plan, want_index=want_index)
        if index is not None:
            index = index.long() + int(p_start[lo])
        parts.append((rows, seg_off, index, seg_global))
    if not parts:
        return SequenceCrop(torch.zeros((0, 4), dtype=torch.float64, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev),
                            torch.zeros((0,), dtype=torch.int64, device=dev) if want_index else None, 0)
    if len(parts) == 1:
        rows, seg_off, index, _ = parts[0]
        return SequenceCrop(rows, seg_off, index, 1)
    # several groups: segment lengths scattered to their global places, one prefix, one gather of the groups' rows
    lens = torch.zeros((nb,), dtype=torch.int64, device=dev)
    src0 = torch.zeros((nb,), dtype=torch.int64, device=dev)      # first row of every global segment in the groups' concatenation
    base = 0
    for rows, seg_off, _, seg_global in parts:
        g = torch.from_numpy(np.ascontiguousarray(seg_global, dtype=np.int64)).to(dev)
        so = seg_off.long()
        lens[g] = so[1:] - so[:-1]
        src0[g] = so[:-1] + base
        base += int(rows.shape[0])
    if base >= 2 ** 31:
        raise DetZeroHipError('crop_sequence: %d kept rows reach 2^31' % base)
    offsets = torch.zeros((nb + 1,), dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
    all_rows = torch.cat([p[0] for p in parts], dim=0)
    if rank is None:                                              # groups already follow each other in segment order
        rows, index = all_rows, (torch.cat([p[2] for p in parts]) if want_index else None)
    else:
        src = torch.repeat_interleave(src0 - offsets[:-1], lens, output_size=base) + torch.arange(base, device=dev)
        rows = all_rows[src]
        index = torch.cat([p[2] for p in parts])[src] if want_index else None
    return SequenceCrop(rows, offsets.to(torch.int32), index, len(parts))
