"""Test infrastructure: the numpy twin of object_crop.HipCropOps.  Same interface, built on the oracle's inside test
(oracle.cref.points_in_boxes_v2), so that the CPU tests drive the object-data orchestration (object_crop.crop_sequence,
object_data.WaymoObjectDataPrepare) end to end without a device."""
import numpy as np
import torch

from oracle import cref


class NumpyCropOps:
    device = torch.device('cpu')

    def __init__(self, chunk=256):
        self.chunk = chunk
        self.calls = 0

    def chunk_points(self):
        return self.chunk

    def seq_crop(self, xyz, boxes, payload, plan, want_index=False):
        """ops.seq_crop on host tensors: per frame the dense mask of the oracle, boolean-indexed per box as the reference does."""
        self.calls += 1
        xyz, boxes = xyz.numpy(), boxes.numpy()
        segs = [np.zeros(0, dtype=np.int64)] * plan.nb
        for f in range(plan.n_frames):
            p0, p1, b0, b1 = plan.pt_off[f], plan.pt_off[f + 1], plan.box_off[f], plan.box_off[f + 1]
            if b1 == b0 or p1 == p0:
                continue
            mask = cref.points_in_boxes_v2(np.ascontiguousarray(xyz[p0:p1]), np.ascontiguousarray(boxes[b0:b1])).astype(bool)
            for k in range(b1 - b0):
                segs[plan.rank[b0 + k]] = p0 + np.nonzero(mask[k])[0]
        index = np.concatenate(segs) if segs else np.zeros(0, dtype=np.int64)
        seg_off = np.zeros(plan.nb + 1, dtype=np.int32)
        np.cumsum([len(s) for s in segs], out=seg_off[1:])
        rows = payload[torch.from_numpy(index.astype(np.int64))]
        return rows, (torch.from_numpy(index.astype(np.int32)) if want_index else None), torch.from_numpy(seg_off), int(index.shape[0])
