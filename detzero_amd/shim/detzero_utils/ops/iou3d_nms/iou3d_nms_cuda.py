"""detzero_utils.ops.iou3d_nms.iou3d_nms_cuda - the calling convention of the reference's pybind module (iou3d_nms.h:9-13,
iou3d_nms.cpp:60-160) on the HIP kernels: the matrix functions fill a preallocated device tensor and return 1; the NMS functions
take boxes already in descending score order, write the kept indices into a CPU int64 tensor and return their number."""
import torch

from detzero_amd import iou3d_nms_utils as _utils
from detzero_amd import ops as _ops


def _fill(out, values):
    out.copy_(values.reshape(out.shape))
    return 1


def boxes_overlap_bev_gpu(boxes_a, boxes_b, ans_overlap):
    return _fill(ans_overlap, _utils.boxes_overlap_bev_gpu(boxes_a, boxes_b))


def boxes_iou_bev_gpu(boxes_a, boxes_b, ans_iou):
    return _fill(ans_iou, _utils.boxes_iou_bev(boxes_a, boxes_b))


def boxes_union_bev_gpu(boxes_a, boxes_b, ans_union):
    return _fill(ans_union, _utils.boxes_union_bev_gpu(boxes_a, boxes_b))


def _nms(fn, boxes, keep, thresh):
    n = boxes.shape[0]
    if n == 0:
        return 0
    d_keep, d_nk = fn(boxes[:, :7].float().contiguous(), None, thresh, n)
    nk = int(d_nk.item())
    keep[:nk] = d_keep[:nk].to(device=keep.device, dtype=torch.int64)
    return nk


def nms_gpu(boxes, keep, nms_overlap_thresh):
    return _nms(_ops.nms_rotated_nosync, boxes, keep, nms_overlap_thresh)


def nms_normal_gpu(boxes, keep, nms_overlap_thresh):
    return _nms(_ops.nms_normal_nosync, boxes, keep, nms_overlap_thresh)
