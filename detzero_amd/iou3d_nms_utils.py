"""Function names of /root/reference/utils/detzero_utils/ops/iou3d_nms/iou3d_nms_utils.py on the HIP
backend (seam 3 of SURVEY.md §8b).  Device tensors in, device tensors out, no D2H mask copy."""
import torch

from . import ops
from .lib import DetZeroHipError


def boxes_overlap_bev_gpu(boxes_a, boxes_b):
    """iou3d_nms_cuda.boxes_overlap_bev_gpu: (N,7),(M,7) -> (N,M) overlap areas."""
    return ops.boxes_pairwise(boxes_a[:, :7].float().contiguous(), boxes_b[:, :7].float().contiguous(), iou=False)


def boxes_iou_bev(boxes_a, boxes_b):
    """iou3d_nms_utils.py:60-72."""
    assert boxes_a.shape[1] == boxes_b.shape[1] == 7
    return ops.boxes_pairwise(boxes_a.float().contiguous(), boxes_b.float().contiguous(), iou=True)


def boxes_iou3d_gpu(boxes_a, boxes_b):
    """iou3d_nms_utils.py:74-107: BEV overlap x height overlap / union volume, in one kernel (the reference's operation
    sequence in fp32, bit-identical to its torch composition around boxes_overlap_bev_gpu)."""
    assert boxes_a.shape[1] == boxes_b.shape[1] == 7
    return ops.boxes_pairwise_metric(boxes_a.float().contiguous(), boxes_b.float().contiguous(), ops.BOXM_IOU3D)


def boxes_iou3d_paired_gpu(boxes_a, boxes_b):
    """(N,7),(N,7) -> (N,): boxes_iou3d_gpu(boxes_a, boxes_b).diag() bit for bit, one thread per pair instead of the N x N matrix
    (what the refining models' recall records take from it, geometry_refine_model.py:114-122, position_refine_model.py:106-114)."""
    assert boxes_a.shape[1] == boxes_b.shape[1] == 7 and boxes_a.shape[0] == boxes_b.shape[0]
    return ops.boxes_paired_metric(boxes_a.float().contiguous(), boxes_b.float().contiguous(), ops.BOXM_IOU3D)


def boxes_giou3d_gpu(boxes_a, boxes_b, exact_height=False):
    """iou3d_nms_utils.py:110-151 as written: its enclosing height is min(tops) - min(bottoms) (:139), and the tracker's
    numbers depend on that.  exact_height=True takes max(tops) - min(bottoms), the textbook GIoU."""
    assert boxes_a.shape[1] == boxes_b.shape[1] == 7
    return ops.boxes_pairwise_metric(boxes_a.float().contiguous(), boxes_b.float().contiguous(),
                                     ops.BOXM_GIOU3D_EXACT if exact_height else ops.BOXM_GIOU3D)


def boxes_union_bev_gpu(boxes_a, boxes_b):
    """iou3d_nms_cuda.boxes_union_bev_gpu: (N,7),(M,7) -> (N,M) areas of the convex hull of the two footprints."""
    return ops.boxes_pairwise_metric(boxes_a[:, :7].float().contiguous(), boxes_b[:, :7].float().contiguous(), ops.BOXM_UNION_BEV)


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
    """iou3d_nms_utils.py:154-170.  Returns (kept indices into `boxes`, None)."""
    assert boxes.shape[1] == 7
    order = scores.sort(0, descending=True)[1]
    if pre_maxsize is not None:
        order = order[:pre_maxsize]
    b = boxes[order].float().contiguous()
    if b.shape[0] == 0:
        return order, None
    keep, d_nk = ops.nms_rotated_nosync(b, None, thresh, b.shape[0])
    nk = int(d_nk.item())
    return order[keep[:nk].long()].contiguous(), None


NMS_MAX_BOXES = 4096        # n_cap limit of dz_nms_rotated / dz_nms_normal


def nms_normal_gpu(boxes, scores, thresh, **kwargs):
    """iou3d_nms_utils.py:173-187: axis-aligned NMS, the heading ignored; no pre_maxsize, as in the reference.
    Returns (kept indices into `boxes`, None)."""
    assert boxes.shape[1] == 7
    if boxes.shape[0] > NMS_MAX_BOXES:
        raise DetZeroHipError('nms_normal_gpu: %d boxes > %d (the limit of the device NMS)' % (boxes.shape[0], NMS_MAX_BOXES))
    order = scores.sort(0, descending=True)[1]
    b = boxes[order].float().contiguous()
    if b.shape[0] == 0:
        return order, None
    keep, d_nk = ops.nms_normal_nosync(b, None, thresh, b.shape[0])
    nk = int(d_nk.item())
    return order[keep[:nk].long()].contiguous(), None
