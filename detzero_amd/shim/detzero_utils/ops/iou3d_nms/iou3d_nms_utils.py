"""detzero_utils.ops.iou3d_nms.iou3d_nms_utils - the device functions of the reference's module of that name
(utils/detzero_utils/ops/iou3d_nms/iou3d_nms_utils.py:57-187), re-exported from detzero_amd.iou3d_nms_utils, and
boxes_iou3d_paired_gpu, the diagonal of boxes_iou3d_gpu without the matrix."""
from detzero_amd.iou3d_nms_utils import (boxes_giou3d_gpu, boxes_iou3d_gpu, boxes_iou3d_paired_gpu, boxes_iou_bev,  # noqa: F401
                                         boxes_overlap_bev_gpu, boxes_union_bev_gpu, nms_gpu, nms_normal_gpu)
