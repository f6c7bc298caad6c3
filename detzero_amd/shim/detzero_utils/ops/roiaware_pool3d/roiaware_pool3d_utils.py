"""detzero_utils.ops.roiaware_pool3d.roiaware_pool3d_utils - re-export of detzero_amd.roiaware_pool3d_utils."""
from detzero_amd.roiaware_pool3d_utils import points_in_boxes_gpu_v2, points_in_boxes_num_gpu  # noqa: F401
