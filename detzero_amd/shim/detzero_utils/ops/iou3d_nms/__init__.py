"""``detzero_utils.ops.iou3d_nms``: ``iou3d_nms_utils`` (the Python functions) and ``iou3d_nms_cuda`` (the pybind calling convention)."""
