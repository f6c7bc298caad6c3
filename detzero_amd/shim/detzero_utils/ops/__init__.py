"""``detzero_utils.ops`` - the reference's native-op packages (utils/detzero_utils/ops/) on the HIP backend: ``iou3d_nms`` and
``roiaware_pool3d``, the two the tracker imports (tracking/.../data_association/distance.py:5-6, datasets/data_processor.py)."""
