"""``detzero_utils.ops.roiaware_pool3d``: ``roiaware_pool3d_utils`` on the HIP backend."""
