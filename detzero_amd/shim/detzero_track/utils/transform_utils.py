"""detzero_track.utils.transform_utils (tracking/detzero_track/utils/transform_utils.py:4-59)."""
from detzero_amd.track_adapter import get_inverse_transform_mat, transform_boxes3d, yaw_filter  # noqa: F401
