"""detzero_track.utils.track_calculation (tracking/detzero_track/utils/track_calculation.py)."""
from detzero_amd.track_assign import get_gt_id_data, get_iou_mat_dict  # noqa: F401
from detzero_amd.track_recall import get_trajectory_similarity  # noqa: F401
