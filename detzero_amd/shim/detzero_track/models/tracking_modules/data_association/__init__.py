"""detzero_track.models.tracking_modules.data_association: the two functions other stages of the reference import from here
(post_process.py:7, track_manager.py:276, target_assign.py:5)."""
from detzero_amd.track_adapter import bev_overlap_gpu  # noqa: F401
from detzero_amd.track_models import GNN_assignment  # noqa: F401
