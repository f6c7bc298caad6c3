"""detzero_track.models.tracking_modules.target_assign (tracking/detzero_track/models/tracking_modules/target_assign.py)."""
from detzero_amd.track_assign import assign_track_target  # noqa: F401
