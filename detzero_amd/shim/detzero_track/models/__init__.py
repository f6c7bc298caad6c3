"""detzero_track.models (tracking/detzero_track/models/__init__.py:1-63)."""
from detzero_amd.track_models import DetZeroTracker, __all__, build_model, run_model  # noqa: F401
