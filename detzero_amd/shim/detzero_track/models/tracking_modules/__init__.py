"""detzero_track.models.tracking_modules (tracking/detzero_track/models/tracking_modules/__init__.py)."""
from detzero_amd.track_models import PostProcessor, TrackManager  # noqa: F401

__all__ = {'TrackManager': TrackManager, 'PostProcessor': PostProcessor}
