"""detzero_track.utils.track_recall (tracking/detzero_track/utils/track_recall.py): what tracking/tools/eval_track.py imports."""
from detzero_amd.track_recall import TrackRecall  # noqa: F401
