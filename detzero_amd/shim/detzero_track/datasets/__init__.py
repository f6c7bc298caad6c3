"""detzero_track.datasets (tracking/detzero_track/datasets/__init__.py:1-29): an in-process loader, no worker processes."""
from detzero_amd.track_models import DATASETS as __all__  # noqa: F401
from detzero_amd.track_models import SequenceLoader, WaymoTrackDataset, build_dataloader  # noqa: F401
