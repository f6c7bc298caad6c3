"""detzero_refine.datasets (refining/detzero_refine/datasets/__init__.py:1-79), test mode: ``build_dataloader`` and the dataset
classes of detzero_amd.refine_dataset."""
from detzero_amd.refine_dataset import (DatasetTemplate, RefineLoader, WaymoConfidenceDataset, WaymoGeometryDataset,  # noqa: F401
                                        WaymoPositionDataset, __all__, build_dataloader)
