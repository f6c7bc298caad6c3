"""detzero_refine.models (refining/detzero_refine/models/__init__.py:1-48)."""
from detzero_amd.refine_models import (ConfidenceRefineModel, GeometryRefineModel, PositionRefineModel, RefineTemplate,  # noqa: F401
                                       __all__, build_network, load_data_to_gpu, model_fn_decorator)
