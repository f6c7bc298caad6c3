"""Import shims: the package names the reference's tools import, re-exporting the MI355X mirrors.

``detection/tools/test.py`` and ``eval_utils.py`` of the reference import (test.py:1-19, eval_utils.py:1-11)

    tensorboardX.SummaryWriter, detzero_utils.{common_utils, config_utils, model_utils},
    detzero_det.datasets.build_dataloader, detzero_det.models.{build_network, load_data_to_gpu}

Putting THIS directory on ``PYTHONPATH`` (``python -m detzero_amd.shim`` prints it) makes those names resolve to
``detzero_amd`` - the reference's ``test.py`` then runs unchanged on the HIP backend (``--workers 0``: frames are
voxelized on the device, which forked DataLoader workers cannot own).  ``tensorboardX`` / ``easydict`` fall-backs live in
``_fallbacks`` and are appended at the END of ``sys.path`` by ``install()``, so real installations win.

``refining/tools/test.py`` and its ``eval_utils.py`` import (test.py:11-19, eval_utils.py:8-12) the same utilities and

    detzero_refine.datasets.build_dataloader, detzero_refine.models.{build_network, load_data_to_gpu}

which resolve to ``detzero_amd.refine_dataset`` (test mode, not distributed: batches of tracks are turned into model inputs
on the device, in-process) and ``detzero_amd.refine_models`` (GRM / PRM / CRM with their recall records).

``tracking/tools/run_track.py`` imports (run_track.py:8-12) ``detzero_utils.config_utils.log_cfg_info``,
``detzero_utils.common_utils.get_log_info`` and

    detzero_track.models.{build_model, run_model}, detzero_track.datasets.build_dataloader

which resolve to ``detzero_amd.track_models`` (the tracker on a device-resident track table, one sequence after another in this
process; ``--split test``).  ``detzero_track.utils.{data_utils, transform_utils}`` (daemon/combine_output.py:14-15) and
``detzero_track.models.tracking_modules.data_association`` (``bev_overlap_gpu``, ``GNN_assignment``) resolve to
``detzero_amd.track_adapter`` / ``detzero_amd.track_models``.
"""
import os
import sys

SHIM_DIR = os.path.dirname(os.path.abspath(__file__))
FALLBACK_DIR = os.path.join(SHIM_DIR, '_fallbacks')


def install():
    """Make ``detzero_det`` / ``detzero_refine`` / ``detzero_track`` / ``detzero_utils`` (and, if missing, ``tensorboardX`` / ``easydict``) importable in this process."""
    root = os.path.dirname(os.path.dirname(SHIM_DIR))
    for p in (root, SHIM_DIR):
        if p not in sys.path:
            sys.path.insert(0, p)
    if FALLBACK_DIR not in sys.path:
        sys.path.append(FALLBACK_DIR)
    return SHIM_DIR
