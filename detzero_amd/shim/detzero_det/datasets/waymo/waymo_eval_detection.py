"""detzero_det.datasets.waymo.waymo_eval_detection (detection/detzero_det/datasets/waymo/waymo_eval_detection.py): the
evaluator class under the reference's import path, with the matching on the device (detzero_amd/waymo_eval.py)."""
from detzero_amd.waymo_eval import WaymoDetectionMetricsEstimator, limit_period, main  # noqa: F401

if __name__ == '__main__':
    main()
