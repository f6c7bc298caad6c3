"""detzero_det.datasets.waymo (detection/detzero_det/datasets/waymo/): the dataset and its evaluator under the reference's paths."""
