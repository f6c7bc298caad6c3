"""points_in_boxes_gpu_v2 / points_in_boxes_num_gpu of /root/reference/utils/detzero_utils/ops/roiaware_pool3d/
roiaware_pool3d_utils.py:45-58 on the HIP backend (refiner object crop, daemon/prepare_object_data.py:250-273)."""
from . import ops


def points_in_boxes_gpu_v2(points, boxes):
    """points (B,M,3), boxes (B,T,7) -> (B,T,M) int32, 1 = inside."""
    assert boxes.shape[0] == points.shape[0]
    assert boxes.shape[2] == 7 and points.shape[2] == 3
    return ops.points_in_boxes_v2(points.float().contiguous(), boxes.float().contiguous())


def points_in_boxes_num_gpu(points, boxes):
    """roiaware_pool3d_utils.points_in_boxes_num_gpu as tracking/.../datasets/data_processor.py:64-69 calls it:
    points (B,M,3), boxes (B,T,7) -> (B,T) int32 device tensor of points per box (dz_points_in_boxes_count, one call per item;
    the inside test of points_in_boxes_gpu_v2, no (T,M) mask)."""
    import torch
    from . import lib as L
    assert boxes.shape[0] == points.shape[0]
    assert boxes.shape[2] == 7 and points.shape[2] == 3
    points, boxes = points.float().contiguous(), boxes.float().contiguous()
    L.require_cuda(points, boxes)
    lib = L.load()
    counts = [torch.zeros((boxes.shape[1],), dtype=torch.int32, device=boxes.device) for _ in range(boxes.shape[0])]      # (own allocations: aligned)
    for i, c in enumerate(counts):
        rc = lib.dz_points_in_boxes_count(L.ptr(boxes[i]), L.ptr(points[i]), boxes.shape[1], points.shape[1], L.ptr(c), L.stream())
        L.check(rc, 'dz_points_in_boxes_count')
    return torch.stack(counts) if counts else torch.zeros((0, boxes.shape[1]), dtype=torch.int32, device=boxes.device)
