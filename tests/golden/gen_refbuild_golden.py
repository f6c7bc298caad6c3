"""Golden outputs of the REFERENCE's own host routines as oracle/refbuild.py compiles them (iou3d_cpu.cpp: rotated BEV IoU and the
NMS sweep over it; roiaware_pool3d.cpp: points_in_boxes_cpu), on the seeded inputs of
tests/test_oracle_golden.py::test_rotated_iou_against_live_reference_build / test_points_in_boxes_against_live_reference_build.

    python tests/golden/gen_refbuild_golden.py      (build container only; needs the reference sources oracle/refbuild.py builds)

The point-in-box flags are stored as the (box, point) indices of the set flags.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def iou_inputs():
    from detzero_amd.synth import synth_boxes
    a, b = synth_boxes(21, 120), synth_boxes(22, 90)
    b[:25] = a[:25]
    return a, b


PIB_CASES = ((3, 60000, 80), (5, 5000, 7))


def pib_inputs(seed, n, t):
    from detzero_amd.synth import synth_boxes, synth_waymo_frame
    pts = synth_waymo_frame(seed, n)[:, :3]
    boxes = synth_boxes(seed + 2, t, 60.0)
    boxes[:, 2] = np.random.default_rng(seed).uniform(-0.5, 1.5, t)
    return pts, boxes


def main():
    from oracle import refbuild
    a, b = iou_inputs()
    out = {'iou': refbuild.boxes_iou_bev_reference(a, b), 'keep': np.asarray(refbuild.nms_with_reference_iou(a, 0.7), np.int64)}
    for seed, n, t in PIB_CASES:
        pts, boxes = pib_inputs(seed, n, t)
        flags = refbuild.points_in_boxes_cpu_reference(pts, boxes)
        out['pib%d_shape' % seed] = np.array(flags.shape, np.int64)
        out['pib%d_nonzero' % seed] = np.stack(np.nonzero(flags)).astype(np.int32)
    path = os.path.join(HERE, 'refbuild_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
