"""Golden vectors for the evaluator's conversion step (info dicts -> flat arrays -> distance mask) from the REFERENCE's own code, CPU.

    python tests/golden/gen_waymo_eval_golden.py      (build container only; needs /root/reference)

detection/detzero_det/datasets/waymo/waymo_eval_detection.py imports TensorFlow and waymo_open_dataset at module level, so it cannot
be imported: ``limit_period`` and the methods ``generate_waymo_type_results`` and ``mask_by_distance`` are extracted with `ast` and
executed as they are (globals: numpy) on seeded infos.  The file holds arrays only: the inputs (per frame) and, for every case
(fake_gt_infos, bev, distance_thresh), the flat arrays the reference hands to its metric.
"""
import ast
import copy
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
CLASS_NAMES = ['Vehicle', 'Pedestrian', 'Cyclist']
CASES = [(fake, bev, dist) for fake in (False, True) for bev in (False, True) for dist in (30, 1000)]
N_FRAMES = 5


def reference_functions():
    src = open(REF + '/detection/detzero_det/datasets/waymo/waymo_eval_detection.py').read()
    glb = {'np': np}
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.FunctionDef) and node.name in ('limit_period', 'generate_waymo_type_results', 'mask_by_distance'):
            exec(compile(ast.Module(body=[node], type_ignores=[]), 'waymo_eval_detection.py:' + node.name, 'exec'), glb)
    return glb['generate_waymo_type_results'], glb['mask_by_distance']


class Self:
    WAYMO_CLASSES = ['unknown', 'Vehicle', 'Pedestrian', 'Truck', 'Cyclist']


def synth_infos(seed=7):
    rng = np.random.RandomState(seed)
    names = np.array(['Vehicle', 'Pedestrian', 'Cyclist', 'Sign', 'unknown'])
    pds, gts = [], []
    for f in range(N_FRAMES):
        n_gt, n_pd = (0 if f == 3 else rng.randint(4, 12)), (0 if f == 1 else rng.randint(3, 14))
        box = lambda n, w: np.concatenate([rng.uniform(-60, 60, (n, 2)), rng.uniform(-1, 2, (n, 1)), rng.uniform(0.5, 5, (n, 3)),
                                           rng.uniform(-7, 7, (n, w - 6))], axis=1).astype(np.float32)
        gts.append({'name': names[rng.randint(0, 5, n_gt)], 'difficulty': rng.randint(0, 3, n_gt).astype(np.int32),
                    'num_points_in_gt': rng.choice([0, 1, 5, 6, 40], n_gt).astype(np.int64), 'gt_boxes_lidar': box(n_gt, 9)})
        pds.append({'name': names[rng.randint(0, 3, n_pd)], 'score': rng.uniform(0, 1, n_pd).astype(np.float32), 'boxes_lidar': box(n_pd, 7)})
    return pds, gts


def main():
    generate, mask = reference_functions()
    pds, gts = synth_infos()
    out = {}
    for f in range(N_FRAMES):
        for k, v in pds[f].items():
            out['in_pd%d_%s' % (f, k)] = v
        for k, v in gts[f].items():
            out['in_gt%d_%s' % (f, k)] = v
    for fake, bev, dist in CASES:
        tag = 'fake%d_bev%d_dist%d' % (fake, bev, dist)
        p = generate(Self(), copy.deepcopy(pds), CLASS_NAMES, is_gt=False, bev=bev)
        g = generate(Self(), copy.deepcopy(gts), CLASS_NAMES, is_gt=True, fake_gt_infos=fake, bev=bev)
        pb, pf, pt, ps = mask(Self(), dist, p[1], p[0], p[2], p[3])
        gb, gf, gt_, gd = mask(Self(), dist, g[1], g[0], g[2], g[5])
        for k, v in (('pd_frame', pf), ('pd_box', pb), ('pd_type', pt), ('pd_score', ps), ('gt_frame', gf), ('gt_box', gb), ('gt_type', gt_),
                     ('gt_diff', gd)):
            out['%s_%s' % (tag, k)] = np.asarray(v)
    path = os.path.join(HERE, 'waymo_eval_golden.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
