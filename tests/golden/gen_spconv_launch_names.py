"""Ordered kernel names the 21 sparse convolutions of `backbone3d.run` report to ops.LaunchProfiler, per engine configuration, on the
smallest detector and frame of tests/test_gpu_route_matrix.py (0.2 m voxels, masked_frame(0, 20000)).  Needs a GPU:

    python tests/golden/gen_spconv_launch_names.py [out.json]  ->  tests/golden/spconv_launch_names.json

The fixture pins the launch sequence across refactors of the Python side that picks the engines, so it is recorded at the commit
BEFORE such a change, never with the code under test.  The committed file was recorded at 577410c ("Test the bf16x3 engines at their
siblings' edges and frame counts"), the parent of the commit that introduced ops.NeighborTable and ops.spconv_route.
tests/test_gpu_spconv_launch_names.py runs the same `record` against it.
"""
import itertools
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

# (id, math, set_sparse_engine keywords, PACKED_TABLES)
CONFIGS = [('f32/%s/%s' % (e, g), 'f32', {'engine': 'xrun', 'f32_engine': e, 'f32_gather': g}, False)
           for e, g in itertools.product(('gather', 'xrun', 'xrun_bf16x3'), ('mfma32', 'bf16x3'))]
CONFIGS += [('f16x2/%s/%s' % (e, 'packed' if p else 'plain'), 'f16x2', {'engine': e, 'f32_engine': 'gather', 'f32_gather': 'mfma32'}, p)
            for e, p in itertools.product(('gather', 'xrun'), (False, True))]


def frame():
    """-> (voxel features (m, 5) f32, voxel coordinates (m, 4) i32 [b, z, y, x], the seeded detector on the CPU)."""
    from detzero_amd.synth import POINT_CLOUD_RANGE, VOXEL_SIZE_02
    from oracle import voxelize as ov
    from tests.util import make_model, masked_frame
    model, _, info = make_model(VOXEL_SIZE_02, seed=0)
    vox, czyx, nump = ov.hard_voxelize(masked_frame(0, 20000), POINT_CLOUD_RANGE, VOXEL_SIZE_02, 5, info.max_voxels['test'])
    coords = np.concatenate([np.zeros((czyx.shape[0], 1), np.int32), czyx], 1).astype(np.int32)
    return ov.mean_vfe(vox, nump).astype(np.float32), coords, model


def record(model, feats, coords, config):
    """One `backbone3d.run` of `model` (on the device) in `config` under a LaunchProfiler -> (kernel names in launch order,
    {stage: its active rows})."""
    from detzero_amd import det_modules as dm
    from detzero_amd import ops
    from detzero_amd.centerpoint import set_math, set_sparse_engine
    _, math, engines, packed = config
    was = dm.PACKED_TABLES
    dm.PACKED_TABLES = packed
    ops.PROFILER = ops.LaunchProfiler()
    try:
        set_math(model, math)
        set_sparse_engine(model, **engines)
        res = model.backbone3d.run(feats, coords, 1)
        names = [r[0] for r in ops.PROFILER.records]
    finally:
        ops.PROFILER = None
        dm.PACKED_TABLES = was
    torch.cuda.synchronize()
    return names, {k: x[:lvl.num_active()].clone() for k, (x, lvl) in res.items()}


def main():
    sys.path.insert(0, ROOT)
    feats, coords, model = frame()
    dev = torch.device('cuda')
    model = model.to(dev).eval()
    feats, coords = torch.from_numpy(feats).to(dev), torch.from_numpy(coords).to(dev)
    out = {}
    with torch.no_grad():
        for cfg in CONFIGS:
            out[cfg[0]], _ = record(model, feats, coords, cfg)
            assert len(out[cfg[0]]) == 21, (cfg[0], out[cfg[0]])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'spconv_launch_names.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    print(len(out), 'configurations ->', path)


if __name__ == '__main__':
    main()
