"""GPU (MI355X): the launch sequence of the sparse backbone is pinned.  `backbone3d.run` on the smallest detector and frame of
tests/test_gpu_route_matrix.py under ops.LaunchProfiler, once per engine configuration (f32 x f32_engine x f32_gather; f16x2 x engine x
PACKED_TABLES): the 21 reported kernel names, in order, equal tests/golden/spconv_launch_names.json - recorded by
tests/golden/gen_spconv_launch_names.py at the commit before ops.spconv_route existed (the commit is named there); two consecutive
runs agree bit for bit on every stage; and every tensor a stage's tables own was handed from the index side stream to the main one."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _gen(golden_dir):
    spec = importlib.util.spec_from_file_location('gen_spconv_launch_names', os.path.join(golden_dir, 'gen_spconv_launch_names.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_launch_names_outputs_and_hand_over_per_configuration(device, golden_dir, monkeypatch):
    from detzero_amd import det_modules as dm
    gen = _gen(golden_dir)
    with open(os.path.join(golden_dir, 'spconv_launch_names.json')) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(c[0] for c in gen.CONFIGS) and len(golden) == 10
    feats, coords, model = gen.frame()
    model = model.to(device).eval()
    feats, coords = torch.from_numpy(feats).to(device), torch.from_numpy(coords).to(device)

    handed, pyramids = [], []          # (the recorded tensors themselves, kept alive: an identity cannot be reused while they are)
    real_record = torch.Tensor.record_stream

    def record_stream(self, stream):
        handed.append(self)
        return real_record(self, stream)
    monkeypatch.setattr(torch.Tensor, 'record_stream', record_stream)
    real_build = dm.VoxelResBackBone8x.build_pyramid

    def build_pyramid(self, *a, **k):
        pyramids.append(real_build(self, *a, **k))
        return pyramids[-1]
    monkeypatch.setattr(dm.VoxelResBackBone8x, 'build_pyramid', build_pyramid)

    with torch.no_grad():
        for cfg in gen.CONFIGS:
            del handed[:], pyramids[:]
            names, first = gen.record(model, feats, coords, cfg)
            assert len(names) == 21 and names == golden[cfg[0]], (cfg[0], names, golden[cfg[0]])
            # every stage is built on the side stream (run: overlap=True): all that its tables own crossed over
            steps = pyramids[-1]['steps']
            assert len(steps) == 5
            tables = [t for st in steps for t in st[:2] if t is not None]
            assert len(tables) == 8 and all(len(t.tensors()) >= 2 for t in tables), cfg[0]
            for t in tables:
                # what a table built by the library owns is written out here, not taken from tensors()
                owned = [t.words, t.tile_masks] + [x for x in (t.xwin or ()) if torch.is_tensor(x)] + list(t.tiles or ())
                assert t.tile_masks is not None and all(any(x is h for h in handed) for x in owned), \
                    (cfg[0], 'a tensor of a table was not handed to the main stream')
                assert len(t.tensors()) == len(owned) and all(any(x is y for y in t.tensors()) for x in owned), cfg[0]
            if 'xrun' in cfg[0]:
                # the tables of neighbors_xrun: windows always, the tap-set order at 64 and 128 channels
                xw = [st[1].xwin for st in steps[1:4]]
                assert all(w is not None and torch.is_tensor(w.windows) for w in xw), cfg[0]
                assert [w.sorted_table is not None and w.perm is not None for w in xw] == [False, True, True], cfg[0]
            names2, second = gen.record(model, feats, coords, cfg)
            assert names2 == names
            assert sorted(first) == sorted(second) == ['encoded', 'x_conv1', 'x_conv2', 'x_conv3', 'x_conv4']
            for stage in first:
                assert first[stage].shape[0] > 0 and torch.equal(first[stage], second[stage]), (cfg[0], stage)
