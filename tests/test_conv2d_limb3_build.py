"""CPU: the generic three-limb (bf16x3) engine of the f32 mode's dense layers as built (csrc/conv2d_t.hip, dz_conv2d_limb3_*) - which
layers the entry point covers and which instance runs them (answered by host code), the resources of the kernel instances from the
compiler's resource report, the weight packing, and the switch (centerpoint.set_dense_engine's f32_generic)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from detzero_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'detzero_amd', 'csrc', 'conv2d_t.hip')


@pytest.fixture(scope='module')
def lib():
    from detzero_amd import lib as L
    from detzero_amd.build import build
    build(verbose=False)
    return L.load()


def _instance_names():
    """The names the selector can return: the kC2T table of the source."""
    return sorted(set(re.findall(r'"(k_conv2d_t<\d+x\d+x\d+>)"', open(SRC).read())))


def _desc(**over):
    """The strided 3 x 3 layer of the BEV backbone on a small image, with fields overridden."""
    from detzero_amd import lib as L
    f = dict(batch=2, ho=10, wo=20, in_hp=22, in_wp=42, in_cstride=128, in_coff=0, cin=128, kh=3, kw=3, stride=2, in_off=0,
             out_hp=12, out_wp=22, out_cstride=256, out_coff=0, out_sy=1, out_sx=1, out_dy=1, out_dx=1, groups=1, cout_pad=256, relu=1)
    f.update(over)
    d = L.Conv2dDesc()
    g_cout = f.pop('g_cout', None)
    for k, v in f.items():
        setattr(d, k, v)
    for g in range(max(1, min(f['groups'], 8))):
        d.g_cout[g] = g_cout[g] if g_cout else f['cout_pad']
    return d


def _production():
    """The four layer classes the 3 x 3 stride-1 engine refuses, from the detector's own f32 pass (host only)."""
    from detzero_amd import lib as L
    from tests.test_gpu_dense_conv import _cdesc, production_cases
    lib = L.load()
    return [c for c in production_cases('f32', 'single') if not lib.dz_conv3x3_limb3_supported(ctypes.byref(_cdesc(c.desc)))]


ACCEPTED = [
    (dict(), 'k_conv2d_t<128x128x16>'),                                                          # strided 3 x 3, 128 -> 256
    (dict(kh=3, kw=3, stride=1, cin=64, in_cstride=64, cout_pad=128, out_cstride=128), 'k_conv2d_t<128x128x16>'),     # a plain 3 x 3 stride-1 layer
    (dict(kh=1, kw=1, stride=1, in_off=1, out_coff=256, out_cstride=512), 'k_conv2d_t<128x128x16>'),               # deblock 1
    (dict(kh=1, kw=1, stride=1, in_off=1, cin=256, in_cstride=256, out_sy=2, out_sx=2, out_dy=2, out_dx=1, out_hp=24, out_wp=44,
          out_cstride=512), 'k_conv2d_t<128x128x16>'),                                           # a deblock-2 phase
    (dict(stride=1, groups=6, cin=64, in_cstride=384, cout_pad=16, g_cout=[2, 1, 3, 2, 1, 3], out_cstride=12, out_dy=0, out_dx=0,
          relu=0), 'k_conv2d_t<128x32x32>'),                                                     # the head's grouped output layer
    (dict(cout_pad=32, out_cstride=32), 'k_conv2d_t<128x32x32>'),
    (dict(cout_pad=48, out_cstride=48), 'k_conv2d_t<128x64x32>'),
    (dict(cout_pad=64, out_cstride=64), 'k_conv2d_t<128x64x32>'),
    (dict(cout_pad=192, out_cstride=192), 'k_conv2d_t<128x64x32>'),
    (dict(cout_pad=384, out_cstride=384), 'k_conv2d_t<128x128x16>'),
    (dict(cin=32, in_cstride=64, in_coff=32), 'k_conv2d_t<128x128x16>'),
    (dict(groups=8, cin=32, in_cstride=256, cout_pad=16, out_cstride=128), 'k_conv2d_t<128x32x32>'),
    (dict(batch=0), 'k_conv2d_t<128x128x16>'),
]
# refused: the fields of dz_conv2d_forward / _forward_split this engine has no arm for, an input at or beyond the 2 GiB window, and
# widths and kernels no instance covers
EXCLUDED = [dict(group_shift=64), dict(group_max=1), dict(phase_groups=1), dict(in_rowidx=64), dict(in_tiles=64),
            dict(batch=1024, in_hp=64, in_wp=64), dict(batch=4096, in_hp=192, in_wp=192),           # exactly 2^31 bytes, and beyond
            dict(cin=48), dict(cin=16), dict(cin=0), dict(cout_pad=24), dict(cout_pad=8), dict(cout_pad=0),
            dict(kh=5, kw=5), dict(kh=1), dict(kw=1), dict(kh=2, kw=2), dict(stride=3), dict(stride=0), dict(groups=0), dict(groups=9)]


def test_supported_and_variant_answer_without_a_gpu(lib):
    reached = set()
    for over, name in ACCEPTED:
        d = _desc(**over)
        assert lib.dz_conv2d_limb3_supported(ctypes.byref(d)) == 1, over
        assert lib.dz_conv2d_limb3_variant(ctypes.byref(d)).decode() == name, over
        reached.add(name)
    for bad in EXCLUDED:
        d = _desc(**bad)
        assert lib.dz_conv2d_limb3_supported(ctypes.byref(d)) == 0, bad
        assert lib.dz_conv2d_limb3_variant(ctypes.byref(d)) == b'none', bad
    assert lib.dz_conv2d_limb3_supported(None) == 0 and lib.dz_conv2d_limb3_variant(None) == b'none'
    # the table reaches every instance, and no instance exists that it cannot reach
    assert reached == set(_instance_names()), (sorted(reached), _instance_names())
    assert ops.conv2d_limb3_supported(dict(kh=1, kw=1, stride=1, groups=1, cin=32, cout_pad=16, batch=1, in_hp=5, in_wp=5, in_cstride=32))
    assert not ops.conv2d_limb3_supported(dict(kh=1, kw=1, stride=1, groups=1, cin=32, cout_pad=16, batch=1, in_hp=5, in_wp=5, in_cstride=32,
                                               phase_groups=1))


def test_production_layers_are_covered(lib):
    """The strided layer, deblock 1, the four deblock-2 phases and the grouped output layer of the detector's f32 pass: each one
    refused by the 3 x 3 stride-1 engine and taken by this one."""
    from tests.test_gpu_dense_conv import _cdesc
    cases = _production()
    kinds = set()
    for c in cases:
        d = _cdesc(c.desc)
        assert lib.dz_conv2d_limb3_supported(ctypes.byref(d)) == 1, c.label
        assert lib.dz_conv2d_limb3_variant(ctypes.byref(d)).decode() in _instance_names(), c.label
        dd = c.desc
        kinds.add('strided' if dd['stride'] == 2 else 'grouped' if dd['groups'] > 1 else 'deblock2' if dd['out_sy'] == 2 else 'deblock1')
    assert kinds == {'strided', 'deblock1', 'deblock2', 'grouped'}, (kinds, [c.label for c in cases])
    assert sum(c.desc['out_sy'] == 2 for c in cases) == 4


def _resource_report(tmp_path):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-c', SRC, '-o', str(tmp_path / 'c2t.o'),
           '-Rpass-analysis=kernel-resource-usage']
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    kernels, cur = [], None
    for line in run.stderr.splitlines():
        m = re.search(r'remark: +([A-Za-z \[\]/]+): +(\S+)', line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == 'Function Name':
            cur = {'name': v}
            kernels.append(cur)
        elif cur is not None:
            cur[k] = v
    return [k for k in kernels if 'k_conv2d_t' in k['name']]


def test_kernels_have_no_scratch_and_fit_lds(tmp_path):
    """As many instances as the selector has names; each: 0 bytes of scratch, no spilled VGPR, registers for at least two waves per SIMD
    (two 256-thread workgroups per CU); the dynamic LDS of a launch is C2TTile::LDS_BYTES, held to 160 KiB by a static_assert of the
    file (compiling it is that check) and restated here from the tile in the instance's name."""
    names = _instance_names()
    kernels = _resource_report(tmp_path)
    assert len(kernels) == len(names) == 3, ([k['name'] for k in kernels], names)
    for k in kernels:
        print(k)
        assert int(k['ScratchSize [bytes/lane]']) == 0 and int(k['VGPRs Spill']) == 0, k
        assert int(k['LDS Size [bytes/block]']) <= 160 * 1024, k
        assert int(k['VGPRs']) + int(k['AGPRs']) <= 256, k
    txt = open(os.path.join(os.path.dirname(SRC), 'limb3.h')).read()           # the tile C2TTile derives from
    assert 'static_assert(LDS_BYTES <= 160 * 1024' in txt
    for n in names:
        bp, bc, kc = (int(v) for v in re.match(r'k_conv2d_t<(\d+)x(\d+)x(\d+)>', n).groups())
        rowb = kc // 8 * 48 + 16
        assert (rowb // 16) % 2 == 1, n
        lds = 2 * (bp + bc) * rowb
        assert 2 * lds <= 160 * 1024, (n, lds)                          # two workgroups per CU
        # the mangled name of the instance carries the tile
        assert any('Li%dELi%dELi%dE' % (bp, bc, kc) in k['name'] for k in kernels), n


def test_weight_packing_of_a_grouped_layer():
    """(groups, taps, cin, cout_pad) -> (groups * taps, round_up(cout_pad, 32), cin * 3 / 2): the transposed weights bit for bit, zero
    rows behind cout_pad."""
    g = torch.Generator().manual_seed(2)
    w = torch.randn(6, 9, 64, 16, generator=g)
    p = ops.pack_weight_limb3_generic(w)
    assert p.shape == (54, 32, 96) and p.dtype == torch.float32
    u = ops.limb3_unpack(p)
    assert torch.equal(u[:, :16].contiguous().view(torch.int32), w.reshape(54, 64, 16).transpose(1, 2).contiguous().view(torch.int32))
    assert bool((p[:, 16:].contiguous().view(torch.int32) == 0).all())
    assert ops.pack_weight_limb3_generic(torch.randn(1, 128, 256, generator=g)).shape == (1, 256, 192)
    assert ops.pack_weight_limb3_generic(torch.randn(9, 32, 48, generator=g)).shape == (9, 64, 48)


def test_generic_engine_switch(lib):
    from detzero_amd import det_modules
    from detzero_amd.centerpoint import SyntheticDatasetInfo, build_network, set_dense_engine
    from detzero_amd.config import centerpoint_1sweep_cfg
    from detzero_amd.lib import DetZeroHipError
    assert ops.DENSE_F32_ENGINES == ('mfma32', 'bf16x3') and ops.DENSE_F32_GENERIC_ENGINES == ('mfma32', 'bf16x3')
    cfg = centerpoint_1sweep_cfg((0.1, 0.1, 0.15))
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), SyntheticDatasetInfo(cfg))
    mods = (model.backbone2d, model.dense_head)
    assert all(m.f32_dense_generic == 'mfma32' for m in mods)                                       # off by default, whatever the environment
    set_dense_engine(model, 'mfma32', f32_generic='mfma32')
    entry = {'w': torch.randn(6, 9, 64, 16)}
    assert model.backbone2d._l3g(entry) is None                                                      # switch off
    gen = det_modules.CACHE_GEN[0]
    with pytest.raises(DetZeroHipError):
        set_dense_engine(model, 'mfma32', f32_generic='bf16x2')
    with pytest.raises(DetZeroHipError):
        set_dense_engine(model, 'bf16x2', f32_generic='bf16x3')
    assert all(m.f32_dense_generic == 'mfma32' and m.f32_dense_engine == 'mfma32' for m in mods) and det_modules.CACHE_GEN[0] == gen
    set_dense_engine(model, 'mfma32', f32_generic='bf16x3')
    assert all(m.f32_dense_generic == 'bf16x3' and m.f32_dense_engine == 'mfma32' for m in mods) and det_modules.CACHE_GEN[0] > gen
    set_dense_engine(model, 'bf16x3')                                                                # None keeps the value
    assert all(m.f32_dense_generic == 'bf16x3' and m.f32_dense_engine == 'bf16x3' for m in mods)
    set_dense_engine(model, 'mfma32', None)
    assert all(m.f32_dense_generic == 'bf16x3' and m.f32_dense_engine == 'mfma32' for m in mods)
    # the weights are handed over in limb form only in f32 mode with the switch on: packed once, cached in the entry
    packed = model.dense_head._l3g(entry)
    assert packed().shape == (54, 32, 96) and packed() is entry['w_limb3g']
    assert model.backbone2d._l3(entry) is None                                                       # (the 3 x 3 engine's accessor follows its own switch)
    model.dense_head.set_math('f16x2')
    assert model.dense_head._l3g(entry) is None                                                      # split modes ignore the switch
    model.dense_head.set_math('f32')
    gen = det_modules.CACHE_GEN[0]
    set_dense_engine(model, 'mfma32', f32_generic='mfma32')
    assert all(m.f32_dense_generic == 'mfma32' for m in mods) and det_modules.CACHE_GEN[0] > gen
    assert model.dense_head._l3g(entry) is None
    with pytest.raises(DetZeroHipError):
        ops.conv2d(dict(g_cout=[64], g_ooff=[0]), f32_generic='tiles')
