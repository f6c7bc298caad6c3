"""CPU: the three-limb (bf16x3) engine of the f32 mode's dense 3x3 layers as built - the exact split and its packers, which layers the
entry point covers (answered by host code), the resources of the two kernel instances from the compiler's resource report (what
tools/kernel_regs.py reads), and the engine switch."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from detzero_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16_MAX = 3.3895313892515355e38
FP32_MAX = 3.4028234663852886e38


@pytest.fixture(scope='module')
def lib():
    from detzero_amd import lib as L
    from detzero_amd.build import build
    build(verbose=False)
    return L.load()


def _values():
    """fp32 test values (N, 8): random sign x [1, 2) mantissas x 2^e, e in [-100, 100], with the special values in front."""
    g = torch.Generator().manual_seed(5)
    n = 1 << 16
    mant = (torch.randint(0, 1 << 23, (n,), generator=g, dtype=torch.int32) | 0x3F800000).view(torch.float32)
    e = torch.randint(-100, 101, (n,), generator=g)
    sign = torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
    x = torch.ldexp(mant * sign, e)
    special = torch.tensor([0.0, -0.0, FP32_MAX, -FP32_MAX, 1 + 2.0 ** -23, 2 - 2.0 ** -23, 2.0 ** -100, -(2.0 ** 100)], dtype=torch.float32)
    x[:8] = special
    assert torch.isfinite(x).all() and (x[8:].abs() >= 2.0 ** -100).all() and (x[8:].abs() < 2.0 ** 101).all()
    return x.reshape(-1, 8)


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_round_trip_is_bit_exact():
    x = _values()
    p = ops.limb3_pack(x)
    assert p.dtype == torch.float32 and p.shape == (x.shape[0], 12)
    assert torch.equal(_bits(ops.limb3_unpack(p)), _bits(x))
    limbs = p.view(torch.bfloat16).float()
    assert torch.isfinite(limbs).all()                              # +-fp32-max: no inf limb
    # higher ranks keep their leading dimensions; groups of 8 channels are independent
    x3 = x[:64].reshape(4, 2, 64)
    p3 = ops.limb3_pack(x3)
    assert p3.shape == (4, 2, 96) and torch.equal(_bits(ops.limb3_unpack(p3)), _bits(x3))
    with pytest.raises(Exception):
        ops.limb3_pack(torch.zeros(3, 12))


def test_limbs_are_roundings_of_their_remainders():
    """h = rn(clamp(x)), m = rn(x - h), l = rn(x - h - m) = x - h - m, restated in torch; layout: 16 B of h, 16 of m, 16 of l per group."""
    x = _values()
    t = ops.limb3_pack(x).view(torch.bfloat16).reshape(-1, 3, 8)
    h, m, l = t[:, 0].float(), t[:, 1].float(), t[:, 2].float()
    eh = x.clamp(-BF16_MAX, BF16_MAX).to(torch.bfloat16).float()
    r1 = x - eh
    em = r1.to(torch.bfloat16).float()
    r2 = r1 - em
    assert torch.equal(h, eh) and torch.equal(m, em) and torch.equal(l, r2.to(torch.bfloat16).float())
    assert torch.equal(l, r2)                                        # the last rounding is exact
    assert torch.equal(x.double(), h.double() + m.double() + l.double())
    # 24 bits: each limb is at most half an ulp of the one before it (m of a saturated h - |x| beyond bf16-max - is a whole ulp)
    plain = x.abs() <= BF16_MAX
    assert (m.abs() <= h.abs() * 2.0 ** -8)[plain].all() and (m.abs() <= h.abs() * 2.0 ** -6).all() and (l.abs() <= m.abs() * 2.0 ** -8).all()


def test_pack_weight_pads_cout_with_zero_rows():
    g = torch.Generator().manual_seed(1)
    w = torch.randn(9, 32, 70, generator=g)
    p = ops.pack_weight_limb3(w)
    assert p.shape == (9, 128, 48) and p.dtype == torch.float32
    u = ops.limb3_unpack(p)
    assert torch.equal(u[:, :70], w.transpose(1, 2)) and (_bits(p[:, 70:]) == 0).all()
    assert ops.pack_weight_limb3(torch.randn(9, 64, 64, generator=g)).shape == (9, 64, 96)


def _desc(**over):
    from detzero_amd import lib as L
    f = dict(batch=2, ho=20, wo=40, in_hp=22, in_wp=42, in_cstride=64, in_coff=0, cin=64, kh=3, kw=3, stride=1, in_off=0,
             out_hp=22, out_wp=42, out_cstride=128, out_coff=0, out_sy=1, out_sx=1, out_dy=1, out_dx=1, groups=1, cout_pad=128, relu=1)
    f.update(over)
    d = L.Conv2dDesc()
    for k, v in f.items():
        setattr(d, k, v)
    d.g_cout[0] = f['cout_pad']
    return d


EXCLUDED = [dict(kh=1), dict(kw=1), dict(stride=2), dict(groups=2), dict(cin=48), dict(cin=16), dict(cout_pad=32), dict(cout_pad=96),
            dict(phase_groups=1), dict(in_rowidx=64), dict(in_tiles=64), dict(group_shift=64), dict(group_max=1),
            dict(batch=4096, in_hp=192, in_wp=192)]           # 4096 x 192 x 192 x 64 x 4 bytes: beyond the 2 GiB window


def test_supported_answers_without_a_gpu(lib):
    assert lib.dz_conv3x3_limb3_supported(ctypes.byref(_desc())) == 1
    for ok in (dict(cin=32, cout_pad=64), dict(cin=512, in_cstride=512, cout_pad=64), dict(cout_pad=384), dict(in_coff=32, in_cstride=128),
               dict(relu=0), dict(batch=40, in_hp=190, in_wp=190, in_cstride=128, cin=128)):
        assert lib.dz_conv3x3_limb3_supported(ctypes.byref(_desc(**ok))) == 1, ok
    for bad in EXCLUDED:
        assert lib.dz_conv3x3_limb3_supported(ctypes.byref(_desc(**bad))) == 0, bad
        assert lib.dz_conv3x3_limb3_variant(ctypes.byref(_desc(**bad))) == b'none', bad
    assert ops.conv3x3_limb3_supported(dict(kh=3, kw=3, stride=1, groups=1, cin=32, cout_pad=64, batch=1, in_hp=5, in_wp=5, in_cstride=32))
    assert not ops.conv3x3_limb3_supported(dict(kh=3, kw=3, stride=2, groups=1, cin=32, cout_pad=64, batch=1, in_hp=5, in_wp=5, in_cstride=32))


def test_variant_names(lib):
    name = lambda **kw: lib.dz_conv3x3_limb3_variant(ctypes.byref(_desc(**kw))).decode()
    assert name(cout_pad=128) == 'k_conv3x3_t<8x32x128>' and name(cout_pad=384) == 'k_conv3x3_t<8x32x128>'
    assert name(cout_pad=64) == 'k_conv3x3_t<8x32x64>' and name(cout_pad=192) == 'k_conv3x3_t<8x32x64>'
    assert name(cout_pad=128, batch=1, ho=9, wo=13, in_hp=11, in_wp=15) == 'k_conv3x3_t<8x32x128>'      # no tile-count floor: one engine
    assert name(cout_pad=32) == 'none'


def test_kernels_have_no_scratch_and_fit_lds(tmp_path):
    """Exactly two instances; each: 0 bytes of scratch, no spilled register; the dynamic LDS of the launch is T3Cfg::LDS_BYTES, held
    to 160 KiB by a static_assert of the file (compiling it is that check), restated here from the file's constants."""
    src = os.path.join(ROOT, 'detzero_amd', 'csrc', 'conv3x3_t.hip')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-c', src, '-o', str(tmp_path / 't3.o'), '-Rpass-analysis=kernel-resource-usage']
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
    kernels = [k for k in kernels if 'k_conv3x3_t' in k['name']]
    assert len(kernels) == 2, [k['name'] for k in kernels]
    for k in kernels:
        print(k)
        assert int(k['ScratchSize [bytes/lane]']) == 0 and int(k['VGPRs Spill']) == 0, k     # (scalar spills go to VGPR lanes, outside the tap loop)
        assert int(k['LDS Size [bytes/block]']) <= 160 * 1024, k
        assert int(k['VGPRs']) + int(k['AGPRs']) <= 256, k            # two waves per SIMD
    txt = open(src).read()
    assert 'static_assert(LDS_BYTES <= 160 * 1024' in txt
    for bc in (64, 128):
        lds = (340 * 13 + 2 * bc * 13) * 16 + 2 * bc * 4             # input planes + two weight buffers + scale / shift
        assert lds <= 160 * 1024, (bc, lds)


def test_math_modes_unchanged():
    assert ops.MATH_MODES == {'f32': 0, 'f16x2': 1, 'bf16x2': 2, 'f16': 3}
    assert [ops.storage_math(m) for m in range(4)] == [0, 1, 2, 1]
    assert ops.DENSE_F32_ENGINES == ('mfma32', 'bf16x3')


def test_dense_engine_switch(lib):
    from detzero_amd import det_modules
    from detzero_amd.centerpoint import SyntheticDatasetInfo, build_network, set_dense_engine
    from detzero_amd.config import centerpoint_1sweep_cfg
    from detzero_amd.lib import DetZeroHipError
    cfg = centerpoint_1sweep_cfg((0.1, 0.1, 0.15))
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), SyntheticDatasetInfo(cfg))
    mods = (model.backbone2d, model.dense_head)
    if 'DZ_TUNE_DENSE_F32_ENGINE' not in os.environ:
        assert all(m.f32_dense_engine == 'mfma32' for m in mods)
    before = [m.f32_dense_engine for m in mods]
    gen = det_modules.CACHE_GEN[0]
    with pytest.raises(DetZeroHipError):
        set_dense_engine(model, 'bf16x2')
    assert [m.f32_dense_engine for m in mods] == before and det_modules.CACHE_GEN[0] == gen      # a refused call changes nothing
    set_dense_engine(model, 'bf16x3')
    assert all(m.f32_dense_engine == 'bf16x3' for m in mods) and det_modules.CACHE_GEN[0] > gen
    gen = det_modules.CACHE_GEN[0]
    set_dense_engine(model, 'mfma32')
    assert all(m.f32_dense_engine == 'mfma32' for m in mods) and det_modules.CACHE_GEN[0] > gen
    # the weights are handed over in limb form only in f32 mode with the engine on
    entry = {'w': torch.randn(9, 32, 64)}
    assert model.backbone2d._l3(entry) is None
    set_dense_engine(model, 'bf16x3')
    packed = model.backbone2d._l3(entry)
    assert packed().shape == (9, 64, 48) and packed() is entry['w_limb3']                          # packed once, cached in the entry
    model.backbone2d.set_math('f16x2')
    assert model.backbone2d._l3(entry) is None                                                      # split modes ignore the switch
    with pytest.raises(DetZeroHipError):
        ops.conv2d(dict(g_cout=[64], g_ooff=[0]), f32_engine='tiles')
