"""CPU: the bf16x3 x-run sparse convolution of the exact-fp32 mode (csrc/sparse_conv_xt.hip) as built - which layers it covers, the
resources of its kernels from the compiler's resource report (taken as tests/test_xrun_f32_build.py does), the engine switch of the
backbone, and the limb layout of its weights."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIPPED = (32, 64, 128)         # the widths the selector offers (a width ships only where it beat both fp32 kernels)


@pytest.fixture(scope='module')
def lib():
    from detzero_amd import lib as L
    from detzero_amd.build import build
    build(verbose=False)
    return L.load()


def test_covered_layers(lib):
    for c in SHIPPED:
        assert lib.dz_spconv_x_limb3_variant(c, c).decode() == 'k_spconv_xt<%d>' % c
    for cin, cout in ((16, 16), (32, 64), (64, 128), (256, 256)):
        assert lib.dz_spconv_x_limb3_variant(cin, cout) == b'none', (cin, cout)
    for cin, cout in ((16, 16), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (256, 256)):
        rows = lib.dz_spconv_x_limb3_window_rows(cin, cout)
        assert (rows > 0) == (cin == cout and cin in SHIPPED), (cin, cout, rows)
        assert (lib.dz_spconv_x_limb3_variant(cin, cout) != b'none') == (rows > 0)
        if rows:
            # one index serves every arithmetic: the units are the pair16 engine's
            assert lib.dz_spconv_x_tile_rows(cin, cout) != 0 and rows % 16 == 0


def test_kernels_have_no_scratch_and_fit_lds(tmp_path):
    """One kernel instance per shipped width: 0 bytes of scratch, no spilled register, static LDS within 160 KiB (the dynamic LDS of
    the launch is XTCfg::LDS_BYTES, held to 160 KiB by a static_assert of the file: compiling it is that check)."""
    src = os.path.join(ROOT, 'detzero_amd', 'csrc', 'sparse_conv_xt.hip')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-c', src, '-o', str(tmp_path / 'xt.o'), '-Rpass-analysis=kernel-resource-usage']
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
    kernels = [k for k in kernels if 'k_spconv_xt' in k['name']]
    assert len(kernels) == len(SHIPPED), [k['name'] for k in kernels]
    for c in SHIPPED:
        assert sum('XTCfgILi%dE' % c in k['name'] for k in kernels) == 1, (c, [k['name'] for k in kernels])
    for k in kernels:
        print(k)
        assert int(k['ScratchSize [bytes/lane]']) == 0 and int(k['VGPRs Spill']) == 0 and int(k['SGPRs Spill']) == 0, k
        assert int(k['LDS Size [bytes/block]']) <= 160 * 1024, k
    txt = open(src).read()
    assert 'static_assert(LDS_BYTES <= 160 * 1024' in txt


def test_fp32_engine_switch():
    import torch
    from detzero_amd import ops
    from detzero_amd.centerpoint import SyntheticDatasetInfo, build_network, set_sparse_engine
    from detzero_amd.config import centerpoint_1sweep_cfg
    from detzero_amd.lib import DetZeroHipError
    assert ops.SPARSE_F32_ENGINES == ('gather', 'xrun', 'xrun_bf16x3')
    cfg = centerpoint_1sweep_cfg((0.1, 0.1, 0.15))
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), SyntheticDatasetInfo(cfg))
    bb = model.backbone3d
    if 'DZ_TUNE_SPCONV_F32_ENGINE' not in os.environ:
        assert bb.f32_engine == 'gather'
    before = (bb.engine, bb.f32_engine)
    set_sparse_engine(model, 'xrun', f32_engine='xrun_bf16x3')
    assert (bb.engine, bb.f32_engine) == ('xrun', 'xrun_bf16x3')
    with pytest.raises(DetZeroHipError):
        set_sparse_engine(model, 'gather', f32_engine='tiles')
    assert (bb.engine, bb.f32_engine) == ('xrun', 'xrun_bf16x3')            # a refused call changes nothing
    set_sparse_engine(model, 'gather')                                      # one-argument form: the fp32 engine is left alone
    assert (bb.engine, bb.f32_engine) == ('gather', 'xrun_bf16x3')
    set_sparse_engine(model, before[0], f32_engine=before[1])
    assert (bb.engine, bb.f32_engine) == before


@pytest.mark.parametrize('channels', (32, 64, 128))
def test_weight_limb_layout(channels):
    """(27, cin, cout) -> (27, cout, cin * 3 / 2) words: per tap, output channel and group of 8 input channels 16 B of h, 16 of m, 16 of
    l; unpacked, the transposed weights come back bit for bit."""
    import torch
    from detzero_amd import ops
    g = torch.Generator().manual_seed(channels)
    w = torch.randn((27, channels, channels), generator=g) * torch.exp2(torch.randint(-40, 17, (27, channels, channels), generator=g).float())
    p = ops.pack_weight_limb3(w, cout_mult=32)
    assert tuple(p.shape) == (27, channels, channels * 3 // 2) and p.dtype == torch.float32 and p.is_contiguous()
    back = ops.limb3_unpack(p)
    assert torch.equal(back.view(torch.int32), w.transpose(1, 2).contiguous().view(torch.int32))
    # the group layout the kernel's A operand reads: words [12 g, 12 g + 4) are the h limbs of input channels 8 g .. 8 g + 7
    h = p.view(torch.bfloat16).reshape(27, channels, channels // 8, 3, 8)[..., 0, :].reshape(27, channels, channels)
    assert torch.equal(h, w.transpose(1, 2).to(torch.bfloat16))
