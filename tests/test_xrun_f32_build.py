"""CPU: the exact-fp32 x-run sparse convolution (csrc/sparse_conv_xf.hip) as built - which layers it covers, the resources of its
kernels from the compiler's resource report (what tools/kernel_regs.py reads), and the engine switch of the backbone."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVERED = (32, 64, 128)


@pytest.fixture(scope='module')
def lib():
    from detzero_amd import lib as L
    from detzero_amd.build import build
    build(verbose=False)
    return L.load()


def test_covered_layers(lib):
    for c in COVERED:
        assert lib.dz_spconv_x_f32_variant(c, c).decode() == 'k_spconv_xf<%d>' % c
    assert lib.dz_spconv_x_f32_variant(16, 16) == b'none' and lib.dz_spconv_x_f32_variant(32, 64) == b'none'
    for cin, cout in ((16, 16), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (256, 256)):
        rows = lib.dz_spconv_x_f32_window_rows(cin, cout)
        assert (rows > 0) == (cin == cout and cin in COVERED), (cin, cout, rows)
        if rows:
            # one index serves both arithmetics: the units of the fp32 kernel are the pair16 engine's
            assert lib.dz_spconv_x_tile_rows(cin, cout) in (128, 256) and rows % 16 == 0


def test_kernels_have_no_scratch_and_fit_lds(tmp_path):
    """Every kernel of the file: 0 bytes of scratch, no spilled register, static LDS within 160 KiB (the dynamic LDS of the launch is
    XFCfg::LDS_BYTES, held to 160 KiB by a static_assert of the file: compiling it is that check)."""
    src = os.path.join(ROOT, 'detzero_amd', 'csrc', 'sparse_conv_xf.hip')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-c', src, '-o', str(tmp_path / 'xf.o'), '-Rpass-analysis=kernel-resource-usage']
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
    kernels = [k for k in kernels if 'k_spconv_xf' in k['name']]
    assert len(kernels) == len(COVERED), [k['name'] for k in kernels]
    for k in kernels:
        print(k)
        assert int(k['ScratchSize [bytes/lane]']) == 0 and int(k['VGPRs Spill']) == 0 and int(k['SGPRs Spill']) == 0, k
        assert int(k['LDS Size [bytes/block]']) <= 160 * 1024, k
    txt = open(src).read()
    assert 'static_assert(LDS_BYTES <= 160 * 1024' in txt


def test_fp32_engine_switch():
    import torch
    from detzero_amd.centerpoint import SyntheticDatasetInfo, build_network, set_sparse_engine
    from detzero_amd.config import centerpoint_1sweep_cfg
    from detzero_amd.lib import DetZeroHipError
    cfg = centerpoint_1sweep_cfg((0.1, 0.1, 0.15))
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), SyntheticDatasetInfo(cfg))
    bb = model.backbone3d
    if 'DZ_TUNE_SPCONV_F32_ENGINE' not in os.environ:
        assert bb.f32_engine == 'gather'
    before = (bb.engine, bb.f32_engine)
    with pytest.raises(DetZeroHipError):
        set_sparse_engine(model, 'xrun', f32_engine='tiles')
    assert (bb.engine, bb.f32_engine) == before            # a refused call changes nothing
    set_sparse_engine(model, 'gather')                      # one-argument form: the fp32 engine is left alone
    assert (bb.engine, bb.f32_engine) == ('gather', before[1])
    set_sparse_engine(model, 'xrun', 'xrun')
    assert (bb.engine, bb.f32_engine) == ('xrun', 'xrun')
    set_sparse_engine(model, 'xrun', f32_engine='gather')
    assert (bb.engine, bb.f32_engine) == ('xrun', 'gather')
