"""CPU: the wave-private bf16x3 sparse convolution of the exact-fp32 mode's 16-channel layers (csrc/sparse_conv_wt.hip) as built - its
three entry points in the header, the library and the ctypes table, which layers it covers, the resources of its two kernels from
the compiler's resource report (taken as tests/test_spconv_gather_limb3_build.py does), and the backbone's switch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('dz_spconv_forward_limb3_w', 'dz_spconv_limb3_w_tile_rows', 'dz_spconv_limb3_w_variant')
# (cin, cout) -> instance name, waves per workgroup, slots per chunk (csrc/sparse_conv_wt.hip: WT_16_16, WT_16_32)
SHIPPED = {(16, 16): ('k_spconv_wt<16x16>', 4, 4), (16, 32): ('k_spconv_wt<16x32>', 12, 3)}
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope='module')
def lib():
    from detzero_amd import lib as L
    from detzero_amd.build import build
    build(verbose=False)
    return L.load()


def test_symbols_in_header_library_and_ctypes_table(lib):
    from detzero_amd import lib as L
    from detzero_amd.build import LIB
    header = open(os.path.join(ROOT, 'include', 'detzero_hip.h')).read()
    exported = subprocess.run(['nm', '-D', '--defined-only', LIB], capture_output=True, text=True, check=True).stdout
    table = open(L.__file__).read()
    for name in SYMBOLS:
        assert re.search(r'\b%s\(' % name, header), name
        assert re.search(r' T %s$' % name, exported, re.M), name
        assert "'%s':" % name in table and callable(getattr(lib, name)), name
    # the forward's prototype: dz_spconv_forward_limb3's arguments, then max_workgroups, then the stream
    proto = re.search(r'int dz_spconv_forward_limb3_w\(([^;]*)\);', header).group(1)
    base = re.search(r'int dz_spconv_forward_limb3\(([^;]*)\);', header).group(1)
    norm = lambda s: [' '.join(a.split()) for a in s.split(',')]           # noqa: E731
    assert norm(proto) == norm(base)[:-1] + ['int max_workgroups', 'void *stream']


def test_covered_layers(lib):
    for (cin, cout), (name, waves, _) in SHIPPED.items():
        assert lib.dz_spconv_limb3_w_variant(cin, cout).decode() == name
        assert lib.dz_spconv_limb3_w_tile_rows(cin, cout) == 32 * waves
    for cin, cout in ((32, 32), (16, 64), (48, 48), (32, 16), (64, 64), (128, 128)):
        assert lib.dz_spconv_limb3_w_variant(cin, cout) == b'none', (cin, cout)
        assert lib.dz_spconv_limb3_w_tile_rows(cin, cout) == 0, (cin, cout)


def test_kernels_have_no_scratch_and_fit_lds(tmp_path):
    """Both k_spconv_wt instances: 0 bytes of scratch, no spilled register, three waves per SIMD, static LDS within 160 KiB; the
    dynamic LDS of the launch (all 27 taps of limb weights, 24 bytes per lane, + scale / shift) is held to 160 KiB per CU by a
    static_assert of the file - compiling it is that check - and is restated here."""
    src = os.path.join(ROOT, 'detzero_amd', 'csrc', 'sparse_conv_wt.hip')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-c', src, '-o', str(tmp_path / 'wt.o'), '-Rpass-analysis=kernel-resource-usage']
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
    kernels = [k for k in kernels if 'k_spconv_wt' in k['name']]
    assert len(kernels) == len(SHIPPED), [k['name'] for k in kernels]
    for (cin, cout), (_, waves, g) in SHIPPED.items():
        hit = [k for k in kernels if 'k_spconv_wtILi%dELi%dELi%dE' % (cout, g, waves) in k['name']]
        assert len(hit) == 1, ((cin, cout), [k['name'] for k in kernels])
        k = hit[0]
        print(k)
        assert int(k['ScratchSize [bytes/lane]']) == 0 and int(k['VGPRs Spill']) == 0 and int(k['SGPRs Spill']) == 0, k
        assert int(k['Occupancy [waves/SIMD]']) >= 3, k
        assert int(k['LDS Size [bytes/block]']) <= LDS_LIMIT, k
        lds = 27 * (cout // 16) * 64 * 24 + 64 * 4
        per_cu = max(1, 12 // waves)
        assert lds <= LDS_LIMIT and per_cu * lds <= LDS_LIMIT, ((cin, cout), lds, per_cu)
        # the hand-counted load stream: indices + gathers + residual loads outstanding at a wait fit the 6-bit counter
        assert 2 * g + 2 * g + 2 * (cout // 16) <= 63
    txt = open(src).read()
    assert 'static_assert(LDS_BYTES <= 160 * 1024' in txt and 'static_assert(NI + NL + NR <= 63' in txt
    # 32 -> 32 would not fit: the reason it is out of this kernel's reach
    assert 27 * 32 * 32 * 6 > LDS_LIMIT


def test_fp32_small_switch():
    import torch
    from detzero_amd import ops
    from detzero_amd.centerpoint import SyntheticDatasetInfo, build_network, set_sparse_engine
    from detzero_amd.config import centerpoint_1sweep_cfg
    from detzero_amd.lib import DetZeroHipError
    assert ops.SPARSE_F32_SMALL_ENGINES == ('gather', 'wave_bf16x3')
    assert ops.SPARSE_F32_ENGINES == ('gather', 'xrun', 'xrun_bf16x3') and ops.SPARSE_F32_GATHER_ENGINES == ('mfma32', 'bf16x3')
    assert ops.SpconvRoute._fields == ('engine', 'weights', 'variant')
    cfg = centerpoint_1sweep_cfg((0.1, 0.1, 0.15))
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), SyntheticDatasetInfo(cfg))
    bb = model.backbone3d
    assert bb.f32_small == 'gather'                                         # the default, and no environment variable behind it
    before = (bb.engine, bb.f32_engine, bb.f32_gather, bb.f32_small)
    set_sparse_engine(model, 'xrun', f32_small='wave_bf16x3')
    assert (bb.engine, bb.f32_engine, bb.f32_gather, bb.f32_small) == ('xrun',) + before[1:3] + ('wave_bf16x3',)
    for bad in (dict(f32_small='bf16x3'), dict(f32_small='nonsense'), dict(f32_gather='nonsense', f32_small='gather')):
        with pytest.raises(DetZeroHipError):
            set_sparse_engine(model, 'gather', **bad)
        assert (bb.engine, bb.f32_small) == ('xrun', 'wave_bf16x3')          # a refused call changes nothing
    set_sparse_engine(model, 'gather', f32_engine='xrun_bf16x3', f32_gather='bf16x3')           # None leaves the switch alone
    assert (bb.engine, bb.f32_engine, bb.f32_gather, bb.f32_small) == ('gather', 'xrun_bf16x3', 'bf16x3', 'wave_bf16x3')
    bb.set_engine('xrun', f32_small='gather')
    assert bb.f32_small == 'gather'
    set_sparse_engine(model, before[0], f32_engine=before[1], f32_gather=before[2], f32_small=before[3])
    assert (bb.engine, bb.f32_engine, bb.f32_gather, bb.f32_small) == before
    src = ''.join(open(os.path.join(ROOT, 'detzero_amd', f)).read() for f in ('ops.py', 'det_modules.py', 'centerpoint.py'))
    assert 'F32_SMALL' not in re.sub(r'SPARSE_F32_SMALL_ENGINES', '', src)       # no DZ_TUNE_* knob for it
