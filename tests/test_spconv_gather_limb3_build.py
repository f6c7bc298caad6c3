"""CPU: the bf16x3 gather-path sparse convolution of the exact-fp32 mode (csrc/sparse_conv_gt.hip) as built - which layers it covers,
the resources of its kernels from the compiler's resource report (taken as tests/test_xrun_limb3_build.py does), the arithmetic
switch of the backbone, and the limb layout of its (non-square, padded) weights."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the layers the selector offers and their instances (a layer ships only where it beat k_spconv in both rounds)
SHIPPED = {(16, 16): 'k_spconv_gt<128x32x16>', (16, 32): 'k_spconv_gt<128x32x16>', (32, 32): 'k_spconv_gt<128x32x32>',
           (32, 64): 'k_spconv_gt<128x64x32>', (64, 64): 'k_spconv_gt<128x64x32>', (64, 128): 'k_spconv_gt<128x128x16>',
           (128, 128): 'k_spconv_gt<128x128x16>'}
BACKBONE_LAYERS = ((16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128))


@pytest.fixture(scope='module')
def lib():
    from detzero_amd import lib as L
    from detzero_amd.build import build
    build(verbose=False)
    return L.load()


def test_covered_layers(lib):
    for cin, cout in BACKBONE_LAYERS:
        name, rows = lib.dz_spconv_limb3_variant(cin, cout).decode(), lib.dz_spconv_limb3_tile_rows(cin, cout)
        assert name == SHIPPED.get((cin, cout), 'none'), (cin, cout, name)
        assert (rows > 0) == ((cin, cout) in SHIPPED), (cin, cout, rows)
        if rows:
            # the first template number is the row tile, a whole number of the table's 32-row tile masks
            assert rows == int(name[name.index('<') + 1:].split('x')[0]) and rows % 32 == 0
    for cin, cout in ((48, 48), (256, 256), (32, 16), (128, 64), (16, 64)):
        assert lib.dz_spconv_limb3_variant(cin, cout) == b'none', (cin, cout)
        assert lib.dz_spconv_limb3_tile_rows(cin, cout) == 0, (cin, cout)


def test_kernels_have_no_scratch_and_fit_lds(tmp_path):
    """Every k_spconv_gt instance: 0 bytes of scratch, no spilled register, static LDS within 160 KiB (the dynamic LDS of the launch is
    GTile::LDS_BYTES, held to 160 KiB by a static_assert of the file: compiling it is that check)."""
    src = os.path.join(ROOT, 'detzero_amd', 'csrc', 'sparse_conv_gt.hip')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-c', src, '-o', str(tmp_path / 'gt.o'), '-Rpass-analysis=kernel-resource-usage']
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
    kernels = [k for k in kernels if 'k_spconv_gt' in k['name']]
    tiles = sorted({tuple(int(v) for v in n[n.index('<') + 1:-1].split('x')) for n in SHIPPED.values()})
    assert len(kernels) == len(tiles), [k['name'] for k in kernels]
    for bp, bc, kc in tiles:
        assert sum('GTileILi%dELi%dELi%dE' % (bp, bc, kc) in k['name'] for k in kernels) == 1, ((bp, bc, kc), [k['name'] for k in kernels])
    for k in kernels:
        print(k)
        assert int(k['ScratchSize [bytes/lane]']) == 0 and int(k['VGPRs Spill']) == 0 and int(k['SGPRs Spill']) == 0, k
        assert int(k['LDS Size [bytes/block]']) <= 160 * 1024, k
    txt = open(os.path.join(os.path.dirname(src), 'limb3.h')).read()           # the tile GTile derives from
    assert 'static_assert(LDS_BYTES <= 160 * 1024' in txt
    # rows of KC / 8 limb groups + 16 bytes: the dynamic LDS of each instance, restated
    for bp, bc, kc in tiles:
        assert 2 * (bp + bc) * (kc // 8 * 48 + 16) <= 160 * 1024, (bp, bc, kc)


def test_fp32_gather_switch():
    import torch
    from detzero_amd import ops
    from detzero_amd.centerpoint import SyntheticDatasetInfo, build_network, set_sparse_engine
    from detzero_amd.config import centerpoint_1sweep_cfg
    from detzero_amd.lib import DetZeroHipError
    assert ops.SPARSE_F32_ENGINES == ('gather', 'xrun', 'xrun_bf16x3')
    assert ops.SPARSE_F32_GATHER_ENGINES == ('mfma32', 'bf16x3')
    cfg = centerpoint_1sweep_cfg((0.1, 0.1, 0.15))
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), SyntheticDatasetInfo(cfg))
    bb = model.backbone3d
    if 'DZ_TUNE_SPCONV_F32_GATHER' not in os.environ:
        assert bb.f32_gather == 'mfma32'
    before = (bb.engine, bb.f32_engine, bb.f32_gather)
    set_sparse_engine(model, 'xrun', f32_engine='xrun_bf16x3', f32_gather='bf16x3')
    assert (bb.engine, bb.f32_engine, bb.f32_gather) == ('xrun', 'xrun_bf16x3', 'bf16x3')
    for bad in (dict(f32_gather='xrun'), dict(f32_engine='gather', f32_gather='nonsense'), dict(f32_engine='tiles', f32_gather='mfma32')):
        with pytest.raises(DetZeroHipError):
            set_sparse_engine(model, 'gather', **bad)
        assert (bb.engine, bb.f32_engine, bb.f32_gather) == ('xrun', 'xrun_bf16x3', 'bf16x3')           # a refused call changes nothing
    set_sparse_engine(model, 'gather')                                      # None leaves both fp32 switches alone
    assert (bb.engine, bb.f32_engine, bb.f32_gather) == ('gather', 'xrun_bf16x3', 'bf16x3')
    set_sparse_engine(model, 'gather', f32_engine='gather')
    assert (bb.f32_engine, bb.f32_gather) == ('gather', 'bf16x3')
    bb.set_engine('xrun', f32_gather='mfma32')
    assert (bb.engine, bb.f32_engine, bb.f32_gather) == ('xrun', 'gather', 'mfma32')
    set_sparse_engine(model, before[0], f32_engine=before[1], f32_gather=before[2])
    assert (bb.engine, bb.f32_engine, bb.f32_gather) == before


@pytest.mark.parametrize('cin,cout,kvol', ((16, 16, 27), (16, 32, 27), (32, 64, 27), (64, 128, 27), (128, 128, 3)))
def test_weight_limb_layout(cin, cout, kvol):
    """(kvol, cin, cout) -> (kvol, max(cout, 32), cin * 3 / 2) words: per tap, output channel and group of 8 input channels 16 B of h, 16
    of m, 16 of l; rows at or beyond cout are zero; unpacked, the transposed weights come back bit for bit."""
    import torch
    from detzero_amd import ops
    g = torch.Generator().manual_seed(1000 * cin + cout)
    w = torch.randn((kvol, cin, cout), generator=g) * torch.exp2(torch.randint(-40, 17, (kvol, cin, cout), generator=g).float())
    p = ops.pack_weight_limb3(w, cout_mult=32)
    cp = max(cout, 32)
    assert tuple(p.shape) == (kvol, cp, cin * 3 // 2) and p.dtype == torch.float32 and p.is_contiguous()
    back = ops.limb3_unpack(p)
    assert torch.equal(back[:, :cout].contiguous().view(torch.int32), w.transpose(1, 2).contiguous().view(torch.int32))
    assert not bool(p[:, cout:].view(torch.int32).any())
    # the group layout the kernel's A operand reads: words [12 g, 12 g + 4) are the h limbs of input channels 8 g .. 8 g + 7, the next
    # four the m limbs, the last four the l limbs
    limbs = p.view(torch.bfloat16).reshape(kvol, cp, cin // 8, 3, 8)[:, :cout]
    h = limbs[..., 0, :].reshape(kvol, cout, cin)
    assert torch.equal(h, w.transpose(1, 2).to(torch.bfloat16))
    total = limbs.float()
    assert torch.equal((total[..., 0, :] + (total[..., 1, :] + total[..., 2, :])).reshape(kvol, cout, cin), w.transpose(1, 2))
