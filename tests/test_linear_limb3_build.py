"""CPU: the three-limb (bf16x3) engine of the f32 mode's linear layers as built (csrc/linear_t.hip, dz_linear_limb3_*) - which layers
the entry point covers and which instance runs them (answered by host code), the resources of the kernel instances from the compiler's
resource report, the symbols, and the switch (_Cached.set_linear_engine, centerpoint.set_linear_engine) with its cached limb weights."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from detzero_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'detzero_amd', 'csrc', 'linear_t.hip')
HEADER = os.path.join(ROOT, 'include', 'detzero_hip.h')


@pytest.fixture(scope='module')
def lib():
    from detzero_amd import lib as L
    from detzero_amd.build import build
    build(verbose=False)
    return L.load()


def _instance_names():
    """The names the selector can return: the kLT table of the source."""
    return sorted(set(re.findall(r'"(k_linear_t<\d+x\d+x\d+>)"', open(SRC).read())))


#            cin x_stride cout cout_pad y_stride
ACCEPTED = [((128, 128, 512, 512, 512), 'k_linear_t<128x128x16>'),            # GRM / PRM memory MLP (with the addend)
            ((128, 128, 128, 128, 128), 'k_linear_t<128x128x16>'),            # encoder layers 2 and 3
            ((512, 512, 256, 256, 256), 'k_linear_t<128x128x16>'),
            ((32, 32, 128, 128, 128), 'k_linear_t<128x128x16>'),              # PRM's first encoder layer
            ((256, 256, 256, 256, 256), 'k_linear_t<128x128x16>'),            # attention projections, the feed-forward block
            ((256, 256, 64, 64, 64), 'k_linear_t<128x64x32>'),                # the prediction heads' hidden layer
            ((64, 64, 3, 16, 3), 'k_linear_t<128x32x32>'),                    # ... and their output layers
            ((64, 64, 9, 16, 9), 'k_linear_t<128x32x32>'),
            ((64, 72, 19, 32, 24), 'k_linear_t<128x32x32>'),
            ((96, 128, 130, 192, 132), 'k_linear_t<128x64x32>'),
            ((192, 192, 192, 192, 192), 'k_linear_t<128x64x32>'),             # the PDV encoder layer's projections
            ((192, 192, 100, 128, 128), 'k_linear_t<128x128x16>'),
            ((32, 36, 48, 48, 50), 'k_linear_t<128x64x32>'),
            ((41472, 41472, 256, 256, 256), 'k_linear_t<128x128x16>')]
EXCLUDED = [(16, 16, 64, 64, 64), (48, 48, 64, 64, 64), (0, 0, 64, 64, 64),                                      # cin
            (64, 64, 24, 24, 24), (64, 64, 8, 8, 8), (64, 64, 0, 0, 0),                                           # cout_pad
            (64, 64, 65, 64, 65), (64, 64, 0, 64, 64),                                                            # cout
            (64, 60, 64, 64, 64), (64, 66, 64, 64, 64),                                                           # x_stride
            (64, 64, 64, 64, 63)]                                                                                 # y_stride


def test_supported_and_variant_answer_without_a_gpu(lib):
    reached = set()
    for sizes, name in ACCEPTED:
        cin, _, _, cout_pad, _ = sizes
        assert lib.dz_linear_limb3_supported(*sizes) == 1, sizes
        assert ops.linear_limb3_supported(*sizes), sizes
        assert lib.dz_linear_limb3_variant(cin, cout_pad).decode() == name, sizes
        reached.add(name)
    for sizes in EXCLUDED:
        assert lib.dz_linear_limb3_supported(*sizes) == 0, sizes
        assert not ops.linear_limb3_supported(*sizes), sizes
    for cin, cout_pad in [(16, 64), (48, 64), (0, 64), (64, 24), (64, 8), (64, 0)]:
        assert lib.dz_linear_limb3_variant(cin, cout_pad) == b'none', (cin, cout_pad)
    # weights at or beyond 2 GiB: round_up(cout_pad, 32) * cin * 6 bytes
    assert lib.dz_linear_limb3_supported(1 << 20, 1 << 20, 512, 512, 512) == 0 and lib.dz_linear_limb3_variant(1 << 20, 512) == b'none'
    # the table reaches every instance, and no instance exists that it cannot reach
    assert reached == set(_instance_names()) and len(reached) == 3, (sorted(reached), _instance_names())


def test_refusals_need_no_gpu(lib):
    """Every refusal is decided before any launch (and before the pointers are looked at): the answers come without a device."""
    fwd = lambda sizes, x=1 << 20, y=1 << 20, w=1 << 20, rows=5, mlr=0, gs=None, gr=0: lib.dz_linear_limb3_forward(     # noqa: E731
        x, rows, sizes[0], sizes[1], w, sizes[2], sizes[3], None, None, gs, gr, 0, y, sizes[4], mlr, None)
    for sizes, word in zip(EXCLUDED, ['cin (a'] * 3 + ['cout_pad (a'] * 3 + ['cout (1'] * 2 + ['x_stride (at'] * 2 + ['y_stride (at']):
        assert fwd(sizes) == -4 and word in lib.dz_last_error().decode(), sizes
    ok = (64, 64, 64, 64, 64)
    for kw, word in [(dict(x=None), 'null'), (dict(y=None), 'null'), (dict(w=None), 'null'), (dict(rows=-1), 'rows'), (dict(mlr=-1), 'max_launch_rows')]:
        assert fwd(ok, **kw) == -1 and word in lib.dz_last_error().decode(), kw
    assert fwd(ok, mlr=36, gs=1 << 20, gr=37) == -4 and 'max_launch_rows' in lib.dz_last_error().decode()
    assert fwd((64, 1 << 24, 64, 64, 64), gs=1 << 20, gr=37) == -4 and 'window' in lib.dz_last_error().decode()
    assert fwd(ok, rows=0) == 0                               # no rows: no launch, no device needed


def _resource_report(tmp_path):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-c', SRC, '-o', str(tmp_path / 'lt.o'),
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
    return [k for k in kernels if 'k_linear_t' in k['name']]


def test_kernels_have_no_scratch_and_fit_lds(tmp_path):
    """As many instances as the selector has names; each: 0 bytes of scratch, no spilled VGPR, at most 256 registers (two waves per
    SIMD = two 256-thread workgroups per CU); the dynamic LDS of a launch is the tile's LDS_BYTES, restated here from the tile in the
    instance's name and held to two workgroups per CU."""
    names = _instance_names()
    kernels = _resource_report(tmp_path)
    assert len(kernels) == len(names) == 3, ([k['name'] for k in kernels], names)
    for k in kernels:
        print(k)
        assert int(k['ScratchSize [bytes/lane]']) == 0 and int(k['VGPRs Spill']) == 0, k
        assert int(k['LDS Size [bytes/block]']) <= 80 * 1024, k
        assert int(k['VGPRs']) + int(k['AGPRs']) <= 256, k
    txt = open(SRC).read()
    assert '"two workgroups per CU"' in txt and 'Limb3Tile<BP, BC, KC, WP, WC>' in txt            # the shared tile, not a copy
    for n in names:
        bp, bc, kc = (int(v) for v in re.match(r'k_linear_t<(\d+)x(\d+)x(\d+)>', n).groups())
        rowb = kc // 8 * 48 + 16
        assert (rowb // 16) % 2 == 1, n
        lds = 2 * (bp + bc) * rowb
        assert 2 * lds <= 160 * 1024, (n, lds)                          # two workgroups per CU
        assert any('Li%dELi%dELi%dE' % (bp, bc, kc) in k['name'] for k in kernels), n


def test_symbols_match_the_header(lib):
    from detzero_amd import lib as L
    table = L.exported_symbols()
    hdr = re.sub(r'\s+', ' ', open(HEADER).read())
    c_int, c_long, c_void_p, c_char_p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p, ctypes.c_char_p
    ctype = {'int': c_int, 'long': c_long}
    for name, ret in (('dz_linear_limb3_forward', c_int), ('dz_linear_limb3_supported', c_int), ('dz_linear_limb3_variant', c_char_p)):
        m = re.search(r'(int|const char \*) ?%s\(([^)]*)\);' % name, hdr)
        assert m, name
        args = [c_void_p if '*' in a else ctype[a.strip().split(' ')[0]] for a in m.group(2).split(',')]
        fn = getattr(lib, name)
        assert fn.restype is ret and list(fn.argtypes) == args, (name, fn.argtypes, args)
        assert name in table
    assert len(lib.dz_linear_limb3_forward.argtypes) == 16


def test_switch_and_cached_limb_weights(lib):
    from detzero_amd import det_modules, refine_modules
    from detzero_amd.centerpoint import set_linear_engine
    from detzero_amd.lib import DetZeroHipError
    from tests.test_pdv import _head
    from tests.test_refine import _models
    assert ops.LINEAR_F32_ENGINES == ('mfma32', 'bf16x3')
    grm, prm = _models()
    head = _head()
    mods = (grm, prm, head)
    assert all(m.f32_linear_engine == 'mfma32' for m in mods)                        # off by default
    gen = det_modules.CACHE_GEN[0]
    for m in mods:
        with pytest.raises(DetZeroHipError):
            m.set_linear_engine('bf16x2')
    with pytest.raises(DetZeroHipError):
        set_linear_engine(head, 'tiles')
    assert all(m.f32_linear_engine == 'mfma32' for m in mods) and det_modules.CACHE_GEN[0] == gen       # a bad name changes nothing
    assert grm.set_math('f32').set_linear_engine('bf16x3') is grm and grm.f32_linear_engine == 'bf16x3'
    assert det_modules.CACHE_GEN[0] > gen
    gen = det_modules.CACHE_GEN[0]

    class Det(torch.nn.Module):                     # a detector with a second stage: the switch reaches the module that runs linears
        def __init__(self):
            super().__init__()
            self.roi_head = head
    assert isinstance(set_linear_engine(Det(), 'bf16x3'), Det) and head.f32_linear_engine == 'bf16x3' and det_modules.CACHE_GEN[0] > gen
    with pytest.raises(DetZeroHipError):
        ops.linear(torch.zeros(1, 32), torch.zeros(32, 16), None, None, False, 16, f32_engine='tiles')
    # the limb weights: packed once per layer, cached beside the fp32 ones in the plan entry, dropped with the plan
    layer = grm.plan()['memory'].mlp[0]
    x = torch.zeros(4, layer['w'].shape[0])
    assert refine_modules._limb3_ok(x, layer['w'], layer['cout'], 0, 'bf16x3')
    assert not refine_modules._limb3_ok(x, layer['w'], layer['cout'], 0, 'mfma32')
    for m in (1, 2):
        assert not refine_modules._limb3_ok(x, layer['w'], layer['cout'], m, 'bf16x3')           # split modes ignore the switch
    assert not refine_modules._limb3_ok(torch.zeros(4, 16), torch.zeros(16, 128), 128, 0, 'bf16x3')  # a 16-column input: cin % 32 != 0
    assert 'w_limb3' not in layer
    wl = refine_modules._limb_w(layer)
    assert refine_modules._limb_w(layer) is wl and layer['w_limb3'] is wl
    cin, cp = layer['w'].shape
    assert wl.shape == (1, (cp + 31) // 32 * 32, cin * 3 // 2)
    assert torch.equal(ops.limb3_unpack(wl)[0, :cp].view(torch.int32), layer['w'].t().contiguous().view(torch.int32))
    plan = grm._plan
    grm.load_state_dict(grm.state_dict())
    assert grm._plan is None and grm.f32_linear_engine == 'bf16x3'                  # the plan (and the limb weights in it) is gone, the switch stays
    assert 'w_limb3' not in grm.plan()['memory'].mlp[0] and grm.plan() is not plan
    # the engine reaches the helper the way the math does: set by the model's forward, restored behind it
    assert refine_modules._REFINE_LINEAR == ['mfma32']
    with refine_modules._math_mode(0, 'bf16x3'):
        assert refine_modules._REFINE_LINEAR == ['bf16x3'] and refine_modules._REFINE_MATH == [0]
    assert refine_modules._REFINE_LINEAR == ['mfma32']
