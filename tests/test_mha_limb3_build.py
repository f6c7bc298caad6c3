"""CPU: the three-limb (bf16x3) engine of the f32 mode's attention core as built (csrc/mha_t.hip, dz_mha_core_limb3*) - what the entry
point takes and refuses (answered by host code), the resources of the two kernel instances from the compiler's resource report, the
symbols, the switch (_Cached.set_attention_engine) and its routing state, and the HOST EMULATION of the kernel's formula that
tests/test_gpu_mha_limb3.py compares the kernel with.

The emulation (`emulate`): q times scale * log2(e) in float32, every operand as the three bf16 limbs of ops.limb3_pack's rule
(round to nearest even, the clamp to +-bf16-max in front of the first rounding only); a product is the kernel's MFMA chain on ONE
float32 accumulator: k-steps of 16 ascending (channels for S, keys for P.V), per step the six terms of limb3_terms in order, each
term the exact sum of its 16 limb products added to the accumulator with one rounding to float32; p = exp2(s - max) in float32;
the result divided by the float32 sum of p.  It takes the maximum over the whole row where the kernel takes a running one (so it
never rescales the accumulator).

Numbers.  The rule of tests/test_gpu_refine_kernels.py for its ATT_BASE: the worst normalised error of the host evaluation against
float64 over the cases must stay within ATT_BASE['f32'] = 1.0e-5.  Measured here (test_emulation_stays_in_the_fp32_class prints
them): the 23 MHA_CASES and the EDGE_CASES below.  One case has its own allowance, EDGE_CASES[LONG_RISE] (64 queries x 1000 rising
keys): the float32 host evaluation of the SAME formula is itself above 1.0e-5 there (a 1000-term float32 sum behind a rescale in
every tile), so that case gets max(ATT_BASE['f32'], 1.25 x its float32 host baseline)."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from detzero_amd import ops
from oracle import refine as R
from tests.test_gpu_refine_kernels import ATT_BASE, MHA_CASES, attention_inputs, f32_baseline, mha_case, worst_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'detzero_amd', 'csrc', 'mha_t.hip')
HEADER = os.path.join(ROOT, 'include', 'detzero_hip.h')
F32 = np.float32


@pytest.fixture(scope='module')
def lib():
    from detzero_amd import lib as L
    from detzero_amd.build import build
    build(verbose=False)
    return L.load()


# ------------------------------------------------------------------------------------------------------------------------
# the edge table of the 32-key tile / 64-key block geometry (shared with tests/test_gpu_mha_limb3.py)
# ------------------------------------------------------------------------------------------------------------------------
#              b   lq   lk  heads family   mask
EDGE_CASES = [(2, 33, 31, 1, 'rise', None),              # lk just below a 32-key tile
              (1, 32, 32, 8, 'rise', 'rand'),            # lk exactly one tile
              (2, 31, 33, 1, 'spread', 'last'),          # lk just above a tile; one live key alone in the second tile
              (1, 65, 95, 8, 'fall', 'middle'),          # a third wave with one query; ragged second block
              (1, 40, 97, 1, 'rise', 'start'),           # the first 80 keys dead: a whole staged block while the maximum is still -inf
              (1, 64, 1000, 1, 'rise', 'rand'),          # 16 staged blocks, a rescale in every tile
              (3, 1, 1, 1, 'randn', None),               # one query, one key
              (1, 257, 70, 8, 'randn', 'rand')]          # second workgroup with one query
LONG_RISE = 5


def edge_id(c):
    return '-'.join(str(x) for x in c)


@functools.lru_cache(maxsize=None)
def edge_case(i):
    b, lq, lk, heads, family, mk = EDGE_CASES[i]
    q, k, v, mask = attention_inputs(7000 + i, b, lq, lk, heads, 32, family, mk)
    want, nat = R.attention(q, k, v, mask, heads, 32 ** -0.5)
    return {'q': q, 'k': k, 'v': v, 'mask': mask, 'heads': heads, 'scale': 32 ** -0.5, 'want': want, 'nat': nat}


def edge_allowance(i):
    """The allowance of an edge case on the HOST (the GPU test takes 8 x it, as ATT_BOUND is 8 x ATT_BASE)."""
    if i == LONG_RISE:
        return max(ATT_BASE['f32'], 1.25 * f32_baseline(edge_case(i)))
    return ATT_BASE['f32']


# ------------------------------------------------------------------------------------------------------------------------
# host emulation of k_mha_block_t's formula
# ------------------------------------------------------------------------------------------------------------------------
BF16_MAX = F32(3.3895313892515355e38)


def rn_bf16(x):
    """float32 -> the nearest bf16 (ties to even) as float32; NaN and inf stay."""
    x = np.ascontiguousarray(x, F32)
    u = x.view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(F32)
    return np.where(np.isfinite(x), r, x).astype(F32)


def limbs3(x):
    """ops.limb3_pack's rule: h = rn(clamp(x)), m = rn(x - h), l = rn(x - h - m), all bf16 values held in float32."""
    x = np.ascontiguousarray(x, F32)
    with np.errstate(invalid='ignore', over='ignore'):
        h = rn_bf16(np.clip(x, -BF16_MAX, BF16_MAX))
        r1 = (x - h).astype(F32)
        m = rn_bf16(r1)
        l = rn_bf16((r1 - m).astype(F32))
    return h, m, l


TERMS = [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)]          # limb3_terms: (A limb, B limb), smallest first


def limb3_product(a, b, spec, terms=TERMS):
    """The MFMA chain of one accumulator: A (..., m, k), B (..., n, k) as limbs; k in steps of 16, ascending; per step the terms in
    order, each term one MFMA = the exact sum of its 16 products added to the float32 accumulator and rounded to float32 once."""
    la, lb = [x.astype(np.float64) for x in limbs3(a)], [x.astype(np.float64) for x in limbs3(b)]
    acc = None
    for k0 in range(0, a.shape[-1], 16):
        for i, j in terms:
            t = np.einsum(spec, la[i][..., k0:k0 + 16], lb[j][..., k0:k0 + 16])
            acc = t.astype(F32) if acc is None else (acc.astype(np.float64) + t).astype(F32)
    return acc


def emulate(case, pv_terms=TERMS):
    """The kernel's formula on a case of mha_case / edge_case / sweep_case -> (b, lq, e) float32."""
    q, k, v, mask, heads = case['q'], case['k'], case['v'], case['mask'], case['heads']
    b, lq, e = q.shape
    lk = k.shape[1]
    sc2 = F32(F32(case['scale']) * F32(1.44269504088896340736))
    hs = lambda a, n: np.ascontiguousarray(a.reshape(b, n, heads, 32).transpose(0, 2, 1, 3))          # noqa: E731
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        qh = (hs(np.asarray(q, F32), lq) * sc2).astype(F32)
        s = limb3_product(hs(np.asarray(k, F32), lk), qh, 'bhkd,bhqd->bhqk')          # A = K, B = Q: S^T = K . Q^T
        if mask is not None:
            s = np.where(np.asarray(mask)[:, None, None, :] != 0, F32(-np.inf), s)
        m = s.max(-1, keepdims=True)
        p = np.exp2((s - m).astype(F32)).astype(F32)
        o = limb3_product(np.ascontiguousarray(hs(np.asarray(v, F32), lk).transpose(0, 1, 3, 2)), p, 'bhdk,bhqk->bhqd', pv_terms)          # A = V, B = P: O^T = V^T . P^T
        out = (o / p.sum(-1, keepdims=True, dtype=F32)).astype(F32)
    return out.transpose(0, 2, 1, 3).reshape(b, lq, e)


def emulation_error(case, pv_terms=TERMS):
    return worst_ratio(emulate(case, pv_terms), case['want'], case['nat'])


def test_limbs_of_the_emulation_are_limb3_packs():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(4096) * np.exp2(rng.integers(-140, 120, 4096))).astype(F32)
    x[:8] = [0.0, -0.0, 3.4028234663852886e38, -3.4028234663852886e38, 3.3895313892515355e38, 1e-45, -1e-40, 1.0]
    h, m, l = limbs3(x)
    packed = ops.limb3_pack(torch.from_numpy(x)).view(torch.bfloat16).reshape(-1, 3, 8).float().numpy()
    for mine, theirs in zip((h, m, l), (packed[:, 0], packed[:, 1], packed[:, 2])):
        assert np.array_equal(mine.reshape(-1, 8), theirs)                          # as values (a zero limb's sign is the packer's own)
    big = np.abs(x) >= F32(2.0 ** -109)               # all 24 bits at or above the smallest bf16 subnormal, 2^-133: +-fp32-max included
    assert big[2:5].all() and np.array_equal((h + (m + l))[big], x[big])
    assert (np.abs((h + (m + l)) - x)[~big] <= F32(2.0 ** -134)).all()             # below: limbs are bf16 subnormals, not flushed


def test_edge_table_reaches_each_named_edge():
    assert len(EDGE_CASES) == 8 and EDGE_CASES[LONG_RISE][:3] == (1, 64, 1000)
    lks = [c[2] for c in EDGE_CASES]
    assert {31, 32, 33} <= set(lks)                                                 # around one 32-key tile
    assert any(64 < lk < 128 and lk % 32 for lk in lks)                             # a ragged second block
    assert any(c[1] == 65 for c in EDGE_CASES)                                      # a third wave with one query
    assert any(c[1] == 257 for c in EDGE_CASES)                                     # a second workgroup ((257 + 31) / 32 = 9 waves) with one query
    assert (3, 1, 1, 1, 'randn', None) in EDGE_CASES
    m = edge_case(2)['mask']
    assert m is not None and (m[:, :32] == 1).all() and (m[:, 32] == 0).all()       # one live key, alone in the second tile
    m = edge_case(4)['mask']
    assert (m[:, :80] == 1).all() and not m[:, 80:].all()                           # the whole first staged block and half a tile dead
    assert (1000 + 63) // 64 == 16
    # "rise": in float64 the running maximum of every query rises in every 32-key tile that has a live key
    c = edge_case(LONG_RISE)
    s = np.einsum('qd,kd->qk', c['q'][0].astype(np.float64), c['k'][0].astype(np.float64))
    s = np.where(c['mask'][0][None] != 0, -np.inf, s)
    tmax = np.stack([s[:, t:t + 32].max(-1) for t in range(0, 1000, 32)], -1)
    assert (np.diff(tmax, axis=-1) > 0).all()
    assert {c[4] for c in EDGE_CASES} == {'rise', 'spread', 'fall', 'randn'} and {c[3] for c in EDGE_CASES} == {1, 8}


def test_emulation_stays_in_the_fp32_class():
    """The six-term formula, evaluated on the host, against float64: within ATT_BASE['f32'] on every MHA_CASES and edge case (the long
    rising case: its own allowance, see the module docstring).  With only the three largest terms in P.V it is not - which is why the
    kernel keeps six there."""
    fam, fam32, fam3 = {}, {}, {}
    top3 = TERMS[3:]
    for i, c in enumerate(MHA_CASES):
        d = mha_case(i)
        err = emulation_error(d)
        fam[c[5]] = max(fam.get(c[5], 0.0), err)
        fam32[c[5]] = max(fam32.get(c[5], 0.0), f32_baseline(d))
        fam3[c[5]] = max(fam3.get(c[5], 0.0), emulation_error(d, top3))
        assert err <= ATT_BASE['f32'], (c, err)
    fmt = lambda d: ', '.join('%s %.2e' % kv for kv in sorted(d.items()))          # noqa: E731
    print('  bf16x3 emulation, MHA_CASES by family:        %s -> worst %.2e (ATT_BASE %.2e)' % (fmt(fam), max(fam.values()), ATT_BASE['f32']))
    print('  float32 host baseline, same cases:            %s -> worst %.2e' % (fmt(fam32), max(fam32.values())))
    print('  emulation with three terms in P.V:            %s -> worst %.2e' % (fmt(fam3), max(fam3.values())))
    assert max(fam3.values()) > ATT_BASE['f32']
    for i, c in enumerate(EDGE_CASES):
        d = edge_case(i)
        err, base, allow = emulation_error(d), f32_baseline(d), edge_allowance(i)
        print('  edge %-28s emulation %.2e, float32 host %.2e, allowance %.2e' % (edge_id(c), err, base, allow))
        assert err <= allow, (c, err, allow)


# ------------------------------------------------------------------------------------------------------------------------
# the entry points, without a GPU
# ------------------------------------------------------------------------------------------------------------------------
#            batch  lq   lk  heads
ACCEPTED = [(96, 200, 9600, 8), (96, 200, 200, 8), (1, 1, 1, 1), (0, 5, 5, 1), (5, 0, 5, 1), (65535, 1, 1, 65535), (1, 1 << 20, 1 << 20, 1)]
REFUSED = [(1, 1, 0, 1), (-1, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 1, 0), (1, 1, 1, -8), (65536, 1, 1, 1), (1, 1, 1, 65536)]


def test_supported_and_refusals_answer_without_a_gpu(lib):
    """Every refusal is decided before any launch and before the pointers are looked at: the answers come without a device, in
    dz_mha_core's words."""
    p = 1 << 20
    call = lambda sizes, q=p, k=p, v=p, out=p: lib.dz_mha_core_limb3(q, k, v, None, *sizes, 0.25, out, None)          # noqa: E731
    for sizes in ACCEPTED:
        assert lib.dz_mha_core_limb3_supported(*sizes) == 1 and ops.mha_core_limb3_supported(*sizes), sizes
    for sizes in REFUSED:
        assert lib.dz_mha_core_limb3_supported(*sizes) == 0 and not ops.mha_core_limb3_supported(*sizes), sizes
        assert call(sizes) == -1 and lib.dz_last_error().decode() == 'dz_mha_core_limb3: bad sizes', sizes
    assert lib.dz_mha_core(p, p, p, None, 1, 1, 0, 1, 0.25, p, None) == -1 and lib.dz_last_error().decode() == 'dz_mha_core: bad sizes'
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(out=None)):
        assert call((2, 3, 4, 1), **kw) == -1 and lib.dz_last_error().decode() == 'dz_mha_core_limb3: null pointer', kw
    assert lib.dz_mha_core(None, p, p, None, 2, 3, 4, 1, 0.25, p, None) == -1 and lib.dz_last_error().decode() == 'dz_mha_core: null pointer'
    # no queries: no launch, no device needed - null pointers included, as dz_mha_core
    assert call((0, 3, 4, 1)) == 0 and call((2, 0, 4, 1)) == 0 and call((0, 3, 4, 1), q=None, out=None) == 0
    assert call((0, 3, 0, 1)) == -1                                    # ... but bad sizes come first


def test_symbols_match_the_header(lib):
    from detzero_amd import lib as L
    table = L.exported_symbols()
    hdr = re.sub(r'\s+', ' ', open(HEADER).read())
    c_int, c_float, c_void_p = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    ctype = {'int': c_int, 'float': c_float}
    args_of = {}
    for name in ('dz_mha_core_limb3', 'dz_mha_core_limb3_supported', 'dz_mha_core'):
        m = re.search(r'int %s\(([^)]*)\);' % name, hdr)
        assert m, name
        args_of[name] = [c_void_p if '*' in a else ctype[a.strip().split(' ')[0]] for a in m.group(1).split(',')]
        fn = getattr(lib, name)
        assert fn.restype is c_int and list(fn.argtypes) == args_of[name], (name, fn.argtypes, args_of[name])
        assert name in table
    assert args_of['dz_mha_core_limb3'] == args_of['dz_mha_core'] and len(args_of['dz_mha_core']) == 11           # dz_mha_core's argument list
    assert args_of['dz_mha_core_limb3_supported'] == [c_int] * 4
    nm = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True)
    assert nm.returncode == 0 and ' T dz_mha_core_limb3\n' in nm.stdout and ' T dz_mha_core_limb3_supported\n' in nm.stdout


def _resource_report(tmp_path):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-c', SRC, '-o', str(tmp_path / 'mt.o'),
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
    return [k for k in kernels if 'k_mha_block_t' in k['name']]


def test_kernels_have_no_scratch_and_fit_lds(tmp_path):
    """Two instances (masked, unmasked); each: 0 bytes of scratch, no spilled VGPR, at most 256 registers, static LDS within 80 KB
    (two workgroups per CU)."""
    kernels = _resource_report(tmp_path)
    assert sorted(re.search(r'k_mha_block_tILb([01])E', k['name']).group(1) for k in kernels) == ['0', '1'], [k['name'] for k in kernels]
    for k in kernels:
        print(k)
        assert int(k['ScratchSize [bytes/lane]']) == 0 and int(k['VGPRs Spill']) == 0, k
        assert int(k['VGPRs']) + int(k['AGPRs']) <= 256, k
        assert 0 < int(k['LDS Size [bytes/block]']) <= 80 * 1024, k


def test_source_takes_the_limb_arithmetic_from_limb3_h():
    """Included, not copied: the split and the term order come from limb3.h / hgemm.h; the file has one MFMA statement per product,
    both inside limb3_terms, and no second copy of the order."""
    txt = open(SRC).read()
    code = re.sub(r'//[^\n]*', '', txt)
    assert '#include "limb3.h"' in code and '#include "hgemm.h"' in open(os.path.join(ROOT, 'detzero_amd', 'csrc', 'limb3.h')).read()
    assert len(re.findall(r'limb3_terms\(\[&\]\(auto a, auto c\) \{ \w+ = MathBF16::mma\(', code)) == 2
    assert code.count('MathBF16::mma(') == 2 and code.count('limb3_terms(') == 2
    assert 'split3x8(' in code and 'split3x2(' in code
    for copied in ('integral_constant', 'term(', '__builtin_amdgcn_mfma', 'convertvector', 'fmed3'):
        assert copied not in code, copied


# ------------------------------------------------------------------------------------------------------------------------
# the switch
# ------------------------------------------------------------------------------------------------------------------------
def _crm():
    from detzero_amd.config import AttrDict
    from detzero_amd.refine_modules import ConfidencePointnet
    cfg = {'ENCODER_MLP': [128, 128], 'REGRESSION_MLP': [512], 'SCORE_THRESH': [0.35, 0.7]}
    return ConfidencePointnet(AttrDict(cfg), query_point_dims=32, memory_point_dims=32).eval()


def test_switch(lib):
    from detzero_amd import det_modules, refine_modules
    from detzero_amd.lib import DetZeroHipError
    from tests.test_refine import _models
    assert ops.ATTENTION_F32_ENGINES == ('mfma32', 'bf16x3')
    grm, prm = _models()
    mods = (grm, prm, _crm())
    assert all(m.f32_attention_engine == 'mfma32' for m in mods)                      # off by default
    gen = det_modules.CACHE_GEN[0]
    for m in mods:
        for bad in ('bf16x2', 'tiles', None):
            with pytest.raises(DetZeroHipError):
                m.set_attention_engine(bad)
    assert all(m.f32_attention_engine == 'mfma32' for m in mods) and det_modules.CACHE_GEN[0] == gen       # a bad name changes nothing
    assert prm.set_math('f32').set_linear_engine('bf16x3').set_attention_engine('bf16x3') is prm
    assert prm.f32_attention_engine == 'bf16x3' and prm.f32_linear_engine == 'bf16x3' and det_modules.CACHE_GEN[0] > gen
    gen = det_modules.CACHE_GEN[0]
    assert grm.set_attention_engine('bf16x3') is grm and grm.f32_linear_engine == 'mfma32' and det_modules.CACHE_GEN[0] > gen      # independent of the linear switch
    prm.set_linear_engine('mfma32')
    assert prm.f32_attention_engine == 'bf16x3'
    grm.load_state_dict(grm.state_dict())
    assert grm._plan is None and grm.f32_attention_engine == 'bf16x3'                 # the plan is gone, the switch stays
    assert grm.set_attention_engine('mfma32').f32_attention_engine == 'mfma32'
    assert 'DETZERO' not in ''.join(l for l in open(os.path.join(ROOT, 'detzero_amd', 'det_modules.py')) if 'attention_engine' in l)   # no environment knob
    # the engine reaches the helper the way the math and the linear engine do: set by the model's forward, restored behind it
    rm = refine_modules
    assert rm._REFINE_ATTN == ['mfma32']
    with rm._math_mode(0, 'mfma32', 'bf16x3'):
        assert rm._REFINE_ATTN == ['bf16x3'] and rm._REFINE_LINEAR == ['mfma32'] and rm._REFINE_MATH == [0]
        with rm._math_mode(1, 'bf16x3'):                                              # the two-argument call keeps working
            assert rm._REFINE_ATTN == ['mfma32'] and rm._REFINE_LINEAR == ['bf16x3'] and rm._REFINE_MATH == [1]
        assert rm._REFINE_ATTN == ['bf16x3']
    with pytest.raises(RuntimeError):
        with rm._math_mode(0, 'bf16x3', 'bf16x3'):
            raise RuntimeError('inside')
    assert rm._REFINE_ATTN == ['mfma32'] and rm._REFINE_LINEAR == ['mfma32'] and rm._REFINE_MATH == [0]
    assert isinstance(rm.LIMB3_ATTN_MIN_KEYS, int) and rm.LIMB3_ATTN_MIN_KEYS >= 0


def test_routing_predicate(lib, monkeypatch):
    from detzero_amd import refine_modules as rm
    monkeypatch.setattr(rm, 'LIMB3_ATTN_MIN_KEYS', 64)
    assert not rm._limb3_attn_ok(2, 200, 9600, 8)                                     # switch off
    with rm._math_mode(0, 'mfma32', 'bf16x3'):
        assert rm._limb3_attn_ok(2, 200, 9600, 8) and rm._limb3_attn_ok(2, 200, 64, 8)
        assert not rm._limb3_attn_ok(2, 200, 63, 8)                                   # below the threshold
        assert not rm._limb3_attn_ok(65536, 200, 9600, 8)                             # the engine's own limits
    for m in (1, 2):
        with rm._math_mode(m, 'mfma32', 'bf16x3'):
            assert not rm._limb3_attn_ok(2, 200, 9600, 8) and not rm._limb3_attn_ok(2, 200, 200, 8)      # the split modes ignore the switch
    with rm._math_mode(0, 'bf16x3'):
        assert not rm._limb3_attn_ok(2, 200, 9600, 8)                                 # the linear switch is another switch


def test_mha_core_refuses_unknown_engines_and_split_maths():
    from detzero_amd.lib import DetZeroHipError
    q = torch.zeros(1, 2, 32)
    for kw, word in ((dict(f32_engine='tiles'), 'unknown fp32 attention engine'), (dict(f32_engine='bf16x2'), 'unknown fp32 attention engine'),
                     (dict(math=1, f32_engine='bf16x3'), 'exact-fp32 mode'), (dict(math=2, f32_engine='bf16x3'), 'exact-fp32 mode')):
        with pytest.raises(DetZeroHipError, match=word):
            ops.mha_core(q, q, q, None, 1, 1.0, **kw)
