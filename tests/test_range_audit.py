"""CPU: the range audit's host side - calibration from group maxima, the new keywords and their defaults, the C ABI's two entry points,
and the numpy pair16 decoder the GPU tests use as their reference."""
import inspect
import os
import re

import numpy as np
import torch

from tests import range_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prescale_exponents_from_group_maxima():
    """A group's exponent puts the group's LARGEST tensor at or under the target peak: fed with maxima over all tensors of a group
    (report records) it is never above the exponent of the stage output alone."""
    from detzero_amd.centerpoint import F16_PAIR_TARGET_PEAK, PRESCALE_STAGES, group_peaks, prescale_exponents
    report = [{'name': 'a', 'stage': 'x_conv1', 'peak': 3.0}, {'name': 'b', 'stage': 'x_conv1', 'peak': 700.0},
              {'name': 'c', 'stage': 'spatial_features_2d', 'peak': 5.0}, {'name': 'd', 'stage': 'spatial_features_2d', 'peak': 5.0e6},
              {'name': 'e', 'stage': 'spatial_features_2d', 'peak': 40.0}, {'name': 'f', 'stage': None, 'peak': 1.0e9},
              {'name': 'g', 'stage': 'encoded', 'peak': 2.0 ** -20}]
    peaks = group_peaks(report)
    assert set(peaks) == set(PRESCALE_STAGES)
    assert peaks['x_conv1'] == 700.0 and peaks['spatial_features_2d'] == 5.0e6 and peaks['x_conv2'] == 0.0 and peaks['encoded'] == 2.0 ** -20
    exps = prescale_exponents(peaks)
    for k in PRESCALE_STAGES:
        if peaks[k] > 0:
            assert F16_PAIR_TARGET_PEAK / 2 < peaks[k] * 2.0 ** exps[k] <= F16_PAIR_TARGET_PEAK, (k, exps[k])
        else:
            assert exps[k] == 0
    assert exps['encoded'] == 31 and exps['x_conv1'] == 1 and exps['spatial_features_2d'] == -12
    stages_only = prescale_exponents({'x_conv1': 3.0, 'spatial_features_2d': 40.0, 'encoded': 2.0 ** -20})
    assert all(exps[k] <= stages_only[k] for k in PRESCALE_STAGES)


def test_probe_and_verify_keywords_and_defaults():
    from detzero_amd import centerpoint as cp
    sm = inspect.signature(cp.select_math).parameters
    ar = inspect.signature(cp.activation_range).parameters
    assert sm['probe'].default == 'stages' and sm['verify'].default is False
    assert ar['probe'].default == 'stages'
    ra = inspect.signature(cp.range_audit).parameters
    assert list(ra)[:3] == ['model', 'dataset_info', 'frames'] and ra['math'].default is None and ra['dynamic'].default is False
    assert inspect.signature(cp.FramePipeline.__init__).parameters['audit'].default is None
    assert callable(cp.FramePipeline.check_range) and callable(cp.FramePipeline.check_overflow)
    from detzero_amd import det_modules, range_audit
    assert det_modules.RangeAudit is range_audit.RangeAudit is cp.RangeAudit
    assert range_audit.active() is None
    audit = range_audit.RangeAudit()
    with audit.recording():
        assert range_audit.active() is audit
        with range_audit.RangeAudit().recording() as inner:
            assert range_audit.active() is inner
        assert range_audit.active() is audit
    assert range_audit.active() is None and audit.report() == []


def test_header_and_binding_table_have_the_entry_points():
    from detzero_amd import lib as L
    from detzero_amd import ops
    hdr = open(os.path.join(ROOT, 'include', 'detzero_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for sym in ('dz_range_probe', 'dz_range_reset'):
        assert re.search(r'\bint\s+%s\s*\(' % sym, code), sym
        assert sym in L.exported_symbols()
    assert len(L._SIGS['dz_range_probe'][1]) == 9 and len(L._SIGS['dz_range_reset'][1]) == 3
    for word in ('peak', 'saturated', 'nonfinite', 'elements', '0x7BFF'):      # the record layout is documented where it is declared
        assert word in hdr
    for fn in ('range_table', 'range_probe', 'range_reset', 'range_read'):
        assert callable(getattr(ops, fn))
    assert ops.RANGE_DTYPE.names == ('peak', 'saturated', 'nonfinite', 'elements')


def test_numpy_pair16_decoder_agrees_with_the_packer():
    """The reference decoder of the GPU tests reads the words ops.pair16_pack writes: same halves, same sums as ops.pair16_unpack."""
    from detzero_amd import ops
    x = torch.tensor([[0.0, -0.0, 1.0, -1.5, 65504.0, -65504.0, 1.0e-3, 3.14159274],
                      [1234.567, -0.333333343, 2.0 ** -14, 2.0 ** -24, 7.0e4, -1.0e5, 100.25, -2047.99],
                      [5.9604645e-08, 1.0e-8, -60000.0, 32768.0, 0.1, 0.2, 0.3, -0.7]], dtype=torch.float32)
    x = torch.cat([x, x.flip(1) * 0.5], dim=1)                    # 16 channels: two groups
    for storage in (rr.F16X2, rr.BF16X2):
        words = ops.pair16_pack(x, storage).numpy().view(np.uint32)
        hb, lb, hi, lo = rr.decode_pair16(words, storage)
        dt = torch.float16 if storage == rr.F16X2 else torch.bfloat16
        xc = x.clamp(-65504.0, 65504.0) if storage == rr.F16X2 else x
        want_hi = xc.to(dt)
        want_lo = (xc - want_hi.float()).to(dt)
        assert np.array_equal(hi, want_hi.float().numpy()) and np.array_equal(lo, want_lo.float().numpy())
        assert np.array_equal(hb, want_hi.view(torch.int16).numpy().view(np.uint16))
        assert np.array_equal(hi + lo, ops.pair16_unpack(torch.from_numpy(words.view(np.float32)), storage).numpy())
        assert np.array_equal(rr.encode_pair16(hb, lb), words)
        peak, sat, bad, n = rr.probe_reference(words, storage)
        assert n == x.numel() and bad == 0
        assert sat == (int((x.abs() >= 65504.0).sum()) if storage == rr.F16X2 else 0)
        assert peak == int(np.abs(hi + lo).max().view(np.uint32))
    # fp32 storage: non-finite elements are counted and kept out of the peak; -0.0 is 0
    w = np.array([[0.0, -0.0, np.inf, -np.inf, np.nan, -7.5, 3.0, 1.0]], np.float32).view(np.uint32)
    assert rr.probe_reference(w, rr.F32) == (int(np.float32(7.5).view(np.uint32)), 0, 3, 8)
    assert rr.probe_reference(w[:, :8] * 0, rr.F32) == (0, 0, 0, 8)
    assert rr.probe_reference(w, rr.F32, rows=0) == (0, 0, 0, 0)


def test_argument_checks_answer_without_a_gpu():
    """The entry points' argument checks are host code: a refused call returns the invalid-argument code before anything is launched,
    and an empty tensor is accepted without a launch."""
    import ctypes
    from detzero_amd import lib as L
    lib = L.load()
    slot = (ctypes.c_ulonglong * 4)()                        # (never dereferenced: every call below returns before a launch)
    x = (ctypes.c_float * 64)()
    ps, px = ctypes.addressof(slot), ctypes.addressof(x)

    def call(rows=1, stride=40, c_off=0, c=40, math=0, xp=px, sp=ps):
        return lib.dz_range_probe(xp, rows, None, stride, c_off, c, math, sp, None)
    assert call(c=12) == L.ERR_INVALID and call(c=0) == L.ERR_INVALID
    assert call(c_off=4, c=8) == L.ERR_INVALID
    assert call(c_off=8, c=40) == L.ERR_INVALID and call(c_off=40, c=8) == L.ERR_INVALID
    assert call(stride=42, c=40) == L.ERR_INVALID            # rows of 16-byte units
    assert call(math=4) == L.ERR_INVALID and b'unknown math 4' in lib.dz_last_error()
    assert call(rows=-1) == L.ERR_INVALID
    assert call(xp=None) == L.ERR_INVALID and call(sp=None) == L.ERR_INVALID
    assert call(rows=0, xp=None) == 0 and call(rows=0, c_off=8, c=24, math=3) == 0
    assert lib.dz_range_reset(None, 1, None) == L.ERR_INVALID and lib.dz_range_reset(None, -1, None) == L.ERR_INVALID
    assert lib.dz_range_reset(None, 0, None) == 0
    assert list(slot) == [0, 0, 0, 0]
