"""GPU (MI355X): the range probe kernel alone (csrc/range_probe.hip) against a numpy reference computed from the stored bits
(tests/range_ref.py: for pairs np.float32(hi) + np.float32(lo)).  The peak must be BIT-equal, the three counters exactly equal."""
import numpy as np
import pytest
import torch

from tests import range_ref as rr

pytestmark = pytest.mark.gpu
STORAGES = [('f32', rr.F32), ('f16x2', rr.F16X2), ('bf16x2', rr.BF16X2)]
STRIDE = 40            # words per row of the sliced cases
INF32, NAN32 = 0x7F800000, 0x7FC00001
EXP16 = {rr.F16X2: 0x7C00, rr.BF16X2: 0x7F80}          # all-ones exponent of a 16-bit half
SAT16 = 0x7BFF                                          # fp16 65504


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def _words(device, x, storage):
    """fp32 values (R, C) -> the stored words (R, C) uint32 of `storage`, converted on the device for pairs."""
    from detzero_amd import ops
    if storage == rr.F32:
        return np.ascontiguousarray(x, np.float32).view(np.uint32).copy()
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(device)
    return ops.pair16_from_f32(t, x.shape[1], storage).cpu().numpy().view(np.uint32).copy()


def _data(seed, rows, c):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, c)) * np.exp(rng.uniform(-12, 9, (rows, c)))).astype(np.float32)


def _poison(words, storage, cols=None, rows=None):
    """Overwrite columns (or rows) with what must NOT be counted when they lie outside the probed region: saturated / inf / NaN."""
    sel = (slice(None), cols) if cols is not None else (rows, slice(None))
    if storage == rr.F32:
        pat = np.array([INF32, _bits(65504.0), NAN32, INF32 | 0x80000000], np.uint32)
    else:
        e = EXP16[storage]
        pat = np.array([SAT16 | (SAT16 << 16), e | (e << 16), (e | 1) | (0xFBFF << 16), 0x7BFF | ((e | 0x8000) << 16)], np.uint32)
    region = words[sel]
    words[sel] = np.resize(pat, region.size).reshape(region.shape)


def _upload(device, words):
    return torch.from_numpy(words.view(np.float32).copy()).to(device)


def _read(table):
    """-> list of (peak bits, saturated, nonfinite, elements) per slot, raw from the device words."""
    raw = table.cpu().numpy().view(np.uint64)
    return [(int(r[0]), int(r[1]), int(r[2]), int(r[3])) for r in raw]


def _probe_one(device, words, storage, **kw):
    from detzero_amd import ops
    table = ops.range_table(3, device)
    ops.range_probe(_upload(device, words), table[1], math=storage, **kw)
    got = _read(table)
    assert got[0] == (0, 0, 0, 0) and got[2] == (0, 0, 0, 0)          # neighbouring slots untouched
    rec = ops.range_read(table)[1]
    assert int(np.float32(rec['peak']).view(np.uint32)) == got[1][0] and int(rec['elements']) == got[1][3]      # range_read decodes the same words
    return got[1]


@pytest.mark.parametrize('name,storage', STORAGES)
@pytest.mark.parametrize('rows', [0, 1, 63, 64, 65, 1000])
@pytest.mark.parametrize('c', [8, 16, 24])
def test_slice_of_wider_rows(device, name, storage, rows, c):
    """A channel slice at c_off = 8 of 40-word rows; everything outside the slice is saturated / inf / NaN poison."""
    words = _words(device, _data(rows * 31 + c + storage, max(rows, 1), STRIDE), storage)[:rows]
    outside = np.ones(STRIDE, bool)
    outside[8:8 + c] = False
    if rows:
        _poison(words, storage, cols=outside)
    want = rr.probe_reference(words, storage, c_off=8, c=c)
    assert want[1] == 0 and want[2] == 0 and want[3] == rows * c and (want[0] > 0) == (rows > 0)
    assert _probe_one(device, words.reshape(rows, STRIDE), storage, c_off=8, c=c) == want


@pytest.mark.parametrize('name,storage', STORAGES)
@pytest.mark.parametrize('d_rows', [None, 0, 1, 137, 300, 301, 100000])
def test_device_row_count(device, name, storage, d_rows):
    """d_rows below the capacity (the rows past it are poison), equal, above (clamps to the capacity) and NULL."""
    cap, c = 300, 16
    words = _words(device, _data(7 + storage, cap, c), storage)
    n = cap if d_rows is None else min(d_rows, cap)
    if n < cap:
        _poison(words, storage, rows=slice(n, cap))
    want = rr.probe_reference(words, storage, rows=n)
    assert want[1] == 0 and want[2] == 0 and want[3] == n * c
    d = None if d_rows is None else torch.tensor([d_rows], dtype=torch.int32, device=device)
    assert _probe_one(device, words, storage, d_rows=d) == want
    if d_rows == 137:          # the host-side row limit reads the same rows
        assert _probe_one(device, words, storage, rows=137) == want


def _pair_case(storage, rows, c, where, hi, lo):
    """All-small background with one planted (hi, lo) bit pattern at element `where` = (row, channel)."""
    hb = np.zeros((rows, c), np.uint16)
    lb = np.zeros((rows, c), np.uint16)
    hb[:] = 0x2E66 if storage == rr.F16X2 else 0x3DCC            # ~0.1
    hb[::2] |= 0x8000
    hb[where], lb[where] = hi, lo
    return rr.encode_pair16(hb, lb)


@pytest.mark.parametrize('name,storage', STORAGES)
@pytest.mark.parametrize('where', ['first', 'last'])
@pytest.mark.parametrize('kind', ['plain', 'negative', 'hi_zero', 'lo_adds'])
def test_where_the_peak_sits(device, name, storage, where, kind):
    rows, c = 333, 24
    at = (0, 0) if where == 'first' else (rows - 1, c - 1)
    if storage == rr.F32:
        x = np.full((rows, c), 0.1, np.float32)
        x[::2] *= -1
        val = {'plain': 123.456, 'negative': -987.25, 'hi_zero': 2.5e-3 + 1.0, 'lo_adds': 4097.0}[kind]
        x[at] = val
        words = x.view(np.uint32).copy()
        expect = _bits(abs(np.float32(val)))
    else:
        h16 = (lambda v: int(np.float16(v).view(np.uint16))) if storage == rr.F16X2 else (lambda v: _bits(v) >> 16)
        hi, lo = {'plain': (h16(96.0), h16(0.03125)), 'negative': (h16(-512.0), h16(-0.25)), 'hi_zero': (0x8000, h16(7.0)),
                  'lo_adds': (h16(1024.0), h16(0.5))}[kind]
        words = _pair_case(storage, rows, c, at, hi, lo)
        expect = _bits({'plain': 96.03125, 'negative': 512.25, 'hi_zero': 7.0, 'lo_adds': 1024.5}[kind])
        if kind == 'lo_adds':
            assert expect > _bits(1024.0)                    # |hi + lo| > |hi|
    want = rr.probe_reference(words, storage)
    assert want == (expect, 0, 0, rows * c)
    assert _probe_one(device, words, storage) == want


@pytest.mark.parametrize('name,storage', STORAGES)
def test_zeros_of_either_sign_give_peak_zero(device, name, storage):
    x = np.zeros((65, 16), np.float32)
    x[::2] = -0.0
    words = _words(device, x, storage)
    assert (words != 0).any()                                 # the -0.0 bits are there
    assert _probe_one(device, words, storage) == (0, 0, 0, 65 * 16)


def test_saturated_pairs_are_counted(device):
    """fp16 pairs whose hi is +-65504 (0x7BFF) whatever lo holds - the clamp of split / split2, produced here by the device conversion
    itself and by patched bits; 0x7BFE is not a marker; bf16 pairs holding the same bits never report saturation."""
    from detzero_amd import ops
    x = _data(3, 200, 16)
    x[np.abs(x) >= 60000.0] = 1.0
    x[5, 3], x[6, 4], x[7, 15], x[199, 0] = 70000.0, -1.0e9, 65504.0, -65504.0         # what the clamp leaves: 4 saturated elements
    words = _words(device, x, rr.F16X2)
    hb, lb, _, _ = rr.decode_pair16(words, rr.F16X2)
    assert sorted(map(tuple, np.argwhere((hb & 0x7FFF) == SAT16))) == [(5, 3), (6, 4), (7, 15), (199, 0)]
    hb[10, 0], lb[10, 0] = 0x7BFF, 0x1234                    # (65504, anything)
    hb[11, 1], lb[11, 1] = 0xFBFF, 0xFBFF                    # (-65504, -65504)
    hb[12, 2], lb[12, 2] = 0x7BFE, 0x0000                    # 65472: not saturated
    hb[13, 3], lb[13, 3] = 0xFBFE, 0x7BFF                    # lo = 65504 does not make a marker
    words = rr.encode_pair16(hb, lb)
    want = rr.probe_reference(words, rr.F16X2)
    assert want[1] == 6 and want[2] == 0 and want[0] == _bits(65504.0 * 2)
    assert _probe_one(device, words, rr.F16X2) == want
    # the same words read as bf16 pairs: finite, large, never `saturated`
    want_b = rr.probe_reference(words, rr.BF16X2)
    assert want_b[1] == 0
    assert _probe_one(device, words, rr.BF16X2) == want_b
    # 'f16' math is stored as fp16 pairs
    table = ops.range_table(1, device)
    ops.range_probe(_upload(device, words), table[0], math='f16')
    assert _read(table)[0] == want


@pytest.mark.parametrize('name,storage', STORAGES)
def test_nonfinite_elements_are_counted_and_left_out_of_the_peak(device, name, storage):
    rows, c = 130, 16
    words = _words(device, np.clip(_data(11 + storage, rows, c), -100.0, 100.0), storage)
    if storage == rr.F32:
        for k, (r, ch, b) in enumerate([(0, 0, INF32), (1, 5, INF32 | 0x80000000), (64, 15, NAN32), (129, 15, NAN32 | 0x80000000),
                                        (77, 8, 0x7F800001)]):
            words[r, ch] = b
        n_bad = 5
    else:
        hb, lb, _, _ = rr.decode_pair16(words, storage)
        e = EXP16[storage]
        hb[0, 0] = e                          # hi = inf
        hb[1, 5] = e | 0x8000                 # hi = -inf
        lb[64, 15] = e                        # lo = inf, hi finite
        lb[129, 15] = e | 0x8001              # lo = NaN
        hb[77, 8], lb[77, 8] = e | 0x0200, e  # both
        hb[78, 9] = e - 1                     # largest exponent below all-ones with a zero mantissa field: finite
        words = rr.encode_pair16(hb, lb)
        n_bad = 5
    want = rr.probe_reference(words, storage)
    assert want[2] == n_bad and want[3] == rows * c and 0 < want[0] < INF32
    assert _probe_one(device, words, storage) == want
    # a tensor of non-finite elements only: peak 0
    allbad = np.full((3, 8), INF32, np.uint32) if storage == rr.F32 else rr.encode_pair16(np.full((3, 8), EXP16[storage], np.uint16), np.zeros((3, 8), np.uint16))
    assert _probe_one(device, allbad, storage) == (0, 0, 24, 24)


def test_slots_accumulate_and_reset_clears_exactly_its_records(device):
    from detzero_amd import ops
    a = _words(device, np.clip(_data(1, 100, 16), -50, 50), rr.F16X2)
    b = _words(device, np.clip(_data(2, 77, 8), -5000, 5000), rr.F16X2)
    ha, la, _, _ = rr.decode_pair16(a, rr.F16X2)
    ha[3, 3] = SAT16
    ha[4, 4] = 0x7C00
    a = rr.encode_pair16(ha, la)
    hb_, lb_, _, _ = rr.decode_pair16(b, rr.F16X2)
    hb_[0, 0] = hb_[76, 7] = 0xFBFF
    lb_[5, 5] = 0x7E00
    b = rr.encode_pair16(hb_, lb_)
    wa, wb = rr.probe_reference(a, rr.F16X2), rr.probe_reference(b, rr.F16X2)
    assert wa[1:3] == (1, 1) and wb[1:3] == (2, 1)
    table = ops.range_table(5, device)
    ta, tb = _upload(device, a), _upload(device, b)
    ops.range_probe(ta, table[2], math=1)
    ops.range_probe(tb, table[2], math=1)
    ops.range_probe(tb, table[3], math=1)
    ops.range_probe(ta, table[1], math=1)
    both = (max(wa[0], wb[0]), wa[1] + wb[1], wa[2] + wb[2], wa[3] + wb[3])
    assert _read(table) == [(0, 0, 0, 0), wa, both, wb, (0, 0, 0, 0)]
    ops.range_probe(ta, table[0], math=1)
    ops.range_probe(ta, table[4], math=1)
    ops.range_reset(table[1:3])                              # exactly two records
    assert _read(table) == [wa, (0, 0, 0, 0), (0, 0, 0, 0), wb, wa]
    ops.range_reset(table)
    assert _read(table) == [(0, 0, 0, 0)] * 5


def test_two_streams_into_one_slot(device):
    """The concurrent sub-passes of a split batch probe the same record from two streams: max and sums of both."""
    from detzero_amd import ops
    xa, xb = _data(21, 40000, 64), _data(22, 30000, 64)
    xa[np.abs(xa) > 6.0e4] = 2.0
    xb[np.abs(xb) > 6.0e4] = 2.0
    xa[123, 7] = 1.0e6
    xb[29999, 63] = -1.0e7
    xb[5, 5] = 66000.0
    a, b = _words(device, xa, rr.F16X2), _words(device, xb, rr.F16X2)
    wa, wb = rr.probe_reference(a, rr.F16X2), rr.probe_reference(b, rr.F16X2)
    assert (wa[1], wb[1]) == (1, 2)
    ta, tb = _upload(device, a), _upload(device, b)
    table = ops.range_table(1, device)
    s1, s2 = torch.cuda.Stream(device=device), torch.cuda.Stream(device=device)
    torch.cuda.synchronize(device)
    for _ in range(3):
        with torch.cuda.stream(s1):
            ops.range_probe(ta, table[0], math=1)
        with torch.cuda.stream(s2):
            ops.range_probe(tb, table[0], math=1)
    torch.cuda.synchronize(device)
    assert _read(table)[0] == (max(wa[0], wb[0]), 3 * (wa[1] + wb[1]), 0, 3 * (wa[3] + wb[3]))


@pytest.mark.parametrize('name,storage', STORAGES)
def test_many_workgroups_and_grid_stride(device, name, storage):
    """70 000 rows x 64 channels (2 188 workgroups' worth of items: more than the persistent grid) with a known sprinkling."""
    rows, c = 70000, 64
    x = np.clip(_data(5 + storage, rows, c), -3.0e4, 3.0e4)
    rng = np.random.default_rng(99)
    n_sat, n_nan = 1234, 777
    flat = rng.choice(rows * c, n_sat + n_nan, replace=False)
    sat_at, nan_at = np.unravel_index(flat[:n_sat], (rows, c)), np.unravel_index(flat[n_sat:], (rows, c))
    x[sat_at] = 1.0e5 * np.where(rng.random(n_sat) < 0.5, -1.0, 1.0).astype(np.float32)
    words = _words(device, x, storage)
    if storage == rr.F32:
        words[nan_at] = NAN32
    else:
        hb, lb, _, _ = rr.decode_pair16(words, storage)
        hb[nan_at] = EXP16[storage] | 0x0040
        words = rr.encode_pair16(hb, lb)
    want = rr.probe_reference(words, storage)
    assert want[1] == (n_sat if storage == rr.F16X2 else 0) and want[2] == n_nan and want[3] == rows * c
    assert _probe_one(device, words, storage) == want


def test_byte_offsets_beyond_2_gib(device):
    """One fp32 tensor of 2^31 + 256 bytes, zero except its last element: the peak is found there, `elements` is exact."""
    from detzero_amd import ops
    rows, c = 2 ** 26 + 8, 8
    assert rows * c * 4 > 2 ** 31
    t = torch.zeros((rows, c), dtype=torch.float32, device=device)
    t[rows - 1, c - 1] = -3.5
    table = ops.range_table(1, device)
    ops.range_probe(t, table[0], math='f32')
    assert _read(table)[0] == (_bits(3.5), 0, 0, rows * c)
    t[rows - 1, c - 1] = float('inf')
    d = torch.tensor([rows - 1], dtype=torch.int32, device=device)
    ops.range_probe(t, table[0], math='f32', d_rows=d)       # (the last row is outside: nothing non-finite)
    assert _read(table)[0] == (_bits(3.5), 0, 0, rows * c + (rows - 1) * c)
    del t


def test_bad_arguments_are_refused_without_a_launch(device):
    from detzero_amd import lib as L
    from detzero_amd import ops
    lib = L.load()
    t = torch.full((16, 40), float('inf'), dtype=torch.float32, device=device)
    table = ops.range_table(2, device)
    st = L.stream()

    def call(rows=16, stride=40, c_off=0, c=40, math=0, x=t, slot=table[0]):
        return lib.dz_range_probe(L.ptr(x), rows, None, stride, c_off, c, math, L.ptr(slot), st)
    assert call(c=12) == L.ERR_INVALID                       # c not a multiple of 8
    assert call(c_off=4, c=8) == L.ERR_INVALID               # c_off not a multiple of 8
    assert call(c_off=8, c=40) == L.ERR_INVALID              # slice beyond the row stride
    assert call(c_off=40, c=8) == L.ERR_INVALID
    assert call(math=4) == L.ERR_INVALID and call(math=-1) == L.ERR_INVALID          # unknown math id
    assert b'unknown math' in lib.dz_last_error()
    assert call(x=None) == L.ERR_INVALID                     # null tensor with rows > 0
    assert call(rows=-1) == L.ERR_INVALID
    assert lib.dz_range_reset(None, 2, st) == L.ERR_INVALID
    assert call(rows=0, x=None) == 0 and call(rows=0) == 0   # rows == 0: accepted, no launch
    assert lib.dz_range_reset(None, 0, st) == 0
    with pytest.raises(L.DetZeroHipError):
        ops.range_probe(t, table[0], math=0, c=12)
    with pytest.raises(L.DetZeroHipError):
        ops.range_probe(t, table[0], math=0, rows=17)        # more rows than the tensor holds
    assert _read(table) == [(0, 0, 0, 0)] * 2                # nothing was launched: the all-inf tensor left no trace
    assert call() == 0
    assert _read(table)[0] == (0, 0, 640, 640)
