"""ops.spconv_route and ops.spconv_forward with the f32_small keyword, on the host (no GPU).  The order of tests/test_spconv_route.py
(tables, widths, modes and keywords imported from it) gains one row between its rows 1 and 2:

  1   math 0, f32_engine 'xrun_bf16x3', packed table with windows in the layer's unit, width the bf16x3 x-run kernel covers
  1w  math 0, f32_small 'wave_bf16x3', plain table with tile masks, 16 -> 16 or 16 -> 32, everything below 2 GiB - whatever f32_gather
  2   math 0, f32_gather 'bf16x3', ...

With f32_small None or 'gather' every combination resolves as it does without the keyword."""
import itertools
import types

import pytest
import torch

from detzero_amd import lib as L
from detzero_amd import ops
from tests.test_spconv_route import CAP, FORMS, MATHS, ROWS, WIDTHS, _i32, expected_row, make_table

WAVE_WIDTHS = ((16, 16), (16, 32))                 # the coverage of csrc/sparse_conv_wt.hip, restated
ALL_WIDTHS = WIDTHS + [(16, 32)]
KEYWORDS = list(itertools.product(MATHS, (None,) + ops.SPARSE_F32_ENGINES, (None,) + ops.SPARSE_F32_GATHER_ENGINES))


def test_the_coverage_this_file_writes_out_is_the_librarys():
    lib = L.load()
    for cin, cout in ALL_WIDTHS + [(64, 64), (64, 128), (16, 64), (48, 48)]:
        assert (lib.dz_spconv_limb3_w_tile_rows(cin, cout) > 0) == ((cin, cout) in WAVE_WIDTHS), (cin, cout)
    assert list(ops._SPCONV_ENGINES)[:3] == ['xrun_bf16x3', 'wave_bf16x3', 'gather_bf16x3']
    assert ops._SPCONV_ENGINES['wave_bf16x3'][:3] == ('limb3', 'dz_spconv_forward_limb3_w', 'dz_spconv_limb3_w_variant')


@pytest.mark.parametrize('cin,cout', ALL_WIDTHS)
@pytest.mark.parametrize('form', FORMS)
def test_route_with_the_keyword(form, cin, cout):
    table, _ = make_table(form, cout)
    n_wave = 0
    for math, f32_engine, f32_gather in KEYWORDS:
        what = (form, cin, cout, math, f32_engine, f32_gather)
        row = expected_row(*what)
        if row is None:
            for small in (None,) + ops.SPARSE_F32_SMALL_ENGINES:
                with pytest.raises(L.DetZeroHipError, match='packed neighbour table'):
                    ops.spconv_route(table, cin, cout, math, f32_engine, f32_gather, f32_small=small)
            continue
        today = ops.spconv_route(table, cin, cout, math, f32_engine, f32_gather)
        assert (today.engine, today.weights) == ROWS[row], what
        for small in (None, 'gather'):
            assert ops.spconv_route(table, cin, cout, math, f32_engine, f32_gather, f32_small=small) == today, what + (small,)
            assert ops.spconv_route(table, cin, cout, math, f32_engine, f32_gather, CAP, small) == today, what + (small,)
        got = ops.spconv_route(table, cin, cout, math, f32_engine, f32_gather, f32_small='wave_bf16x3')
        if not math and row != 1 and form in ('plain', 'tiles') and (cin, cout) in WAVE_WIDTHS:
            assert (got.engine, got.weights) == ('wave_bf16x3', 'limb3'), what
            assert got.variant(cin, cout) == b'k_spconv_wt<%dx%d>' % (cin, cout), what
            assert ops.spconv_route(table, cin, cout, math, f32_engine, f32_gather, CAP, 'wave_bf16x3') == got, what
            n_wave += 1
        else:
            assert got == today, what
    covered = form in ('plain', 'tiles') and (cin, cout) in WAVE_WIDTHS
    assert n_wave == (sum(1 for k in KEYWORDS if not k[0]) if covered else 0), (form, cin, cout, n_wave)


def test_the_backbone_prefers_uncovered_requests_fall_through(monkeypatch):
    lib = L.load()
    plain, _ = make_table('plain', 16)
    nomasks, _ = make_table('plain_nomasks', 16)
    packed, _ = make_table('packed', 16)
    route = lambda t, ci, co, **kw: ops.spconv_route(t, ci, co, 0, f32_small='wave_bf16x3', **kw).engine          # noqa: E731
    assert route(plain, 16, 16) == route(plain, 16, 32) == 'wave_bf16x3'
    assert route(plain, 16, 16, f32_gather='mfma32') == route(plain, 16, 16, f32_gather='bf16x3') == 'wave_bf16x3'
    assert route(plain, 32, 32) == 'gather_f32' and route(plain, 32, 32, f32_gather='bf16x3') == 'gather_bf16x3'
    assert route(plain, 16, 64) == 'gather_f32' and route(plain, 48, 48, f32_gather='bf16x3') == 'gather_f32'
    assert route(nomasks, 16, 16, f32_gather='bf16x3') == 'gather_f32'
    with pytest.raises(L.DetZeroHipError, match='packed neighbour table'):
        route(packed, 16, 16)
    rows = 2 ** 31 // (16 * 4)
    assert route(plain, 16, 16, in_rows=rows - 1) == 'wave_bf16x3' and route(plain, 16, 16, in_rows=rows) == 'gather_f32'
    big = ops.NeighborTable(torch.empty((27, 2 ** 31 // (32 * 4)), dtype=torch.int32, device='meta'), tile_masks=plain.tile_masks)
    assert route(big, 16, 32) == 'gather_f32'                    # an output of exactly 2^31 bytes (and a larger table)
    # a layer the library does not ship stays on the kernel it has
    monkeypatch.setattr(lib, 'dz_spconv_limb3_w_tile_rows', lambda cin, cout: 0)
    assert route(plain, 16, 16) == 'gather_f32' and route(plain, 16, 16, f32_gather='bf16x3') == 'gather_bf16x3'


def test_spconv_forward_is_explicit_it_raises_before_any_device_check(monkeypatch):
    """Every operand here lives on the host (or nowhere)."""
    lib = L.load()
    plain, _ = make_table('plain', 16)
    nomasks, _ = make_table('plain_nomasks', 16)
    packed, _ = make_table('packed', 16)
    win, _ = make_table('packed_win', 32)
    lvl = types.SimpleNamespace(d_m=_i32(1))
    x, taps, limbs, limbs32 = torch.zeros((CAP, 16)), torch.zeros((27, 16, 16)), torch.zeros((27, 32, 24)), torch.zeros((27, 32, 48))

    def forward(table, w, feats=x, **kw):
        return ops.spconv_forward(feats, table, lvl, w, None, None, None, relu=False, **kw)
    with pytest.raises(L.DetZeroHipError, match='nonsense'):
        forward(plain, taps, f32_small='nonsense')
    with pytest.raises(L.DetZeroHipError, match='bf16x3'):
        forward(plain, taps, f32_small='bf16x3')                                                  # a name of another switch
    with pytest.raises(L.DetZeroHipError, match='packed'):
        forward(packed, limbs, cout=16, f32_small='wave_bf16x3')
    with pytest.raises(L.DetZeroHipError, match='wave_bf16x3'):
        forward(nomasks, limbs, cout=16, f32_small='wave_bf16x3')
    with pytest.raises(L.DetZeroHipError, match='wave_bf16x3'):                                   # 32 -> 32: not covered
        forward(plain, limbs32, feats=torch.zeros((CAP, 32)), f32_small='wave_bf16x3')
    with pytest.raises(L.DetZeroHipError, match='wave_bf16x3'):                                   # ... nor with the gather arithmetic beside it
        forward(plain, limbs32, feats=torch.zeros((CAP, 32)), f32_gather='bf16x3', f32_small='wave_bf16x3')
    with pytest.raises(L.DetZeroHipError, match='bf16x3'):
        forward(plain, taps, f32_small='wave_bf16x3')                                             # not limb weights
    with pytest.raises(L.DetZeroHipError, match='wave_bf16x3'):
        forward(plain, limbs, cout=16, feats=torch.empty((2 ** 31 // (16 * 4), 16), device='meta'), f32_small='wave_bf16x3')
    with pytest.raises(L.DetZeroHipError, match='max_workgroups'):
        forward(plain, taps, max_workgroups=8)                                                    # the cap belongs to the one engine
    with pytest.raises(TypeError):
        ops.spconv_forward(x, plain, lvl, limbs, None, None, None, True, None, None, 0, 16, None, None, 'wave_bf16x3', 8)     # keyword-only
    # what the resolver honours gets as far as the device check; 'gather' and None ask for nothing; the split modes ignore the keyword
    for table, w, kw in ((plain, limbs, {'cout': 16, 'f32_small': 'wave_bf16x3'}),
                         (plain, limbs, {'cout': 16, 'f32_small': 'wave_bf16x3', 'max_workgroups': 8}),
                         (plain, limbs, {'cout': 16, 'f32_small': 'wave_bf16x3', 'f32_gather': 'bf16x3'}),
                         (plain, limbs, {'cout': 32, 'f32_small': 'wave_bf16x3', 'f32_gather': 'mfma32'}),
                         (plain, taps, {'f32_small': 'gather'}), (plain, limbs, {'cout': 16, 'f32_small': 'gather', 'f32_gather': 'bf16x3'}),
                         (win, torch.zeros((27, 32, 48)), {'f32_engine': 'xrun_bf16x3', 'f32_small': 'wave_bf16x3'}),
                         (packed, torch.zeros((27, 32, 16)), {'math': 1, 'cout': 16, 'f32_small': 'wave_bf16x3'})):
        with pytest.raises(L.DetZeroHipError, match='device tensor'):
            forward(table, w, **kw) if w.shape[-1] != 48 else forward(table, w, feats=torch.zeros((CAP, 32)), **kw)
    monkeypatch.setattr(lib, 'dz_spconv_limb3_w_tile_rows', lambda cin, cout: 0)
    with pytest.raises(L.DetZeroHipError, match='wave_bf16x3'):
        forward(plain, limbs, cout=16, f32_small='wave_bf16x3')
