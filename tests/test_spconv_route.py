"""ops.NeighborTable and ops.spconv_route on the host (no GPU): the table type mirrors its words and owns exactly the tensors it was
given; the resolver returns, for every math mode, engine keyword, table form and layer width, the engine and weight form of the
order below - written out here, row by row, from the library's documented coverage (the x-run kernels: cin == cout of 32 / 64 / 128
channels; the bf16x3 gather kernel: every layer width of the backbone) and not from the resolver:

  1  math 0, f32_engine 'xrun_bf16x3', packed table with windows in the layer's unit, width the bf16x3 x-run kernel covers
  2  math 0, f32_gather 'bf16x3', plain table with tile masks, width the bf16x3 gather kernel covers, everything below 2 GiB
  3  math 0, packed table with windows in the layer's unit, width the fp32 x-run kernel covers
  4  math != 0, packed table with windows, cin == cout
  5  math != 0, kvol >= 3, table with tiles
  6  math != 0, packed table
  7  math != 0
  8  math 0, plain table                      (math 0 on any other packed table: DetZeroHipError)

The backbone's switches prefer (an uncovered request falls through); ops.spconv_forward's keywords are explicit (it raises)."""
import itertools
import types

import pytest
import torch

from detzero_amd import lib as L
from detzero_amd import ops

CAP = 64
MATHS = (ops.math_id('f32'), ops.math_id('f16x2'))
WIDTHS = [(16, 16), (32, 32), (32, 64), (128, 128)]
FORMS = ('plain', 'plain_nomasks', 'packed', 'packed_win', 'packed_win_wrong', 'tiles')
XRUN_WIDTHS = (32, 64, 128)                      # cin == cout widths of k_spconv_x / k_spconv_xf / k_spconv_xt
ROWS = {1: ('xrun_bf16x3', 'limb3'), 2: ('gather_bf16x3', 'limb3'), 3: ('xrun_f32', 'taps'), 4: ('xrun_split', 'split'),
        5: ('tiles', 'split'), 6: ('gather_split_packed', 'split'), 7: ('gather_split', 'split'), 8: ('gather_f32', 'taps')}
ENTRY = {1: b'k_spconv_xt<', 3: b'k_spconv_xf<', 4: b'k_spconv_x<'}


def _i32(*shape):
    return torch.zeros(shape, dtype=torch.int32)


def make_table(form, cout):
    """-> (NeighborTable of CPU tensors, the tensors it was given)."""
    lib = L.load()
    masks = _i32(lib.dz_tile_masks_words(CAP))
    if form in ('plain', 'plain_nomasks', 'tiles'):
        words = _i32(27, CAP)
        tiles = ops.Tiles(_i32(1, 8), _i32(1, 4), torch.zeros((1, 8), dtype=torch.int16), torch.zeros((1, 8), dtype=torch.int16)) if form == 'tiles' else None
        given = [words] + ([masks] if form != 'plain_nomasks' else []) + list(tiles or ())
        return ops.NeighborTable(words, tile_masks=None if form == 'plain_nomasks' else masks, tiles=tiles), given
    words = _i32(9, CAP)
    if form == 'packed':
        return ops.NeighborTable(words, packed=True, tile_masks=masks), [words, masks]
    unit = lib.dz_spconv_x_tile_rows(cout, cout) or 128          # (a width without x-run kernel: windows of some other level's unit)
    unit = unit if form == 'packed_win' else unit // 2
    sort = cout >= 64
    xwin = ops.XWindows(_i32(6 + 16), unit, _i32(9, CAP) if sort else None, _i32(CAP) if sort else None)
    return ops.NeighborTable(words, packed=True, tile_masks=masks, xwin=xwin), [words, masks, xwin.windows] + ([xwin.sorted_table, xwin.perm] if sort else [])


def expected_row(form, cin, cout, math, f32_engine, f32_gather):
    """The first row of the order in the module docstring that matches; None = the packed table no fp32 kernel reads."""
    packed = form.startswith('packed')
    windows = form in ('packed_win', 'packed_win_wrong') and cin == cout
    in_unit = windows and form == 'packed_win' and cout in XRUN_WIDTHS
    if math:
        return 4 if windows else 5 if form == 'tiles' else 6 if packed else 7
    if f32_engine == 'xrun_bf16x3' and in_unit:
        return 1
    if f32_gather == 'bf16x3' and form in ('plain', 'tiles'):
        return 2
    if in_unit:
        return 3
    return None if packed else 8


def test_the_coverage_this_file_writes_out_is_the_librarys():
    lib = L.load()
    for cin, cout in WIDTHS + [(64, 64), (64, 128), (16, 32)]:
        covered = cin == cout and cout in XRUN_WIDTHS
        assert (lib.dz_spconv_x_tile_rows(cin, cout) > 0) == covered
        assert (lib.dz_spconv_x_f32_window_rows(cin, cout) > 0) == covered
        assert (lib.dz_spconv_x_limb3_window_rows(cin, cout) > 0) == covered
        assert lib.dz_spconv_limb3_tile_rows(cin, cout) > 0
        assert ops.xrun_unit(cin, cout, 0) == ops.xrun_unit(cin, cout, 1) == ops.xrun_unit(cin, cout, 0, bf16x3=True) == lib.dz_spconv_x_tile_rows(cin, cout)
    assert lib.dz_spconv_limb3_tile_rows(48, 48) == 0


@pytest.mark.parametrize('cin,cout', WIDTHS)
@pytest.mark.parametrize('form', FORMS)
def test_route_of_every_mode_keyword_and_table(form, cin, cout):
    table, _ = make_table(form, cout)
    for math, f32_engine, f32_gather in itertools.product(MATHS, (None,) + ops.SPARSE_F32_ENGINES, (None,) + ops.SPARSE_F32_GATHER_ENGINES):
        what = (form, cin, cout, math, f32_engine, f32_gather)
        row = expected_row(*what)
        if row is None:
            with pytest.raises(L.DetZeroHipError, match='packed neighbour table'):
                ops.spconv_route(table, cin, cout, math, f32_engine, f32_gather)
            continue
        route = ops.spconv_route(table, cin, cout, math, f32_engine, f32_gather)
        assert (route.engine, route.weights) == ROWS[row], what
        if row in ENTRY and cout in XRUN_WIDTHS:
            assert route.variant(cin, cout).startswith(ENTRY[row]), what
        # the in_rows of an ordinary level change nothing
        assert ops.spconv_route(table, cin, cout, math, f32_engine, f32_gather, in_rows=CAP) == route, what


def test_every_row_is_reached():
    reached = {expected_row(f, ci, co, m, e, g) for f, (ci, co), m, e, g in itertools.product(
        FORMS, WIDTHS, MATHS, (None,) + ops.SPARSE_F32_ENGINES, (None,) + ops.SPARSE_F32_GATHER_ENGINES)}
    assert reached == set(ROWS) | {None}


def test_the_backbone_prefers_uncovered_requests_fall_through(monkeypatch):
    lib = L.load()
    win, _ = make_table('packed_win', 64)
    plain, _ = make_table('plain', 64)
    packed, _ = make_table('packed', 64)
    assert ops.spconv_route(win, 64, 64, 0, 'xrun_bf16x3', 'bf16x3').engine == 'xrun_bf16x3'
    # bf16x3 gather arithmetic: never on a packed table; not on a layer the kernel does not cover; not at 2 GiB
    assert ops.spconv_route(win, 64, 64, 0, 'xrun', 'bf16x3').engine == 'xrun_f32'
    assert ops.spconv_route(plain, 48, 48, 0, None, 'bf16x3').engine == 'gather_f32'
    rows = 2 ** 31 // (64 * 4)
    assert ops.spconv_route(plain, 64, 64, 0, None, 'bf16x3', in_rows=rows - 1).engine == 'gather_bf16x3'
    assert ops.spconv_route(plain, 64, 64, 0, None, 'bf16x3', in_rows=rows) == ops.spconv_route(plain, 64, 64, 0) \
        == ops.SpconvRoute('gather_f32', 'taps', lib.dz_spconv_variant)
    big = ops.NeighborTable(torch.empty((27, rows), dtype=torch.int32, device='meta'), tile_masks=plain.tile_masks)
    assert ops.spconv_route(big, 16, 64, 0, None, 'bf16x3').engine == 'gather_f32'           # an output of exactly 2^31 bytes (and a larger table)
    with pytest.raises(L.DetZeroHipError, match='packed neighbour table'):
        ops.spconv_route(packed, 64, 64, 0, None, 'bf16x3')
    # a width the bf16x3 x-run kernel does not ship for stays on the fp32 x-run kernel
    monkeypatch.setattr(lib, 'dz_spconv_x_limb3_window_rows', lambda cin, cout: 0)
    assert ops.spconv_route(win, 64, 64, 0, 'xrun_bf16x3').engine == 'xrun_f32'
    assert ops.spconv_route(win, 64, 64, 0, 'xrun_bf16x3', 'bf16x3').engine == 'xrun_f32'
    assert ops.xrun_unit(64, 64, 0) == win.xwin.tile_rows and ops.xrun_unit(64, 64, 0, bf16x3=True) == 0


def test_spconv_forward_is_explicit_it_raises_for_the_same_inputs(monkeypatch):
    """Before any device check: every operand here lives on the host (or nowhere)."""
    lib = L.load()
    win, _ = make_table('packed_win', 64)
    plain, _ = make_table('plain', 64)
    packed, _ = make_table('packed', 64)
    lvl = types.SimpleNamespace(d_m=_i32(1))
    x, taps, limbs = torch.zeros((CAP, 64)), torch.zeros((27, 64, 64)), torch.zeros((27, 64, 96))

    def forward(table, w, feats=x, **kw):
        return ops.spconv_forward(feats, table, lvl, w, None, None, None, relu=False, **kw)
    with pytest.raises(L.DetZeroHipError, match='nonsense'):
        forward(plain, taps, f32_engine='nonsense')
    with pytest.raises(L.DetZeroHipError, match='nonsense'):
        forward(plain, taps, f32_gather='nonsense')
    with pytest.raises(L.DetZeroHipError, match='packed neighbour table'):
        forward(packed, taps)
    with pytest.raises(L.DetZeroHipError, match='xrun_bf16x3'):
        forward(packed, limbs, f32_engine='xrun_bf16x3')
    with pytest.raises(L.DetZeroHipError, match='xrun_bf16x3'):
        forward(plain, limbs, f32_engine='xrun_bf16x3')
    with pytest.raises(L.DetZeroHipError, match='packed'):
        forward(win, limbs, f32_gather='bf16x3')
    with pytest.raises(L.DetZeroHipError, match='packed'):
        forward(packed, limbs, f32_gather='bf16x3')
    with pytest.raises(L.DetZeroHipError, match='bf16x3'):
        forward(plain, torch.zeros((27, 64, 72)), feats=torch.zeros((CAP, 48)), f32_gather='bf16x3')          # 48 -> 48: not covered
    with pytest.raises(L.DetZeroHipError, match='bf16x3'):
        forward(plain, taps, f32_gather='bf16x3')                                                                # not limb weights
    with pytest.raises(L.DetZeroHipError, match='bf16x3'):
        forward(plain, limbs, feats=torch.empty((2 ** 31 // (64 * 4), 64), device='meta'), f32_gather='bf16x3')  # an input of 2^31 bytes
    # what the resolver honours gets as far as the device check
    for table, w, kw in ((plain, taps, {}), (plain, limbs, {'f32_gather': 'bf16x3'}), (win, taps, {}), (win, taps, {'f32_engine': 'xrun'}),
                         (win, limbs, {'f32_engine': 'xrun_bf16x3'}), (win, limbs, {'f32_engine': 'xrun_bf16x3', 'f32_gather': 'bf16x3'}),
                         (packed, torch.zeros((27, 64, 64)), {'math': 1, 'f32_engine': 'xrun_bf16x3', 'f32_gather': 'bf16x3'})):
        with pytest.raises(L.DetZeroHipError, match='device tensor'):
            forward(table, w, **kw)
    monkeypatch.setattr(lib, 'dz_spconv_x_limb3_window_rows', lambda cin, cout: 0)
    with pytest.raises(L.DetZeroHipError, match='xrun_bf16x3'):
        forward(win, limbs, f32_engine='xrun_bf16x3')


@pytest.mark.parametrize('form', FORMS)
def test_a_table_owns_exactly_the_tensors_it_was_given(form):
    for cout in (32, 64):
        table, given = make_table(form, cout)
        got = table.tensors()
        assert len(got) == len(given) and {id(t) for t in got} == {id(t) for t in given}, (form, cout)
        assert table.shape == table.words.shape and tuple(table.shape) == ((9 if table.packed else 27), CAP)
        assert table.numel() == table.words.numel() and table.device == table.words.device
        assert table.kvol == 27 and table.packed == form.startswith('packed')
        if table.xwin is not None:
            assert table.xwin[0] is table.xwin.windows and table.xwin[1] == table.xwin.tile_rows
            assert table.xwin[2] is table.xwin.sorted_table and table.xwin[3] is table.xwin.perm
    assert ops.NeighborTable(_i32(3, CAP)).kvol == 3 and ops.NeighborTable(_i32(3, CAP)).tensors()[0].shape == (3, CAP)


def test_pairs_and_unpacking_of_a_hand_written_table():
    """Four rows: 0, 1, 2 side by side along x, 3 on its own; tap t = 3 * group + (left, centre, right)."""
    tab = torch.full((27, 4), -1, dtype=torch.int32)
    tab[12] = torch.tensor([-1, 0, 1, -1])          # centre group: left neighbours
    tab[13] = torch.tensor([0, 1, 2, 3])
    tab[14] = torch.tensor([1, 2, -1, -1])
    tab[3, 3], tab[5, 3] = 0, 1                     # group 1 of row 3: left and right without centre (right follows left)
    tab[23, 0] = 2                                  # group 7 of row 0: right only
    tab[0, 2] = 3                                   # group 0 of row 2: left only
    LEFT, CEN, RIGHT = 1 << 29, 1 << 30, 1 << 31
    words = torch.zeros((9, 4), dtype=torch.int64)
    words[4] = torch.tensor([0 | CEN | RIGHT, 1 | LEFT | CEN | RIGHT, 2 | LEFT | CEN, 3 | CEN])
    words[1, 3] = 1 | LEFT | RIGHT
    words[7, 0] = 2 | RIGHT
    words[0, 2] = 4 | LEFT
    words = torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32)
    plain, packed = ops.NeighborTable(tab), ops.NeighborTable(words, packed=True)
    assert (plain.kvol, packed.kvol, tuple(plain.shape), tuple(packed.shape)) == (27, 27, (27, 4), (9, 4))
    assert ops.unpack_table(plain) is tab and torch.equal(ops.unpack_table(packed), tab)
    for m, pairs in ((4, 12), (3, 9), (2, 6), (1, 3), (0, 0)):
        assert ops.table_pairs(plain, m) == ops.table_pairs(packed, m) == pairs == int((tab[:, :m] >= 0).sum()), m
    # the reads of callers written for the tensor form: the address and rows of the words (a bare tensor, no table); nothing else
    assert type(packed[:, :2]) is torch.Tensor and torch.equal(packed[:, :2], words[:, :2]) and packed.data_ptr() == words.data_ptr()
    for name in ('record_stream', 'clone', 'cpu', 'to', 'kvoll'):
        assert not hasattr(packed, name), name
    # bare words count as a table of their own - plain, or packed where the caller marked them; an unmarked slice of a packed table
    # is refused, not counted as a plain one
    assert ops.unpack_table(tab) is tab and ops.table_pairs(tab, 4) == 12
    with pytest.raises(L.DetZeroHipError, match='packed'):
        ops.table_pairs(packed[:, :3], 3)
    with pytest.raises(L.DetZeroHipError, match='packed'):
        ops.unpack_table(packed[:, :3])
    cut = packed[:, :3].clone()
    cut.packed = True
    assert torch.equal(ops.unpack_table(cut), tab[:, :3]) and ops.table_pairs(cut, 3) == 9
