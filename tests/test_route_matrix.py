"""The route matrix itself (tests/route_matrix.py), on the CPU: the rows cover every valid pair of switch settings, break no condition,
are the same on every call, and the factor tables account for every development switch of the sources."""
import importlib
import itertools

import pytest

from tests import route_matrix as rm

FAMILY_NAMES = sorted(rm.FAMILIES)


def _facs(family):
    cells, rows = rm.FAMILIES[family]
    return rm._index(cells + rows), [f.name for f in rows]


def _support(name, facs):
    """The factor and every factor its condition names, transitively."""
    out, stack = set(), [name]
    while stack:
        n = stack.pop()
        if n not in out:
            out.add(n)
            stack += [k for alt in facs[n].needs for k in alt]
    return out


@pytest.mark.parametrize('family', FAMILY_NAMES)
def test_every_valid_pair_occurs_in_some_row(family):
    """Per cell: every pair of (factor, value) for which ANY assignment exists with both factors in effect - found here by brute force
    over the row factors, independently of the generator's own search - is covered by a row of the cell; rows with deliberately too
    small capacities count only for the pairs that contain that setting.  And every single (factor, value) that can have an effect
    in the cell occurs in effect in an unmasked row (or the row masked by itself)."""
    facs, names = _facs(family)
    total = 0
    for cell in rm.cells(family):
        rows = rm.rows(family, cell)
        got = set()
        for r in rows:
            got |= rm.covered_pairs(r, facs, names)
        want, singles = set(), set()
        default = dict(cell, **{n: facs[n].default for n in names})
        for a, b in itertools.combinations(names, 2):
            free = sorted((_support(a, facs) | _support(b, facs)) - set(cell), key=names.index)
            for combo in itertools.product(*[facs[n].values for n in free]):
                row = dict(default, **dict(zip(free, combo)))
                if rm.effective(a, row, facs) and rm.effective(b, row, facs):
                    want.add(((a, row[a]), (b, row[b])))
        for a in names:
            free = sorted(_support(a, facs) - set(cell), key=names.index)
            for combo in itertools.product(*[facs[n].values for n in free]):
                row = dict(default, **dict(zip(free, combo)))
                if rm.effective(a, row, facs):
                    singles.add((a, row[a]))
        assert singles and (want or family == 'refiner'), (family, cell)
        assert want == set(rm.valid_pairs(family, cell)), sorted(want ^ set(rm.valid_pairs(family, cell)))[:5]
        missing = want - got
        assert not missing, (cell, sorted(missing)[:5])
        for fv in singles:
            assert any(r[fv[0]] == fv[1] and rm.effective(fv[0], r, facs) and rm.masked(r, facs) in (None, fv) for r in rows), (cell, fv)
        total += len(rows)
    print('%s: %d cells, %d rows' % (family, len(rm.cells(family)), total))


@pytest.mark.parametrize('family', FAMILY_NAMES)
def test_no_row_violates_a_condition(family):
    """A factor whose condition does not hold in a row stays at its default there; every value is one of the table's; the first row of
    every cell is the all-default row; no two rows of a cell are the same."""
    facs, names = _facs(family)
    for cell in rm.cells(family):
        rows = rm.rows(family, cell)
        assert not rm.non_default(rows[0], family)
        ids = [rm.row_id(r, family) for r in rows]
        assert len(set(ids)) == len(ids), ids
        for r in rows:
            assert sorted(r) == sorted(list(cell) + names)
            assert all(r[k] == v for k, v in cell.items())
            for n in names:
                assert r[n] in facs[n].values
                assert r[n] == facs[n].default or rm.effective(n, r, facs), (n, rm.row_id(r, family))


def test_conditions_named_in_the_tables_hold_in_the_rows():
    """Spot checks of the conditions themselves, in the words of the sources: PAD_RAGGED needs a list input and the hard voxelizer, the
    fp32 engines need 'f32' math, SKIP_EMPTY_TILES and BEV_DENSE sit on opposite sides of SPARSE_BEV_INPUT, the x-run switches need an
    x-run engine, the grouping switches need more frames than `dense_group`, SPLIT_SA a split mode."""
    for r in rm.all_rows('detector'):
        if r['PAD_RAGGED'] is False:
            assert r['input'] == 'list' and r['dynamic'] is False
        if r['f32_engine'] != 'gather' or r['f32_gather'] != 'mfma32' or r['f32_dense_engine'] != 'mfma32':
            assert r['math'] == 'f32'
        if r['SKIP_EMPTY_TILES'] is False:
            assert r['math'] != 'f32' and r['SPARSE_BEV_INPUT'] is True
        if r['BEV_DENSE'] is False:
            assert r['math'] != 'f32' and r['SPARSE_BEV_INPUT'] is False
        if r['FUSED_XWIN'] is False or r['XRUN_SORT'] is False:
            assert (r['engine'] == 'xrun') if r['math'] != 'f32' else (r['f32_engine'] != 'gather')
        if r['GROUPED_DEEP_BLOCKS'] is False or r['FIRST_BLOCK_WIDE_GROUPS'] is False:
            assert r['dense_group'] == 2
        if r['FIRST_BLOCK_WIDE_GROUPS'] is False:
            assert r['GROUPED_DEEP_BLOCKS'] is True
        if r['engine'] != 'xrun' or r['PACKED_TABLES'] or r['FUSED_DEBLOCK_PHASES'] is False or r['SPARSE_BEV_INPUT'] is False:
            assert r['math'] != 'f32'
    for r in rm.all_rows('pdv'):
        if r['SPLIT_SA'] is False:
            assert r['math'] != 'f32' and r['FUSED_SA'] is True
        if r['FUSED_ENCODER'] is False:
            assert r['math'] != 'f32' and r['FOLDED_ATTENTION'] is True
    for r in rm.all_rows('refiner'):
        if r['math'] == 'f32':
            assert r['SPLIT_ATTENTION'] and r['FUSED_CHAIN'] and r['FUSED_POINTNET']


def test_detector_cells_cover_every_pair_of_math_dynamic_and_input():
    cells = rm.cells('detector')
    assert len(cells) == 8
    cf = rm.cell_table('detector')
    for a, b in itertools.combinations(cf, 2):
        for va in a.values:
            for vb in b.values:
                assert any(c[a.name] == va and c[b.name] == vb for c in cells), (a.name, va, b.name, vb)
    for fam in ('pdv', 'refiner'):
        assert [c['math'] for c in rm.cells(fam)] == ['f32', 'f16x2', 'bf16x2']


@pytest.mark.parametrize('family', FAMILY_NAMES)
def test_rows_are_identical_on_two_calls(family):
    first = [(rm.row_id(r, family), sorted(r.items(), key=str)) for r in rm.all_rows(family)]
    importlib.reload(rm)
    second = [(rm.row_id(r, family), sorted(r.items(), key=str)) for r in rm.all_rows(family)]
    assert first == second and len(first) > 1


def test_row_id_spells_the_non_default_settings():
    for family in FAMILY_NAMES:
        for r in rm.all_rows(family):
            rid = rm.row_id(r, family)
            nd = rm.non_default(r, family)
            assert all('%s=%s' % (n, v) in rid for n, v in nd)
            assert rid.endswith('-default') == (not nd)
            assert rid.count('=') == len(nd)


def test_bit_identity_is_required_only_where_every_flipped_factor_promises_it():
    det = rm._index(rm.table('detector'))
    for f in rm.DETECTOR + rm.PDV + rm.REFINER:
        rels = {f.relation_of(v) for v in f.values}
        assert rels <= {'bits', 'oracle'}
        assert bool(f.promise) == ('bits' in rels), f.name          # a promise is quoted exactly where bit identity is claimed
    assert det['level_caps'].relation_of('small') == 'oracle' and det['dense_group'].relation_of(2) == 'oracle'
    n_base = 0
    for r in rm.all_rows('detector'):
        nd = rm.non_default(r, 'detector')
        want = bool(nd) and all(det[n].relation_of(v, r) == 'bits' for n, v in nd)
        assert rm.bits_required(r, 'detector') == want
        # the route a row must reproduce bit for bit: the same row with its 'bits' factors at their defaults (the all-default row when
        # nothing else is flipped); none for a row that flips no such factor or runs on too small capacities
        base = rm.bits_base(r, 'detector')
        flipped = [(n, v) for n, v in nd if det[n].relation_of(v, r) == 'bits']
        assert (base is not None) == (bool(flipped) and r['level_caps'] != 'small')
        if base is not None:
            n_base += 1
            assert all(det[n].relation_of(v, base) == 'oracle' or (n, v) not in flipped for n, v in rm.non_default(base, 'detector'))
            assert {n: v for n, v in rm.non_default(base, 'detector')} == {n: v for n, v in nd if (n, v) not in flipped}
            assert (not rm.non_default(base, 'detector')) == want
    assert n_base >= 8 * len(rm.cells('detector'))
    # the one promise with a limit: head_at_candidates against the full map is bit identical on the fp32 matrix cores only
    hac = det['head_at_candidates']
    assert hac.relation_of(False, {'math': 'f32', 'f32_dense_engine': 'bf16x3'}) == 'oracle'
    assert hac.relation_of(False, {'math': 'f32', 'f32_dense_engine': 'mfma32'}) == 'bits' == hac.relation_of(False)


def test_factor_tables_account_for_every_development_switch():
    """Every module-level assignment of detzero_amd/*.py commented `development switch`, and every DZ_TUNE_* / DZ_BEV_SCATTER variable
    the sources read, is a factor of a table or an exclusion with its reason - and nothing in the tables names a switch that is gone."""
    envs, attrs = rm.scan_switches()
    known_envs, known_attrs = rm.known_switches()
    assert len(envs) >= 20 and len(attrs) >= 20            # (the scan itself still finds them)
    assert not envs - known_envs, 'environment switches without a factor or an exclusion: %s' % sorted(envs - known_envs)
    assert not attrs - known_attrs, 'development switches without a factor or an exclusion: %s' % sorted(attrs - known_attrs)
    assert not known_envs - envs, 'the tables name variables the sources no longer read: %s' % sorted(known_envs - envs)
    for reason in list(rm.SWITCH_EXCLUSIONS.values()) + list(rm.VALUE_EXCLUSIONS.values()):
        assert isinstance(reason, str) and len(reason) > 20 and '\n' not in reason
    # every module / list-cell factor names an attribute that exists, with the default the table states
    for family in FAMILY_NAMES:
        for f in rm.table(family):
            if f.where[0] in ('module', 'cell'):
                cur = getattr(importlib.import_module(f.where[1]), f.where[2])
                assert (cur[0] if f.where[0] == 'cell' else cur) == f.default, f.name


def test_the_gpu_module_documents_every_factor():
    """The docstring of tests/test_gpu_route_matrix.py holds the factor table: every factor by name, with its relation."""
    import ast
    import os
    with open(os.path.join(rm.ROOT, 'tests', 'test_gpu_route_matrix.py')) as f:
        doc = ast.get_docstring(ast.parse(f.read()))
    lines = doc.splitlines()
    for family in FAMILY_NAMES:
        for f in rm.table(family):
            mine = [ln for ln in lines if ln.startswith('  ') and f.name in ln.split('True')[0].replace('|', ' ').split()]
            assert mine, f.name
            rel = 'bits' if 'bits' in {f.relation_of(v) for v in f.values} else 'oracle'
            assert any(rel in ln for ln in mine), (f.name, rel, mine)


def test_a_switch_added_later_without_a_row_fails_the_scan(tmp_path):
    """However the new switch is written: its variable read through os.environ.get, os.getenv or os.environ[...], in either quote; the
    `development switch` comment on the line or on the line above; a list cell; a continuation of the switch before it."""
    src = tmp_path / 'new_module.py'
    src.write_text("import os\nNEW_ROUTE = os.environ.get('DZ_TUNE_NEW_ROUTE', '1') != '0'   # development switch: 0 = the old route\n"
                   "OTHER = [True]      # development switch: list cell\nAND_MORE = [True]   # ... and its second half\nplain = 3\n"
                   "# development switch: the comment stands above\nABOVE = True\nNOT_ONE = 4\n"
                   'BY_GETENV = bool(os.getenv("DZ_TUNE_BY_GETENV"))\nBY_INDEX = os.environ["DZ_TUNE_BY_INDEX"]\n'
                   "class C:\n    def __init__(self):\n        self.knob = int(os.environ.get(\"DZ_TUNE_KNOB\", 1))\n")
    envs, attrs = rm.scan_switches(str(tmp_path))
    assert envs == {'DZ_TUNE_NEW_ROUTE', 'DZ_TUNE_BY_GETENV', 'DZ_TUNE_BY_INDEX', 'DZ_TUNE_KNOB'}
    assert attrs == {('detzero_amd.new_module', n) for n in ('NEW_ROUTE', 'OTHER', 'AND_MORE', 'ABOVE', 'BY_GETENV', 'BY_INDEX')}
    known_envs, known_attrs = rm.known_switches()
    assert envs - known_envs == envs and attrs - known_attrs == attrs
