"""Pairwise (all-pairs) matrix of the route switches above the kernels (test infrastructure, no GPU needed).

A FAMILY is a declarative table of factors.  A factor names one switch, where it lives, its values (the first one is the default
route), the condition under which it has any effect, and its relation to the default route:
  'bits'    the project promises bit identity with the default route (the promise is quoted in `promise`);
  'oracle'  no such promise - the row is held to the CPU oracle / the golden only.
`rows(family, cell)` turns a table into a deterministic covering array: every valid pair of (factor, value) - valid = some row exists
in which both factors have an effect - occurs in at least one row, no row sets a factor whose condition does not hold, and the list
depends on the table alone (greedy: of a fixed set of candidate rows the one that closes the most open pairs; no randomness).  `row_id(row)` spells a row's non-default settings.

A value may MASK a row (`masks`): a row with deliberately too small capacities checks nothing but the overflow flag, so in such a
row only the pairs that contain the masking value count as covered; every other pair needs a row without it.

`SWITCH_EXCLUSIONS` lists the switches of the sources that are no factor, each with its reason; `scan_switches()` reads the sources
(tests/test_route_matrix.py: a switch added later without a row or an exclusion fails there).
"""
import collections
import glob
import itertools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT = ('f16x2', 'bf16x2', 'f16')          # math modes on pair16 tensors
SPLIT2 = ('f16x2', 'bf16x2')                # ... of the second stage and the refiner


class Factor:
    """name; where = ('module', module, attr) | ('cell', module, attr) [a one-element list] | ('pipeline', attr) | ('ctor', argument)
    | ('engine', selector) [centerpoint.set_sparse_engine / set_dense_engine] | ('input',) | ('run', what);
    values (default first); needs = alternatives, each {factor: allowed values}, () = always effective; relation 'bits' | 'oracle'
    or {value: relation}; promise = where the bit identity is promised; env = the environment variables the sources read it from."""

    def __init__(self, name, where, values, needs=(), relation='oracle', promise='', env=(), masks=(), bits_unless=()):
        self.name, self.where, self.values = name, tuple(where), tuple(values)
        self.needs = tuple(dict(n) for n in needs)
        self.relation, self.promise, self.env, self.masks = relation, promise, tuple(env), tuple(masks)
        # settings of OTHER factors under which the promise is not made (each {factor: values}): the relation is 'oracle' there
        self.bits_unless = tuple(dict(n) for n in bits_unless)

    @property
    def default(self):
        return self.values[0]

    def relation_of(self, value, row=None):
        rel = self.relation[value] if isinstance(self.relation, dict) else self.relation
        if rel == 'bits' and row is not None and any(all(row[k] in v for k, v in alt.items()) for alt in self.bits_unless):
            return 'oracle'
        return rel


_DET, _OPS, _CP = 'detzero_amd.det_modules', 'detzero_amd.ops', 'detzero_amd.centerpoint'
_PDV, _REF = 'detzero_amd.pdv_modules', 'detzero_amd.refine_modules'
_XRUN_ON = ({'math': SPLIT, 'engine': ('xrun',)}, {'math': ('f32',), 'f32_engine': ('xrun', 'xrun_bf16x3')})

# ---------------------------------------------------------------------------------------------------------------- detector
# cell factors: a row is compared only inside its own (math, dynamic, input) cell
DETECTOR_CELL = [
    Factor('math', ('ctor', 'math'), ('f32', 'f16x2', 'bf16x2', 'f16')),
    Factor('dynamic', ('ctor', 'dynamic'), (False, True)),
    Factor('input', ('input',), ('stacked', 'list')),
]
DETECTOR = [
    Factor('ways', ('ctor', 'ways'), (1, 2), relation='bits', env=('DZ_TUNE_WAYS', 'DZ_TUNE_SPLIT_MIN'),
           promise='FramePipeline._call_split: "Frames are independent, so the results are those of the single pass bit for bit"'),
    Factor('PAD_RAGGED', ('module', _CP, 'PAD_RAGGED'), (True, False), needs=({'input': ('list',), 'dynamic': (False,)},), relation='bits',
           env=('DZ_TUNE_PAD_RAGGED',),
           promise='test_ragged_list_padded_route_equals_the_per_frame_route: "Same boxes bit for bit, same per-frame voxel sets"'),
    Factor('head_at_candidates', ('pipeline', 'head_at_candidates'), (True, False), relation='bits',
           promise='tests/test_gpu_head_candidates.py: "the criterion at both levels is bit identity with the full-map route"; not with '
                   'the bf16x3 dense engine - set_dense_engine: "the head-at-candidates kernel stay[s] where [it is]" while the full-map '
                   'head moves to "another accumulation order"',
           bits_unless=({'math': ('f32',), 'f32_dense_engine': ('bf16x3',)},)),
    Factor('SPARSE_BEV_INPUT', ('module', _DET, 'SPARSE_BEV_INPUT'), (True, False), needs=({'math': SPLIT},), env=('DZ_TUNE_SPARSE_BEV',)),
    Factor('SKIP_EMPTY_TILES', ('module', _DET, 'SKIP_EMPTY_TILES'), (True, False), needs=({'math': SPLIT, 'SPARSE_BEV_INPUT': (True,)},),
           relation='bits', env=('DZ_TUNE_SKIP_EMPTY_TILES',),
           promise='test_zero_response_tiles_do_not_change_a_bit: "Same detections, bit for bit, as with every tile computed"'),
    Factor('BEV_DENSE', ('module', _OPS, 'BEV_DENSE'), (True, False), needs=({'math': SPLIT, 'SPARSE_BEV_INPUT': (False,)},),
           env=('DZ_BEV_SCATTER',)),
    Factor('level_caps', ('pipeline', 'level_caps'), ('worst', 'fit', 'small'), relation={'worst': 'bits', 'fit': 'bits', 'small': 'oracle'},
           masks=('small',),
           promise='test_calibrated_capacities_and_overflow_flag: "Calibrated (measured x1.5) row capacities ... give bit-identical '
                   'detections to the worst-case capacities"'),
    Factor('captured', ('run', 'captured'), (False, True), relation='bits',
           promise='test_hip_graph_capture_of_frame_pipeline: "replays from a HIP graph and reproduces eager results" (torch.equal)'),
    Factor('dense_group', ('pipeline', 'dense_group'), (16, 2), env=('DZ_TUNE_DENSE_GROUP',)),
    Factor('GROUPED_DEEP_BLOCKS', ('module', _CP, 'GROUPED_DEEP_BLOCKS'), (True, False), needs=({'dense_group': (2,)},),
           env=('DZ_TUNE_GROUPED_DEEP',)),
    Factor('FIRST_BLOCK_WIDE_GROUPS', ('module', _DET, 'FIRST_BLOCK_WIDE_GROUPS'), (True, False),
           needs=({'dense_group': (2,), 'GROUPED_DEEP_BLOCKS': (True,)},), env=('DZ_TUNE_FIRST_BLOCK_WIDE',)),
    Factor('FUSED_DEBLOCK_PHASES', ('module', _DET, 'FUSED_DEBLOCK_PHASES'), (True, False), needs=({'math': SPLIT},),
           env=('DZ_TUNE_DEBLOCK_PHASES',)),
    Factor('STAGGERED_PYRAMID', ('module', _CP, 'STAGGERED_PYRAMID'), (True, False), env=('DZ_TUNE_EAGER_PYRAMID',)),
    Factor('PACKED_TABLES', ('module', _DET, 'PACKED_TABLES'), (False, True), needs=({'math': SPLIT},), env=('DZ_TUNE_PACKED_TABLES',)),
    Factor('engine', ('engine', 'engine'), ('xrun', 'gather'), needs=({'math': SPLIT},), env=('DZ_TUNE_SPCONV_ENGINE',)),
    Factor('f32_engine', ('engine', 'f32_engine'), ('gather', 'xrun', 'xrun_bf16x3'), needs=({'math': ('f32',)},),
           env=('DZ_TUNE_SPCONV_F32_ENGINE',)),
    Factor('f32_gather', ('engine', 'f32_gather'), ('mfma32', 'bf16x3'), needs=({'math': ('f32',)},), env=('DZ_TUNE_SPCONV_F32_GATHER',)),
    Factor('f32_dense_engine', ('engine', 'f32_dense_engine'), ('mfma32', 'bf16x3'), needs=({'math': ('f32',)},),
           env=('DZ_TUNE_DENSE_F32_ENGINE',)),
    Factor('FUSED_XWIN', ('module', _OPS, 'FUSED_XWIN'), (True, False), needs=_XRUN_ON, relation='bits', env=('DZ_TUNE_FUSED_XWIN',),
           promise='ops.neighbors_xrun: "what `build_windows(level.neighbors_to(level, ..., packed=True), level, channels)` returns, '
                   'bit for bit" (the same tables, so the same convolutions)'),
    Factor('XRUN_SORT', ('module', _OPS, 'XRUN_SORT'), (True, False), needs=_XRUN_ON, env=('DZ_TUNE_XRUN_SORT',)),
]

# ---------------------------------------------------------------------------------------------------------------- PDV second stage
PDV_CELL = [Factor('math', ('ctor', 'math'), ('f32', 'f16x2', 'bf16x2'))]
PDV = [
    Factor('FUSED_SA', ('cell', _PDV, 'FUSED_SA'), (True, False)),
    Factor('SPLIT_SA', ('cell', _PDV, 'SPLIT_SA'), (True, False), needs=({'math': SPLIT2, 'FUSED_SA': (True,)},)),
    Factor('PART_COUNTS_BINNED', ('module', _PDV, 'PART_COUNTS_BINNED'), (True, False), relation='bits', env=('DZ_TUNE_PART_BINNED',),
           promise='pdv_modules.part_counts: "dz_pdv_part_counts_binned: the same counts, bit for bit"'),
    Factor('FOLDED_ATTENTION', ('cell', _PDV, 'FOLDED_ATTENTION'), (True, False), needs=({'math': SPLIT2},)),
    Factor('FUSED_ENCODER', ('cell', _PDV, 'FUSED_ENCODER'), (True, False), needs=({'math': SPLIT2, 'FOLDED_ATTENTION': (True,)},)),
]

# ---------------------------------------------------------------------------------------------------------------- refiner (GRM / PRM)
REFINER_CELL = [Factor('math', ('ctor', 'math'), ('f32', 'f16x2', 'bf16x2'))]
REFINER = [
    Factor('FOLDED_XATTN', ('cell', _REF, 'FOLDED_XATTN'), (True, False)),
    Factor('SPLIT_ATTENTION', ('cell', _REF, 'SPLIT_ATTENTION'), (True, False), needs=({'math': SPLIT2},)),
    Factor('FUSED_CHAIN', ('cell', _REF, 'FUSED_CHAIN'), (True, False), needs=({'math': SPLIT2},)),
    Factor('FUSED_POINTNET', ('cell', _REF, 'FUSED_POINTNET'), (True, False), needs=({'math': SPLIT2},)),
]

FAMILIES = {'detector': (DETECTOR_CELL, DETECTOR), 'pdv': (PDV_CELL, PDV), 'refiner': (REFINER_CELL, REFINER)}

# switches of the sources that are NO factor: environment variable or (module file, attribute) -> one-line reason
SWITCH_EXCLUSIONS = {
    'DZ_TUNE_SIDE_PRIORITY': 'performance only: the priority of the index pyramid\'s side stream, no second code path',
    'DZ_TUNE_LAYOUT': 'experimental build only: the brick row order serves the tile engine; set_engine derives the layout from the engine',
    'DZ_TUNE_SPCONV_TILE_COUTS': 'experimental build only: the widths of the tile engine (DZ_BUILD_EXPERIMENTAL=1)',
    'DZ_TUNE_XRUN_COUTS': 'a width filter of the x-run engine, read from the environment at every call (no attribute to set): every '
                          'width goes to one of the two engines the `engine` / `f32_engine` factors already run',
    'DZ_TUNE_XRUN_SORT_MIN': 'a width threshold of XRUN_SORT, not a route of its own: the factor XRUN_SORT runs both sides of it',
    (_OPS, 'XRUN_SORT_MIN_CHANNELS'): 'the attribute behind DZ_TUNE_XRUN_SORT_MIN: a width threshold, the factor XRUN_SORT runs both sides of it',
}
# values of a factor that stay out, with their reason
VALUE_EXCLUSIONS = {
    ('engine', 'tiles'): 'experimental build only: set_engine refuses it by name in a default build (asserted beside the matrix)',
}


def table(family):
    return FAMILIES[family][1]


def cell_table(family):
    return FAMILIES[family][0]


# ---------------------------------------------------------------------------------------------------------------- generator
def _index(factors):
    return collections.OrderedDict((f.name, f) for f in factors)


def _complete(assign, facs):
    """Smallest extension of the partial assignment {factor: value} in which every assigned ROW factor has an effect (one of its
    alternatives holds, the factors it names assigned and effective themselves), or None.  Deterministic: alternatives and values in
    table order."""
    for name in assign:
        f = facs[name]
        if not f.needs or any(all(k in assign and assign[k] in v for k, v in alt.items()) for alt in f.needs):
            continue
        for alt in f.needs:
            if any(k in assign and assign[k] not in v for k, v in alt.items()):
                continue
            missing = [k for k in alt if k not in assign]
            for combo in itertools.product(*[alt[k] for k in missing]):
                got = _complete(dict(assign, **dict(zip(missing, combo))), facs)
                if got is not None:
                    return got
        return None
    return dict(assign)


def effective(name, row, facs):
    """Whether factor `name` has any effect in the (full) row."""
    f = facs[name]
    return not f.needs or any(all(row[k] in v and effective(k, row, facs) for k, v in alt.items()) for alt in f.needs)


def masked(row, facs):
    """The (factor, value) of the row that masks it, or None."""
    for name, v in row.items():
        if v in facs[name].masks:
            return (name, v)
    return None


def valid_pairs(family, cell):
    """Every unordered pair of (factor, value) of the family's row factors for which a row exists in the cell where both have an effect."""
    cells, rows_ = FAMILIES[family]
    facs = _index(cells + rows_)
    out = []
    names = [f.name for f in rows_]
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for va in facs[a].values:
                for vb in facs[b].values:
                    if _complete(dict(cell, **{a: va, b: vb}), facs) is not None:
                        out.append(((a, va), (b, vb)))
    return out


def covered_pairs(row, facs, row_names):
    """The pairs a full row covers: both factors effective; in a masked row only the pairs that contain the masking value."""
    act = [(n, row[n]) for n in row_names if effective(n, row, facs)]
    m = masked(row, facs)
    return {(a, b) for a, b in itertools.combinations(act, 2) if m is None or m in (a, b)}


# How the rows are built (`_build_rows`), and what must stay true when it is changed:
#   - `_complete` is the only place that knows the conditions: it extends a partial assignment until every factor in it has an
#     effect, or says that it cannot.  A row is `default` overlaid with such an assignment, so no row can break a condition.
#   - a row is grown from a SEED pair (an open pair; this guarantees progress: every row closes at least its seed) by giving each
#     further factor the value that closes the most open pairs with what the row already holds (`candidate`).
#   - a masking value (too small capacities) enters a row only through its seed, and then only pairs that contain it count -
#     `covered_pairs` applies the same rule, and it is the single definition of "covered" for the generator and for the CPU test.
#   - correctness does not depend on the heuristics: the loop ends only when no valid pair is open, and tests/test_route_matrix.py
#     recomputes the valid pairs by brute force.  SEEDS and the two factor orders only make the list shorter: a dependent factor
#     (FIRST_BLOCK_WIDE_GROUPS needs dense_group = 2 ...) is only reachable in table order if its parent already chose the right value,
#     the reverse order lets it choose for its parent; of the candidates the one that closes the most pairs is kept.  16 seeds took
#     the detector from 206 rows (one seed, table order) to 164; the floor is about 16 rows per split cell, because the two dependent
#     chains (SPARSE_BEV_INPUT -> SKIP_EMPTY_TILES | BEV_DENSE, dense_group -> GROUPED_DEEP_BLOCKS -> FIRST_BLOCK_WIDE_GROUPS) each
#     have four end states that must all meet.
SEEDS = 16          # open pairs tried as the seed of each new row


_ROWS = {}           # (family, cell) -> rows: the table is fixed, so are they


def rows(family, cell):
    """The covering rows of `family` inside `cell` ({cell factor: value}): full {factor: value} dicts, the all-default row first."""
    key = (family, tuple(sorted(cell.items())))
    if key not in _ROWS:
        _ROWS[key] = _build_rows(family, cell)
    return [dict(r) for r in _ROWS[key]]


def _build_rows(family, cell):
    cells, rows_ = FAMILIES[family]
    facs = _index(cells + rows_)
    names = [f.name for f in rows_]
    default = dict(cell, **{n: facs[n].default for n in names})
    out = [default]
    todo = [p for p in valid_pairs(family, cell) if p not in covered_pairs(default, facs, names)]
    def candidate(seed, order, open_):
        part = _complete(dict(cell, **dict(seed)), facs)
        mask = next((fv for fv in seed if fv[1] in facs[fv[0]].masks), None)
        for name in order:
            if name in part:
                continue
            # the value that covers the most open pairs with what the row already holds; ties go to the value with the most open
            # pairs left anywhere, then to the first value (the default)
            best, best_score = None, (0, 0)
            for v in facs[name].values:
                if mask is None and v in facs[name].masks:
                    continue
                got = _complete(dict(part, **{name: v}), facs)
                if got is None:
                    continue
                mine = (name, v)
                score = (sum(1 for o in got.items() if o[0] in names and o != mine and (mask is None or mask in (o, mine))
                             and ((o, mine) in open_ or (mine, o) in open_)),
                         sum(1 for p in open_ if mine in p and (mask is None or mask in p)))
                if best is None or score > best_score:
                    best, best_score = got, score
            if best is not None:
                part = best
        return dict(default, **part)

    while todo:
        # candidates: the first open pairs as seeds, the factors in table order and in reverse (a dependent factor first switches
        # the factors it needs); the row that closes the most open pairs goes in, ties to the first candidate
        open_ = set(todo)
        row, gain = None, -1
        for seed in todo[:SEEDS]:
            for order in (names, names[::-1]):
                cand = candidate(seed, order, open_)
                g = len(covered_pairs(cand, facs, names) & open_)
                if g > gain:
                    row, gain = cand, g
        # a factor without effect in the row stays at its default
        assert all(row[n] == facs[n].default or effective(n, row, facs) for n in names), row
        assert gain > 0, row
        out.append(row)
        done = covered_pairs(row, facs, names)
        todo = [p for p in todo if p not in done]
    # a value whose factor has no partner in the cell (no pair to cover) still gets its row
    for name in names:
        for v in facs[name].values:
            if any(r[name] == v and effective(name, r, facs) and masked(r, facs) in (None, (name, v)) for r in out):
                continue
            part = _complete(dict(cell, **{name: v}), facs)
            if part is not None:
                out.append(dict(default, **part))
    return out


def cells(family):
    """The cells of a family: rows of the cell table covering every pair of cell factors (the detector: 8 of the 16)."""
    cf = FAMILIES[family][0]
    names = [f.name for f in cf]
    if len(cf) == 1:
        return [{names[0]: v} for v in cf[0].values]
    pairs = [((a.name, va), (b.name, vb)) for a, b in itertools.combinations(cf, 2) for va in a.values for vb in b.values]
    full = [dict(zip(names, combo)) for combo in itertools.product(*[f.values for f in cf])]
    out = []
    while pairs:
        # the assignment that covers the most pairs still open; ties go to the first in table order
        best = max(full, key=lambda c: sum(1 for p in pairs if all(c[n] == v for n, v in p)))
        out.append(best)
        pairs = [p for p in pairs if not all(best[n] == v for n, v in p)]
    return out


def non_default(row, family):
    cells_, rows_ = FAMILIES[family]
    return [(f.name, row[f.name]) for f in rows_ if row[f.name] != f.default]


def row_id(row, family):
    """'<cell>-<non-default settings>', e.g. 'f16x2.dyn0.list-ways=2+PAD_RAGGED=False'; the all-default row ends in 'default'."""
    cells_, _ = FAMILIES[family]
    cell = '.'.join(('%s' % row[f.name]) if not isinstance(row[f.name], bool) else '%s%d' % (f.name[:3], row[f.name]) for f in cells_)
    nd = non_default(row, family)
    return cell + '-' + ('+'.join('%s=%s' % (n, v) for n, v in nd) if nd else 'default')


def bits_required(row, family):
    """Bit identity with the cell's all-default row is required when every non-default factor of the row promises it."""
    facs = _index(table(family))
    nd = non_default(row, family)
    return bool(nd) and all(facs[n].relation_of(v, row) == 'bits' for n, v in nd)


def bits_base(row, family):
    """The row with every factor of relation 'bits' back at its default: the route whose results the row must reproduce bit for bit
    (the promises are made against the default route; the other switches are the same on both sides of the comparison).  Equal to
    the cell's all-default row exactly when `bits_required`.  None when the row flips no such factor, or is masked."""
    cells_, rows_ = FAMILIES[family]
    facs = _index(cells_ + rows_)
    flipped = [n for n, v in non_default(row, family) if facs[n].relation_of(v, row) == 'bits']
    if not flipped or masked(row, facs) is not None:
        return None
    base = dict(row, **{n: facs[n].default for n in flipped})
    assert all(base[f.name] == f.default or effective(f.name, base, facs) for f in rows_), base
    return base


def all_rows(family):
    return [r for c in cells(family) for r in rows(family, c)]


# ---------------------------------------------------------------------------------------------------------------- completeness
_ENV = re.compile(r'DZ_TUNE_[A-Z0-9_]+|DZ_BEV_SCATTER')              # the variable's name anywhere in the text, however it is read
_ASSIGN = re.compile(r'^([A-Z][A-Z0-9_]*)\s*=')                      # a module-level assignment (no indentation)
_MARK = 'development switch'


def scan_switches(src_dir=None):
    """-> (environment variables named, [(module, attribute)] of the module-level switch assignments) of detzero_amd/*.py.
    A variable counts wherever its name stands (os.environ.get, os.getenv, os.environ[...], either quote, a comment).  A module-level
    assignment is a switch when it carries the comment `development switch` on its own line or in the comment lines directly above
    it, when its right-hand side names one of the variables, or when its comment continues ('...') the switch on the line before."""
    src_dir = src_dir or os.path.join(ROOT, 'detzero_amd')
    envs, attrs = set(), set()
    for path in sorted(glob.glob(os.path.join(src_dir, '*.py'))):
        mod = 'detzero_amd.' + os.path.basename(path)[:-3]
        with open(path) as f:
            lines = f.read().splitlines()
        above = prev = False                   # the comment block directly above is marked / the line before was a switch assignment
        for line in lines:
            envs.update(_ENV.findall(line))
            if line.startswith('#'):
                above, prev = above or _MARK in line, False
                continue
            m = _ASSIGN.match(line)
            comment = line.split('#', 1)[1].strip() if '#' in line else ''
            is_switch = bool(m) and (above or _MARK in comment or bool(_ENV.search(line.split('#', 1)[0])) or (prev and comment.startswith('...')))
            if is_switch:
                attrs.add((mod, m.group(1)))
            above, prev = False, is_switch
    return envs, attrs


def known_switches():
    """-> (environment variables, (module, attribute) pairs) the tables account for: factors and exclusions."""
    envs = set(k for k in SWITCH_EXCLUSIONS if isinstance(k, str))
    attrs = set(k for k in SWITCH_EXCLUSIONS if isinstance(k, tuple))
    for _, rows_ in FAMILIES.values():
        for f in rows_:
            envs.update(f.env)
            if f.where[0] in ('module', 'cell'):
                attrs.add((f.where[1], f.where[2]))
    return envs, attrs


def describe(family):
    """The factor table as text (the GPU module's docstring carries it)."""
    lines = []
    for f in table(family):
        rel = f.relation if isinstance(f.relation, str) else ', '.join('%s: %s' % kv for kv in f.relation.items())
        lines.append('  %-24s %-34s %-8s %s' % (f.name, ' | '.join(str(v) for v in f.values), rel, f.promise or '-'))
    return '\n'.join(lines)
