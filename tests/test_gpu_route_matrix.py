"""GPU (MI355X): the route switches above the kernels, flipped in PAIRS (tests/route_matrix.py builds the covering rows; its CPU tests
are tests/test_route_matrix.py).  Every row runs on a fresh model (a deep copy of one CPU model, moved to the device, and a fresh
FramePipeline built after the switches are set), so no cached plan of another row is in play.

A row asserts
  (a) oracle    per frame, boxes against tests.util.oracle_detect (computed once per frame and voxelizer) with match_boxes at the
                project's own numbers: 1e-3 for f32 / f16x2 (tests/test_gpu_e2e.py), 1e-2 for bf16x2 (BOX_TOL of
                tests/test_gpu_full_parity.py: 16-bit pairs are not fp32-class), 3e-2 for f16 with its count allowance of 3
                (tests/test_gpu_f16.py); at most 2 oracle boxes of a frame unmatched; every ordinary frame has >= 30 oracle boxes;
  (b) bits      torch.equal on counts and boxes[:count] against the SAME row with its 'bits' factors back at their defaults (the
                cell's all-default row when nothing else is flipped), in every cell: the dynamic voxelizer sums 64-bit fixed-point
                integers (csrc/voxelize.hip k_dyn_accumulate: "the result does not depend on the order the atomics land in");
  (c) overflow  check_overflow() is clean - except with level_caps = [64, 64, 64, 64] (the values of
                test_calibrated_capacities_and_overflow_flag), where the row asserts only that the flag is raised and reaches the
                parent pipeline, and that every route of the row ran;
  (d) routes    every factor's route is shown to have run (or not to have run) by call counters on the launch wrappers, the plan
                key ('zero_resp', ...) and the skippable-tile counts of dz_bev_tile_list.
Captured rows run eagerly on the frames, are captured on OTHER frames of the same shapes, refilled and replayed once; the replay is
what (a) and (b) see, and it equals the eager result of the same pipeline bit for bit.

Frames (tests.util.make_model): [20 000 points, all points out of range, 18 000 points, ONE point in range, 16 000 points]; as a
ragged list, and stacked with out-of-range rows up to the longest.  Two concurrent sub-passes get frames [0:2] and [2:5];
dense_group = 2 makes groups (0,1) (2,3) (4).  Every row runs on the 0.2 m grid; the rows with the sparse BEV input run again on the
0.1 m grid with the same frames, because the resident-tile kernel - the one that leaves zero-response tiles out - takes a layer only
from 384 pixel tiles per launch: never at 0.2 m (36 tiles per frame), at 0.1 m from three frames per launch (144 per frame).  Both
sizes are asserted as what they are (`tiles_resident` / `tiles_generic` below).

Factor table (route_matrix.DETECTOR; cells = math x dynamic x input, 8 of the 16 cover their pairs):
  factor                   values                       relation  where the relation is promised
  ways                     1 | 2 (split_min = 4)        bits      FramePipeline._call_split: "the results are those of the single pass bit for bit"
  PAD_RAGGED               True | False                 bits      test_ragged_list_padded_route_equals_the_per_frame_route: "Same boxes bit for bit"
  head_at_candidates       True | False                 bits      tests/test_gpu_head_candidates.py: "bit identity with the full-map route"; oracle with
                                                                  f32_dense_engine = bf16x3: set_dense_engine keeps the candidates kernel on the
                                                                  fp32 matrix cores while the full-map head runs "in another accumulation order"
  SPARSE_BEV_INPUT         True | False                 oracle    -
  SKIP_EMPTY_TILES         True | False                 bits      test_zero_response_tiles_do_not_change_a_bit: "Same detections, bit for bit"
  BEV_DENSE                True | False                 oracle    -
  level_caps               worst | fit | small          bits      test_calibrated_capacities_and_overflow_flag: "bit-identical detections to the
                                                                  worst-case capacities" (small: the overflow flag only)
  captured                 False | True                 bits      test_hip_graph_capture_of_frame_pipeline: "reproduces eager results"
  dense_group              16 | 2                       oracle    - (another launch size selects another convolution instance)
  GROUPED_DEEP_BLOCKS      True | False                 oracle    -
  FIRST_BLOCK_WIDE_GROUPS  True | False                 oracle    -
  FUSED_DEBLOCK_PHASES     True | False                 oracle    -
  STAGGERED_PYRAMID        True | False                 oracle    -
  PACKED_TABLES            False | True                 oracle    -
  engine                   xrun | gather                oracle    -
  f32_engine               gather | xrun | xrun_bf16x3  oracle    -
  f32_gather               mfma32 | bf16x3              oracle    -
  f32_dense_engine         mfma32 | bf16x3              oracle    -
  FUSED_XWIN               True | False                 bits      ops.neighbors_xrun: "what `build_windows(...)` returns, bit for bit"
  XRUN_SORT                True | False                 oracle    -
PDV second stage (route_matrix.PDV; cells = math f32 | f16x2 | bf16x2; tests/golden/pdv_golden.npz at tests/test_pdv.py's tolerances):
  FUSED_SA                 True | False                 oracle    -
  SPLIT_SA                 True | False                 oracle    -
  PART_COUNTS_BINNED       True | False                 bits      pdv_modules.part_counts: "the same counts, bit for bit" (the count column)
  FOLDED_ATTENTION         True | False                 oracle    -
  FUSED_ENCODER            True | False                 oracle    -
Refiner, GRM and PRM (route_matrix.REFINER; same cells; tests/golden/refine_golden.npz at tests/test_refine.py's tolerances):
  FOLDED_XATTN | SPLIT_ATTENTION | FUSED_CHAIN | FUSED_POINTNET   True | False   oracle   -
Conditions, exclusions and their reasons: tests/route_matrix.py.
"""
import collections
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from detzero_amd.synth import VOXEL_SIZE_01, VOXEL_SIZE_02
from tests import route_matrix as rm
from tests.util import cpu_state_dict, make_model, masked_frame, match_boxes, oracle_detect

pytestmark = pytest.mark.gpu

BOX_TOL = {'f32': 1e-3, 'f16x2': 1e-3, 'bf16x2': 1e-2, 'f16': 3e-2}
COUNT_ALLOWANCE = {'f32': 2, 'f16x2': 2, 'bf16x2': 2, 'f16': 3}
UNMATCHED = 2                      # oracle boxes of a frame that may go unmatched: on-threshold score / NMS decisions
SMALL_CAPS = [64, 64, 64, 64]
ORDINARY = (0, 2, 4)
FAR = 1.0e6                        # x of a padding row: outside the range, dropped by the xy mask inside the kernels

DET_ROWS = rm.all_rows('detector')
# the grids: every row on the small detector (0.2 m voxels, 94 x 94 BEV cells); the rows with the sparse BEV input (split math modes,
# SPARSE_BEV_INPUT on: where SKIP_EMPTY_TILES has its effect) again at 0.1 m (188 x 188): at 0.2 m five frames are 180 pixel tiles per launch, under the 384 from which the layers behind the sparse-input convolution run
# on the resident-tile kernel - there the generic kernel computes every pixel and the fill rewrites the skippable tiles, which is a
# route of its own, but not the one SKIP_EMPTY_TILES exists for
GRIDS = {'0.2m': VOXEL_SIZE_02, '0.1m': VOXEL_SIZE_01}
DET_CASES = [('0.2m', r) for r in DET_ROWS] + [('0.1m', r) for r in DET_ROWS if r['math'] != 'f32' and r['SPARSE_BEV_INPUT']]
PDV_ROWS = rm.all_rows('pdv')
REF_ROWS = rm.all_rows('refiner')


def _ids(rows, family):
    return [rm.row_id(r, family) for r in rows]


# ---------------------------------------------------------------------------------------------------------------- frames and oracle
def _pad(pts, n):
    out = np.zeros((n, pts.shape[1]), np.float32)
    out[:, 0] = FAR
    out[:pts.shape[0]] = pts[:n]
    return out


def _frame_sets():
    """-> (A, B): the frames of every row, and the frames a captured row is captured on (same lengths, other points, no empty slot)."""
    far = masked_frame(5, 3000).copy()
    far[:, 0] += 1000.0
    one = _pad(masked_frame(7, 2000)[:1], 1000)
    a = [masked_frame(0, 20000), far, masked_frame(12, 18000), one, masked_frame(11, 16000)]
    b = [_pad(masked_frame(40 + i, 20000), f.shape[0]) for i, f in enumerate(a)]
    return a, b


@pytest.fixture(scope='module')
def dets():
    """Per grid, built at its first use: one CPU model, the frames, and the CPU oracle's boxes per (frame, dynamic) - computed once,
    never changed - and the results of the rows already run."""
    return {}


@pytest.fixture(scope='module')
def det(dets):
    return _det(dets, '0.2m')


def _det(dets, grid):
    if grid not in dets:
        dets[grid] = _build_det(grid)
    return dets[grid]


def _build_det(grid):
    model, cfg, info = make_model(GRIDS[grid], seed=0)
    sd = cpu_state_dict(model)
    a, b = _frame_sets()
    refs = {}
    for dyn in (False, True):
        for i, f in enumerate(a):
            rb = oracle_detect(sd, f, info, dynamic=dyn)['final'][0]
            refs[(i, dyn)] = (rb['pred_boxes'].numpy().copy(), rb['pred_scores'].numpy().copy())
            refs[(i, dyn)][0].setflags(write=False)
            refs[(i, dyn)][1].setflags(write=False)
    for dyn in (False, True):
        for i in ORDINARY:
            assert refs[(i, dyn)][0].shape[0] >= 30, (i, dyn, refs[(i, dyn)][0].shape)      # two unmatched boxes cannot hide a broken frame
        assert refs[(1, dyn)][0].shape[0] == 0 and refs[(3, dyn)][0].shape[0] == 0      # (the rows then require no box there either)
    return {'grid': grid, 'model': model, 'info': info, 'a': a, 'b': b, 'refs': refs, 'results': {}}


def _inputs(frames, form, device):
    if form == 'stacked':
        n = max(f.shape[0] for f in frames)
        return torch.from_numpy(np.stack([_pad(f, n) for f in frames])).to(device)
    return [torch.from_numpy(f).to(device) for f in frames]


def _refill(static, new):
    if torch.is_tensor(static):
        static.copy_(new)
    else:
        for s, n in zip(static, new):
            s.copy_(n)


# ---------------------------------------------------------------------------------------------------------------- route evidence
class Evidence(collections.Counter):
    """Call counters of the launch wrappers a route goes through (the pattern of tests/test_gpu_head_candidates.py::_count_calls)."""

    def __init__(self):
        super().__init__()
        self.tile_lists, self.level0_batches, self.run_batches = [], [], []

    def wrap(self, mp, obj, name, note=None, key=None):
        real, key = getattr(obj, name), key or name

        def counted(*a, **k):
            self[key] += 1
            if note is not None:
                note(a, k)
            return real(*a, **k)
        mp.setattr(obj, name, counted)
        return real


def _watch_detector(mp, ev):
    from detzero_amd import det_modules as dm
    from detzero_amd import ops
    lib = ops.L.load()
    for name in ('voxelize_to_level', 'voxelize_hard_mean_into', 'voxelize_dynamic_nosync', 'head_at_candidates', 'bev_row_index',
                 'sparse_to_bev', 'build_windows'):
        ev.wrap(mp, ops, name)

    def fill_note(a, k):
        ev['fill_zero_resp'] += (k.get('zero_resp') is not None)
    ev.wrap(mp, ops, 'bev_fill_empty_tiles', fill_note)
    real_list = ops.bev_tile_list

    def tile_list(*a, **k):
        ev['bev_tile_list'] += 1
        lst = real_list(*a, **k)
        if not torch.cuda.is_current_stream_capturing():
            ev.tile_lists.append(lst)
        return lst
    mp.setattr(ops, 'bev_tile_list', tile_list)
    real_xrun = ops.neighbors_xrun

    def neighbors_xrun(*a, **k):
        ev['neighbors_xrun'] += 1
        ev['in_xrun'] += 1
        try:
            return real_xrun(*a, **k)
        finally:
            ev['in_xrun'] -= 1
    mp.setattr(ops, 'neighbors_xrun', neighbors_xrun)

    def nbr_note(a, k):
        if k.get('packed') and not ev['in_xrun']:
            ev['packed_plain_table'] += 1
    ev.wrap(mp, ops.SparseLevel, 'neighbors_to', nbr_note)

    def spconv_note(a, k):
        nbr = a[1]
        xwin = getattr(nbr, 'xwin', None)
        ev['spconv_xwin'] += xwin is not None
        ev['spconv_xwin_sorted'] += xwin is not None and xwin[2] is not None
        ev['spconv_packed_gather'] += xwin is None and bool(getattr(nbr, 'packed', False))
        ev['spconv_x_limb3'] += k.get('f32_engine') == 'xrun_bf16x3'
        ev['spconv_g_limb3'] += k.get('f32_gather') == 'bf16x3'
    ev.wrap(mp, ops, 'spconv_forward', spconv_note)

    def conv2d_note(a, k):
        ev['conv2d_limb3'] += k.get('f32_engine') == 'bf16x3'
        if k.get('tiles') is not None and a[0].get('in_rowidx') is None:
            # a layer behind the sparse-input convolution that was handed a tile list: the kernel the library selects for it (host only)
            name = lib.dz_conv2d_variant_split(ctypes.byref(ops._conv2d_desc(a[0])), 1 if k.get('out_f32') else 0).decode()
            ev['tiles_resident' if name.startswith('k_conv3x3_h') else 'tiles_generic'] += 1
    ev.wrap(mp, ops, 'conv2d', conv2d_note)

    def layer_note(a, k):
        ev['deblock_phase_groups'] += bool(k.get('phase_groups'))
    ev.wrap(mp, dm, 'conv_layer', layer_note)

    def pyramid_note(a, k):
        ev['pyramid_staggered'] += bool(k.get('staggered'))
    ev.wrap(mp, dm.VoxelResBackBone8x, 'build_pyramid', pyramid_note)
    ev.wrap(mp, dm.BaseBEVBackbone, 'run', lambda a, k: ev.run_batches.append(int(a[2])), key='bev_run')
    ev.wrap(mp, dm.BaseBEVBackbone, 'run_grouped', key='bev_run_grouped')

    def level_note(a, k):
        if int(a[1]) == 0:
            ev.level0_batches.append(int(a[7]))
    ev.wrap(mp, dm.BaseBEVBackbone, '_level_convs', level_note)
    ev.wrap(mp, lib, 'dz_sparse_to_bev_split_dense', key='lib_bev_dense')
    ev.wrap(mp, lib, 'dz_sparse_to_bev_split', key='lib_bev_scatter')


def _check_detector_routes(row, ev, pipe, model, nb, grid):
    """Every factor of the row: its route ran, and the route it replaces did not (where the two exclude each other)."""
    split = row['math'] != 'f32'
    rid = rm.row_id(row, 'detector')
    # input form, voxelizer, PAD_RAGGED
    if row['dynamic']:
        assert ev['voxelize_dynamic_nosync'] > 0 and ev['voxelize_to_level'] == 0 and ev['voxelize_hard_mean_into'] == 0, (rid, ev)
    elif row['input'] == 'stacked' or row['PAD_RAGGED']:
        assert ev['voxelize_to_level'] > 0 and ev['voxelize_hard_mean_into'] == 0, (rid, ev)
    else:
        assert ev['voxelize_hard_mean_into'] >= nb and ev['voxelize_to_level'] == 0, (rid, ev)
    assert (pipe._subs is not None) == (row['ways'] == 2), rid
    assert (ev['head_at_candidates'] > 0) == row['head_at_candidates'], (rid, ev)
    # BEV hand-over
    sparse_bev = split and row['SPARSE_BEV_INPUT']
    assert (ev['bev_row_index'] > 0) == sparse_bev and (ev['sparse_to_bev'] > 0) == (not sparse_bev), (rid, ev)
    if sparse_bev and row['SKIP_EMPTY_TILES']:
        assert ev['bev_tile_list'] > 0 and ev['bev_fill_empty_tiles'] > ev['fill_zero_resp'] > 0, (rid, ev)       # first layer + the five behind it
        assert any(isinstance(k, tuple) and k[0] == 'zero_resp' for k in model.backbone2d.plan()[0]), rid
        skipped = sum(int(t[:, 1].sum()) for t in ev.tile_lists)
        assert skipped > 0, (rid, 'no tile was skippable')
        # the layers that were handed a list: on the resident-tile kernel, which leaves the listed tiles out, from 384 tiles per launch
        # (three frames at 0.1 m); below that on the generic kernel, which computes every pixel (the fill rewrites the skippable tiles)
        if grid == '0.1m' and max(ev.level0_batches) >= 3:
            assert ev['tiles_resident'] > 0, (rid, ev)
        else:
            assert ev['tiles_generic'] > 0 and (ev['tiles_resident'] == 0 or grid == '0.1m'), (rid, ev)
    else:
        assert ev['bev_tile_list'] == 0 and ev['bev_fill_empty_tiles'] == 0, (rid, ev)
    if split and not row['SPARSE_BEV_INPUT']:
        assert (ev['lib_bev_dense'] > 0) == row['BEV_DENSE'] and (ev['lib_bev_scatter'] > 0) == (not row['BEV_DENSE']), (rid, ev)
    # frame groups of the dense stage
    if row['dense_group'] == 2:
        assert max(ev.run_batches + [0]) <= 2, (rid, ev.run_batches)
        if row['GROUPED_DEEP_BLOCKS']:
            assert ev['bev_run_grouped'] > 0, (rid, ev)
            wide = [b for b in ev.level0_batches if b > 2]
            assert bool(wide) == row['FIRST_BLOCK_WIDE_GROUPS'], (rid, ev.level0_batches)
        else:
            assert ev['bev_run_grouped'] == 0 and ev['bev_run'] >= 3, (rid, ev)
    else:
        assert ev['bev_run_grouped'] == 0 and max(ev.run_batches) == (nb if row['ways'] == 1 else nb - nb // 2), (rid, ev.run_batches)
    if split:
        assert (ev['deblock_phase_groups'] > 0) == row['FUSED_DEBLOCK_PHASES'], (rid, ev)
        assert (ev['packed_plain_table'] > 0) == row['PACKED_TABLES'] == (ev['spconv_packed_gather'] > 0), (rid, ev)
    assert (ev['pyramid_staggered'] > 0) == row['STAGGERED_PYRAMID'], (rid, ev)
    # sparse engines
    xrun = (row['engine'] == 'xrun') if split else (row['f32_engine'] != 'gather')
    assert (ev['neighbors_xrun'] > 0) == xrun == (ev['spconv_xwin'] > 0), (rid, ev)
    if xrun:
        assert (ev['build_windows'] == 0) == row['FUSED_XWIN'], (rid, ev)
        assert (ev['spconv_xwin_sorted'] > 0) == row['XRUN_SORT'], (rid, ev)
    assert (ev['spconv_x_limb3'] > 0) == (row['f32_engine'] == 'xrun_bf16x3'), (rid, ev)
    assert (ev['spconv_g_limb3'] > 0) == (row['f32_gather'] == 'bf16x3'), (rid, ev)
    assert (ev['conv2d_limb3'] > 0) == (row['f32_dense_engine'] == 'bf16x3'), (rid, ev)


# ---------------------------------------------------------------------------------------------------------------- one detector row
def _set_module_switches(mp, row, family):
    import importlib
    for f in rm.table(family):
        if f.where[0] == 'module':
            mp.setattr(importlib.import_module(f.where[1]), f.where[2], row[f.name])
        elif f.where[0] == 'cell':
            mp.setattr(importlib.import_module(f.where[1]), f.where[2], [row[f.name]])       # (a one-element list, read as NAME[0])


def _same_boxes(a, b, what):
    """Counts and boxes[:count] per frame: torch.equal."""
    (out, cnt), (out2, cnt2) = a, b
    assert torch.equal(cnt, cnt2), (what, cnt.tolist(), cnt2.tolist())
    for i in range(cnt.shape[0]):
        n = int(cnt[i])
        assert torch.equal(out[i, :n], out2[i, :n]), (what, 'frame %d' % i, float((out[i, :n] - out2[i, :n]).abs().max()))


def _run_detector_row(row, det, device):
    """The row on a fresh model -> (boxes (B, K, 9), counts (B,)) on the host, or None for a row on too small capacities."""
    from detzero_amd import centerpoint as cpm
    from detzero_amd.lib import DetZeroHipError
    rid = rm.row_id(row, 'detector')
    with pytest.MonkeyPatch.context() as mp:
        _set_module_switches(mp, row, 'detector')
        model = copy.deepcopy(det['model']).to(device)
        cpm.set_sparse_engine(model, row['engine'], row['f32_engine'], row['f32_gather'])
        cpm.set_dense_engine(model, row['f32_dense_engine'])
        pipe = cpm.FramePipeline(model, det['info'], dynamic=row['dynamic'], math=row['math'], ways=row['ways'])
        pipe.split_min = 4                       # (the default splits batches of 12 frames and more)
        pipe.head_at_candidates = row['head_at_candidates']
        pipe.dense_group = row['dense_group']
        inp_a, inp_b = _inputs(det['a'], row['input'], device), _inputs(det['b'], row['input'], device)
        nb = len(det['a'])
        assert pipe.splits(nb) == (row['ways'] == 2)
        if row['level_caps'] == 'fit':
            caps = pipe.calibrate([torch.from_numpy(f).to(device) for k, f in enumerate(det['a'] + det['b']) if k % nb in ORDINARY])
            assert len(caps) == 4 and all(c > 4096 for c in caps)
        elif row['level_caps'] == 'small':
            pipe.level_caps = list(SMALL_CAPS)
        ev = Evidence()
        _watch_detector(mp, ev)
        small = row['level_caps'] == 'small'
        if row['captured']:
            static = inp_a.clone() if torch.is_tensor(inp_a) else [f.clone() for f in inp_a]
            eo, en = pipe(static)
            eager = (eo.clone(), en.clone())
            _refill(static, inp_b)
            pipe(static)                         # (two eager passes, the second on the shapes and the stream state of the capture)
            torch.cuda.synchronize()
            cap = pipe.capture(static)
            assert cap.branches == row['ways']
            _refill(static, inp_a)
            cap.replay()
            torch.cuda.synchronize()
            out, cnt = cap.boxes, cap.counts
            if not small:
                _same_boxes((out, cnt), eager, rid + ': replay against the eager pass on the same frames')
        else:
            out, cnt = pipe(inp_a)
            torch.cuda.synchronize()
        if small:
            if not row['captured']:
                assert bool(pipe.last_overflow.item()), rid
            with pytest.raises(DetZeroHipError, match='overflowed'):
                pipe.check_overflow()            # (with two sub-passes: the flag of a sub-pass reached the parent)
            pipe.check_overflow()                # read and cleared
        else:
            if row['level_caps'] == 'fit' and not row['captured']:
                assert pipe.last_overflow is not None and not bool(pipe.last_overflow.item()), rid
            pipe.check_overflow()
        _check_detector_routes(row, ev, pipe, model, nb, det['grid'])
        return None if small else (out.cpu(), cnt.cpu())


def _against_oracle(res, det, row):
    """-> (worst box difference over the matched boxes, unmatched oracle boxes) over the frames; asserts the per-frame allowances."""
    out, cnt = res
    tol, allow = BOX_TOL[row['math']], COUNT_ALLOWANCE[row['math']]
    worst_all, unmatched_all = 0.0, 0
    for i in range(cnt.shape[0]):
        rb, rs = det['refs'][(i, row['dynamic'])]
        n, n_ref = int(cnt[i]), rb.shape[0]
        got = out[i, :n].numpy()
        assert np.isfinite(got).all() and set(got[:, 8].astype(int).tolist()) <= {1, 2, 3}
        nm, worst = match_boxes(rb, rs, got[:, :7], got[:, 7], tol=tol)
        worst_all, unmatched_all = max(worst_all, worst), unmatched_all + (n_ref - nm)
        assert abs(n - n_ref) <= allow and n_ref - nm <= UNMATCHED, (rm.row_id(row, 'detector'), 'frame %d' % i, n, n_ref, nm, worst)
        if n_ref == 0:
            assert n == 0, (rm.row_id(row, 'detector'), 'frame %d: %d boxes where the oracle has none' % (i, n))
    return worst_all, unmatched_all


def _result(row, det, device):
    """Result of a row, run at most once per module (a row is also the bit-identity base of other rows)."""
    rid = rm.row_id(row, 'detector')
    if rid not in det['results']:
        det['results'][rid] = _run_detector_row(row, det, device)
    return det['results'][rid]


@pytest.mark.parametrize('grid,row', DET_CASES, ids=['%s/%s' % (g, rm.row_id(r, 'detector')) for g, r in DET_CASES])
def test_detector_row(dets, device, grid, row):
    det = _det(dets, grid)
    rid = '%s/%s' % (grid, rm.row_id(row, 'detector'))
    res = _result(row, det, device)
    if res is None:
        print('\n[detector] %s: overflow flag raised and seen by the parent; routes ran; no box comparison (capacities %s)' % (rid, SMALL_CAPS))
        return
    worst, unmatched = _against_oracle(res, det, row)
    base = rm.bits_base(row, 'detector')
    bits = 'no'
    if base is not None:
        _same_boxes(res, _result(base, det, device), '%s against %s' % (rid, rm.row_id(base, 'detector')))
        bits = 'equal to ' + rm.row_id(base, 'detector')
    print('\n[detector] %s: worst box difference %.2e, %d oracle boxes unmatched, bit identity required: %s' % (rid, worst, unmatched, bits))


def test_the_experimental_tile_engine_is_refused_by_name(det, device):
    """engine = 'tiles' is the one value the table leaves out (route_matrix.VALUE_EXCLUSIONS): a default build refuses it with an
    error that names the option, and the refused call changes nothing."""
    from detzero_amd import centerpoint as cpm
    from detzero_amd import ops
    from detzero_amd.lib import DetZeroHipError
    model = copy.deepcopy(det['model']).to(device)
    before = (model.backbone3d.engine, model.backbone3d.layout, model.backbone3d.f32_engine)
    with pytest.raises(DetZeroHipError, match='nosuch'):
        cpm.set_sparse_engine(model, 'xrun', f32_engine='nosuch')
    with pytest.raises(DetZeroHipError, match='nosuch'):
        cpm.set_dense_engine(model, 'nosuch')
    assert (model.backbone3d.engine, model.backbone3d.layout, model.backbone3d.f32_engine) == before
    if ops.L.load().dz_spconv_tile_rows() != 0:
        # an experimental build serves the engine (tests/test_gpu_sparse_conv.py runs it there): the selector takes it, with its row order
        cpm.set_sparse_engine(model, 'tiles')
        assert (model.backbone3d.engine, model.backbone3d.layout) == ('tiles', ops.LAYOUT_BRICK)
        return
    with pytest.raises(DetZeroHipError, match="'tiles'"):
        cpm.set_sparse_engine(model, 'tiles')
    assert (model.backbone3d.engine, model.backbone3d.layout, model.backbone3d.f32_engine) == before


def test_fp32_xrun_engines_on_an_overflowed_level(det, device):
    """The pair (f32_engine = xrun | xrun_bf16x3, level_caps too small), which no test ran before the matrix, through the pipeline:
    both engines, eager, the capacities of the existing overflow test - the flag is raised, the outputs are finite - and the same
    pipeline afterwards, without capacities, gives the boxes of a pipeline that never overflowed, bit for bit.  The kernel branch
    this pair was fixed in is shown to run by test_fp32_xrun_gather_mode_skips_ranks_past_the_input below."""
    from detzero_amd import centerpoint as cpm
    from detzero_amd.lib import DetZeroHipError
    frames = [torch.from_numpy(det['a'][i]).to(device) for i in (0, 2)]
    for engine in ('xrun', 'xrun_bf16x3'):
        model = copy.deepcopy(det['model']).to(device)
        cpm.set_sparse_engine(model, 'xrun', engine, 'mfma32')
        ref = cpm.FramePipeline(model, det['info'], math='f32', ways=1)(frames)
        pipe = cpm.FramePipeline(model, det['info'], math='f32', ways=1)
        pipe.level_caps = list(SMALL_CAPS)
        out, cnt = pipe(frames)
        assert bool(pipe.last_overflow.item()) and torch.isfinite(out).all()
        with pytest.raises(DetZeroHipError, match='overflowed'):
            pipe.check_overflow()
        pipe.level_caps = None
        _same_boxes(pipe(frames), ref, engine)
        assert pipe.last_overflow is None and int(ref[1].min()) >= 30


@pytest.mark.parametrize('channels', [32, 64])
@pytest.mark.parametrize('engine', ['xrun', 'xrun_bf16x3'])
def test_fp32_xrun_gather_mode_skips_ranks_past_the_input(device, engine, channels):
    """Kernel level, the branch itself.  A level that overflowed its row capacity (built with fewer rows than it has sites, as
    `downsample(cap=...)` leaves it: the bitmap and the prefix hold every site, the rows and the tables stop at the capacity) whose
    first slab is nearly empty and whose second is nearly full, cut inside the second: the first unit's window into the slab above
    is longer than the kernel stages (dz_spconv_x_f32_window_rows / dz_spconv_x_limb3_window_rows -> the gather mode) and ends past
    the capacity - both asserted on the window table.  k_spconv_xf / k_spconv_xt read such ranks through a plain pointer past the end
    of the feature rows before; now a rank at or past the input's rows adds nothing, so the rows below the capacity equal a float64
    evaluation of the table with those ranks absent (the bound of tests/test_gpu_xrun_f32.py), and rows past it are not written."""
    from detzero_amd import lib as L
    from detzero_amd import ops
    from tests.test_gpu_xrun import K3, P1, S1, _t
    from tests.test_gpu_xrun_f32 import SENTINEL, TOL, _ref64
    lib = L.load()
    rng = np.random.default_rng(31 * channels)
    shape, dens = [4, 48, 64], (0.01, 0.9, 0.02, 0.5)
    slab = shape[1] * shape[2]
    lin = np.unique(np.concatenate([z * slab + np.nonzero(rng.random(slab) < dens[z])[0] for z in range(shape[0])]))
    coords = np.stack([lin * 0, lin // slab, (lin // shape[2]) % shape[1], lin % shape[2]], 1).astype(np.int32)
    n0 = int((coords[:, 1] == 0).sum())
    cap = n0 + 1500                                     # inside the dense slab: its sites from here on have no row
    assert 0 < n0 < 64 and cap + 1000 < int((coords[:, 1] <= 1).sum())
    lvl = ops.SparseLevel(1, shape, cap, device)
    lvl.build_from_coords(_t(coords, device), want_rank=False)
    assert int(lvl.d_m.item()) == coords.shape[0] > cap                                   # overflowed: more sites than rows
    plain = lvl.neighbors_to(lvl, K3, S1, P1)
    xt = ops.build_windows(lvl.neighbors_to(lvl, K3, S1, P1, packed=True), lvl, channels)
    assert getattr(xt, 'xwin', None) is not None and tuple(plain.shape) == (27, cap)
    rcap = (lib.dz_spconv_x_f32_window_rows if engine == 'xrun' else lib.dz_spconv_x_limb3_window_rows)(channels, channels)
    assert rcap > 0
    win = xt.xwin[0][:-16].view(-1, 3, 2)[:max(cap // xt.xwin[1], 1)].cpu()              # (first row, rows) per unit and slab offset
    reach = (win[..., 1] > rcap) & (win[..., 0] + win[..., 1] > cap)
    assert bool(reach.any()), (rcap, cap, win[:2].tolist())                               # a gather-mode window that ends past the input's rows
    assert int((plain.words >= cap).sum()) > 0                                                  # ... and the table does name such ranks
    x = _t(rng.standard_normal((cap, channels)).astype(np.float32), device)
    r = _t(rng.standard_normal((cap, channels)).astype(np.float32), device)
    w = _t((rng.standard_normal((27, channels, channels)) / np.sqrt(channels * 8)).astype(np.float32), device)
    sc = _t(rng.uniform(0.5, 1.5, channels).astype(np.float32), device)
    sh = _t((rng.standard_normal(channels) * 0.1).astype(np.float32), device)
    out = torch.full((cap, channels), SENTINEL, dtype=torch.float32, device=device)
    if engine == 'xrun':
        ops.spconv_forward(x, xt, lvl, w, sc, sh, r, relu=False, out=out)
    else:
        ops.spconv_forward(x, xt, lvl, ops.pack_weight_limb3(w, cout_mult=32), sc, sh, r, relu=False, out=out, f32_engine='xrun_bf16x3')
    torch.cuda.synchronize(device)
    tab = torch.where(plain.words < cap, plain.words, torch.full_like(plain.words, -1))
    acc, _ = _ref64(x, tab, w, cap)
    ref = (acc * sc.double() + sh.double() + r.double()).float()
    err = float((out - ref).abs().max())
    print('\n[fp32 %s, %d channels] overflowed level, %d of %d sites have rows, %d gather-mode windows end past them: max |got - ref64| %.2e'
          % (engine, channels, cap, coords.shape[0], int(reach.sum()), err))
    assert torch.isfinite(out).all()
    torch.testing.assert_close(out, ref, rtol=TOL, atol=TOL)


# ---------------------------------------------------------------------------------------------------------------- PDV second stage
@pytest.fixture(scope='module')
def pdv(golden_dir):
    return {'g': np.load(os.path.join(golden_dir, 'pdv_golden.npz')), 'results': {}}


def _run_pdv_row(row, pdv, device):
    from detzero_amd import ops
    from detzero_amd import pdv_modules as pm
    from tests import test_pdv as tp
    rid = rm.row_id(row, 'pdv')
    with pytest.MonkeyPatch.context() as mp:
        _set_module_switches(mp, row, 'pdv')
        ev = Evidence()
        for name in ('sa_pool', 'sa_pool_split'):
            ev.wrap(mp, pm, name)
        for name in ('_attention_fused', '_attention_split'):
            ev.wrap(mp, pm.PDVHead, name)
        lib = ops.L.load()
        ev.wrap(mp, lib, 'dz_pdv_part_counts_binned')
        ev.wrap(mp, lib, 'dz_pdv_part_counts')
        head = tp._head().to(device)
        head.set_math(ops.math_id(row['math']))
        out = head(tp._batch(pdv['g'], device))
        r = head.forward_ret_dict
        res = {k: r[k].detach().cpu() for k in ('pooled_features', 'attention_output', 'positional_input', 'key_padding_mask')}
        res.update({k: out[k].detach().cpu() for k in ('batch_box_preds', 'batch_cls_preds')})
    split = row['math'] != 'f32'
    branches = sum(len(layer.nsamples) for layer in head.roi_grid_pool_layers)
    want_split_pool = row['FUSED_SA'] and split and row['SPLIT_SA']
    assert ev['sa_pool_split'] == (branches if want_split_pool else 0), (rid, ev)
    assert ev['sa_pool'] == (branches if row['FUSED_SA'] and not want_split_pool else 0), (rid, ev)
    assert (ev['dz_pdv_part_counts_binned'] > 0) == row['PART_COUNTS_BINNED'] == (ev['dz_pdv_part_counts'] == 0), (rid, ev)
    folded = split and row['FOLDED_ATTENTION']
    assert (ev['_attention_fused'] > 0) == (folded and row['FUSED_ENCODER']), (rid, ev)
    assert (ev['_attention_split'] > 0) == (folded and not row['FUSED_ENCODER']), (rid, ev)
    return res


@pytest.mark.parametrize('row', PDV_ROWS, ids=_ids(PDV_ROWS, 'pdv'))
def test_pdv_row(pdv, device, row):
    """PDVHead on the golden scene: the tolerances of tests/test_pdv.py for the mode (test_pooled_features_positional_input_and_attention,
    test_final_boxes_and_confidences; test_grid_pooling_on_split_operands, test_head_on_split_operands) - none is new."""
    g = pdv['g']
    rid = rm.row_id(row, 'pdv')
    if rid not in pdv['results']:
        pdv['results'][rid] = _run_pdv_row(row, pdv, device)
    res = pdv['results'][rid]
    sub = g['roi_subset']
    pool_tol = {'f32': 1e-4, 'f16x2': 1e-4, 'bf16x2': 2e-3}[row['math']]
    att_tol = {'f32': 2e-3, 'f16x2': 2e-3, 'bf16x2': 5e-3}[row['math']]
    box_tol = 1e-3 if row['math'] == 'f32' else 2e-3
    err = {'pooled': float((res['pooled_features'][sub] - torch.from_numpy(g['pooled'])).abs().max()),
           'attention': float((res['attention_output'][sub] - torch.from_numpy(g['pooled'] + g['attention'])).abs().max()),
           'boxes': float((res['batch_box_preds'] - torch.from_numpy(g['batch_box_preds'])).abs().max()),
           'cls': float((res['batch_cls_preds'] - torch.from_numpy(g['batch_cls_preds'])).abs().max())}
    base = rm.bits_base(row, 'pdv')
    print('\n[pdv] %s: worst difference to the golden: pooled %.2e, attention %.2e, boxes %.2e, confidences %.2e; bit identity required: %s'
          % (rid, err['pooled'], err['attention'], err['boxes'], err['cls'], 'no' if base is None else 'part counts equal to ' + rm.row_id(base, 'pdv')))
    torch.testing.assert_close(res['pooled_features'][sub], torch.from_numpy(g['pooled']), rtol=pool_tol, atol=pool_tol)
    np.testing.assert_array_equal(res['key_padding_mask'].numpy(), g['key_padding_mask'])
    pos = res['positional_input'].numpy()
    np.testing.assert_allclose(pos[..., :3], g['positional_input'][..., :3], rtol=0, atol=1e-6)
    diff = np.abs(pos[..., 3] - g['positional_input'][..., 3]) > 1e-5
    assert diff.mean() < 2e-3, diff.mean()
    torch.testing.assert_close(res['attention_output'][sub], torch.from_numpy(g['pooled'] + g['attention']), rtol=att_tol, atol=att_tol)
    torch.testing.assert_close(res['batch_box_preds'], torch.from_numpy(g['batch_box_preds']), rtol=box_tol, atol=box_tol)
    torch.testing.assert_close(res['batch_cls_preds'], torch.from_numpy(g['batch_cls_preds']), rtol=box_tol, atol=box_tol)
    if base is not None:
        bid = rm.row_id(base, 'pdv')
        if bid not in pdv['results']:
            pdv['results'][bid] = _run_pdv_row(base, pdv, device)
        assert torch.equal(res['positional_input'][..., 3], pdv['results'][bid]['positional_input'][..., 3]), rid
        assert torch.equal(res['key_padding_mask'], pdv['results'][bid]['key_padding_mask']), rid


# ---------------------------------------------------------------------------------------------------------------- refiner
@pytest.fixture(scope='module')
def refine(golden_dir):
    return np.load(os.path.join(golden_dir, 'refine_golden.npz'))


# which model of the pair shows a route at the golden's sizes (GRM: 3 queries over 320 memory rows per object; PRM: 200 queries over
# 200 x 48 = 9600 memory rows per object)
REFINER_ROUTES = {'FOLDED_XATTN': ('xattn_folded', 'grm'), 'SPLIT_ATTENTION': ('mha_core_split', 'prm'),
                  'FUSED_CHAIN': ('mlp_chain', 'grm'), 'FUSED_POINTNET': ('pointnet3', 'grm')}


@pytest.mark.parametrize('row', REF_ROWS, ids=_ids(REF_ROWS, 'refiner'))
def test_refiner_row(refine, device, row):
    """GRM and PRM on the goldens of tests/test_refine.py, at its tolerances (the same in every mode), its split stacks forced on."""
    from detzero_amd import ops
    from detzero_amd import refine_modules
    from detzero_amd.synth import synth_state_dict
    from tests import test_refine as tr
    g = refine
    rid = rm.row_id(row, 'refiner')
    seen, worst = {}, {}
    for tag, seed, model in (('grm', 5, tr._models()[0]), ('prm', 6, tr._models()[1])):
        with pytest.MonkeyPatch.context() as mp:
            _set_module_switches(mp, row, 'refiner')
            mp.setattr(refine_modules, 'SPLIT_MIN_ROWS', 1)          # the fixture is small: force the split stacks on
            ev = seen[tag] = Evidence()
            for name in ('xattn_folded', 'mlp_chain', 'pointnet3'):
                ev.wrap(mp, ops, name)
            ev.wrap(mp, ops, 'mha_core', lambda a, k, ev=ev: ev.update(mha_core_split=int(bool(k.get('math')))))
            model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=seed), strict=True)
            model = model.to(device).set_math(row['math'])
            data = {k[len(tag + '_in_'):]: torch.from_numpy(g[k]).to(device) for k in g.files if k.startswith(tag + '_in_')}
            res = model(data)
        if tag == 'grm':
            checks = [(res['memory'], g['grm_memory'], 1e-4), (res['query'], g['grm_query'], 1e-4),
                      (model.preds_dict['geometry_cls'], g['grm_cls'], 2e-4), (model.preds_dict['geometry_reg'], g['grm_reg'], 2e-4),
                      (res['batch_box_preds'], g['grm_boxes'], 1e-3)]
        else:
            valid = torch.from_numpy(g['prm_in_padding_mask']) == 0          # padded queries attend to nothing meaningful
            checks = [(res['query'], g['prm_query'], 1e-4), (res['memory'][:, :, ::16], g['prm_memory'], 1e-4)]
            checks += [(model.preds_dict[k][valid.to(device)], g['prm_' + k][valid.numpy()], 2e-4) for k in ('center_reg', 'heading_cls', 'heading_reg')]
            checks.append((res['batch_box_preds'][valid.to(device)], g['prm_boxes'][valid.numpy()], 1e-3))
        seen[tag + '_checks'] = [(x.detach().cpu(), torch.from_numpy(np.asarray(y)), t) for x, y, t in checks]
        worst[tag] = max(float((x - y).abs().max()) for x, y, _ in seen[tag + '_checks'])
    print('\n[refiner] %s: worst difference to the golden: GRM %.2e, PRM %.2e; bit identity required: no' % (rid, worst['grm'], worst['prm']))
    split = row['math'] != 'f32'
    for name, (key, tag) in REFINER_ROUTES.items():
        on = row[name] and (split or name == 'FOLDED_XATTN')
        assert (seen[tag][key] > 0) == on, (rid, name, dict(seen['grm']), dict(seen['prm']))
    for tag in ('grm', 'prm'):
        for a, b, atol in seen[tag + '_checks']:
            torch.testing.assert_close(a, b, rtol=1e-3, atol=atol)
