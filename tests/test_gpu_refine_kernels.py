"""The kernels of the object refiner (GRM / PRM / CRM: csrc/mha.hip, mha_h.hip, xattn_fold.hip, pointnet.hip, mlp_chain.hip, refine.hip
and the linear entry points of conv2d.hip / conv2d_h.hip) one by one against the float64 references of oracle/refine.py - the third
stage's counterpart of tests/test_gpu_dense_conv.py / test_gpu_sparse_conv.py / test_gpu_head_post.py / test_gpu_pdv_kernels.py.
tests/test_refine.py holds the stage together at the workload's shapes on randn inputs; here every input is made by hand so that a
lost rescale, a dropped partial, a late flush or a wrong lane shows.  Every GPU test writes into buffers with TAIL sentinel rows behind
(and sentinel columns beside) what the call may write, launches twice and wants the same bits.

dz_mha_core (fp32).  Routes, from the entry point: lq <= 32 -> k_mha_core, one WAVE per 16 queries, four per workgroup ("wave");
  32 < lq <= 256 -> k_mha_block, one workgroup per (batch, head) ("block"); lq > 256 -> k_mha_block with two workgroups per (batch,
  head) ("blocks").  MHA_CASES names the route of every case; test_attention_case_tables_reach_every_route checks the names against
  the entry point's conditions and that every route has masked and unmasked cases.
    wave    lq 1 / 16 / 17 / 32: one item (three waves of the workgroup idle), five items (a second workgroup with one live wave), a ragged
            second query tile, lk 1 / 15 / 16 / 17 / 63 / 65 / 129 / 200 (less than one 16-key tile ... 13 tiles)
    block   lq 33 / 64 / 96 / 97 / 256: waves without queries (33 -> two of four), eight waves (256); lk 1 / 5 below a tile, 63 / 64 / 65
            around one staged 64-key block, 129 / 200 with a ragged last block
    blocks  lq 257 / 300: the second workgroup holds one / two waves' worth of queries (a wave of it has 1 and 12 live queries)
  Input families: randn; "rise" - keys ordered so that EVERY 16-key tile raises the running maximum of every query (the rescale of the
  accumulator runs in every tile, late ones included), "fall" - the same keys reversed (the maximum arrives first, alpha == 1 from
  then on: the wave-uniform shortcut); "spread" - logits spread over about +-60 natural-log units (most probabilities underflow);
  "equal" - all keys equal (uniform probabilities, the output is the mean of v).  Masks: random; "start" - the first 80 keys dead (a
  whole staged block and a tile while the running maximum is still -inf); "middle" / "end" - whole tiles and staged blocks dead in the
  middle / at the end; "first" / "last" - one live key, at position 0 / lk - 1.  In every masked case the K rows of the masked keys
  hold NaN and 1e30 alternately (the reference REPLACES those scores by -inf: the result must not notice).  A fully masked batch
  entry is NaN for that entry only, on all three routes.  Exact: a masked tail of padding keys up to the next multiples of 16 and 64,
  a permutation of batch entries or heads, v scaled by 2^+-20.

dz_mha_core_split (f16x2, bf16x2; one route: k_mha_block_h).  The same cases, the poison 1e30 replaced by the largest magnitude the mode
  holds (65504 / 3.39e38: 1e30 saturates fp16 anyway, and is an ordinary bf16), and a gain sweep 2^-12 .. 2^8 on q.k and on v.

dz_attention_single_head.  l <= 64 or E in {64, 256} -> k_mha_core<E> ("wave"); 64 < l <= 256 and E in {128, 192} -> k_attn1h_block
  ("staged"); l = 257 is refused.  ATT1H_CASES: l 1 / 16 / 63 / 64 / 65 / 255 / 256 x E 64 / 128 / 192 / 256, rise / fall / spread, dead
  tiles and blocks.

dz_xattn_folded.  splits = min(4 CUs / b, max(1, (lk / 16) / 16)): lk <= 496 -> one split, 512 -> two, 1000 -> three.  FOLD_CASES:
  lk 1 / 15 / 16 / 17 (waves of the workgroup without a key block), 255 / 256 / 257, 496 / 497 (the edge between one and two splits), 512 / 1000; lq * heads 1 / 3 / 24 / 32 (1, 3 and 24:
  padding rows of the folded query tile); "half" - the first half of all keys dead (every early split is empty, the first one
  included: k_fold_out meets max -inf / sum 0 first), "third" - the middle half dead (an empty split between two live ones),
  "last" / "first" - one live key (all splits but one empty); rise / fall across the split boundaries.  A workspace of exactly
  dz_xattn_folded_workspace_bytes inside a sentinel buffer; one byte less is refused.

dz_pointnet3_forward / dz_mlp_chain_forward (persistent: every wave gets ceil(tiles / waves) 32-row tiles).  ROW_GEOMETRY: 1, 2 and 9
  tiles (fewer tiles than the 8 / 4 waves of a workgroup; 9: a second workgroup with one busy wave - idle waves must keep up with the
  barriers), one group over two workgroups (1 x 288), groups of 3 / 5 / 33 tiles, and 3 x waves + 1 tiles (waves computed from the
  device's CU count as the host code does): four tiles per wave, the last wave's range runs past the end, groups of 5 / 7 tiles start
  inside a wave's range while the group before is shared with the previous wave or workgroup - where the atomic flush of the running
  maximum goes wrong.  PointNet: c3 128 / 256 / 512, pair16 / 16-column / 32-column fp32 input, tap on / off; the first and the last
  row of every group are the large ones (maxima in the first row for some channels, the last row for others), one group is all zero
  under non-positive biases (pooled row exactly 0).  Chain: with / without K and V, with / without the group addend, ldg 512 / 640.

Linear layers (dz_linear_forward, _split, _splitk).  Rows 1 / 31 / 127 / 128 / 129 / 300, cout < cout_pad, x_stride > cin with NaN in the
  unused columns, y_stride > cout with sentinel columns, group addends with group_rows 1 / 37 / 100 / 129 and a ragged last group;
  the fused group max with group_rows 128 / 384, ReLU on / off, negative maxima, -0.0 next to +0.0; split-k with 1 / 2 / 8 splits at the
  smallest cin each takes, its workspace inside a sentinel buffer.

dz_group_max (len 1 .. 5, 37 x c 1 / 63 / 64 / 65 / 192 x groups 1 / 3; -inf, +-0.0, all negative: exact; NaN: see the test),
dz_add_layernorm (every c, rows 1 / 3 / 4 / 5 / 77, y null / given, norm off exact, the four row families), dz_add_layernorm_combine
(group_rows 1 / 5 / 216, skip flags), dz_rows_all_zero (1 - 4 tensors of widths 4 / 16 / 64, rows 1 / 255 / 256 / 257, 0x80000000).

Numbers in this file.
  BOUND       the project's per-mode bound on |got - want| / sum |x w| (tests/test_gpu_dense_conv.py), per layer; through a stack of
              layers the allowance is propagated as oracle.refine.layer_stack states.
  ATT_BASE    a little above the worst error of the SAME formula evaluated on the host against float64, normalised by
              sum_j p_j |v_j|, over the cases of each kernel in this module (test_attention_host_baselines prints the figures and
              checks that the constants cover them):
                  float32 numpy (einsum loops, no BLAS), dz_mha_core cases                 5.6e-6 -> ATT_BASE['f32']   1.0e-5
                      (by family: randn 4e-7, equal 8e-8, rise 3e-6, fall 2e-6, spread 6e-6)
                  float32 numpy, dz_attention_single_head cases                            1.0e-5 -> ATT_BASE['att1h'] 1.6e-5
                  float32 numpy, project-then-attend on the dz_xattn_folded cases
                      with more than one live key                                          8.1e-6 -> ATT_BASE['fold']  1.2e-5
                      with ONE live key (the output is one projected value row: its small
                      elements are all cancellation of the projection, fold_key())         5.6e-4 -> ATT_BASE['fold1'] 8.0e-4
                  split_pair / split_product emulation of the split cores, f16x2 / bf16x2  4.2e-4 / 3.3e-4 -> 5.0e-4 / 4.0e-4
                      (f16x2 is no better than bf16x2 here: where one key carries all the weight the output is that key's v, and an
                      element of it below 2^-3 has a subnormal fp16 lo half - 2^-25 absolute, any size relative to |v|; the randn
                      cases sit at 2e-7 / 7e-6)
  ATT_BOUND   8 x ATT_BASE: the kernels sum up to 1000 keys in another order, scale q into log2 units and use the 1-ulp hardware exp2.
              Every GPU test prints the kernel's own worst value next to its bound.
  LN_K        LayerNorm, derived at layernorm_allowance() and verified there against the float32 host evaluation.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from detzero_amd import lib as L
from detzero_amd import ops
from oracle import refine as R
from tests.test_gpu_dense_conv import BOUND, SENTINEL

F64 = np.float64
U32 = 2.0 ** -24                     # unit roundoff of float32
TAIL = 8                             # sentinel rows behind every output
MATH = {'f16x2': 1, 'bf16x2': 2}
SPLIT_U2 = {'f16x2': 2.0 ** -22, 'bf16x2': 2.0 ** -16}          # |x - hi - lo| <= SPLIT_U2 |x| (oracle.refine.split_pair) ...
SPLIT_FLOOR = {'f16x2': 2.0 ** -25, 'bf16x2': 0.0}               # ... or this absolute error once an fp16 lo half is subnormal
POISON = {'f32': 1e30, 'f16x2': 65504.0, 'bf16x2': 3.3895313892515355e38}
ATT_BASE = {'f32': 1.0e-5, 'att1h': 1.6e-5, 'fold': 1.2e-5, 'fold1': 8.0e-4, 'f16x2': 5.0e-4, 'bf16x2': 4.0e-4}
ATT_BOUND = {m: 8.0 * v for m, v in ATT_BASE.items()}
# gains (powers of two on q.k, on v) over which the split emulation stays within ATT_BASE: test_split_gain_range_on_the_host
SPLIT_GAIN_RANGE = {'f16x2': {'qk': (-12, 8), 'v': (-12, 8)}, 'bf16x2': {'qk': (-12, 4), 'v': (-12, 8)}}
SENT_F = float(np.array([SENTINEL], np.int32).view(np.float32)[0])


# ------------------------------------------------------------------------------------------------------------------------
# comparison helper (CPU and GPU tests)
# ------------------------------------------------------------------------------------------------------------------------
def worst_ratio(got, want, allow):
    """max |got - want| / allow over the elements; NaN must sit exactly where the reference has NaN (else inf)."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    allow = np.broadcast_to(np.asarray(allow, F64), want.shape)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return float('inf')
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    err = np.abs(got - want)[ok]
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0.0, 0.0, err / allow[ok])
    return float(ratio.max())


def assert_within(got, want, allow, what, unit=None):
    """|got - want| <= allow element by element; prints the worst |got - want| / allow (with `unit`, the bound the allowance was built
    from, the worst normalised error itself)."""
    w = worst_ratio(got, want, allow)
    if unit is None:
        print('  %s: worst |got - want| / allowance %.3f' % (what, w))
    else:
        print('  %s: worst normalised error %.2e (bound %.2e)' % (what, w * unit, unit))
    assert w <= 1.0, (what, w)
    return w


# ------------------------------------------------------------------------------------------------------------------------
# attention inputs (numpy; shared by the CPU and the GPU tests)
# ------------------------------------------------------------------------------------------------------------------------
def make_mask(rng, b, lk, kind):
    if kind is None:
        return None
    m = np.zeros((b, lk), np.uint8)
    if kind == 'rand':
        m[:] = rng.random((b, lk)) < 0.35
    elif kind == 'start':
        m[:, :min(lk - 1, 80)] = 1
    elif kind == 'middle':
        lo, hi = (16, lk - 16) if lk > 48 else (lk // 3, max(lk // 3 + 1, 2 * lk // 3))
        m[:, lo:hi] = 1
    elif kind == 'end':
        m[:, min(16, max(lk // 2, 1)):] = 1
    elif kind == 'first':
        m[:, 1:] = 1
    elif kind == 'last':
        m[:, :lk - 1] = 1
    elif kind == 'half':
        m[:, :lk // 2] = 1
    elif kind == 'third':
        m[:, lk // 4:3 * lk // 4] = 1
    else:
        raise ValueError(kind)
    if kind in ('start', 'middle', 'end', 'half', 'third') and b > 1:
        m[1:] |= (rng.random((b - 1, lk)) < 0.2).astype(np.uint8)
    for i in range(b):
        if m[i].all():
            m[i, lk - 1] = 0
    return m


def attention_inputs(seed, b, lq, lk, heads, hd, family, mask_kind):
    """q (b, lq, heads * hd), k, v (b, lk, heads * hd) float32 and the mask; scale is hd^-1/2.
    rise / fall: per (batch, head) one unit direction u; q_i = a_i sqrt(hd) u + noise with a_i in [1, 2], k_j = ramp_j c u + noise with
    ramp_j = (j + 1) / lk (reversed for fall) and c = max(12, lk / 8): score(i, j) = a_i c ramp_j + O(0.2 a_i) - a tile of 16 keys
    raises it by at least 2 a_i, ten times the noise."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((b, lq, heads, hd))
    k = rng.standard_normal((b, lk, heads, hd))
    v = 2.0 * rng.standard_normal((b, lk, heads, hd))
    if family in ('rise', 'fall'):
        u = rng.standard_normal((b, 1, heads, hd))
        u /= np.linalg.norm(u, axis=-1, keepdims=True)
        a = rng.uniform(1.0, 2.0, (b, lq, heads, 1))
        q = a * np.sqrt(hd) * u + 0.1 * q
        ramp = (np.arange(lk) + 1.0) / lk
        if family == 'fall':
            ramp = ramp[::-1]
        k = ramp[None, :, None, None] * max(12.0, lk / 8.0) * u + 0.1 * k
    elif family == 'spread':
        k = 20.0 * k
    elif family == 'equal':
        k = np.repeat(k[:, :1], lk, axis=1)
    elif family != 'randn':
        raise ValueError(family)
    mask = make_mask(rng, b, lk, mask_kind)
    f = lambda a: np.ascontiguousarray(a.reshape(a.shape[0], a.shape[1], heads * hd), np.float32)        # noqa: E731
    return f(q), f(k), f(v), mask


def poison_keys(k, mask, big):
    """A copy of k with the rows of the masked keys NaN (even positions) and `big` (odd positions)."""
    if mask is None:
        return k
    k = k.copy()
    bi, ki = np.nonzero(mask)
    k[bi, ki, :] = np.where(ki % 2 == 0, np.nan, big).astype(np.float32)[:, None]
    return k


def mha_route(lq):
    """The route of dz_mha_core for lq queries (batch, heads <= 65535): the conditions of the entry point in csrc/mha.hip."""
    if lq > 32:
        qw = (lq + 31) // 32
        return 'block' if (qw + 7) // 8 == 1 else 'blocks'
    return 'wave'


#             route     b   lq   lk  heads family    mask
MHA_CASES = [('wave', 1, 1, 1, 1, 'randn', None),              # b * heads * ceil(lq / 16) = 1: three waves of the workgroup have no item
             ('wave', 5, 16, 15, 1, 'randn', 'rand'),          # ... = 5: the second workgroup has one live wave; lk below one tile
             ('wave', 3, 17, 16, 8, 'rise', None),             # a second query tile with one live query; exactly one key tile
             ('wave', 1, 32, 200, 8, 'fall', 'start'),         # the first five tiles dead: the running maximum stays -inf
             ('wave', 1, 16, 65, 8, 'spread', 'middle'),
             ('wave', 3, 1, 17, 1, 'equal', 'last'),           # one live key, the last one (alone in its tile)
             ('wave', 1, 17, 129, 1, 'rise', 'first'),         # one live key, the first one: eight dead tiles behind it
             ('wave', 1, 32, 63, 1, 'rise', 'end'),
             ('block', 3, 33, 63, 1, 'randn', None),           # two of the four waves have no query; lk one short of a staged block
             ('block', 1, 64, 64, 8, 'rise', None),            # exactly one staged block, the rescale in each of its four tiles
             ('block', 1, 96, 65, 1, 'spread', 'rand'),        # a second staged block holding one key
             ('block', 3, 97, 129, 8, 'rise', 'middle'),       # tiles 1 .. 6 dead: block 1 whole
             ('block', 1, 256, 200, 1, 'fall', None),          # eight waves; the maximum arrives with the first key
             ('block', 1, 64, 200, 8, 'fall', 'start'),        # the first staged block and the tile behind it dead
             ('block', 1, 33, 200, 1, 'rise', 'end'),          # blocks 1 .. 3 dead at the end
             ('block', 1, 96, 5, 8, 'randn', 'first'),
             ('block', 3, 33, 129, 1, 'equal', 'last'),        # only the one key of the third staged block lives
             ('block', 1, 64, 1, 1, 'randn', None),
             ('blocks', 1, 257, 200, 8, 'rise', 'start'),      # second workgroup: one query
             ('blocks', 3, 300, 129, 1, 'randn', None),
             ('blocks', 1, 300, 65, 8, 'equal', 'rand'),
             ('blocks', 1, 257, 15, 1, 'fall', None),
             ('blocks', 1, 300, 200, 1, 'spread', 'middle')]


def case_id(c):
    return '-'.join(str(x) for x in c)


@functools.lru_cache(maxsize=None)
def mha_case(i):
    route, b, lq, lk, heads, family, mk = MHA_CASES[i]
    q, k, v, mask = attention_inputs(1000 + i, b, lq, lk, heads, 32, family, mk)
    want, nat = R.attention(q, k, v, mask, heads, 32 ** -0.5)
    return {'q': q, 'k': k, 'v': v, 'mask': mask, 'heads': heads, 'scale': 32 ** -0.5, 'want': want, 'nat': nat}


def att1h_route(l, e):
    """dz_attention_single_head (csrc/pdv.hip -> attention_1h_mfma in csrc/mha.hip): the staged kernel for 64 < l <= 256 where E has an
    instance of it."""
    return 'staged' if 64 < l <= 256 and e in (128, 192) else 'wave'


# (l = 257 is no case: dz_attention_single_head refuses l > 256, csrc/pdv.hip - see test_refusals_write_nothing)
#               route     r   l    e   family    mask
ATT1H_CASES = [('wave', 2, 1, 64, 'randn', None),
               ('wave', 3, 16, 128, 'rise', None),
               ('wave', 2, 63, 192, 'spread', 'rand'),
               ('wave', 2, 64, 256, 'rise', 'start'),           # the upper edge of the per-wave window
               ('staged', 2, 65, 128, 'fall', 'middle'),        # the lower edge of the staged window: a second block with one key
               ('wave', 3, 65, 64, 'rise', None),               # inside the window, but E = 64 has no staged instance
               ('staged', 2, 255, 192, 'rise', 'end'),
               ('staged', 2, 256, 128, 'spread', None),         # the upper edge: eight waves, four full blocks
               ('wave', 1, 256, 256, 'fall', 'rand'),           # E = 256 has no staged instance
               ('wave', 2, 255, 64, 'spread', 'start'),
               ('staged', 2, 100, 192, 'rise', 'first'),
               ('staged', 2, 200, 128, 'fall', 'last')]


@functools.lru_cache(maxsize=None)
def att1h_case(i):
    route, r, l, e, family, mk = ATT1H_CASES[i]
    q, k, v, mask = attention_inputs(2000 + i, r, l, l, 1, e, family, mk)
    want, nat = R.attention(q, k, v, mask, 1, float(e) ** -0.5)
    return {'q': q, 'k': k, 'v': v, 'mask': mask, 'heads': 1, 'scale': float(e) ** -0.5, 'want': want, 'nat': nat}


def fold_splits(b, lk, cus):
    """xf_splits of csrc/xattn_fold.hip."""
    nblk = (lk + 15) // 16
    s = min((4 * cus + b - 1) // b, max(1, nblk // 16))
    return max(1, min(s, 64))


#              b  lq heads lk   family   mask
FOLD_CASES = [(1, 1, 1, 1, 'randn', None),               # lq * heads = 1; one key: three waves without a block
              (2, 3, 1, 15, 'randn', 'rand'),            # 3 rows
              (1, 3, 8, 16, 'rise', None),               # 24 rows
              (3, 4, 8, 17, 'randn', 'last'),            # 32 rows; the live key alone in the second block
              (1, 1, 1, 255, 'rise', 'half'),
              (2, 3, 8, 256, 'fall', 'third'),
              (1, 4, 8, 257, 'rise', None),
              (1, 3, 8, 496, 'rise', 'half'),            # the largest lk with one split (31 key blocks) ...
              (2, 3, 8, 497, 'fall', 'half'),            # ... and the smallest with two: the first one empty
              (2, 3, 8, 512, 'rise', 'half'),            # two splits, the first empty
              (1, 4, 8, 512, 'fall', None),
              (3, 3, 8, 1000, 'randn', 'half'),          # three splits: the first empty, the second half empty
              (1, 3, 1, 1000, 'rise', 'third'),          # the middle split empty
              (2, 4, 8, 1000, 'fall', 'last'),           # all splits but the last empty
              (1, 32, 1, 1000, 'rise', 'first'),         # 32 rows of one head; all splits but the first empty
              (1, 2, 16, 512, 'randn', 'rand')]


def fold_key(i):
    """Which baseline a folded case belongs to: 'fold1' where one key is live (the output IS one projected value row; its small
    elements are all cancellation of the float32 projection, whatever the attention does), 'fold' otherwise."""
    b, lq, heads, lk, family, mk = FOLD_CASES[i]
    return 'fold1' if lk == 1 or mk in ('first', 'last') else 'fold'


@functools.lru_cache(maxsize=None)
def fold_case(i):
    """x_q (= the projected queries: wq = I, bq = 0), mem, the projections.  rise / fall: the raw memory rows climb along one
    direction u of the 256 channels; head h sees them through a_h = Wk_h u, so its queries point along a_h and the ramp is scaled by
    the smallest |a_h| (every head's scores rise by at least max(12, lk / 16) in all, at least 1 per 16-key block)."""
    b, lq, heads, lk, family, mk = FOLD_CASES[i]
    e, hd = 256, 256 // heads
    rng = np.random.default_rng(3000 + i)
    x_q = rng.standard_normal((b, lq, e))
    mem = 1.5 * rng.standard_normal((b, lk, e))
    wk, wv = (rng.standard_normal((e, e)) / np.sqrt(e) for _ in range(2))
    bk, bv = (0.2 * rng.standard_normal(e) for _ in range(2))
    if family in ('rise', 'fall'):
        u = rng.standard_normal(e)
        u /= np.linalg.norm(u)
        a = (wk @ u).reshape(heads, hd)
        an = np.linalg.norm(a, axis=1, keepdims=True)
        alpha = rng.uniform(1.0, 2.0, (b, lq, heads, 1))
        x_q = (alpha * np.sqrt(hd) * (a / an)[None, None] + 0.1 * x_q.reshape(b, lq, heads, hd)).reshape(b, lq, e)
        ramp = (np.arange(lk) + 1.0) / lk
        if family == 'fall':
            ramp = ramp[::-1]
        mem = ramp[None, :, None] * (max(12.0, lk / 16.0) / float(an.min())) * u + 0.1 * mem
    mask = make_mask(rng, b, lk, mk)
    f = lambda a: np.ascontiguousarray(a, np.float32)        # noqa: E731
    x_q, mem, wk, wv, bk, bv = f(x_q), f(mem), f(wk), f(wv), f(bk), f(bv)
    eye, zero = np.eye(e, dtype=np.float32), np.zeros(e, np.float32)
    want, nat, q = R.folded_attention(x_q, mem, eye, zero, wk, bk, wv, bv, heads, mask)
    return {'x_q': x_q, 'mem': mem, 'wk': wk, 'bk': bk, 'wv': wv, 'bv': bv, 'mask': mask, 'heads': heads, 'want': want, 'nat': nat,
            'args32': (x_q, mem, eye, zero, wk, bk, wv, bv, heads, mask)}


def f32_baseline(case):
    out32, _ = R.attention(case['q'], case['k'], case['v'], case['mask'], case['heads'], case['scale'], dtype=np.float32)
    return worst_ratio(out32, case['want'], case['nat'])


def split_baseline(case, mode):
    return worst_ratio(R.attention_split(case['q'], case['k'], case['v'], case['mask'], case['heads'], case['scale'], mode), case['want'], case['nat'])


def sweep_case(kind, gain_exp):
    """The gain sweep of the split cores: one small shape (2 x 40 queries x 130 keys x 2 heads, a random mask), randn operands with
    2^gain_exp on q.k (half of it on q, half on k) or on v."""
    q, k, v, mask = attention_inputs(4000, 2, 40, 130, 2, 32, 'randn', 'rand')
    f = np.float32
    if kind == 'qk':
        q, k = q * f(2.0 ** (gain_exp // 2)), k * f(2.0 ** (gain_exp - gain_exp // 2))
    else:
        v = v * f(2.0 ** gain_exp)
    want, nat = R.attention(q, k, v, mask, 2, 32 ** -0.5)
    return {'q': q, 'k': k, 'v': v, 'mask': mask, 'heads': 2, 'scale': 32 ** -0.5, 'want': want, 'nat': nat}


SWEEP = [(kind, g) for kind in ('qk', 'v') for g in range(-12, 9, 2)]


# ------------------------------------------------------------------------------------------------------------------------
# LayerNorm: inputs and bound
# ------------------------------------------------------------------------------------------------------------------------
LN_K = 16.0


def layernorm_allowance(x, y, gamma, beta, eps):
    """Per element, with v = x + y, n = (v - mean) rstd the normalised value, vmax = max |v| of the row, u = 2^-24:

        LN_K u (|gamma| (1 + |n|) vmax rstd + |gamma n| + |beta|),   LN_K = 16.

    Two-pass form in float32.  d = v - mean carries the rounding of v (1), of the row sum (PER_LANE - 1 <= 7 serial additions and 6
    butterfly steps, each relative to a partial sum <= C vmax), of the division (1) and of the subtraction (1): <= 16 u vmax, ABSOLUTE,
    which rstd turns into the first term.  The variance does not see the error of the mean in first order (sum d = 0), only the
    d-errors of the single elements and its own 6 + 7 + 4 roundings (squares, sums, division, + eps, sqrt, reciprocal), halved by the
    square root: a relative error of rstd below 16 u (1 + vmax rstd), which multiplies n - hence the factor (1 + |n|).  The last
    three operations (x rstd, x gamma, + beta) add 3 u of |gamma n| + |out|.  A one-pass variance E[v^2] - mean^2 errs by u vmax^2
    rstd^2 relative instead - 1e8 u at an offset of 1e4 - and a lost eps changes rstd itself: both are far outside."""
    v = np.asarray(x, F64) + (0.0 if y is None else np.asarray(y, F64))
    mean = v.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((v - mean) ** 2).mean(-1, keepdims=True) + eps)
    n = (v - mean) * rstd
    g, b = np.abs(np.asarray(gamma, F64)), np.abs(np.asarray(beta, F64))
    return LN_K * U32 * (g * (1.0 + np.abs(n)) * np.abs(v).max(-1, keepdims=True) * rstd + g * np.abs(n) + b)


def layernorm_rows(c, rows, seed):
    """x, y (rows, c), gamma, beta: the row families in turn - unit variance on an offset of 1e4; constant rows (variance 0: the result
    is beta, governed by eps); one element of 1e6 among zeros; variance about 1e-8 around 1 (comparable to an eps of 1e-8, far below
    one of 1e-5); plain randn."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, c))
    y = 0.5 * rng.standard_normal((rows, c))
    for r in range(rows):
        fam = r % 5
        if fam == 0:
            x[r] += 1e4
        elif fam == 1:
            x[r] = 3.7 * (r + 1)
            y[r] = -1.2
        elif fam == 2:
            x[r] = 0.0
            y[r] = 0.0
            x[r, (7 * r) % c] = 1e6
        elif fam == 3:
            x[r] = 1.0 + 1e-4 * x[r]
            y[r] = 1e-5 * y[r]
    gamma = rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)
    beta = 0.3 * rng.standard_normal(c)
    f = lambda a: np.ascontiguousarray(a, np.float32)        # noqa: E731
    return f(x), f(y), f(gamma), f(beta)


def layernorm_f32(x, y, gamma, beta, eps, one_pass=False, drop_eps=False):
    """The two-pass form in float32 on the host (numpy; sums in numpy's own order).  one_pass / drop_eps: the planted faults."""
    f = np.float32
    v = x if y is None else (x + y).astype(f)
    c = f(v.shape[-1])
    mean = (v.sum(-1, keepdims=True, dtype=f) / c).astype(f)
    d = (v - mean).astype(f)
    if one_pass:
        var = ((v * v).astype(f).sum(-1, keepdims=True, dtype=f) / c - mean * mean).astype(f)
    else:
        var = ((d * d).astype(f).sum(-1, keepdims=True, dtype=f) / c).astype(f)
    with np.errstate(divide='ignore', invalid='ignore'):
        rstd = (f(1) / np.sqrt((var + (f(0) if drop_eps else f(eps))).astype(f))).astype(f)
        return ((d * rstd).astype(f) * gamma + beta).astype(f)


# ------------------------------------------------------------------------------------------------------------------------
# point-wise stacks: inputs
# ------------------------------------------------------------------------------------------------------------------------
#               groups, group_rows
ROW_GEOMETRY = [(1, 32), (2, 32), (9, 32), (1, 64), (3, 96), (1, 288), (5, 160), (2, 1056)]
#                  geometry c3  x_cols tap
POINTNET_CASES = [(0, 128, 0, True), (1, 256, 16, False), (2, 512, 32, True), (3, 256, 0, False), (4, 128, 32, True), (5, 512, 16, False),
                  (6, 256, 0, True), (7, 128, 32, False)]
#               geometry kv    group addend  ldg
CHAIN_CASES = [(0, True, True, 512), (1, False, False, 0), (2, True, True, 640), (3, False, True, 512), (4, True, False, 0), (5, False, True, 640),
               (6, True, True, 512), (7, False, True, 512)]


def split_allowance_args(mode):
    return {'bound': BOUND[mode], 'u2': SPLIT_U2[mode], 'floor': SPLIT_FLOOR[mode]}


def pointnet_inputs(seed, groups, group_rows, c3, x_cols, zero_group=True):
    """Rows (zero-padded to 32 columns) and three layers.  The first and the last row of every group are 4x the others (their
    activations dominate: the group's maximum sits in the first row for some channels and in the last for others -
    first_last_share() counts them); group `groups // 2` is all zero and every bias is <= 0 (b3 < 0): its pre-ReLU values are b1, b2
    (<= 0) and b3 (< 0), its pooled row exactly 0.  The weight rows of the padding columns are random: the kernel must feed zeros."""
    rng = np.random.default_rng(seed)
    rows = groups * group_rows
    cin = {0: 29, 16: 11, 32: 30}[x_cols]
    x = np.zeros((rows, 32), np.float32)
    x[:, :cin] = 0.4 * rng.standard_normal((rows, cin))
    x[0::group_rows, :cin] *= 4.0
    x[group_rows - 1::group_rows, :cin] *= 4.0
    zg = groups // 2 if zero_group and groups > 1 else -1
    if zg >= 0:
        x[zg * group_rows:(zg + 1) * group_rows] = 0.0
    layers = []
    for li, (ci, co) in enumerate(((32, 128), (128, 128), (128, c3))):
        w = (rng.standard_normal((ci, co)) / np.sqrt(cin if li == 0 else ci)).astype(np.float32)
        s = (rng.uniform(0.5, 1.5, co) * rng.choice([-1.0, 1.0], co)).astype(np.float32)
        b = (-np.abs(0.3 * rng.standard_normal(co)) - (0.05 if li == 2 else 0.0)).astype(np.float32)
        layers.append((w, s, b))
    return x, layers, zg


def first_last_share(x, layers, group_rows):
    """Share of the (group, channel) maxima of the float64 reference that sit in the group's first / last row."""
    acts, _ = R.layer_stack(x, layers, None, 0.0, 0.0)
    rows, c3 = acts[2].shape
    am = acts[2].reshape(rows // group_rows, group_rows, c3).argmax(1)
    pos = acts[2].reshape(rows // group_rows, group_rows, c3).max(1) > 0
    return float(((am == 0) & pos).sum()) / max(int(pos.sum()), 1), float(((am == group_rows - 1) & pos).sum()) / max(int(pos.sum()), 1)


def split_layers(layers, mode):
    return [(R.split_value(w, mode), s, b) for w, s, b in layers]


def chain_inputs(seed, groups, group_rows, ldg):
    rng = np.random.default_rng(seed)
    rows = groups * group_rows
    f = np.float32
    x = np.maximum(rng.standard_normal((rows, 128)), 0).astype(f)
    dims = [(128, 512), (512, 256), (256, 256), (256, 256)]
    ws = [(rng.standard_normal(d) / np.sqrt(d[0])).astype(f) for d in dims]
    sc = [(rng.uniform(0.5, 1.5, d[1]) * rng.choice([-1.0, 1.0], d[1])).astype(f) for d in dims[:2]]
    sh = [(0.3 * rng.standard_normal(d[1])).astype(f) for d in dims]
    gs = None
    if ldg:
        gs = np.full((groups, ldg), np.nan, f)
        gs[:, :512] = rng.standard_normal((groups, 512))
    return x, ws, sc, sh, gs


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the references by hand, against differently written code, on planted faults; the host baselines
# ------------------------------------------------------------------------------------------------------------------------
def test_attention_reference_by_hand():
    # two keys, one masked: the output is the live key's value, whatever the masked key holds; sum p |v| = |v|
    q = np.array([[[1.0, 2.0]]])
    k = np.array([[[0.5, -1.0], [np.nan, 1e30]]])
    v = np.array([[[3.0, -4.0], [100.0, 100.0]]])
    out, nat = R.attention(q, k, v, np.array([[0, 1]]), 1, 0.5)
    assert out.tolist() == [[[3.0, -4.0]]] and nat.tolist() == [[[3.0, 4.0]]]
    # two live keys with scores ln 3 apart: p = (1/4, 3/4)
    k = np.array([[[0.0, 0.0], [np.log(3.0), 0.0]]])
    out, nat = R.attention(np.array([[[2.0, 7.0]]]), k, v, None, 1, 0.5)
    assert np.allclose(out, [[[0.25 * 3 + 0.75 * 100, 0.25 * -4 + 0.75 * 100]]], rtol=1e-14)
    assert np.allclose(nat, [[[0.25 * 3 + 0.75 * 100, 0.25 * 4 + 0.75 * 100]]], rtol=1e-14)
    # two heads of one channel each see their own channel only; every key masked -> NaN for that batch entry only
    q2 = np.array([[[1.0, 1.0]], [[1.0, 1.0]]])
    k2 = np.array([[[0.0, 50.0], [50.0, 0.0]]] * 2)
    v2 = np.array([[[1.0, 2.0], [3.0, 4.0]]] * 2)
    out, _ = R.attention(q2, k2, v2, np.array([[0, 0], [1, 1]]), 2, 1.0)
    assert np.allclose(out[0], [[3.0, 2.0]], atol=1e-12) and np.isnan(out[1]).all()
    # the folded form: identity projections and zero biases reduce it to attention()
    e = np.eye(2)
    o3, n3, q3 = R.folded_attention(q, v, e, np.zeros(2), e, np.zeros(2), e, np.zeros(2), 1, None)
    o4, n4 = R.attention(q, v, v, None, 1, 2 ** -0.5)
    assert np.array_equal(o3, o4) and np.array_equal(n3, n4) and np.array_equal(q3, q)


def test_pointwise_references_by_hand():
    # a chain of 1 x 1 layers with identity weights: ReLU of the input, the group maximum of it
    x = np.array([[1.0, -2.0], [0.5, 3.0], [-1.0, -1.0], [-4.0, -0.5]])
    eye = (np.eye(2), np.ones(2), np.zeros(2))
    pooled, tap = R.pointnet3(x, [eye, eye, eye], 2)
    assert pooled.tolist() == [[1.0, 3.0], [0.0, 0.0]] and tap.tolist() == np.maximum(x, 0).tolist()
    # linear: (x w + addend of the row's group) * scale + shift, the last group ragged (rows 0, 1 | 2)
    y, den = R.linear(np.array([[1.0, 2.0], [0.0, -1.0], [3.0, 0.0]]), np.array([[2.0], [-1.0]]), np.array([-2.0]), np.array([1.0]), False,
                      np.array([[10.0], [-20.0]]), 2, with_den=True)
    assert y.tolist() == [[-19.0], [-21.0], [29.0]] and den.tolist() == [[29.0], [23.0], [53.0]]
    assert R.linear(np.array([[1.0, 2.0]]), np.array([[2.0], [-1.0]]), None, np.array([-1.0]), True).tolist() == [[0.0]]
    # the chain: h = ReLU((x wa + addend) sa + ba), mem = ReLU(h wb sb + bb), k = mem wk + bk
    one, zero = np.ones(1), np.zeros(1)
    mem, kk, vv = R.mlp_chain(np.array([[2.0], [2.0]]), (np.array([[3.0]]), one, -one), (np.array([[0.5]]), 2 * one, zero), np.array([[1.0], [-7.0]]), 1,
                              kv=(np.array([[2.0]]), one, np.array([[-1.0]]), zero))
    assert mem.tolist() == [[6.0], [0.0]] and kk.tolist() == [[13.0], [1.0]] and vv.tolist() == [[-6.0], [0.0]]


def test_small_op_references_by_hand():
    # a LayerNorm row of [1, 2, 3, 4] * 16 + 1e4: mean 1e4 + 40, deviations -24, -8, 8, 24, variance 320
    x = np.array([[1.0, 2.0, 3.0, 4.0]]) * 16 + 1e4
    out = R.add_layernorm(x, None, np.ones(4), np.zeros(4), 0.0)
    assert np.allclose(out, np.array([[-24.0, -8.0, 8.0, 24.0]]) / np.sqrt(320.0), rtol=1e-12)
    out = R.add_layernorm(x - 1e4, np.full((1, 4), 1e4), 2 * np.ones(4), np.ones(4), 80.0)
    assert np.allclose(out, 2 * np.array([[-24.0, -8.0, 8.0, 24.0]]) / 20.0 + 1, rtol=1e-12)
    assert np.array_equal(R.add_layernorm(x, np.ones((1, 4)), None, None, 0.0, norm=False), x + 1)
    # combine: group 0 (rows 0, 1) skipped -> 2 post; group 1 -> post + LN
    xx = np.array([[0.0, 2.0], [5.0, 7.0], [1.0, 3.0]])
    post = np.array([[1.0, 1.0], [2.0, 3.0], [10.0, 20.0]])
    out = R.add_layernorm_combine(xx, None, np.ones(2), np.zeros(2), 0.0, post, np.array([1, 0]), 2)
    assert out[:2].tolist() == [[2.0, 2.0], [4.0, 6.0]] and np.allclose(out[2], [9.0, 21.0], rtol=1e-12)
    # group max: -0.0 < +0.0 in either order, only -0.0 stays -0.0, -inf is a value
    gm = R.group_max(np.array([[-0.0, 0.0, -0.0, -np.inf], [0.0, -0.0, -0.0, -np.inf], [-1.0, -2.0, -3.0, -np.inf], [5.0, -7.0, -1.0, 2.0]], np.float32), 2, 2)
    assert gm.tolist() == [[0.0, 0.0, -0.0, -np.inf], [5.0, -2.0, -1.0, 2.0]]
    assert np.signbit(gm[0]).tolist() == [False, False, True, True]
    z = np.zeros((3, 4), np.int32)
    t2 = z.copy()
    t2[1, 3] = -2 ** 31
    assert R.rows_all_zero([z]).tolist() == [True] * 3 and R.rows_all_zero([z, t2]).tolist() == [True, False, True]


def test_split_pair_by_hand_and_round_trip():
    """hi + lo reproduces a float32 to 22 bits (f16x2) / 16 bits (bf16x2) over [2^-6, 2^6] - for fp16 only while the lo half is a normal
    number: from |x| < 2^-3 down the error is bounded by 2^-25 absolute instead (oracle.refine.split_pair states it; shown here)."""
    # by hand: 1 + 2^-11 + 2^-20 is just above the tie between 1 and 1 + 2^-10: hi rounds up, lo = the (negative) rest, exactly
    x = np.array([1.0 + 2.0 ** -11 + 2.0 ** -20], np.float32)
    hi, lo = R.split_pair(x, 'f16x2')
    assert hi[0] == 1.0 + 2.0 ** -10 and lo[0] == -(2.0 ** -11) + 2.0 ** -20 and hi[0] + lo[0] == float(x[0])
    hi, lo = R.split_pair(np.array([1.0 + 2.0 ** -11], np.float32), 'f16x2')          # the tie itself goes to even
    assert hi[0] == 1.0 and lo[0] == 2.0 ** -11
    hi, lo = R.split_pair(np.array([1.0 + 2.0 ** -8 + 2.0 ** -9 + 2.0 ** -16], np.float32), 'bf16x2')
    assert hi[0] == 1.0 + 2.0 ** -7 and lo[0] == -(2.0 ** -9) + 2.0 ** -16
    hi, lo = R.split_pair(np.array([1e6, -1e30], np.float32), 'f16x2')                   # saturation, both halves
    assert hi.tolist() == [65504.0, -65504.0] and lo.tolist() == [65504.0, -65504.0]
    assert R.split_product(np.array([3.0], np.float32), np.array([0.5], np.float32), 'bf16x2')[0] == 1.5
    rng = np.random.default_rng(5)
    x = (rng.uniform(1.0, 2.0, 200000) * 2.0 ** rng.integers(-6, 6, 200000) * rng.choice([-1.0, 1.0], 200000)).astype(np.float32)
    x64 = x.astype(F64)
    for mode in R.MODES:
        hi, lo = R.split_pair(x, mode)
        err = np.abs(x64 - hi - lo)
        assert (err <= np.maximum(SPLIT_U2[mode] * np.abs(x64), SPLIT_FLOOR[mode])).all()
        big = np.abs(x64) >= 2.0 ** -3
        rel, rel_small = float((err[big] / np.abs(x64[big])).max()), float((err[~big] / np.abs(x64[~big])).max())
        print('  split_pair %s: |x - hi - lo| / |x| worst %.2e for |x| >= 2^-3, %.2e below (u^2 = %.2e)' % (mode, rel, rel_small, SPLIT_U2[mode]))
        assert rel <= SPLIT_U2[mode] and rel > SPLIT_U2[mode] / 8
        if mode == 'f16x2':
            assert rel_small > SPLIT_U2[mode]              # the subnormal lo halves: the relative bound does NOT hold below 2^-3
        else:
            assert rel_small <= SPLIT_U2[mode]
        # the same rounding as the host packer the weights go through
        packed = ops.pair16_unpack(ops.pair16_pack(torch.from_numpy(x[:4096].reshape(512, 8)), MATH[mode]), MATH[mode]).numpy().reshape(-1)
        assert np.array_equal(packed, (hi[:4096] + lo[:4096]).astype(np.float32))


def test_references_against_torch_float64():
    rng = np.random.default_rng(9)
    tt = lambda a: torch.from_numpy(np.asarray(a, F64))        # noqa: E731
    # attention against nn.functional.multi_head_attention_forward-free torch code: softmax / bmm with a boolean mask
    b, lq, lk, heads, hd = 2, 5, 19, 4, 8
    q, k, v = rng.standard_normal((b, lq, 32)), rng.standard_normal((b, lk, 32)), rng.standard_normal((b, lk, 32))
    mask = rng.random((b, lk)) < 0.4
    mask[:, 0] = False
    out, nat = R.attention(q, k, v, mask, heads, hd ** -0.5)
    th = lambda a: tt(a).reshape(b, -1, heads, hd).transpose(1, 2)        # noqa: E731
    ref = F.scaled_dot_product_attention(th(q), th(k), th(v), attn_mask=~torch.from_numpy(mask)[:, None, None, :])
    assert np.allclose(out, ref.transpose(1, 2).reshape(b, lq, 32).numpy(), rtol=1e-12, atol=1e-13)
    p = torch.softmax((th(q) * hd ** -0.5 @ th(k).transpose(-1, -2)).masked_fill(torch.from_numpy(mask)[:, None, None, :], float('-inf')), -1)
    assert np.allclose(nat, (p @ th(v).abs()).transpose(1, 2).reshape(b, lq, 32).numpy(), rtol=1e-12)
    # folded attention against nn.functional.multi_head_attention_forward (sequence first; no out projection: identity)
    e = 32
    x_q, mem = rng.standard_normal((b, lq, e)), rng.standard_normal((b, lk, e))
    wq, wk, wv = (rng.standard_normal((e, e)) / 4 for _ in range(3))
    bq, bk, bv = (rng.standard_normal(e) for _ in range(3))
    o2, _, _ = R.folded_attention(x_q, mem, wq, bq, wk, bk, wv, bv, heads, mask)
    ref2, _ = F.multi_head_attention_forward(tt(x_q).transpose(0, 1), tt(mem).transpose(0, 1), tt(mem).transpose(0, 1), e, heads,
                                             torch.cat([tt(wq), tt(wk), tt(wv)]), torch.cat([tt(bq), tt(bk), tt(bv)]), None, None, False, 0.0,
                                             torch.eye(e, dtype=torch.float64), torch.zeros(e, dtype=torch.float64), training=False,
                                             key_padding_mask=torch.from_numpy(mask), need_weights=False)
    assert np.allclose(o2, ref2.transpose(0, 1).numpy(), rtol=1e-11, atol=1e-12)
    # linear / pointnet3 / mlp_chain against F.linear, F.relu, F.max_pool1d
    rows, gr = 24, 4
    x = rng.standard_normal((rows, 6))
    layers = [(rng.standard_normal((6, 5)), rng.uniform(0.5, 1.5, 5), rng.standard_normal(5)), (rng.standard_normal((5, 7)), -rng.uniform(0.5, 1.5, 7), rng.standard_normal(7)),
              (rng.standard_normal((7, 3)), rng.uniform(0.5, 1.5, 3), rng.standard_normal(3))]
    h = tt(x)
    hs = []
    for w, s, bb in layers:
        h = F.relu(F.linear(h, tt(w).T) * tt(s) + tt(bb))
        hs.append(h)
    pooled, tap = R.pointnet3(x, layers, gr)
    assert np.allclose(tap, hs[1].numpy(), rtol=1e-12, atol=1e-13)
    assert np.allclose(pooled, F.max_pool1d(hs[2].T[None], gr)[0].T.numpy(), rtol=1e-12, atol=1e-13)
    gs = rng.standard_normal((rows // gr, 5))
    mem2, k2, v2 = R.mlp_chain(x, layers[0], layers[1], gs, gr, kv=(layers[2][0], layers[2][2], -layers[2][0], layers[2][1]))
    h1 = F.relu((F.linear(tt(x), tt(layers[0][0]).T) + tt(gs).repeat_interleave(gr, 0)) * tt(layers[0][1]) + tt(layers[0][2]))
    h2 = F.relu(F.linear(h1, tt(layers[1][0]).T) * tt(layers[1][1]) + tt(layers[1][2]))
    assert np.allclose(mem2, h2.numpy(), rtol=1e-12, atol=1e-13)
    assert np.allclose(k2, F.linear(h2, tt(layers[2][0]).T, tt(layers[2][2])).numpy(), rtol=1e-12, atol=1e-13)
    assert np.allclose(v2, F.linear(h2, -tt(layers[2][0]).T, tt(layers[2][1])).numpy(), rtol=1e-12, atol=1e-13)
    y5 = R.linear(x[:22], layers[0][0], layers[0][1], layers[0][2], False, gs, gr)              # ragged last group
    assert np.allclose(y5, ((F.linear(tt(x), tt(layers[0][0]).T) + tt(gs).repeat_interleave(gr, 0)) * tt(layers[0][1]) + tt(layers[0][2]))[:22].numpy(), rtol=1e-12)
    # small operations
    xs, ys, g, bt = rng.standard_normal((7, 64)) + 3, rng.standard_normal((7, 64)), rng.standard_normal(64), rng.standard_normal(64)
    assert np.allclose(R.add_layernorm(xs, ys, g, bt, 1e-5), F.layer_norm(tt(xs) + tt(ys), (64,), tt(g), tt(bt), 1e-5).numpy(), rtol=1e-11, atol=1e-12)
    post, skip = rng.standard_normal((7, 64)), np.array([0, 1, 0, 1], np.uint8)
    ln = F.layer_norm(tt(xs) + tt(ys), (64,), tt(g), tt(bt), 1e-5)
    ref = tt(post) + torch.where(torch.from_numpy(skip).bool().repeat_interleave(2)[:7, None], tt(post), ln)
    assert np.allclose(R.add_layernorm_combine(xs, ys, g, bt, 1e-5, post, skip, 2), ref.numpy(), rtol=1e-11, atol=1e-12)
    xm = rng.standard_normal((12, 5)).astype(np.float32)
    assert np.array_equal(R.group_max(xm, 3, 4), torch.from_numpy(xm).reshape(3, 4, 5).max(1).values.numpy())
    ti = (rng.random((9, 8)) < 0.05).astype(np.int32)
    assert np.array_equal(R.rows_all_zero([ti, ti[::-1].copy()]), ((torch.from_numpy(ti) == 0).all(1) & (torch.from_numpy(ti[::-1].copy()) == 0).all(1)).numpy())


def test_planted_faults_fail_the_comparison():
    """The comparison helper with each test's own allowance must refuse: an attention with one key dropped, a group maximum over
    group_rows - 1 rows, a variance without the mean subtracted, a LayerNorm without eps - and must accept the honest float32 result."""
    c = mha_case(8)                                                       # block, randn, 63 keys: each carries about 1 / 63 of the weight
    good, _ = R.attention(c['q'], c['k'], c['v'], c['mask'], c['heads'], c['scale'], dtype=np.float32)
    assert_within(good, c['want'], ATT_BOUND['f32'] * c['nat'], 'attention, float32 host', ATT_BOUND['f32'])
    for drop in (0, 31, 62):
        keep = np.arange(63) != drop
        bad, _ = R.attention(c['q'], c['k'][:, keep], c['v'][:, keep], None, c['heads'], c['scale'])
        with pytest.raises(AssertionError):
            assert_within(bad, c['want'], ATT_BOUND['f32'] * c['nat'], 'attention without key %d' % drop, ATT_BOUND['f32'])
    x, layers, zg = pointnet_inputs(77, 3, 96, 128, 0)
    for mode in R.MODES:
        xs, ls = R.split_value(x, mode), split_layers(layers, mode)
        pooled, tap, a_pool, a_tap = R.pointnet3(xs, ls, 96, **split_allowance_args(mode))
        acts, _ = R.layer_stack(xs, ls, None, 0.0, 0.0)
        for cut in (slice(1, None), slice(0, -1)):                        # the group's first / last row left out
            bad = acts[2].reshape(3, 96, 128)[:, cut].max(1)
            with pytest.raises(AssertionError):
                assert_within(bad, pooled, a_pool, 'pooled without a row (%s)' % mode)
        assert_within(R.pointnet3(x, layers, 96)[0], pooled, 10 * a_pool, 'pooled, unsplit operands (%s)' % mode)
    xx, yy, g, b = layernorm_rows(256, 20, 1)
    for eps in (1e-5, 1e-8):
        want, allow = R.add_layernorm(xx, yy, g, b, eps), layernorm_allowance(xx, yy, g, b, eps)
        assert_within(layernorm_f32(xx, yy, g, b, eps), want, allow, 'LayerNorm, float32 host, eps %g' % eps)
        for fault in ('one_pass', 'drop_eps'):
            with np.errstate(all='ignore'):
                bad = layernorm_f32(xx, yy, g, b, eps, **{fault: True})
            with pytest.raises(AssertionError):
                assert_within(np.nan_to_num(bad, nan=1e30), want, allow, 'LayerNorm with %s' % fault)


def test_attention_case_tables_reach_every_route():
    seen = set()
    for route, b, lq, lk, heads, family, mk in MHA_CASES:
        assert route == mha_route(lq) and heads in (1, 8) and b in (1, 3, 5)
        seen.add((route, mk is not None))
    assert seen == {(r, m) for r in ('wave', 'block', 'blocks') for m in (False, True)}
    assert {c[2] for c in MHA_CASES} == {1, 16, 17, 32, 33, 64, 96, 97, 256, 257, 300}
    assert {c[3] for c in MHA_CASES} == {1, 5, 15, 16, 17, 63, 64, 65, 129, 200}
    items = {c[1] * c[4] * ((c[2] + 15) // 16) for c in MHA_CASES if c[0] == 'wave'}
    assert 1 in items and 5 in items
    assert {f for c in MHA_CASES for f in (c[5],)} == {'randn', 'rise', 'fall', 'spread', 'equal'}
    seen = set()
    for route, r, l, e, family, mk in ATT1H_CASES:
        assert route == att1h_route(l, e)
        seen.add((route, mk is not None))
    assert seen == {(r, m) for r in ('wave', 'staged') for m in (False, True)}
    assert {c[2] for c in ATT1H_CASES} == {1, 16, 63, 64, 65, 100, 200, 255, 256} and {c[3] for c in ATT1H_CASES} == {64, 128, 192, 256}
    assert {c[3] for c in FOLD_CASES} == {1, 15, 16, 17, 255, 256, 257, 496, 497, 512, 1000} and {c[1] * c[2] for c in FOLD_CASES} == {1, 3, 24, 32}
    assert [fold_splits(1, lk, 256) for lk in (257, 496, 497, 512, 1000)] == [1, 1, 2, 2, 3]
    # the rise family does what it is there for: in float64 the running maximum of EVERY query rises in every 16-key tile
    for i, c in enumerate(MHA_CASES):
        if c[5] == 'rise' and c[6] is None:
            d = mha_case(i)
            b, lq, lk, heads = c[1], c[2], c[3], c[4]
            s = np.einsum('bqhd,bkhd->bhqk', d['q'].reshape(b, lq, heads, 32).astype(F64), d['k'].reshape(b, lk, heads, 32).astype(F64))
            tmax = np.stack([s[..., t:t + 16].max(-1) for t in range(0, lk, 16)], -1)
            assert (np.diff(tmax, axis=-1) > 0).all()


def test_attention_host_baselines():
    """ATT_BASE: the worst normalised error, against float64, of the host evaluations over every attention case of this module - the
    same formula in float32 numpy for the fp32 kernels, the split_pair / split_product emulation for the split cores.  The constants
    must cover what is measured here and not be more than twice as large."""
    worst = {'f32': 0.0, 'att1h': 0.0, 'fold': 0.0, 'fold1': 0.0, 'f16x2': 0.0, 'bf16x2': 0.0}
    fam = {}
    for i, c in enumerate(MHA_CASES):
        d = mha_case(i)
        e32 = f32_baseline(d)
        worst['f32'] = max(worst['f32'], e32)
        fam[c[5]] = max(fam.get(c[5], 0.0), e32)
        for mode in R.MODES:
            worst[mode] = max(worst[mode], split_baseline(d, mode))
    for i in range(len(ATT1H_CASES)):
        worst['att1h'] = max(worst['att1h'], f32_baseline(att1h_case(i)))
    for i in range(len(FOLD_CASES)):
        d = fold_case(i)
        out32, _, _ = R.folded_attention(*d['args32'], dtype=np.float32)
        worst[fold_key(i)] = max(worst[fold_key(i)], worst_ratio(out32, d['want'], d['nat']))
    print('  attention host baselines: ' + ', '.join('%s %.2e (ATT_BASE %.2e, bound %.2e)' % (m, worst[m], ATT_BASE[m], ATT_BOUND[m]) for m in worst))
    print('  float32, dz_mha_core cases by family: ' + ', '.join('%s %.2e' % kv for kv in sorted(fam.items())))
    for m in worst:
        assert worst[m] <= ATT_BASE[m], (m, worst[m])


def test_split_gain_range_on_the_host():
    """The operand range of the split cores, from the emulation alone: the gains of the sweep at which split operands keep the
    normalised error within ATT_BASE (what the module's other cases need).  SPLIT_GAIN_RANGE states it; ops.mha_core's docstring
    repeats it (the sweep on the kernel itself is test_mha_core_split_gain_sweep)."""
    for mode in R.MODES:
        for kind in ('qk', 'v'):
            errs = {g: split_baseline(sweep_case(kind, g), mode) for k2, g in SWEEP if k2 == kind}
            print('  split emulation %s, gain on %s: ' % (mode, kind) + ', '.join('2^%d %.1e' % (g, errs[g]) for g in sorted(errs)))
            lo, hi = SPLIT_GAIN_RANGE[mode][kind]
            inside = [g for g in errs if lo <= g <= hi]
            assert all(errs[g] <= ATT_BASE[mode] for g in inside), (mode, kind)


def test_pointnet_inputs_put_maxima_in_first_and_last_rows():
    for geo, c3, x_cols, tap in POINTNET_CASES:
        groups, gr = ROW_GEOMETRY[geo]
        x, layers, zg = pointnet_inputs(500 + geo, groups, gr, c3, x_cols)
        first, last = first_last_share(x, layers, gr)
        pooled, _ = R.pointnet3(x, layers, gr)
        print('  pointnet %d x %d: %.0f %% of the maxima in the first row, %.0f %% in the last' % (groups, gr, 100 * first, 100 * last))
        assert first > 0.1 and last > 0.1 and pooled.max() > 0 and (zg < 0 or not pooled[zg].any())


# ------------------------------------------------------------------------------------------------------------------------
# GPU plumbing
# ------------------------------------------------------------------------------------------------------------------------
def dev(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


class Out:
    """A (rows + TAIL, cols) buffer of 32-bit words filled with SENTINEL; the kernel under test is handed its start."""

    def __init__(self, rows, cols, device):
        self.rows, self.cols = rows, cols
        self.raw = torch.full((rows + TAIL, cols), SENTINEL, dtype=torch.int32, device=device)

    @property
    def ptr(self):
        return self.raw.data_ptr()

    def f32(self, cols=None):
        return self.raw.view(torch.float32)[:self.rows, :cols]

    def run_twice(self, launch):
        """Launch, keep the bits, refill, launch again: the same bits."""
        launch()
        first = self.raw.clone()
        self.raw.fill_(SENTINEL)
        launch()
        assert torch.equal(first, self.raw), 'two launches differ'

    def check(self, cols=None):
        """The tail rows and the columns from `cols` on keep the sentinel word for word."""
        assert bool((self.raw[self.rows:] == SENTINEL).all()), 'tail rows written'
        if cols is not None and cols < self.cols:
            assert bool((self.raw[:self.rows, cols:] == SENTINEL).all()), 'columns beside the result written'

    def untouched(self):
        return bool((self.raw == SENTINEL).all())


def refused(rc, outs, what):
    msg = L.load().dz_last_error()
    assert rc != 0 and msg, what
    assert all(o.untouched() for o in outs), what
    return msg.decode()


def run_attention(device, case, math, b, lq, lk, single_head_e=None):
    """dz_mha_core / dz_mha_core_split / dz_attention_single_head on a case, masked keys poisoned -> (b, lq, e) float64."""
    lib = L.load()
    e = case['q'].shape[-1]
    dq, dk, dv = dev(case['q'], device), dev(poison_keys(case['k'], case['mask'], POISON[math]), device), dev(case['v'], device)
    dm = dev(case['mask'], device)
    out = Out(b * lq, e, device)

    def launch():
        if single_head_e:
            rc = lib.dz_attention_single_head(L.ptr(dq), L.ptr(dk), L.ptr(dv), L.ptr(dm), b, lq, e, case['scale'], out.ptr, L.stream())
        elif math == 'f32':
            rc = lib.dz_mha_core(L.ptr(dq), L.ptr(dk), L.ptr(dv), L.ptr(dm), b, lq, lk, case['heads'], case['scale'], out.ptr, L.stream())
        else:
            rc = lib.dz_mha_core_split(L.ptr(dq), L.ptr(dk), L.ptr(dv), L.ptr(dm), b, lq, lk, case['heads'], case['scale'], out.ptr, MATH[math], L.stream())
        L.check(rc, 'attention')
    out.run_twice(launch)
    out.check()
    return out.f32().cpu().numpy().astype(F64).reshape(b, lq, e)


# ------------------------------------------------------------------------------------------------------------------------
# GPU: attention
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(MHA_CASES)), ids=[case_id(c) for c in MHA_CASES])
def test_mha_core_f32(device, i):
    """dz_mha_core on MHA_CASES[i] (the route is the case's first field) within ATT_BOUND['f32'] of float64, normalised by
    sum_j p_j |v_j|; masked keys hold NaN / 1e30 in K."""
    route, b, lq, lk, heads, family, mk = MHA_CASES[i]
    c = mha_case(i)
    got = run_attention(device, c, 'f32', b, lq, lk)
    assert_within(got, c['want'], ATT_BOUND['f32'] * c['nat'], 'dz_mha_core %s' % case_id(MHA_CASES[i]), ATT_BOUND['f32'])


@pytest.mark.gpu
@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('i', range(len(MHA_CASES)), ids=[case_id(c) for c in MHA_CASES])
def test_mha_core_split(device, i, mode):
    """dz_mha_core_split on the same cases within ATT_BOUND[mode]; masked keys hold NaN and the largest magnitude of the mode in K."""
    route, b, lq, lk, heads, family, mk = MHA_CASES[i]
    c = mha_case(i)
    got = run_attention(device, c, mode, b, lq, lk)
    assert_within(got, c['want'], ATT_BOUND[mode] * c['nat'], 'dz_mha_core_split %s %s' % (mode, case_id(MHA_CASES[i])), ATT_BOUND[mode])


@pytest.mark.gpu
@pytest.mark.parametrize('mode', R.MODES)
def test_mha_core_split_gain_sweep(device, mode):
    """Gains 2^-12 .. 2^8 on q.k and on v at one small shape: the normalised error against float64 per gain, next to the host
    emulation's.  Inside SPLIT_GAIN_RANGE the module's bound holds; outside it (fp16 lo halves of v in the subnormal range) the kernel
    must still be within 8 x the emulation of the same roundings."""
    for kind in ('qk', 'v'):
        line = []
        for k2, g in SWEEP:
            if k2 != kind:
                continue
            c = sweep_case(kind, g)
            got = run_attention(device, c, mode, 2, 40, 130)
            err, emu = worst_ratio(got, c['want'], c['nat']), split_baseline(c, mode)
            lo, hi = SPLIT_GAIN_RANGE[mode][kind]
            bound = ATT_BOUND[mode] if lo <= g <= hi else 8.0 * emu
            line.append('2^%d %.1e (host %.1e)' % (g, err, emu))
            assert err <= bound, (mode, kind, g, err, bound)
        print('  dz_mha_core_split %s, gain on %s: ' % (mode, kind) + ', '.join(line))


@pytest.mark.gpu
@pytest.mark.parametrize('lq', [17, 64, 300], ids=['wave', 'block', 'blocks'])
def test_mha_core_exact_properties(device, lq):
    """No tolerance: keys padded with a masked tail up to the next multiples of 16 and of 64 (random K / V rows behind the mask) give the
    bits of the unpadded call, with and without a mask of its own; permuting batch entries and heads permutes the output; scaling v by
    2^+-20 scales it."""
    b, lk, heads = 3, 129, 8
    q, k, v, mask = attention_inputs(5000 + lq, b, lq, lk, heads, 32, 'randn', 'rand')
    rng = np.random.default_rng(lq)

    def run(q_, k_, v_, m_):
        c = {'q': q_, 'k': k_, 'v': v_, 'mask': m_, 'heads': heads, 'scale': 32 ** -0.5}
        return run_attention(device, c, 'f32', q_.shape[0], lq, k_.shape[1]).astype(np.float32)
    for m in (None, mask):
        base = run(q, k, v, m)
        for lkp in (144, 192):
            kp = np.concatenate([k, rng.standard_normal((b, lkp - lk, heads * 32)).astype(np.float32)], 1)
            vp = np.concatenate([v, rng.standard_normal((b, lkp - lk, heads * 32)).astype(np.float32)], 1)
            mp = np.ones((b, lkp), np.uint8)
            mp[:, :lk] = 0 if m is None else m
            assert np.array_equal(run(q, kp, vp, mp).view(np.int32), base.view(np.int32)), ('padding', lkp, m is None)
    base = run(q, k, v, mask)
    pb, ph = np.array([2, 0, 1]), rng.permutation(heads)
    hp = lambda a: np.ascontiguousarray(a.reshape(a.shape[0], a.shape[1], heads, 32)[:, :, ph].reshape(a.shape))        # noqa: E731
    assert np.array_equal(run(q[pb], k[pb], v[pb], mask[pb]).view(np.int32), base[pb].view(np.int32)), 'batch permutation'
    assert np.array_equal(run(hp(q), hp(k), hp(v), mask).view(np.int32), hp(base).view(np.int32)), 'head permutation'
    for g in (2.0 ** 20, 2.0 ** -20):
        assert np.array_equal(run(q, k, v * np.float32(g), mask).view(np.int32), (base * np.float32(g)).view(np.int32)), ('v gain', g)


@pytest.mark.gpu
@pytest.mark.parametrize('math', ['f32', 'f16x2', 'bf16x2'])
@pytest.mark.parametrize('lq', [17, 64, 300], ids=['wave', 'block', 'blocks'])
def test_mha_core_fully_masked_entry_is_nan_for_that_entry_only(device, lq, math):
    """torch.softmax over a row of -inf is NaN (multi_head_attention.py:273-282); so is every route of dz_mha_core and the split core -
    for the masked batch entry only, its neighbours within the bound."""
    b, lk, heads = 3, 70, 8
    q, k, v, mask = attention_inputs(6000 + lq, b, lq, lk, heads, 32, 'randn', 'rand')
    mask[1] = 1
    want, nat = R.attention(q, k, v, mask, heads, 32 ** -0.5)
    assert np.isnan(want[1]).all() and np.isfinite(want[[0, 2]]).all()
    c = {'q': q, 'k': k, 'v': v, 'mask': mask, 'heads': heads, 'scale': 32 ** -0.5}
    got = run_attention(device, c, math, b, lq, lk)
    assert_within(got, want, ATT_BOUND[math] * nat, 'fully masked entry, %s lq %d' % (math, lq), ATT_BOUND[math])


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(ATT1H_CASES)), ids=[case_id(c) for c in ATT1H_CASES])
def test_attention_single_head(device, i):
    """dz_attention_single_head on ATT1H_CASES[i] (route in the first field) within ATT_BOUND['f32']."""
    route, r, l, e, family, mk = ATT1H_CASES[i]
    c = att1h_case(i)
    got = run_attention(device, c, 'f32', r, l, l, single_head_e=e)
    assert_within(got, c['want'], ATT_BOUND['att1h'] * c['nat'], 'dz_attention_single_head %s' % case_id(ATT1H_CASES[i]), ATT_BOUND['att1h'])


def run_folded(device, d, b, lq, lk, ws_short=0, expect_refusal=False):
    lib = L.load()
    e = 256
    dq, dmem, dm = dev(d['x_q'], device), dev(d['mem'], device), dev(d['mask'], device)
    dwk, dwv, dbv = dev(d['wk'], device), dev(np.ascontiguousarray(d['wv'].T), device), dev(d['bv'], device)
    nbytes = lib.dz_xattn_folded_workspace_bytes(b, lk)
    assert nbytes % 4 == 0
    ws = Out(1, nbytes // 4, device)                     # the workspace is row 0; TAIL rows of the same length behind it
    out = Out(b * lq, e, device)

    def launch():
        return lib.dz_xattn_folded(L.ptr(dq), L.ptr(dmem), L.ptr(dm), L.ptr(dwk), L.ptr(dwv), L.ptr(dbv), b, lq, lk, e, d['heads'], float(256 // d['heads']) ** -0.5,
                                   ws.ptr, nbytes - ws_short, out.ptr, L.stream())
    if expect_refusal:
        return launch(), out, ws
    launch_ok = lambda: L.check(launch(), 'dz_xattn_folded')        # noqa: E731
    out.run_twice(launch_ok)
    out.check()
    ws.check()
    return out.f32().cpu().numpy().astype(F64).reshape(b, lq, e)


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(FOLD_CASES)), ids=[case_id(c) for c in FOLD_CASES])
def test_xattn_folded(device, i):
    """dz_xattn_folded on FOLD_CASES[i] within ATT_BOUND['f32'] of the project-then-attend float64 reference (key bias included there:
    it cancels), its workspace of exactly dz_xattn_folded_workspace_bytes inside a sentinel buffer."""
    b, lq, heads, lk, family, mk = FOLD_CASES[i]
    d = fold_case(i)
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    got = run_folded(device, d, b, lq, lk)
    print('  (%d splits)' % fold_splits(b, lk, cus))
    assert_within(got, d['want'], ATT_BOUND[fold_key(i)] * d['nat'], 'dz_xattn_folded %s' % case_id(FOLD_CASES[i]), ATT_BOUND[fold_key(i)])


# ------------------------------------------------------------------------------------------------------------------------
# GPU: fused PointNet encoder and memory chain
# ------------------------------------------------------------------------------------------------------------------------
def device_layers(layers, mid, device):
    return [(ops.pack_weight_split(dev(w, device), mid), dev(s, device), dev(b, device)) for w, s, b in layers]


def run_pointnet(device, mode, x, layers, groups, gr, c3, x_cols, want_tap, zg):
    lib = L.load()
    mid = MATH[mode]
    rows = groups * gr
    trip = device_layers(layers, mid, device)
    xp = ops.pair16_from_f32(dev(x, device), 32, mid)
    xin = xp if x_cols == 0 else dev(x[:, :x_cols], device)
    out, tap = Out(groups, c3, device), Out(rows, 128, device)
    (w1, s1, b1), (w2, s2, b2), (w3, s3, b3) = trip

    def launch():
        L.check(lib.dz_pointnet3_forward(L.ptr(xin), rows, L.ptr(w1), L.ptr(s1), L.ptr(b1), L.ptr(w2), L.ptr(s2), L.ptr(b2), L.ptr(w3), L.ptr(s3), L.ptr(b3), c3, gr,
                                         tap.ptr if want_tap else None, out.ptr, x_cols, mid, L.stream()), 'dz_pointnet3_forward')
    out.run_twice(launch)                                 # (the tap's bits: compared with the layered path below)
    out.check()
    tap.check()
    assert want_tap or tap.untouched()
    got = out.f32()
    # (c) the layer-by-layer path, bit for bit
    h = xp
    for li, (w, s, b) in enumerate(trip):
        h = ops.linear_split(h, w, s, b, True, w.shape[0], mid, out_f32=li == 2)
        if li == 1:
            tap_layered = h
    assert torch.equal(got, ops.group_max(h, groups, gr)), 'pooled differs from the layered path'
    if want_tap:
        assert torch.equal(tap.f32().view(torch.int32), tap_layered.view(torch.int32)), 'tap differs from the layered path'
    # (a) float64 on the split operands, (b) on the unsplit ones under 10 x the allowance
    pooled, tap_ref, a_pool, a_tap = R.pointnet3(R.split_value(x, mode), split_layers(layers, mode), gr, **split_allowance_args(mode))
    got_np = got.cpu().numpy()
    what = 'dz_pointnet3_forward %s %d x %d c3 %d x_cols %d' % (mode, groups, gr, c3, x_cols)
    assert_within(got_np, pooled, a_pool, what + ', split operands')
    assert_within(got_np, R.pointnet3(x, layers, gr)[0], 10 * a_pool, what + ', unsplit operands')
    if want_tap:
        assert_within(ops.pair16_unpack(tap.f32().cpu(), mid).numpy(), tap_ref, a_tap, what + ', tap')
    if zg >= 0:
        assert not got_np[zg].any() and not np.signbit(got_np[zg]).any(), 'the all-zero group must pool to +0'


@pytest.mark.gpu
@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('case', POINTNET_CASES, ids=[case_id(c) for c in POINTNET_CASES])
def test_pointnet3(device, case, mode):
    """dz_pointnet3_forward at ROW_GEOMETRY[case[0]]: pooled rows (and the tap) against float64 on the split operands within the
    propagated BOUND, against float64 on the unsplit inputs within 10 x that, and bit for bit against the layer-by-layer path."""
    geo, c3, x_cols, tap = case
    groups, gr = ROW_GEOMETRY[geo]
    x, layers, zg = pointnet_inputs(500 + geo, groups, gr, c3, x_cols)
    run_pointnet(device, mode, x, layers, groups, gr, c3, x_cols, tap, zg)


def persistent_geometry(device, waves_per_group, factors=(5, 7, 3, 11, 13)):
    """3 x waves + 1 tiles of 32 rows for a persistent kernel with `waves_per_group` waves per workgroup on min(CUs, ...) workgroups
    (the grid of the host code), in groups of f tiles with f the first of `factors` dividing the tile count."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    tiles = 3 * cus * waves_per_group + 1
    f = next((f for f in factors if tiles % f == 0), 1)
    return tiles // f, 32 * f, tiles, cus * waves_per_group


@pytest.mark.gpu
@pytest.mark.parametrize('mode', R.MODES)
def test_pointnet3_more_tiles_than_waves(device, mode):
    """3 x waves + 1 tiles: four tiles per wave, so groups (of 5 tiles on 256 CUs) start inside a wave's range while the group before is
    shared with the previous wave or workgroup - the atomic flush at a group change - and the last busy wave's range runs past the end."""
    groups, gr, tiles, nwaves = persistent_geometry(device, 8)
    assert -(-tiles // nwaves) == 4
    x, layers, zg = pointnet_inputs(77, groups, gr, 128, 16)
    print('  %d tiles on %d waves, %d groups of %d rows' % (tiles, nwaves, groups, gr))
    run_pointnet(device, mode, x, layers, groups, gr, 128, 16, False, zg)


def run_chain(device, mode, x, ws, sc, sh, gs, groups, gr, kv):
    lib = L.load()
    mid = MATH[mode]
    rows = groups * gr
    xp = ops.pair16_from_f32(dev(x, device), 128, mid)
    dw = [ops.pack_weight_split(dev(w, device), mid) for w in ws]
    dsc, dsh, dgs = [dev(a, device) for a in sc], [dev(a, device) for a in sh], dev(gs, device)
    ldg = 0 if gs is None else gs.shape[1]
    outs = [Out(rows, 256, device) for _ in range(3 if kv else 1)]

    def launch():
        L.check(lib.dz_mlp_chain_forward(L.ptr(xp), rows, L.ptr(dw[0]), L.ptr(dsc[0]), L.ptr(dsh[0]), L.ptr(dgs), ldg, gr, L.ptr(dw[1]), L.ptr(dsc[1]), L.ptr(dsh[1]),
                                         L.ptr(dw[2]) if kv else None, L.ptr(dsh[2]) if kv else None, L.ptr(dw[3]) if kv else None, L.ptr(dsh[3]) if kv else None,
                                         outs[0].ptr, outs[1].ptr if kv else None, outs[2].ptr if kv else None, mid, L.stream()), 'dz_mlp_chain_forward')
    launch()
    first = [o.raw.clone() for o in outs]
    for o in outs:
        o.raw.fill_(SENTINEL)
    launch()
    for o, f in zip(outs, first):
        assert torch.equal(o.raw, f), 'two launches differ'
        o.check()
    # the layered path, bit for bit
    g512 = None if gs is None else dgs[:, :512].contiguous()
    h = ops.linear_split(xp, dw[0], dsc[0], dsh[0], True, 512, mid, group_shift=g512, group_rows=gr if gs is not None else 0)
    mem_l = ops.linear_split(h, dw[1], dsc[1], dsh[1], True, 256, mid, out_f32=True)
    assert torch.equal(outs[0].f32(), mem_l), 'memory differs from the layered path'
    if kv:
        one, mp = torch.ones(256, device=device), ops.pair16_from_f32(mem_l, 256, mid)
        for o, w, b in ((outs[1], dw[2], dsh[2]), (outs[2], dw[3], dsh[3])):
            assert torch.equal(o.f32(), ops.linear_split(mp, w, one, b, False, 256, mid, out_f32=True)), 'K / V differ from the layered path'
    # float64 on the split operands, ALL rows
    sw = [R.split_value(w, mode) for w in ws]
    ref = R.mlp_chain(R.split_value(x, mode), (sw[0], sc[0], sh[0]), (sw[1], sc[1], sh[1]), None if gs is None else gs[:, :512], gr,
                      kv=(sw[2], sh[2], sw[3], sh[3]) if kv else None, **split_allowance_args(mode))
    what = 'dz_mlp_chain_forward %s %d x %d kv %d addend %d' % (mode, groups, gr, kv, ldg)
    for j, name in enumerate(('memory', 'K', 'V')[:len(outs)]):
        assert_within(outs[j].f32().cpu().numpy(), ref[2 * j], ref[2 * j + 1], what + ', ' + name)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('case', CHAIN_CASES, ids=[case_id(c) for c in CHAIN_CASES])
def test_mlp_chain(device, case, mode):
    """dz_mlp_chain_forward at ROW_GEOMETRY[case[0]]: memory (and K, V) bit for bit against the layered path and against float64 on the
    split operands on ALL rows; the addend rows 512 or 640 floats apart (NaN in the columns beyond 512)."""
    geo, kv, addend, ldg = case
    groups, gr = ROW_GEOMETRY[geo]
    x, ws, sc, sh, gs = chain_inputs(700 + geo, groups, gr, ldg if addend else 0)
    run_chain(device, mode, x, ws, sc, sh, gs, groups, gr, kv)


@pytest.mark.gpu
def test_mlp_chain_more_tiles_than_waves(device):
    """3 x waves + 1 tiles (four per wave, the last range past the end), groups of 7 tiles on 256 CUs starting inside a wave's range."""
    groups, gr, tiles, nwaves = persistent_geometry(device, 4, factors=(7, 5, 3, 11, 13))
    assert -(-tiles // nwaves) == 4
    x, ws, sc, sh, gs = chain_inputs(99, groups, gr, 512)
    print('  %d tiles on %d waves, %d groups of %d rows' % (tiles, nwaves, groups, gr))
    run_chain(device, 'f16x2', x, ws, sc, sh, gs, groups, gr, False)


# ------------------------------------------------------------------------------------------------------------------------
# GPU: linear layers
# ------------------------------------------------------------------------------------------------------------------------
#                rows cin x_extra cout cout_pad y_extra group_rows relu
LINEAR_CASES = [(1, 32, 0, 16, 16, 0, 0, True),
                (31, 64, 8, 19, 32, 5, 1, False),
                (127, 64, 8, 100, 128, 28, 37, True),
                (128, 32, 0, 64, 64, 0, 100, True),
                (129, 96, 32, 130, 192, 2, 129, False),
                (300, 64, 16, 250, 256, 6, 37, True)]


def linear_inputs(seed, rows, cin, cout_pad, group_rows):
    rng = np.random.default_rng(seed)
    f = np.float32
    x = rng.standard_normal((rows, cin)).astype(f)
    w = (rng.standard_normal((cin, cout_pad)) / np.sqrt(cin)).astype(f)              # the padding columns too: they must not be written
    s = (rng.uniform(0.5, 1.5, cout_pad) * rng.choice([-1.0, 1.0], cout_pad)).astype(f)
    b = (0.3 * rng.standard_normal(cout_pad)).astype(f)
    gs = rng.standard_normal((-(-rows // group_rows), cout_pad)).astype(f) if group_rows else None
    return x, w, s, b, gs


def embed(x, extra, fill):
    if not extra:
        return x
    out = np.full((x.shape[0], x.shape[1] + extra), fill, x.dtype)
    out[:, :x.shape[1]] = x
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('case', LINEAR_CASES, ids=[case_id(c) for c in LINEAR_CASES])
def test_linear_forward_f32(device, case):
    """dz_linear_forward within BOUND['f32'] of float64, normalised by what was summed: cout < cout_pad, NaN in the unused input columns,
    sentinel columns beside the result, group addends whose boundaries fall inside a tile (the last group ragged)."""
    rows, cin, x_extra, cout, cout_pad, y_extra, gr, relu = case
    x, w, s, b, gs = linear_inputs(rows + cin, rows, cin, cout_pad, gr)
    dx, dw, ds, db, dgs = dev(embed(x, x_extra, np.nan), device), dev(w, device), dev(s, device), dev(b, device), dev(gs, device)
    out = Out(rows, cout + y_extra, device)
    out.run_twice(lambda: L.check(L.load().dz_linear_forward(L.ptr(dx), rows, cin, cin + x_extra, L.ptr(dw), cout, cout_pad, L.ptr(ds), L.ptr(db), L.ptr(dgs), gr,
                                                             1 if relu else 0, out.ptr, cout + y_extra, L.stream()), 'dz_linear_forward'))
    out.check(cout)
    want, den = R.linear(x, w[:, :cout], s[:cout], b[:cout], relu, None if gs is None else gs[:, :cout], max(gr, 1), with_den=True)
    assert_within(out.f32(cout).cpu().numpy(), want, BOUND['f32'] * den, 'dz_linear_forward %s' % case_id(case), BOUND['f32'])


@pytest.mark.gpu
@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('out_f32', [True, False], ids=['f32out', 'pair16out'])
@pytest.mark.parametrize('case', LINEAR_CASES, ids=[case_id(c) for c in LINEAR_CASES])
def test_linear_forward_split(device, case, out_f32, mode):
    """dz_linear_forward_split on pair16 rows (cin, cout_pad in multiples of 32) with fp32 and pair16 results: float64 on the split
    operands within BOUND[mode] (a pair16 result is rounded once more: + u^2 |y| + the subnormal floor)."""
    rows, cin, x_extra, cout, cout_pad, y_extra, gr, relu = case
    cout_pad = -(-cout_pad // 32) * 32
    if not out_f32:
        cout, y_extra = cout // 8 * 8, -(-y_extra // 8) * 8
    mid = MATH[mode]
    x, w, s, b, gs = linear_inputs(rows + cin + 1, rows, cin, cout_pad, gr)
    xp = ops.pair16_pack(torch.from_numpy(x), mid).numpy()
    dx = dev(embed(xp, x_extra, np.nan), device)
    dw, ds, db, dgs = ops.pack_weight_split(dev(w, device), mid), dev(s, device), dev(b, device), dev(gs, device)
    out = Out(rows, cout + y_extra, device)
    out.run_twice(lambda: L.check(L.load().dz_linear_forward_split(L.ptr(dx), rows, cin, cin + x_extra, L.ptr(dw), cout, cout_pad, L.ptr(ds), L.ptr(db), L.ptr(dgs), gr,
                                                                   1 if relu else 0, out.ptr, cout + y_extra, mid, 1 if out_f32 else 0, 0, L.stream()),
                                  'dz_linear_forward_split'))
    out.check(cout)
    want, den = R.linear(R.split_value(x, mode), R.split_value(w, mode)[:, :cout], s[:cout], b[:cout], relu, None if gs is None else gs[:, :cout], max(gr, 1),
                         with_den=True)
    allow = BOUND[mode] * den
    got = out.f32(cout).contiguous().cpu()
    if not out_f32:
        got = ops.pair16_unpack(got, mid)
        allow = allow + SPLIT_U2[mode] * np.abs(want) + SPLIT_FLOOR[mode]
    assert_within(got.numpy(), want, allow, 'dz_linear_forward_split %s %s %s' % (mode, 'fp32' if out_f32 else 'pair16', case_id(case)))


@pytest.mark.gpu
@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('groups, gr, relu, addend', [(2, 128, True, False), (3, 384, False, True), (1, 384, True, True), (5, 128, False, False)])
def test_linear_fused_group_max(device, mode, groups, gr, relu, addend):
    """The group max in the epilogue of dz_linear_forward_split (integer atomics on the fp32 bits) equals dz_group_max over the layer's
    own fp32 rows BIT FOR BIT and the float64 maximum within BOUND: cout 40 < cout_pad 64, four sentinel columns beside the result,
    ReLU off with every maximum negative, and channels whose rows are all -0.0 (channel 0: the maximum is -0.0), -0.0 among negative
    values (channel 1) and +0.0 among negative values (channel 2).  Both kernels order the zeros: -0.0 < +0.0."""
    mid, cin, cout, cout_pad = MATH[mode], 64, 40, 64
    rows = groups * gr
    x, w, s, b, gs = linear_inputs(groups * gr + relu, rows, cin, cout_pad, gr if addend else 0)
    if not relu:
        b -= 12.0
        # zero rows give acc = +0: (+0) * scale + shift with shift = -0.0 is -0.0 for scale < 0 and +0.0 for scale > 0
        x[::3] = 0.0
        s[0], s[1], s[2] = -1.0, -1.0, 1.0
        b[0:3] = -0.0
        w[:, 0] = 0.0                                      # channel 0: every row -0.0
        w[:, 1] = np.abs(w[:, 1])
        w[:, 2] = -np.abs(w[:, 2])
        x[1::3] = np.abs(x[1::3])                          # channels 1, 2: the other rows negative
        x[2::3] = np.abs(x[2::3])
        if gs is not None:
            gs[:, 0:3] = 0.0
    dx = ops.pair16_from_f32(dev(x, device), cin, mid)
    dw, ds, db, dgs = ops.pack_weight_split(dev(w, device), mid), dev(s, device), dev(b, device), dev(gs, device)
    lib = L.load()
    full = Out(rows, cout, device)
    L.check(lib.dz_linear_forward_split(L.ptr(dx), rows, cin, cin, L.ptr(dw), cout, cout_pad, L.ptr(ds), L.ptr(db), L.ptr(dgs), gr, 1 if relu else 0, full.ptr, cout,
                                        mid, 1, 0, L.stream()), 'dz_linear_forward_split')
    out = Out(groups, cout + 4, device)
    out.run_twice(lambda: L.check(lib.dz_linear_forward_split(L.ptr(dx), rows, cin, cin, L.ptr(dw), cout, cout_pad, L.ptr(ds), L.ptr(db), L.ptr(dgs), gr,
                                                              1 if relu else 0, out.ptr, cout + 4, mid, 1, 1, L.stream()), 'dz_linear_forward_split(group_max)'))
    out.check(cout)
    gm = Out(groups, cout, device)
    gm.run_twice(lambda: L.check(lib.dz_group_max(full.ptr, groups, gr, cout, gm.ptr, L.stream()), 'dz_group_max'))
    gm.check()
    got = out.f32(cout).contiguous()
    assert torch.equal(got.view(torch.int32), gm.f32().view(torch.int32)), 'fused group max differs from dz_group_max'
    assert np.array_equal(gm.f32().cpu().numpy().view(np.int32), R.group_max(full.f32().cpu().numpy(), groups, gr).view(np.int32))
    want, den = R.linear(R.split_value(x, mode), R.split_value(w, mode)[:, :cout], s[:cout], b[:cout], relu, None if gs is None else gs[:, :cout], gr, with_den=True)
    assert_within(got.cpu().numpy(), want.reshape(groups, gr, cout).max(1), BOUND[mode] * den.reshape(groups, gr, cout).max(1), 'fused group max %s' % mode, BOUND[mode])
    g = got.cpu().numpy()
    if not relu:
        assert float(g.max()) <= 0.0
        zero = g[:, :3].view(np.int32)
        print('  zeros of the fused group max (channels 0 1 2): %s' % [hex(int(v) & 0xFFFFFFFF) for v in zero[0]])
        assert (zero[:, 0] == -2 ** 31).all() and (zero[:, 1] == -2 ** 31).all() and (zero[:, 2] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('rows, splits, cin, cout, cout_pad', [(1, 1, 32, 19, 32), (31, 2, 64, 100, 128), (129, 8, 256, 19, 32), (300, 8, 512, 64, 64),
                                                              (127, 2, 128, 16, 16), (128, 1, 64, 100, 128)])
def test_linear_forward_splitk(device, rows, splits, cin, cout, cout_pad):
    """dz_linear_forward_splitk with 1 / 2 / 8 splits at the smallest cin each takes (32 channels per split) and above: within
    BOUND['f32']; NaN in the unused input columns, sentinel columns beside the result, the workspace of exactly
    dz_linear_splitk_workspace_bytes inside a sentinel buffer."""
    lib = L.load()
    x, w, s, b, _ = linear_inputs(rows + splits, rows, cin, cout_pad, 0)
    dx, dw, ds, db = dev(embed(x, 4, np.nan), device), dev(w, device), dev(s, device), dev(b, device)
    nbytes = lib.dz_linear_splitk_workspace_bytes(rows, cout_pad, splits)
    ws, out = Out(1, nbytes // 4, device), Out(rows, cout + 3, device)
    for relu in (0, 1):
        out.raw.fill_(SENTINEL)
        out.run_twice(lambda: L.check(lib.dz_linear_forward_splitk(L.ptr(dx), rows, cin, cin + 4, L.ptr(dw), cout, cout_pad, L.ptr(ds), L.ptr(db), relu, out.ptr,
                                                                   cout + 3, splits, ws.ptr, nbytes, L.stream()), 'dz_linear_forward_splitk'))
        out.check(cout)
        ws.check()
        want, den = R.linear(x, w[:, :cout], s[:cout], b[:cout], bool(relu), with_den=True)
        assert_within(out.f32(cout).cpu().numpy(), want, BOUND['f32'] * den, 'dz_linear_forward_splitk %d rows, %d splits of %d' % (rows, splits, cin // splits),
                      BOUND['f32'])


# ------------------------------------------------------------------------------------------------------------------------
# GPU: the small kernels of csrc/refine.hip
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('family', ['inf', 'zeros', 'negative', 'nan'])
def test_group_max(device, family):
    """dz_group_max, exact, for len 1 .. 5, 37 x c 1 / 63 / 64 / 65 / 192 x groups 1 / 3: values with -inf (a whole column of them too), with
    -0.0 / +0.0 in both orders (bit patterns compared: -0.0 < +0.0), all negative.  NaN is outside the kernel's contract (its inputs
    are ReLU outputs); what it does is fixed here all the same: fmaxf drops a NaN - the maximum of the other values, -inf when the
    group holds nothing else - where torch.max would return NaN."""
    lib = L.load()
    rng = np.random.default_rng(len(family))
    for groups in (1, 3):
        for length in (1, 2, 3, 4, 5, 37):
            for c in (1, 63, 64, 65, 192):
                x = rng.standard_normal((groups * length, c)).astype(np.float32)
                if family == 'inf':
                    x[rng.random(x.shape) < 0.3] = -np.inf
                    x[:, c // 2] = -np.inf
                elif family == 'zeros':
                    x = np.where(rng.random(x.shape) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
                    x[rng.random(x.shape) < 0.2] = -1.0
                    x[:length, 0] = -0.0
                elif family == 'negative':
                    x = -np.abs(x) - 1.0
                clean = x.copy()
                if family == 'nan':
                    hit = rng.random(x.shape) < 0.3
                    hit[:length, 0] = True
                    x[hit] = np.nan
                    clean[hit] = -np.inf
                out = Out(groups, c, device)
                dx = dev(x, device)
                out.run_twice(lambda: L.check(lib.dz_group_max(L.ptr(dx), groups, length, c, out.ptr, L.stream()), 'dz_group_max'))
                out.check()
                want = R.group_max(clean, groups, length)
                assert np.array_equal(out.f32().cpu().numpy().view(np.int32), want.view(np.int32)), (family, groups, length, c)
    print('  dz_group_max %s: exact over 60 shapes' % family)


def run_layernorm(device, x, y, gamma, beta, eps, norm, post=None, skip=None, group_rows=1):
    lib = L.load()
    rows, c = x.shape
    out = Out(rows, c, device)
    dx, dy, dg, db, dp, dsk = (dev(a, device) for a in (x, y, gamma, beta, post, skip))

    def launch():
        if post is None:
            rc = lib.dz_add_layernorm(L.ptr(dx), L.ptr(dy), L.ptr(dg), L.ptr(db), rows, c, eps, 1 if norm else 0, out.ptr, L.stream())
        else:
            rc = lib.dz_add_layernorm_combine(L.ptr(dx), L.ptr(dy), L.ptr(dg), L.ptr(db), rows, c, eps, L.ptr(dp), L.ptr(dsk), group_rows, out.ptr, L.stream())
        L.check(rc, 'dz_add_layernorm')
    out.run_twice(launch)
    out.check()
    return out.f32().cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('c', [64, 128, 192, 256, 512])
def test_add_layernorm(device, c):
    """dz_add_layernorm for every channel count it has, rows 1 / 3 / 4 / 5 / 77 (four rows per workgroup), y null and given, eps 1e-5 and
    1e-8, on the row families of layernorm_rows() within layernorm_allowance(); norm off: x + y exactly."""
    x, y, gamma, beta = layernorm_rows(c, 77, c)
    worst = 0.0
    for rows in (1, 3, 4, 5, 77):
        for yy in (None, y[:rows]):
            for eps in (1e-5, 1e-8):
                got = run_layernorm(device, x[:rows], yy, gamma, beta, eps, True)
                want, allow = R.add_layernorm(x[:rows], yy, gamma, beta, eps), layernorm_allowance(x[:rows], yy, gamma, beta, eps)
                w = worst_ratio(got, want, allow)
                worst = max(worst, w)
                assert w <= 1.0, (c, rows, yy is None, eps, w)
            got = run_layernorm(device, x[:rows], yy, None, None, 1e-5, False)
            assert np.array_equal(got, x[:rows] if yy is None else x[:rows] + yy), (c, rows)
    print('  dz_add_layernorm c %d: worst |got - want| / allowance %.3f (LN_K = %g)' % (c, worst, LN_K))


@pytest.mark.gpu
@pytest.mark.parametrize('group_rows', [1, 5, 216])
def test_add_layernorm_combine(device, group_rows):
    """dz_add_layernorm_combine (c = 192): skip flags all 0, all 1, alternating, none; a skipped row is exactly 2 post, the others
    post + LayerNorm(x + y) within the LayerNorm allowance (+ one rounding of the sum)."""
    rows = 2 * group_rows + max(group_rows // 2, 1)                  # the last group ragged
    x, y, gamma, beta = layernorm_rows(192, rows, group_rows)
    post = np.random.default_rng(group_rows).standard_normal((rows, 192)).astype(np.float32)
    for flags in ([0, 0, 0], [1, 1, 1], [0, 1, 0], [1, 0, 1], None):
        skip = None if flags is None else np.array(flags, np.uint8)
        got = run_layernorm(device, x, y, gamma, beta, 1e-5, True, post=post, skip=skip, group_rows=group_rows)
        want = R.add_layernorm_combine(x, y, gamma, beta, 1e-5, post, skip, group_rows)
        allow = layernorm_allowance(x, y, gamma, beta, 1e-5) + U32 * np.abs(want)
        srow = np.zeros(rows, bool) if skip is None else skip[np.arange(rows) // group_rows] != 0
        assert np.array_equal(got[srow], 2 * post[srow]), (group_rows, flags)
        assert_within(got[~srow], want[~srow], allow[~srow], 'dz_add_layernorm_combine group_rows %d flags %s' % (group_rows, flags))


@pytest.mark.gpu
@pytest.mark.parametrize('rows', [1, 255, 256, 257])
def test_rows_all_zero(device, rows):
    """dz_rows_all_zero for 1 - 4 tensors of widths 4 / 16 / 64: all zero; a single non-zero int in the first word, the last word, in each
    tensor in turn; the value 0x80000000 (a sign bit alone); the flag bytes behind `rows` untouched."""
    lib = L.load()
    rng = np.random.default_rng(rows)
    for widths in ([4], [16], [64], [4, 64], [64, 16, 4], [16, 4, 64, 4]):
        ts = [np.zeros((rows, w), np.int32) for w in widths]
        for r in range(rows):
            kind = r % 5
            k = r % len(ts)
            if kind == 1:
                ts[k][r, 0] = int(rng.integers(1, 1000))
            elif kind == 2:
                ts[k][r, -1] = -int(rng.integers(1, 1000))
            elif kind == 3:
                ts[k][r, int(rng.integers(0, widths[k]))] = -2 ** 31
            elif kind == 4:
                ts[k][r, int(rng.integers(0, widths[k]))] = 1 << int(rng.integers(0, 31))
        dts = [dev(t, device) for t in ts]
        out = torch.full((rows + 64,), 0xAB, dtype=torch.uint8, device=device)
        ptrs = (ctypes.c_void_p * len(dts))(*[t.data_ptr() for t in dts])
        wsz = (ctypes.c_int * len(dts))(*widths)
        for _ in range(2):
            L.check(lib.dz_rows_all_zero(ptrs, wsz, len(dts), rows, out.data_ptr(), L.stream()), 'dz_rows_all_zero')
            got = out.cpu().numpy()
            assert np.array_equal(got[:rows].astype(bool), R.rows_all_zero(ts)) and set(got[:rows].tolist()) <= {0, 1} and (got[rows:] == 0xAB).all(), widths
            out[:rows] = 0xAB


# ------------------------------------------------------------------------------------------------------------------------
# GPU: refusals (arguments the host code rejects before any launch; each line cites its DZ_CHECK_ARG)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_write_nothing(device):
    lib = L.load()
    st = L.stream()
    z = torch.zeros((1024, 512), device=device)
    p = z.data_ptr()
    o1, o2, o3 = Out(64, 512, device), Out(64, 512, device), Out(64, 512, device)
    outs = [o1, o2, o3]
    pn = lambda c3, gr, math, xc=0: lib.dz_pointnet3_forward(p, 96, p, p, p, p, p, p, p, p, p, c3, gr, o2.ptr, o1.ptr, xc, math, st)        # noqa: E731
    # pointnet.hip: "c3 in {128, 256, 512}, group_rows a multiple of 32"; "math %d is not a split mode"; "fp32 input rows of 16 or 32 columns"
    assert 'group_rows' in refused(pn(256, 48, 1), outs, 'pointnet group_rows 48')
    assert 'c3' in refused(pn(64, 32, 1), outs, 'pointnet c3 64')
    assert 'split mode' in refused(pn(256, 32, 0), outs, 'pointnet math 0')
    assert '16 or 32' in refused(pn(256, 32, 1, 8), outs, 'pointnet x_cols 8')
    assert 'multiple of group_rows' in refused(pn(256, 64, 2), outs, 'pointnet 96 rows in groups of 64')
    # mlp_chain.hip: "group_rows a multiple of 32 (got %d), ldg >= 512"; "not a split mode"
    ch = lambda gr, ldg, math: lib.dz_mlp_chain_forward(p, 96, p, p, p, p, ldg, gr, p, p, p, p, p, p, p, o1.ptr, o2.ptr, o3.ptr, math, st)        # noqa: E731
    assert 'group_rows' in refused(ch(48, 512, 1), outs, 'chain group_rows 48')
    assert 'ldg' in refused(ch(32, 256, 1), outs, 'chain ldg 256')
    assert 'split mode' in refused(ch(32, 512, 0), outs, 'chain math 0')
    # refine.hip: "c=%d not in {64,128,192,256,512}"; combine: "c = 192, group_rows >= 1"; "dz_group_max: bad sizes"; "1..4 tensors"; widths
    assert 'c=96' in refused(lib.dz_add_layernorm(p, p, p, p, 8, 96, 1e-5, 1, o1.ptr, st), outs, 'LayerNorm c 96')
    assert 'c = 192' in refused(lib.dz_add_layernorm_combine(p, p, p, p, 8, 256, 1e-5, p, p, 1, o1.ptr, st), outs, 'combine c 256')
    assert 'group_rows' in refused(lib.dz_add_layernorm_combine(p, p, p, p, 8, 192, 1e-5, p, p, 0, o1.ptr, st), outs, 'combine group_rows 0')
    assert 'dz_group_max' in refused(lib.dz_group_max(p, 2, 0, 64, o1.ptr, st), outs, 'group max of 0 rows')
    ptrs, w5, w6 = (ctypes.c_void_p * 5)(*([p] * 5)), (ctypes.c_int * 5)(*([4] * 5)), (ctypes.c_int * 1)(6)
    assert '1..4' in refused(lib.dz_rows_all_zero(ptrs, w5, 5, 8, o1.ptr, st), outs, 'five tensors')
    assert 'multiples of 4' in refused(lib.dz_rows_all_zero(ptrs, w6, 1, 8, o1.ptr, st), outs, 'width 6')
    # xattn_fold.hip: "needs E = 256 and heads * queries <= 32"; "workspace of %zu bytes, need %zu"
    nb = lib.dz_xattn_folded_workspace_bytes(1, 64)
    fold = lambda lq, e, heads, nbytes: lib.dz_xattn_folded(p, p, None, p, p, p, 1, lq, 64, e, heads, 1.0, o2.ptr, nbytes, o1.ptr, st)        # noqa: E731
    assert 'heads * queries' in refused(fold(5, 256, 8, nb), outs, 'folded 40 rows')
    assert 'E = 256' in refused(fold(3, 128, 4, nb), outs, 'folded E 128')
    assert 'workspace' in refused(fold(3, 256, 8, nb - 1), outs, 'folded workspace one byte short')
    # mha.hip / mha_h.hip: "bad sizes" (lk = 0), "not a split mode"; pdv.hip: "L <= 256, E <= 256, E %% 4 == 0"
    assert 'bad sizes' in refused(lib.dz_mha_core(p, p, p, None, 1, 4, 0, 1, 1.0, o1.ptr, st), outs, 'mha lk 0')
    assert 'split mode' in refused(lib.dz_mha_core_split(p, p, p, None, 1, 4, 16, 1, 1.0, o1.ptr, 0, st), outs, 'split mha math 0')
    assert 'L <= 256' in refused(lib.dz_attention_single_head(p, p, p, None, 1, 257, 64, 1.0, o1.ptr, st), outs, 'single head l 257')
    assert 'L <= 256' in refused(lib.dz_attention_single_head(p, p, p, None, 1, 64, 258, 1.0, o1.ptr, st), outs, 'single head E 258')
    # conv2d_h.hip: "bad sizes (cin and cout_pad in multiples of 32)"; "group_max needs fp32 output, group_rows %% 128 == 0"
    ls = lambda cin, cout_pad, gr, f32, gmax: lib.dz_linear_forward_split(p, 256, cin, cin, p, 32, cout_pad, p, p, None, gr, 1, o1.ptr, 32, 1, f32, gmax, st)        # noqa: E731
    assert 'multiples of 32' in refused(ls(48, 32, 0, 1, 0), outs, 'split linear cin 48')
    assert 'multiples of 32' in refused(ls(64, 48, 0, 1, 0), outs, 'split linear cout_pad 48')
    assert 'group_max' in refused(ls(64, 32, 100, 1, 1), outs, 'fused max over groups of 100')
    assert 'group_max' in refused(ls(64, 32, 128, 0, 1), outs, 'fused max into a pair16 result')
    # conv2d.hip: "dz_linear_forward: bad sizes"; split-k: "1..8 splits of a multiple of 32 channels each"; "workspace too small"
    assert 'bad sizes' in refused(lib.dz_linear_forward(p, 8, 64, 32, p, 32, 32, p, p, None, 0, 1, o1.ptr, 32, st), outs, 'x_stride < cin')
    sk = lambda cin, splits, nbytes: lib.dz_linear_forward_splitk(p, 8, cin, cin, p, 32, 32, p, p, 1, o1.ptr, 32, splits, o2.ptr, nbytes, st)        # noqa: E731
    assert 'splits' in refused(sk(96, 2, 1 << 20), outs, 'split-k 96 channels in 2')
    assert 'splits' in refused(sk(512, 9, 1 << 20), outs, 'split-k 9 splits')
    assert 'workspace' in refused(sk(256, 8, lib.dz_linear_splitk_workspace_bytes(8, 32, 8) - 1), outs, 'split-k workspace one byte short')
