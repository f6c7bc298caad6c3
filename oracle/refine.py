"""ORACLE (test infrastructure only): float64 references of the object refiner's operations (GRM / PRM / CRM), numpy only.

One function per kernel family of the third stage (csrc/mha.hip, mha_h.hip, xattn_fold.hip, pointnet.hip, mlp_chain.hip, refine.hip and
the linear entry points of conv2d.hip / conv2d_h.hip), written the plain way - every intermediate tensor is materialised, nothing is
tiled, streamed, split or fused - so that tests/test_gpu_refine_kernels.py can hold the kernels' register-level dataflow against them.

  linear / pointnet3 / mlp_chain     point-wise layers y = act((x @ w + group addend) * scale + shift); with `with_den` they also return
                                     the magnitude of what was summed (den) and, through a stack of layers, an error allowance
  attention / folded_attention       multi_head_attention.py:199-288 of the reference: scale q, scores, masked scores filled with -inf,
                                     softmax, weighted sum; both also return sum_j p_j |v_j|, the natural scale of every output element
  group_max, add_layernorm, add_layernorm_combine, rows_all_zero
  split_pair / split_product         the (hi, lo) 16-bit pair arithmetic of csrc/hgemm.h
"""
import numpy as np

F64 = np.float64
MODES = ('f16x2', 'bf16x2')


# ------------------------------------------------------------------------------------------------------------------------
# split precision
# ------------------------------------------------------------------------------------------------------------------------
def _round_bf16(x32):
    """float32 -> nearest bfloat16 (ties to even), returned as float32.  NaN stays NaN."""
    x32 = np.ascontiguousarray(x32, np.float32)
    u = x32.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x32), x32, r).astype(np.float32)


def _round_f16(x32):
    """float32 -> nearest float16 (ties to even, gradual underflow) after saturating at +-65504, returned as float32."""
    with np.errstate(over='ignore', invalid='ignore'):
        return np.clip(np.asarray(x32, np.float32), -65504.0, 65504.0).astype(np.float16).astype(np.float32)


def split_pair(x, mode):
    """(hi, lo) of float32 values as float64 arrays, the rounding of split2<MathF16> / split2<MathBF16> (csrc/hgemm.h):

      f16x2   hi = RNE_fp16(clamp(x, +-65504));  lo = RNE_fp16(clamp(x - hi, +-65504))      (x - hi in float32: exact, Sterbenz)
      bf16x2  hi = RNE_bf16(x);                  lo = RNE_bf16(x - hi)

    Both conversions round to nearest even (v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32); nothing is truncated, fp16 saturates instead of
    overflowing to inf and underflows gradually.  With u the unit roundoff of the half format (2^-11 for fp16: 11 significant bits;
    2^-8 for bf16) |x - hi| <= u |x| and |x - hi - lo| <= u |x - hi| <= u^2 |x|: hi + lo carries 22 bits (f16x2) / 16 bits (bf16x2)
    of a float32's 24.  For fp16 that holds only while lo is a NORMAL fp16, |x - hi| >= 2^-14, which is certain for no x but can
    fail only below |x| = 2^-3: from there down lo is a subnormal with quantum 2^-24 and the error is bounded by 2^-25 ABSOLUTE
    instead (19 bits at |x| = 2^-6, 11 bits - hi alone - at 2^-14, nothing below 2^-25).  Above, values beyond 65504 * (1 + 2^-11)
    are cut off.  bf16 has float32's exponent range: no floor, no ceiling."""
    x32 = np.ascontiguousarray(x, np.float32)
    rnd = {'f16x2': _round_f16, 'bf16x2': _round_bf16}[mode]
    hi = rnd(x32)
    with np.errstate(invalid='ignore', over='ignore'):
        lo = rnd((x32 - hi).astype(np.float32))
    return hi.astype(F64), lo.astype(F64)


def split_value(x, mode):
    """hi + lo in float64: the value a pair16 tensor holds for x."""
    hi, lo = split_pair(x, mode)
    return hi + lo


def split_product(a, b, mode):
    """hi.hi + hi.lo + lo.hi element by element in float64 (lo.lo is dropped): what the split kernels' three 16-bit MFMAs per product
    sum before their fp32 accumulation."""
    ah, al = split_pair(a, mode)
    bh, bl = split_pair(b, mode)
    return ah * bh + ah * bl + al * bh


def split_matmul(a, b, mode):
    """a (.., m, k) @ b (.., k, n) with every product taken as split_product, summed in float64."""
    ah, al = split_pair(a, mode)
    bh, bl = split_pair(b, mode)
    return ah @ bh + ah @ bl + al @ bh


# ------------------------------------------------------------------------------------------------------------------------
# point-wise layers
# ------------------------------------------------------------------------------------------------------------------------
def _group_of(rows, group_rows):
    return np.arange(rows) // int(group_rows)


def linear(x, w, scale, shift, relu, group_shift=None, group_rows=1, with_den=False):
    """y = act((x @ w + group_shift[row // group_rows]) * scale + shift): x (rows, cin), w (cin, cout), scale / shift (cout) or None,
    group_shift (ceil(rows / group_rows), cout) or None (the last group may be ragged).  with_den: also |scale| (|x| @ |w| + |addend|) +
    |shift|, the magnitude of what was summed into each element."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    acc = x @ w
    den = np.abs(x) @ np.abs(w) if with_den else None
    if group_shift is not None:
        gs = np.asarray(group_shift, F64)[_group_of(x.shape[0], group_rows)]
        acc = acc + gs
        if with_den:
            den = den + np.abs(gs)
    if scale is not None:
        acc = acc * np.asarray(scale, F64)
        if with_den:
            den = den * np.abs(np.asarray(scale, F64))
    if shift is not None:
        acc = acc + np.asarray(shift, F64)
        if with_den:
            den = den + np.abs(np.asarray(shift, F64))
    y = np.maximum(acc, 0.0) if relu else acc
    return (y, den) if with_den else y


def layer_stack(x, layers, bound=None, u2=0.0, floor=0.0, first_group_shift=None, group_rows=1):
    """Rows through ReLU layers (w (cin, cout), scale, shift).  Returns the activations of every layer and, with bound given, an
    allowance per element for a kernel that errs by `bound` x (what was summed) in every layer and re-splits every hidden activation
    into a 16-bit pair (u2 relative, `floor` absolute): err_l = |scale| (err_{l-1} @ |w|) + bound den_l, then + u2 |h_l| + floor for a
    layer whose output is split again.  ReLU is 1-Lipschitz, so the error passes through it unamplified."""
    h, err, acts, errs = np.asarray(x, F64), None, [], []
    for li, (w, s, b) in enumerate(layers):
        gs = first_group_shift if li == 0 else None
        y, den = linear(h, w, s, b, True, gs, group_rows, with_den=True)
        if bound is not None:
            e = bound * den
            if err is not None:
                e = e + (err @ np.abs(np.asarray(w, F64))) * (1.0 if s is None else np.abs(np.asarray(s, F64)))
            errs.append(e)
            err = e + u2 * y + floor                   # what the NEXT layer sees of this one
        acts.append(y)
        h = y
    return acts, errs


def pointnet3(x, layers, group_rows, bound=None, u2=0.0, floor=0.0):
    """The fused encoder: three ReLU layers on every row, then the max over each group of `group_rows` consecutive rows ->
    (pooled (groups, c3), tap (rows, 128) = the second layer's output).  With `bound` also their allowances (see layer_stack; the max over
    rows is 1-Lipschitz in the max norm: the pooled allowance is the largest allowance among the group's rows)."""
    acts, errs = layer_stack(x, layers, bound, u2, floor)
    rows, c3 = acts[2].shape
    pooled = acts[2].reshape(rows // group_rows, group_rows, c3).max(1)
    if bound is None:
        return pooled, acts[1]
    return pooled, acts[1], errs[2].reshape(rows // group_rows, group_rows, c3).max(1), errs[1] + u2 * acts[1] + floor


def mlp_chain(x, la, lb, group_shift, group_rows, kv=None, bound=None, u2=0.0, floor=0.0):
    """The memory chain: h = ReLU(((x @ wa) + group_shift[group]) sa + ba), mem = ReLU((h @ wb) sb + bb) and, with kv = (wk, bk, wv, bv),
    k = mem @ wk + bk, v = mem @ wv + bv (weights (cin, cout)).  -> mem or (mem, k, v); with `bound` each followed by its allowance
    (k and v are computed from the memory RE-SPLIT into 16-bit pairs)."""
    acts, errs = layer_stack(x, [la, lb], bound, u2, floor, first_group_shift=group_shift, group_rows=group_rows)
    mem = acts[1]
    if kv is None:
        return mem if bound is None else (mem, errs[1])
    wk, bk, wv, bv = kv
    outs = []
    for w, b in ((wk, bk), (wv, bv)):
        y, den = linear(mem, w, None, b, False, with_den=True)
        outs.append(y)
        if bound is not None:
            outs.append(bound * den + (errs[1] + u2 * mem + floor) @ np.abs(np.asarray(w, F64)))
    return (mem, outs[0], outs[1]) if bound is None else (mem, errs[1], outs[0], outs[1], outs[2], outs[3])


# ------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------
def _mm(a, b):
    """a @ b over the last two axes.  float32 operands go through einsum's own loops (no BLAS: the float32 baselines of the tests
    must not depend on the BLAS build or its thread count), float64 through matmul."""
    if a.dtype == np.float32:
        return np.einsum('...ij,...jk->...ik', a, b)
    return a @ b


def _heads(x, heads):
    b, l, e = x.shape
    return x.reshape(b, l, heads, e // heads).transpose(0, 2, 1, 3)


def _softmax_weighted(s, v, mask):
    """s (b, h, lq, lk) scores, v (b, h, lk, hd), mask (b, lk) non-zero = padded key -> (out, sum_j p_j |v_j|), both (b, h, lq, hd).
    A masked score is REPLACED by -inf (whatever it held, NaN included); a row without a live key gives NaN, as torch.softmax does."""
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        if mask is not None:
            s = np.where(np.asarray(mask)[:, None, None, :] != 0, -np.inf, s)
        m = s.max(-1, keepdims=True)
        p = np.exp(s - m)                                # a fully masked row: -inf - -inf = NaN
        p = p / p.sum(-1, keepdims=True)
        p = np.where(np.isnan(p), 0.0, p)                # (rows without a live key: set to NaN below)
        out = _mm(p, v)
        nat = _mm(p, np.abs(v))
        dead = ~np.isfinite(m[..., 0])
        out[dead] = np.nan
        nat[dead] = np.nan
    return out, nat


def attention(q, k, v, mask, heads, scale, dtype=F64):
    """q (b, lq, e), k / v (b, lk, e), mask (b, lk) or None -> (out (b, lq, e), sum_j p_j |v_j| (b, lq, e)).  `dtype` float32 evaluates
    the same formula in float32 (the baseline the kernels' bound is derived from)."""
    q, k, v = (np.asarray(a, dtype) for a in (q, k, v))
    b, lq, e = q.shape
    with np.errstate(invalid='ignore', over='ignore'):
        qh = _heads(q * dtype(scale), heads)
        s = _mm(qh, _heads(k, heads).transpose(0, 1, 3, 2))
    out, nat = _softmax_weighted(s, _heads(v, heads), mask)
    back = lambda a: a.transpose(0, 2, 1, 3).reshape(b, lq, e)
    return back(out), back(nat)


def folded_attention(x_q, mem, wq, bq, wk, bk, wv, bv, heads, mask, dtype=F64):
    """The decoder's cross-attention as the reference computes it: q = x_q wq^T + bq, k = mem wk^T + bk, v = mem wv^T + bv (weights
    (out, in)), scale = head_dim^-1/2, then attention().  -> (out, natural scale, q) with q the projected queries (what dz_xattn_folded
    is handed)."""
    x_q, mem, wq, bq, wk, bk, wv, bv = (np.asarray(a, dtype) for a in (x_q, mem, wq, bq, wk, bk, wv, bv))
    q = _mm(x_q, wq.T) + bq
    k = _mm(mem, wk.T) + bk
    v = _mm(mem, wv.T) + bv
    out, nat = attention(q, k, v, mask, heads, (x_q.shape[-1] // heads) ** -0.5, dtype=dtype)
    return out, nat, q


def attention_split(q, k, v, mask, heads, scale, mode):
    """Host emulation of the split cores' operand roundings (csrc/mha_h.hip), everything else in float64: q scaled into log2 units in
    float32 and split, k split, scores = split products; p = 2^(s - max) rounded to float32 and split, v split, out = sum of split
    products / sum of the UNSPLIT p (the kernel's row sum runs on the fp32 probabilities)."""
    f = np.float32
    b, lq, e = q.shape
    sc2 = f(f(scale) * f(1.44269504088896340736))
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        qh = _heads((np.asarray(q, f) * sc2).astype(f), heads)
        kh, vh = _heads(np.asarray(k, f), heads), _heads(np.asarray(v, f), heads)
        s = split_matmul(qh, kh.transpose(0, 1, 3, 2), mode)
        if mask is not None:
            s = np.where(np.asarray(mask)[:, None, None, :] != 0, -np.inf, s)
        m = s.max(-1, keepdims=True)
        p = np.exp2(s - m).astype(f)
        out = split_matmul(p, vh, mode) / p.astype(F64).sum(-1, keepdims=True)
    return out.transpose(0, 2, 1, 3).reshape(b, lq, e)


# ------------------------------------------------------------------------------------------------------------------------
# small operations
# ------------------------------------------------------------------------------------------------------------------------
def group_max(x, groups, length):
    """x (groups * length, c) -> (groups, c) float32: the maximum of every group's rows in the total order of the float bit patterns
    (-0.0 < +0.0: a group of [-0.0, 0.0] gives +0.0 in either order, one of only -0.0 gives -0.0), -inf allowed.  NaN is outside the
    contract of this function (the refiner pools ReLU outputs)."""
    x = np.ascontiguousarray(x, np.float32)
    c = x.shape[1]
    bits = x.view(np.int32).astype(np.int64)
    key = np.where(bits < 0, -(bits & 0x7FFFFFFF) - 1, bits)           # monotone in the value, -0.0 -> -1, +0.0 -> 0
    idx = key.reshape(groups, length, c).argmax(1)
    return np.take_along_axis(x.reshape(groups, length, c), idx[:, None, :], 1)[:, 0, :]


def add_layernorm(x, y, gamma, beta, eps, norm=True):
    """LayerNorm(x + y) over the last dimension in the two-pass form (mean, then the mean of the squared deviations, biased), y may be
    None; norm=False: x + y."""
    v = np.asarray(x, F64) + (0.0 if y is None else np.asarray(y, F64))
    if not norm:
        return v
    mean = v.mean(-1, keepdims=True)
    d = v - mean
    var = (d * d).mean(-1, keepdims=True)
    return d / np.sqrt(var + F64(eps)) * np.asarray(gamma, F64) + np.asarray(beta, F64)


def add_layernorm_combine(x, y, gamma, beta, eps, post, group_skip, group_rows):
    """post + (group_skip[row // group_rows] ? post : LayerNorm(x + y)); group_skip None = no group is skipped."""
    ln = add_layernorm(x, y, gamma, beta, eps)
    post = np.asarray(post, F64)
    if group_skip is None:
        return post + ln
    skip = np.asarray(group_skip)[_group_of(ln.shape[0], group_rows)] != 0
    return post + np.where(skip[:, None], post, ln)


def rows_all_zero(tensors):
    """(rows,) bool: every int of the row is zero in all of the (rows, w_k) int32 tensors."""
    out = np.ones(np.asarray(tensors[0]).shape[0], bool)
    for t in tensors:
        out &= ~(np.asarray(t) != 0).any(1)
    return out
