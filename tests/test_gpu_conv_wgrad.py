"""GPU: the kernels of csrc/head_backward.hip one by one against float64 computed in the test (tests/head_backward_ref.py):
the 3 x 3 weight gradient on the fp32 MFMA, the ReLU-mask pass, the data gradient through the forward kernel, and both halves of the
grouped output layer's backward.  Integer inputs make every summation order exact; random inputs are held to the a-priori bound of
a float32 sum of n rounded products."""
import ctypes

import numpy as np
import pytest
import torch

from tests import head_backward_ref as R

G_OOFF = [0, 2, 3, 6, 8, 9]                      # the head map's column blocks: center, center_z, dim, rot, iou, hm


def g_cout_of(n):
    return [2, 1, 3, 2, 1, n]


def chunk_maps():
    from detzero_amd import ops
    tw, rows, pix = ops.WGRAD_TILE_W, ops.WGRAD_CHUNK_ROWS, ops.WGRAD_CHUNK_PIXELS
    # pixel counts one below, equal to and one above a multiple of the kernel's pixel chunk (one row: the band edge), the same for
    # the rows of a chunk, and a count below one chunk
    return [(1, 1, 2 * pix - 1), (1, 1, 2 * pix), (1, 1, 2 * pix + 1), (1, rows - 1, tw), (1, rows, tw), (2, rows + 1, tw + 1), (1, 3, 5)]


MAPS = [(3, 19, 23), (1, 1, 1), (1, 2, 37)]
CHANNELS = [(16, 16), (48, 64), (64, 384), (512, 64)]


def int_images(rng, b, h, w, cin, cout, border=0):
    """x in [-3, 3] inside a border of `border`, g in [-2, 2] dense."""
    x = R.bordered(rng.integers(-3, 4, (b, h, w, cin)).astype(np.float32), border)
    g = rng.integers(-2, 3, (b, h, w, cout)).astype(np.float32)
    return x, g


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def wgrad_cases():
    cases = [(m, c) for c in CHANNELS for m in MAPS[:1]] + [(m, (48, 64)) for m in MAPS[1:] + chunk_maps()] + [((1, 2, 37), (16, 16))]
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize('shape,channels', wgrad_cases(), ids=lambda v: 'x'.join(str(i) for i in v))
def test_wgrad_exact(device, shape, channels):
    from detzero_amd import ops
    (b, h, w), (cin, cout) = shape, channels
    rng = np.random.default_rng(h * 131 + w * 7 + cin)
    poisoned = (h, w) == (19, 23) and cin == 48                 # the border of x_img non-zero: the reference reads the same image
    x, g = int_images(rng, b, h, w, cin, cout, border=2.0 if poisoned else 0.0)
    ref = R.wgrad_ref(x, g)
    assert np.abs(ref).max() < 2 ** 24
    # g as relu_grad leaves it (bordered, border untouched = zero) and dense
    y_img = dev(R.bordered(np.ones_like(g)), device)
    g_img, _ = ops.relu_grad(dev(g, device), y_img)
    got = ops.conv3x3_wgrad(dev(x, device), g_img, cin, cout)
    assert got.shape == (9, cin, cout) and got.dtype == torch.float32
    np.testing.assert_array_equal(got.cpu().numpy().astype(np.float64), ref)
    got_dense = ops.conv3x3_wgrad(dev(x, device), dev(g, device), cin, cout)
    assert torch.equal(got_dense, got)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 2, 3])
@pytest.mark.parametrize('shape', [(3, 19, 23), (1, 1, 1), (1, 17, 33)], ids=lambda v: 'x'.join(str(i) for i in v))
def test_wgrad_grouped_exact(device, shape, n):
    from detzero_amd import ops
    b, h, w = shape
    rng = np.random.default_rng(n + h)
    x, g = int_images(rng, b, h, w, 6 * 64, 12)
    g[..., 9 + n:] = np.nan                                     # columns no group reads
    ref = R.wgrad_ref(x, g, 6, g_cout_of(n), G_OOFF)
    got = ops.conv3x3_wgrad(dev(x, device), dev(g.reshape(b, h * w, 12), device), 64, 12, groups=6, g_cout=g_cout_of(n), g_ooff=G_OOFF)
    assert got.shape == (6, 9, 64, 16)
    np.testing.assert_array_equal(got.cpu().numpy().astype(np.float64), ref)


@pytest.mark.gpu
@pytest.mark.parametrize('shape,c', [((3, 19, 23), 64), ((3, 19, 23), 384), ((1, 1, 1), 16), ((1, 2, 37), 512), ((2, 7, 5), 4)],
                         ids=lambda v: 'x'.join(str(i) for i in v) if isinstance(v, tuple) else str(v))
def test_relu_grad_exact(device, shape, c):
    from detzero_amd import ops
    b, h, w = shape
    rng = np.random.default_rng(c + h)
    g = rng.integers(-2, 3, (b, h, w, c)).astype(np.float32)
    y = rng.integers(-2, 3, (b, h, w, c)).astype(np.float32)
    y[g == 0] = np.where(rng.random((g == 0).sum()) < 0.5, np.nan, y[g == 0])      # NaN in y where g_y is zero must not leak
    g_nan = g.copy()
    g_nan[(y <= 0) & (rng.random(y.shape) < 0.3)] = np.nan                         # nor a masked-out NaN of g_y: a select
    y_img = dev(R.bordered(y, 1.0), device)                                        # (the activation's border is not read)
    ref_g, ref_s = R.relu_grad_ref(g, y_img.cpu().numpy())
    out = torch.full(y_img.shape, 7.0, dtype=torch.float32, device=device)
    g_img, sums = ops.relu_grad(dev(g_nan, device), y_img, out=out)
    assert g_img is out and sums.dtype == torch.float64
    got = g_img.cpu().numpy()
    np.testing.assert_array_equal(got[:, 1:-1, 1:-1, :].astype(np.float64), ref_g)
    border = got.copy()
    border[:, 1:-1, 1:-1, :] = 7.0
    assert (border == 7.0).all()                                                   # the border is never written
    np.testing.assert_array_equal(sums.cpu().numpy(), ref_s)
    # from the interior of a bordered image, in place
    g_b = dev(R.bordered(g_nan, 5.0), device)
    g2, sums2 = ops.relu_grad(g_b, y_img, out=g_b)
    assert torch.equal(g2[:, 1:-1, 1:-1, :], g_img[:, 1:-1, 1:-1, :]) and torch.equal(sums2, sums) and float(g2[0, 0, 0, 0]) == 5.0
    fresh, _ = ops.relu_grad(dev(g_nan, device), y_img)
    assert float(fresh[:, 0].abs().max()) == 0.0 and torch.equal(fresh[:, 1:-1, 1:-1, :], g_img[:, 1:-1, 1:-1, :])


@pytest.mark.gpu
@pytest.mark.parametrize('shape,channels', [((3, 19, 23), (64, 384)), ((2, 19, 23), (32, 64)), ((1, 1, 1), (16, 16)), ((1, 2, 37), (48, 64))],
                         ids=lambda v: 'x'.join(str(i) for i in v))
def test_dgrad_exact(device, shape, channels):
    from detzero_amd import ops
    (b, h, w), (cin, cout) = shape, channels
    rng = np.random.default_rng(cin + w)
    g = rng.integers(-2, 3, (b, h, w, cout)).astype(np.float32)
    wt = rng.integers(-3, 4, (9, cin, cout)).astype(np.float32)
    scale = rng.integers(-2, 3, (cout,)).astype(np.float32)
    for sc in (None, scale):
        ref = R.dgrad_ref(g, wt, sc)
        assert np.abs(ref).max() < 2 ** 24
        got = ops.conv3x3_dgrad(dev(R.bordered(g), device), dev(wt, device), None if sc is None else dev(sc, device))
        assert got.shape == (b, h, w, cin)
        np.testing.assert_array_equal(got.cpu().numpy().astype(np.float64), ref)
    out = torch.full((b, h + 2, w + 2, cin), 3.0, dtype=torch.float32, device=device)
    assert ops.conv3x3_dgrad(dev(R.bordered(g), device), dev(wt, device), dev(scale, device), out=out) is out
    np.testing.assert_array_equal(out[:, 1:-1, 1:-1, :].cpu().numpy().astype(np.float64), ref)
    assert float(out[:, 0].min()) == 3.0 and float(out[:, :, -1].max()) == 3.0


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 2, 3])
@pytest.mark.parametrize('shape', [(3, 19, 23), (1, 1, 1), (1, 2, 37)], ids=lambda v: 'x'.join(str(i) for i in v))
def test_head_final_backward_exact(device, shape, n):
    from detzero_amd import ops
    b, h, w = shape
    rng = np.random.default_rng(10 * n + w)
    gh = rng.integers(-2, 3, (b, h * w, 12)).astype(np.float32)
    gh[..., 9 + n:] = np.nan                                    # NaN in the unread columns of grad_head
    w2 = rng.integers(-2, 3, (6, 9, 64, 16)).astype(np.float32)
    w2[..., 3:] = np.nan                                        # (nor are the weights' pad columns read)
    for q, nq in enumerate(g_cout_of(n)):
        w2[q, :, :, nq:] = np.nan
    hidden = R.bordered(rng.integers(-1, 3, (b, h, w, 384)).astype(np.float32))
    ref_g, ref_s, ref_w, ref_b = R.final_backward_ref(gh, np.nan_to_num(w2), hidden, g_cout_of(n), G_OOFF)
    out = torch.full(hidden.shape, 7.0, dtype=torch.float32, device=device)
    g_hidden, sums, d_w2, d_b = ops.head_final_backward(dev(gh, device), dev(w2, device), dev(hidden, device), g_cout_of(n), G_OOFF, out=out)
    got = g_hidden.cpu().numpy()
    np.testing.assert_array_equal(got[:, 1:-1, 1:-1, :].astype(np.float64), ref_g)
    got[:, 1:-1, 1:-1, :] = 7.0
    assert (got == 7.0).all()
    np.testing.assert_array_equal(sums.cpu().numpy(), ref_s)
    np.testing.assert_array_equal(d_w2.cpu().numpy().astype(np.float64), ref_w)
    np.testing.assert_array_equal(d_b.cpu().numpy(), ref_b)


@pytest.mark.gpu
@pytest.mark.parametrize('channels', [(48, 64), (64, 384), (512, 64)], ids=lambda v: 'x'.join(str(i) for i in v))
def test_wgrad_random_within_the_a_priori_bound(device, channels):
    """|got - ref64| <= gamma_n * sum |x * g| elementwise, gamma_n = n u / (1 - n u), u = 2^-24, n = B * H * W + 2: the a-priori bound of
    a float32 sum of n rounded products in any order (derived, not measured); the absolute-value sum is formed in float64."""
    from detzero_amd import ops
    cin, cout = channels
    b, h, w = 3, 19, 23
    rng = np.random.default_rng(cin)
    x = R.bordered(rng.standard_normal((b, h, w, cin)).astype(np.float32))
    g = rng.standard_normal((b, h, w, cout)).astype(np.float32)
    ref, mag = R.wgrad_ref(x, g), R.wgrad_ref(x, g, absolute=True)
    got = ops.conv3x3_wgrad(dev(x, device), dev(g, device), cin, cout).cpu().numpy().astype(np.float64)
    bound = R.gamma_n(b * h * w + 2) * mag
    ratio = np.abs(got - ref) / np.maximum(bound, 1e-300)
    print('wgrad %d -> %d: worst |err| / bound %.4f' % (cin, cout, ratio.max()))
    assert (np.abs(got - ref) <= bound).all()


@pytest.mark.gpu
def test_final_backward_and_relu_grad_random_within_the_bound(device):
    from detzero_amd import ops
    b, h, w, n = 2, 19, 23, 2
    rng = np.random.default_rng(8)
    gh = rng.standard_normal((b, h * w, 12)).astype(np.float32)
    gh[..., 9 + n:] = np.nan
    w2 = np.zeros((6, 9, 64, 16), np.float32)
    for q, nq in enumerate(g_cout_of(n)):
        w2[q, :, :, :nq] = rng.standard_normal((9, 64, nq))
    hidden = R.bordered(np.maximum(rng.standard_normal((b, h, w, 384)), 0).astype(np.float32))
    ref = R.final_backward_ref(gh, w2, hidden, g_cout_of(n), G_OOFF)
    mag = R.final_backward_ref(gh, w2, np.abs(hidden), g_cout_of(n), G_OOFF, absolute=True)
    g_hidden, sums, d_w2, d_b = ops.head_final_backward(dev(gh, device), dev(w2, device), dev(hidden, device), g_cout_of(n), G_OOFF)
    got_g = g_hidden[:, 1:-1, 1:-1, :].cpu().numpy().astype(np.float64)
    assert (np.abs(got_g - ref[0]) <= R.gamma_n(27 + 2) * mag[0]).all()                       # 27 products per value
    # the float64 sums of the float32 values the kernel wrote: exact up to float64 rounding of b * h * w terms
    np.testing.assert_allclose(sums.cpu().numpy(), got_g.sum(axis=(0, 1, 2)), rtol=0, atol=1e-12 * np.abs(got_g).sum(axis=(0, 1, 2)).max())
    assert (np.abs(d_w2.cpu().numpy() - ref[2]) <= R.gamma_n(b * h * w + 2) * mag[2]).all()
    np.testing.assert_allclose(d_b.cpu().numpy(), ref[3], rtol=0, atol=1e-12 * mag[3].max())


@pytest.mark.gpu
def test_two_calls_give_the_same_bytes_whatever_the_workspace_held(device):
    from detzero_amd import ops
    rng = np.random.default_rng(4)
    b, h, w = 2, 19, 23
    x = dev(R.bordered(rng.standard_normal((b, h, w, 64)).astype(np.float32)), device)
    g = dev(rng.standard_normal((b, h, w, 384)).astype(np.float32), device)
    first = ops.conv3x3_wgrad(x, g, 64, 384)
    assert torch.equal(ops.conv3x3_wgrad(x, g, 64, 384), first)
    # another shape's call in between
    ops.conv3x3_wgrad(dev(R.bordered(rng.standard_normal((1, 2, 37, 48)).astype(np.float32)), device),
                      dev(rng.standard_normal((1, 2, 37, 64)).astype(np.float32), device), 48, 64)
    assert torch.equal(ops.conv3x3_wgrad(x, g, 64, 384), first)
    # and the library called on a workspace of the caller's that holds NaN in every word
    lib = ops.L.load()
    ws = torch.full((int(lib.dz_conv3x3_wgrad_ws_bytes(b, h, w, 64, 384, 1)) // 4,), float('nan'), dtype=torch.float32, device=device)
    out = torch.empty_like(first)
    rc = lib.dz_conv3x3_wgrad(ops.L.ptr(x), ops.L.ptr(g), 0, b, h, w, 64, 384, 1, None, None, 0, ops.L.ptr(out), ops.L.ptr(ws), ws.numel() * 4,
                              ops.L.stream())
    assert rc == 0 and torch.equal(out, first)
    y_img = dev(R.bordered(rng.standard_normal((b, h, w, 384)).astype(np.float32)), device)
    a, sa = ops.relu_grad(g, y_img)
    b2, sb = ops.relu_grad(g, y_img)
    assert torch.equal(a, b2) and torch.equal(sa, sb)
    gh = dev(rng.standard_normal((b, h * w, 12)).astype(np.float32), device)
    w2 = dev(rng.standard_normal((6, 9, 64, 16)).astype(np.float32), device)
    r1 = ops.head_final_backward(gh, w2, y_img, g_cout_of(3), G_OOFF)
    r2 = ops.head_final_backward(gh, w2, y_img, g_cout_of(3), G_OOFF)
    assert all(torch.equal(p, q) for p, q in zip(r1, r2))


@pytest.mark.gpu
def test_refusals_launch_nothing(device):
    from detzero_amd import lib as L
    from detzero_amd import ops
    lib = L.load()
    b, h, w = 1, 4, 5
    ws = torch.zeros((1 << 20,), dtype=torch.uint8, device=device)
    i6 = (ctypes.c_int * 8)(2, 1, 3, 2, 1, 3, 1, 0)
    o6 = (ctypes.c_int * 8)(0, 2, 3, 6, 8, 9, 0, 0)

    def call(cin, cout, groups=1, n_g=0, x_null=False, out_null=False):
        x = torch.ones((b, h + 2, w + 2, max(groups * cin, 1)), dtype=torch.float32, device=device)
        g = torch.ones((b, h, w, max(cout, 1)), dtype=torch.float32, device=device)
        out = torch.full((6 * 9 * 512 * 16,), 7.0, dtype=torch.float32, device=device)
        rc = lib.dz_conv3x3_wgrad(None if x_null else L.ptr(x), L.ptr(g), 0, b, h, w, cin, cout, groups, i6, o6, n_g,
                                  None if out_null else L.ptr(out), L.ptr(ws), ws.numel(), L.stream())
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and float(ws.max()) == 0.0          # nothing was launched: the outputs are untouched
        return rc, lib.dz_last_error().decode()

    assert call(24, 16)[0] == L.ERR_UNSUPPORTED and call(16, 8)[0] == L.ERR_UNSUPPORTED
    rc, msg = call(64, 12, groups=6, n_g=7)
    assert rc == L.ERR_INVALID and '7' in msg
    assert call(16, 16, x_null=True)[0] == L.ERR_INVALID and call(16, 16, out_null=True)[0] == L.ERR_INVALID
    assert call(16, 0)[0] == L.ERR_INVALID and call(-16, 16)[0] == L.ERR_INVALID
    rc = lib.dz_conv3x3_wgrad(L.ptr(ws), L.ptr(ws), 0, b, h, w, 16, 16, 1, None, None, 0, L.ptr(ws), L.ptr(ws), 16, L.stream())
    assert rc == L.ERR_WORKSPACE
    # the Python layer refuses before the library is reached
    x = torch.ones((b, h + 2, w + 2, 384), dtype=torch.float32, device=device)
    g = torch.ones((b, h * w, 12), dtype=torch.float32, device=device)
    with pytest.raises(L.DetZeroHipError, match='7 g_cout'):
        ops.conv3x3_wgrad(x, g, 64, 12, groups=6, g_cout=[2, 1, 3, 2, 1, 3, 1], g_ooff=[0, 2, 3, 6, 8, 9, 0])
    with pytest.raises(L.DetZeroHipError, match='cin % 16'):
        ops.conv3x3_wgrad(torch.ones((b, h + 2, w + 2, 24), dtype=torch.float32, device=device), torch.ones((b, h, w, 16), dtype=torch.float32, device=device), 24, 16)
    with pytest.raises(L.DetZeroHipError):
        ops.relu_grad(torch.ones((b, h, w, 6), dtype=torch.float32, device=device), torch.ones((b, h + 2, w + 2, 6), dtype=torch.float32, device=device))
    y = torch.ones((b, h + 2, w + 2, 64), dtype=torch.float32, device=device)
    sums = torch.full((64,), 7.0, dtype=torch.float64, device=device)
    assert lib.dz_relu_grad(None, 0, L.ptr(y), b, h, w, 64, L.ptr(y), L.ptr(sums), L.ptr(ws), ws.numel(), L.stream()) == L.ERR_INVALID
    assert lib.dz_relu_grad(L.ptr(y), 0, L.ptr(y), b, 0, w, 64, L.ptr(y), L.ptr(sums), L.ptr(ws), ws.numel(), L.stream()) == L.ERR_INVALID
    assert lib.dz_head_final_backward(None, L.ptr(y), L.ptr(y), b, h, w, 64, 6, i6, o6, 6, L.ptr(y), L.ptr(sums), L.ptr(y), L.ptr(sums),
                                      L.ptr(ws), ws.numel(), L.stream()) == L.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((sums == 7.0).all()) and float(ws.max()) == 0.0
