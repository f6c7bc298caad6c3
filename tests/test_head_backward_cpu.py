"""CPU: the backward of CenterHead's convolutions - the C ABI's new names, the float64 reference helpers of
tests/head_backward_ref.py against plain torch autograd, the adjoint property of the data gradient's weight packing, and the
BatchNorm / bias formulas of head_backward.head_gradients on float64 stand-ins for the device ops."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_backward_ref as R

NAMES = ('dz_conv3x3_wgrad', 'dz_conv3x3_wgrad_ws_bytes', 'dz_relu_grad', 'dz_relu_grad_ws_bytes', 'dz_head_final_backward',
         'dz_head_final_backward_ws_bytes')


def test_new_names_declared_and_exported():
    from detzero_amd import lib as L
    from detzero_amd import ops
    from detzero_amd.build import build
    build(verbose=False)
    cdll = ctypes.CDLL(L.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'detzero_hip.h')).read()
    for name in NAMES:
        assert name + '(' in header and name in L.exported_symbols()
        assert hasattr(cdll, name)
    assert '#define DZ_WGRAD_TILE_W %d' % ops.WGRAD_TILE_W in header and '#define DZ_WGRAD_CHUNK_ROWS %d' % ops.WGRAD_CHUNK_ROWS in header
    assert ops.WGRAD_CHUNK_PIXELS == ops.WGRAD_TILE_W * ops.WGRAD_CHUNK_ROWS


def test_ws_bytes_follow_the_chunks_and_refuse_on_the_host():
    """The workspace functions run on the host: one partial of the result per chunk of a band of WGRAD_TILE_W columns by
    WGRAD_CHUNK_ROWS rows, 0 for the shapes the kernel refuses."""
    from detzero_amd import lib as L
    from detzero_amd import ops
    lib = L.load()
    tw, rows = ops.WGRAD_TILE_W, ops.WGRAD_CHUNK_ROWS
    for b, h, w in ((1, 1, 1), (2, rows, tw), (1, rows + 1, tw), (1, rows, tw + 1), (3, 23, 19)):
        chunks = b * -(-h // rows) * -(-w // tw)
        assert lib.dz_conv3x3_wgrad_ws_bytes(b, h, w, 48, 64, 1) == -(-chunks * 9 * 48 * 64 * 4 // 256) * 256
        assert lib.dz_conv3x3_wgrad_ws_bytes(b, h, w, 64, 12, 6) == -(-chunks * 6 * 9 * 64 * 16 * 4 // 256) * 256
    assert lib.dz_conv3x3_wgrad_ws_bytes(1, 4, 4, 24, 64, 1) == 0 and lib.dz_conv3x3_wgrad_ws_bytes(1, 4, 4, 16, 8, 1) == 0
    assert lib.dz_conv3x3_wgrad_ws_bytes(1, 4, 4, 528, 64, 1) == 0 and lib.dz_conv3x3_wgrad_ws_bytes(0, 4, 4, 16, 16, 1) == 0
    assert lib.dz_conv3x3_wgrad_ws_bytes(1, 1024, 1024, 512, 64, 1) == 0           # an x image of 2 GiB
    assert lib.dz_relu_grad_ws_bytes(1, 4, 4, 6) == 0 and lib.dz_relu_grad_ws_bytes(1, 4, 4, 64) > 0
    assert lib.dz_head_final_backward_ws_bytes(1, 4, 4, 24, 6) == 0 and lib.dz_head_final_backward_ws_bytes(1, 4, 4, 64, 6) > 0


@pytest.mark.parametrize('tag', sorted(R.EACH_HEAD))
def test_reference_helper_equals_plain_autograd(tag):
    """On the chosen seed the float32 and the float64 torch forward have the same ReLU masks in every cell; with those masks in place
    of the ReLUs the helper gives plain autograd's gradients, and so does the written-out graph."""
    seed = R.SEEDS[tag]
    head = R.small_head32(R.EACH_HEAD[tag], seed)
    x = R.seeded_input(seed)
    gh = [g.double() for g in R.seeded_grad_heads(head, seed)]
    h64 = R.module64(head)
    plain, plain_in, own = R.module_backward(h64, x.double(), gh)
    with torch.no_grad():
        sh = head.shared_conv[1](head.shared_conv[0](x))
        m32 = ((sh > 0).double(), [{n: (getattr(sep, n)[0][1](getattr(sep, n)[0][0](torch.relu(sh))) > 0).double() for n in R.ORDER}
                                   for sep in head.heads_list])
    assert R.mask_mismatch(m32, own) == (0, R.mask_mismatch(m32, own)[1])
    masked, masked_in, _ = R.module_backward(h64, x.double(), gh, masks=m32)
    graph, graph_in = R.graph_backward(h64, x.double(), gh, m32)
    assert set(plain) == set(dict(head.named_parameters())) == set(graph)
    for name in plain:
        assert torch.isfinite(plain[name]).all(), name
        np.testing.assert_array_equal(masked[name].numpy(), plain[name].numpy(), err_msg=name)
        np.testing.assert_allclose(graph[name].numpy(), plain[name].numpy(), rtol=1e-10, atol=1e-12, err_msg=name)
    np.testing.assert_array_equal(masked_in.numpy(), plain_in.numpy())
    np.testing.assert_allclose(graph_in.numpy(), plain_in.numpy(), rtol=1e-10, atol=1e-12)
    # the absolute-value run bounds every element
    bound, bound_in = R.graph_backward(h64, x.double(), gh, m32, absolute=True)
    for name in plain:
        assert (plain[name].abs() <= bound[name] * (1 + 1e-12) + 1e-300).all(), name
    assert (plain_in.abs() <= bound_in * (1 + 1e-12)).all()


def test_dgrad_weight_packing_is_the_adjoint():
    """<conv(x, w) * scale, g> == <x, conv(g, packed(w, scale))> in float64, both convolutions in the forward kernel's convention."""
    from detzero_amd import ops
    rng = np.random.default_rng(3)
    b, h, w, cin, cout = 2, 5, 7, 16, 32
    x = rng.standard_normal((b, h, w, cin))
    g = rng.standard_normal((b, h, w, cout))
    wt = rng.standard_normal((9, cin, cout))
    scale = rng.standard_normal(cout)
    packed = ops.conv3x3_dgrad_weights(torch.from_numpy(wt), torch.from_numpy(scale)).numpy()
    np.testing.assert_array_equal(packed, R.dgrad_weights_ref(wt, scale))
    assert packed.shape == (9, cout, cin)
    lhs = (R.conv_taps(R.bordered(x), wt) * scale * g).sum()
    dx = R.conv_taps(R.bordered(g), packed)
    rhs = (x * dx).sum()
    assert abs(lhs - rhs) <= 1e-11 * (np.abs(x) * np.abs(dx)).sum()
    np.testing.assert_allclose(dx, R.dgrad_ref(g, wt, scale), rtol=1e-11, atol=1e-11)
    # and torch's own convolution agrees with the convention
    y = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), R.taps_to_oihw(wt), padding=1).permute(0, 2, 3, 1).numpy()
    np.testing.assert_allclose(y, R.conv_taps(R.bordered(x), wt), rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize('tag', sorted(R.EACH_HEAD))
def test_head_gradients_formulas_on_float64_stand_ins(tag):
    """head_gradients with the device ops replaced by numpy float64: the four BatchNorm / bias formulas, the gamma = 0 and gamma < 0
    channels, the heads' sum at the shared map, the names, shapes and dtypes."""
    from detzero_amd import head_backward as hb
    from detzero_amd.det_modules import nchw_to_padded_nhwc
    seed = R.SEEDS[tag]
    head = R.small_head32(R.EACH_HEAD[tag], seed)
    x = R.seeded_input(seed)
    gh32 = R.seeded_grad_heads(head, seed)
    h64 = R.module64(head)
    ref, ref_in, _ = R.module_backward(h64, x.double(), [g.double() for g in gh32])
    concat = nchw_to_padded_nhwc(x.double())
    grads, grad_in = hb.head_gradients(head, concat, [g.double() for g in gh32], input_grad=True, backend=R.NumpyBackend)
    params = dict(head.named_parameters())
    assert set(grads) == set(params) == set(k for k, v in head.state_dict().items() if v.is_floating_point() and 'running_' not in k)
    bound, bound_in = R.graph_backward(h64, x.double(), [g.double() for g in gh32], R.module_backward(h64, x.double(), [g.double() for g in gh32])[2],
                                       absolute=True)
    for name, g in grads.items():
        assert g.shape == params[name].shape and g.dtype == params[name].dtype, name
        # float32 results of a float64 computation whose folded scale / shift were rounded to float32 once
        err = (g.double() - ref[name]).abs()
        assert (err <= 8 * R.U32 * bound[name] + 1e-30).all(), (name, float((err / (bound[name] + 1e-300)).max()))
    zname, zc = R.ZERO_GAMMA
    assert float(params[zname + '.weight'][zc].detach()) == 0.0 and torch.isfinite(grads[zname + '.weight']).all()
    assert float(ref[zname + '.weight'][zc].abs()) > 0 and float(grads[zname + '.weight'][zc].abs()) > 0
    err = (grad_in.permute(0, 3, 1, 2) - ref_in).abs()
    assert (err <= 8 * R.U32 * bound_in).all()
    assert hb.head_gradients(head, concat, [g.double() for g in gh32], backend=R.NumpyBackend)[1] is None


def test_head_gradients_refusals():
    from detzero_amd import head_backward as hb
    from detzero_amd.det_modules import nchw_to_padded_nhwc
    from detzero_amd.lib import DetZeroHipError
    head = R.small_head32(R.EACH_HEAD['one_head'], 0)
    concat = nchw_to_padded_nhwc(R.seeded_input(0).double())
    gh = [g.double() for g in R.seeded_grad_heads(head, 0)]
    with pytest.raises(DetZeroHipError, match='one .* tensor per head'):
        hb.head_gradients(head, concat, gh + gh, backend=R.NumpyBackend)
    with pytest.raises(DetZeroHipError, match='zero-bordered'):
        hb.head_gradients(head, concat[..., :16], gh, backend=R.NumpyBackend)
    head.train()
    with pytest.raises(DetZeroHipError, match='eval'):
        hb.head_gradients(head, concat, gh, backend=R.NumpyBackend)
    assert hb.frames_per_group(64, 190, 190, 384) == 38
