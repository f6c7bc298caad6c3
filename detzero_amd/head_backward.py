"""CenterHead: backward through the head's three convolution layers (the shared 3 x 3, the six branches' hidden 3 x 3 as one
c -> 6c layer, the grouped 6c -> 12 output layer) down to every parameter of ``dense_head`` and, on request, to
``spatial_features_2d``.  Backed by csrc/head_backward.hip (``ops.conv3x3_wgrad`` / ``ops.relu_grad`` / ``ops.head_final_backward``)
and, for the data gradients, by the fp32 forward kernel on flipped, transposed weights (``ops.conv3x3_dgrad``); DESIGN.md 7q states
the formulas.  BatchNorm stays in eval mode (frozen statistics): one layer is y = relu(scale_c * conv(x, w)_c + shift_c) with
scale = gamma * rstd, shift = beta - mean * scale + bias * scale (``det_modules.fold_bn``), and with g = g_y * [y > 0],
Graw = the raw weight gradient and S_c = sum g_c:

    d conv.weight_c = scale_c * Graw_c                 d conv.bias_c = scale_c * S_c
    d bn.bias_c     = S_c                              d bn.weight_c = rstd_c * (<w_c, Graw_c> + (bias_c - mean_c) * S_c)

(no division by gamma: a channel with gamma == 0 gets finite, correct gradients).  After an optimiser step on these parameters call
``dense_head.invalidate()``: the kernels read the cached plan, not the parameters.
"""
import torch

from . import ops
from .lib import DetZeroHipError

ORDER = ('center', 'center_z', 'dim', 'rot', 'iou', 'hm')      # CenterHead.plan()['order']: the column blocks of the hidden layer
MAX_IMAGE_BYTES = 1 << 31


class DeviceBackend:
    """The device kernels behind head_gradients.  A stand-in with the same five methods (float64 host code) replaces it in the tests
    of the formulas."""

    @staticmethod
    def forward_layer(x_img, w, scale, shift):
        """relu(scale * conv3x3(x_img, w) + shift) -> zero-bordered image: math mode 0, every opt-in engine off."""
        from .det_modules import conv_layer
        b, hp, wp, cin = x_img.shape
        cout = w.shape[2]
        out = torch.zeros((b, hp, wp, cout), dtype=torch.float32, device=x_img.device)
        conv_layer(x_img, (hp, wp), w, scale, shift, True, out, (hp, wp), cin=cin, in_cstride=cin, out_cstride=cout, out_d=(1, 1),
                   ho=hp - 2, wo=wp - 2, batch=b, math=0)
        return out

    @staticmethod
    def final_layer(hidden_img, fin, c):
        """The grouped output layer -> head map (B, H * W, 12), as CenterHead.run_head forms it in math mode 0."""
        from .det_modules import conv_layer
        b, hp, wp, _ = hidden_img.shape
        h, w = hp - 2, wp - 2
        head = torch.empty((b, h * w, 12), dtype=torch.float32, device=hidden_img.device)
        conv_layer(hidden_img, (hp, wp), fin['w'], None, fin['shift'], False, head, (h, w), cin=c, in_cstride=hidden_img.shape[3],
                   out_cstride=12, out_d=(0, 0), groups=len(fin['g_cout']), cout_pad=16, g_cout=fin['g_cout'], g_ooff=fin['g_ooff'], ho=h,
                   wo=w, batch=b, math=0, out_f32=True)
        return head

    relu_grad = staticmethod(lambda g_y, y_img: ops.relu_grad(g_y, y_img))
    wgrad = staticmethod(lambda x_img, g_img, cin, cout: ops.conv3x3_wgrad(x_img, g_img, cin, cout))
    dgrad = staticmethod(lambda g_img, w, scale: ops.conv3x3_dgrad(g_img, w, scale))
    final_backward = staticmethod(lambda grad_head, w2, hidden_img, g_cout, g_ooff: ops.head_final_backward(grad_head, w2, hidden_img, g_cout, g_ooff))


def _refuse_vel(head_module, what):
    if 'vel' in head_module.separate_head_cfg.HEAD_DICT.keys():
        raise DetZeroHipError('%s: a `vel` head is not supported' % what)


def head_forward_f32(head_module, concat, backend=DeviceBackend, want_heads=True):
    """One well-defined fp32 forward of the head on the zero-bordered (B, H + 2, W + 2, Cin) image: math mode 0 with every opt-in
    engine off, whatever the module's inference mode is, in buffers of its own.  -> (shared, [hidden per head], [head map per head])."""
    p = head_module.plan()
    shared = backend.forward_layer(concat, p['shared']['w'], p['shared']['scale'], p['shared']['shift'])
    hidden, heads = [], []
    for hp_ in p['heads']:
        hid = backend.forward_layer(shared, hp_['hidden']['w'], hp_['hidden']['scale'], hp_['hidden']['shift'])
        hidden.append(hid)
        if want_heads:
            heads.append(backend.final_layer(hid, hp_['final'], p['c']))
    return shared, hidden, heads


def _bn_terms(bn):
    f64 = torch.float64
    rstd = 1.0 / torch.sqrt(bn.running_var.detach().to(f64) + bn.eps)
    return bn.weight.detach().to(f64) * rstd, rstd, bn.running_mean.detach().to(f64)


def _layer_grads(grads, prefix, conv, bn, w_taps, graw, sums):
    """The four formulas for one conv + BN layer.  prefix: the state_dict name of the nn.Sequential(conv, bn, relu).  w_taps / graw
    (9, ci, co) in the layer's own columns, sums (co,) f64."""
    f64 = torch.float64
    scale, rstd, mean = _bn_terms(bn)
    g64, w64 = graw.to(f64), w_taps.to(f64)
    co, ci = conv.weight.shape[0], conv.weight.shape[1]
    d_w = (g64 * scale.reshape(1, 1, -1)).permute(2, 1, 0).reshape(co, ci, 3, 3)
    grads[prefix + '.0.weight'] = d_w.to(conv.weight.dtype)
    off = -mean
    if conv.bias is not None:
        grads[prefix + '.0.bias'] = (scale * sums).to(conv.bias.dtype)
        off = conv.bias.detach().to(f64) - mean
    grads[prefix + '.1.weight'] = (rstd * ((w64 * g64).sum(dim=(0, 1)) + off * sums)).to(bn.weight.dtype)
    grads[prefix + '.1.bias'] = sums.to(bn.bias.dtype)


def _group_gradients(head_module, concat, grad_heads, input_grad, backend, state=None):
    p = head_module.plan()
    c = p['c']
    shared, hidden, _ = state if state is not None else head_forward_f32(head_module, concat, backend, want_heads=False)
    grads = {}
    g_shared_y = None
    for i, (hp_, head) in enumerate(zip(p['heads'], head_module.heads_list)):
        hid, fin = hp_['hidden'], hp_['final']
        g_hidden, s_h, d_w2, d_b2 = backend.final_backward(grad_heads[i], fin['w'], hidden[i], fin['g_cout'], fin['g_ooff'])
        graw_h = backend.wgrad(shared, g_hidden, c, len(ORDER) * c)
        for k, name in enumerate(ORDER):
            fc = getattr(head, name)
            prefix = 'heads_list.%d.%s' % (i, name)
            col = slice(k * c, (k + 1) * c)
            _layer_grads(grads, prefix + '.0', fc[0][0], fc[0][1], hid['w'][:, :, col], graw_h[:, :, col], s_h[col])
            conv2, n = fc[1], fin['g_cout'][k]
            grads[prefix + '.1.weight'] = d_w2[k, :, :, :n].permute(2, 1, 0).reshape(n, c, 3, 3).to(conv2.weight.dtype)
            grads[prefix + '.1.bias'] = d_b2[k, :n].to(conv2.bias.dtype)
        d_y = backend.dgrad(g_hidden, hid['w'], hid['scale'])
        g_shared_y = d_y if g_shared_y is None else g_shared_y + d_y          # the heads' gradients at the shared map, in head order
        del g_hidden, d_y
    g_shared, s_s = backend.relu_grad(g_shared_y, shared)
    sc = head_module.shared_conv
    graw_s = backend.wgrad(concat, g_shared, p['shared']['cin'], c)
    _layer_grads(grads, 'shared_conv', sc[0], sc[1], p['shared']['w'], graw_s, s_s)
    grad_input = backend.dgrad(g_shared, p['shared']['w'], p['shared']['scale']) if input_grad else None
    return grads, grad_input


def frames_per_group(batch, hp, wp, channels):
    """Frames of a group whose widest image (channels floats per pixel of the bordered map) stays below 2 GiB."""
    per_frame = hp * wp * channels * 4
    if per_frame >= MAX_IMAGE_BYTES:
        raise DetZeroHipError('head_gradients: one frame\'s %d-channel image of %d x %d reaches 2 GiB' % (channels, hp, wp))
    return max(1, min(batch, (MAX_IMAGE_BYTES - 1) // per_frame))


def head_gradients(head_module, concat, grad_heads, input_grad=False, backend=DeviceBackend, state=None):
    """Gradients of every floating-point parameter of a CenterHead, from the gradients at its head maps.

    concat: the zero-bordered (B, H + 2, W + 2, Cin) fp32 image (``det_modules.nchw_to_padded_nhwc``); grad_heads: one (B, H * W, 12)
    tensor per head (columns 9 + ncls .. 11 are never read).  The function reruns the head's two hidden layers itself in math mode 0
    with every opt-in engine off, in buffers of its own, so the ReLU masks are those of one well-defined fp32 forward whatever the
    module's inference mode is, and ``forward`` is untouched (state: the result of head_forward_f32 on the same image, to spare it).
    -> (grads, grad_input): grads maps the ``state_dict`` name of every floating-point parameter (``shared_conv.0.weight``, ...,
    ``heads_list.0.hm.1.bias``; running statistics get no entry) to a tensor of its shape and dtype; with several heads the
    gradients at the shared map add up in head order.  grad_input: (B, H, W, Cin) or None.  A batch whose widest (6c-channel) image
    would reach 2 GiB is processed in frame groups whose sums are added in group order.  The module must be in eval mode; after an
    optimiser step call ``head_module.invalidate()``."""
    if head_module.training:
        raise DetZeroHipError('head_gradients: BatchNorm stays in eval mode (frozen statistics); call .eval()')
    _refuse_vel(head_module, 'head_gradients')
    p = head_module.plan()
    if concat.dim() != 4 or concat.shape[3] != p['shared']['cin'] or concat.shape[1] < 3 or concat.shape[2] < 3:
        raise DetZeroHipError('head_gradients: concat is the zero-bordered (B, H + 2, W + 2, %d) image, got %s' % (p['shared']['cin'], tuple(concat.shape)))
    grad_heads = list(grad_heads) if isinstance(grad_heads, (list, tuple)) else [grad_heads]
    b, hp, wp = concat.shape[0], concat.shape[1], concat.shape[2]
    if len(grad_heads) != len(p['heads']) or any(tuple(g.shape) != (b, (hp - 2) * (wp - 2), 12) for g in grad_heads):
        raise DetZeroHipError('head_gradients: grad_heads is one (%d, %d, 12) tensor per head (%d heads), got %s'
                              % (b, (hp - 2) * (wp - 2), len(p['heads']), [tuple(g.shape) for g in grad_heads]))
    step = frames_per_group(b, hp, wp, max(len(ORDER) * p['c'], p['shared']['cin']))
    if step >= b:
        return _group_gradients(head_module, concat, grad_heads, input_grad, backend, state)
    grads, inputs = None, []
    for b0 in range(0, b, step):
        g, gi = _group_gradients(head_module, concat[b0:b0 + step], [t[b0:b0 + step] for t in grad_heads], input_grad, backend)
        grads = g if grads is None else {k: grads[k] + v for k, v in g.items()}
        inputs.append(gi)
    return grads, (torch.cat(inputs, dim=0) if input_grad else None)


def loss_backward(head_module, data_dict):
    """CenterHead.loss_backward (see there)."""
    from .det_modules import _inference_only, _recode, nchw_to_padded_nhwc
    from .head_loss import device_targets, loss_weights, tb_dict_of
    _inference_only(head_module)
    _refuse_vel(head_module, 'CenterHead.loss_backward')
    gt_boxes = data_dict.get('gt_boxes', None)
    if gt_boxes is None:
        raise DetZeroHipError('CenterHead.loss_backward: the batch carries no gt_boxes')
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] != 8:
        raise DetZeroHipError('CenterHead.loss_backward: gt_boxes with %d columns (8: a `vel` head is not supported)' % gt_boxes.shape[-1])
    with torch.no_grad():
        concat = data_dict.get('_nhwc_spatial_features_2d', None)
        if concat is None:
            concat = nchw_to_padded_nhwc(data_dict['spatial_features_2d'].float())
        else:
            concat = _recode(concat, data_dict.get('_nhwc_math', 0), 0, int(data_dict.get('_nhwc_exp', 0) or 0), 0)
        concat = concat.contiguous()
        b, hp, wp = concat.shape[0], concat.shape[1], concat.shape[2]
        h, w = hp - 2, wp - 2
        p = head_module.plan()
        step = frames_per_group(b, hp, wp, max(len(ORDER) * p['c'], p['shared']['cin']))
        state = None
        if step >= b:
            state = head_forward_f32(head_module, concat)
            heads = state[2]
        else:
            parts = [head_forward_f32(head_module, concat[b0:b0 + step])[2] for b0 in range(0, b, step)]
            heads = [torch.cat([part[i] for part in parts], dim=0) for i in range(len(p['heads']))]
        targets = device_targets(head_module, gt_boxes.to(concat.device), (h, w))
        weights = loss_weights(head_module.model_cfg)
        totals, recs, grad_heads = [], [], []
        for i, head in enumerate(heads):
            rec, grad = ops.centerhead_loss_nosync(head, targets['heatmaps'][i], targets['target_boxes'][i], targets['inds'][i],
                                                   targets['masks'][i], targets['records'][i], h, w, weights, head_module.feature_map_stride,
                                                   head_module.point_cloud_range, head_module.voxel_size, want_grad=True)
            totals.append(rec[ops.HEAD_LOSS_REC - 1].to(torch.float32))
            recs.append(rec)
            grad_heads.append(grad)
        loss = totals[0] if len(totals) == 1 else torch.stack(totals).sum()
        grads, _ = head_gradients(head_module, concat, grad_heads, state=state)
        params = dict(head_module.named_parameters())
        for name, g in grads.items():
            prm = params[name]
            if prm.grad is None:
                prm.grad = g.clone()
            else:
                prm.grad += g
        tb_dict = tb_dict_of(torch.stack(recs).cpu().numpy(), head_module.iou_weight, {})
    return loss, tb_dict
