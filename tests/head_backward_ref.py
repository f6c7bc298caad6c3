"""Float64 references for the backward of CenterHead's convolutions (host only: numpy and torch on the CPU).

  * wgrad_ref / relu_grad_ref / dgrad_ref / final_backward_ref: the kernels of csrc/head_backward.hip one by one;
  * module_backward: the head deep-copied to float64, its own nn.Sequential branches in eval mode, every ReLU either real or
    replaced by a given mask, loss = sum(head_map * grad_head), backward();
  * graph_backward: the same graph written out on leaf tensors, which also runs with every input, weight, folded scale and incoming
    gradient replaced by its absolute value (masks kept): per gradient element the sum of the absolute values of all monomials;
  * NumpyBackend: float64 stand-ins for head_backward.DeviceBackend.
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F

ORDER = ('center', 'center_z', 'dim', 'rot', 'iou', 'hm')
U32 = 2.0 ** -24


def gamma_n(n):
    return n * U32 / (1.0 - n * U32)


# ---- the kernels one by one -------------------------------------------------------------------------------------
def wgrad_ref(x_img, g, groups=1, g_cout=None, g_ooff=None, absolute=False):
    """x_img (B, H + 2, W + 2, groups * cin), g dense (B, H, W, cols) -> (9, cin, cout) or (groups, 9, cin, 16) float64."""
    x_img, g = np.asarray(x_img, np.float64), np.asarray(g, np.float64)
    if absolute:
        x_img, g = np.abs(x_img), np.abs(g)
    b, hp, wp, ctot = x_img.shape
    h, w = hp - 2, wp - 2
    cin = ctot // groups
    g = g.reshape(b, h, w, -1)
    if groups == 1:
        out = np.zeros((9, cin, g.shape[3]))
        for t in range(9):
            out[t] = np.einsum('bhwi,bhwo->io', x_img[:, t // 3:t // 3 + h, t % 3:t % 3 + w, :], g)
        return out
    out = np.zeros((groups, 9, cin, 16))
    for q in range(groups):
        gq = g[..., g_ooff[q]:g_ooff[q] + g_cout[q]]
        for t in range(9):
            out[q, t, :, :g_cout[q]] = np.einsum('bhwi,bhwo->io', x_img[:, t // 3:t // 3 + h, t % 3:t % 3 + w, q * cin:(q + 1) * cin], gq)
    return out


def relu_grad_ref(g_y, y_img):
    """g_y dense (B, H, W, C), y_img bordered -> (g dense float64, sums)."""
    y = np.asarray(y_img)[:, 1:-1, 1:-1, :]
    g = np.where(y > 0, np.asarray(g_y, np.float64), 0.0)
    return g, g.sum(axis=(0, 1, 2))


def taps_to_oihw(w_taps):
    """(9, cin, cout) -> (cout, cin, 3, 3)."""
    w = torch.as_tensor(np.asarray(w_taps), dtype=torch.float64)
    return w.permute(2, 1, 0).reshape(w.shape[2], w.shape[1], 3, 3)


def dgrad_ref(g, w_taps, scale=None):
    """g dense (B, H, W, cout), w_taps (9, cin, cout) -> d x (B, H, W, cin) float64 of y = scale * conv3x3(x, w), by torch autograd."""
    g = torch.as_tensor(np.asarray(g), dtype=torch.float64)
    b, h, w, _ = g.shape
    x = torch.zeros((b, w_taps.shape[1], h, w), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, taps_to_oihw(w_taps), padding=1)
    if scale is not None:
        y = y * torch.as_tensor(np.asarray(scale), dtype=torch.float64).reshape(1, -1, 1, 1)
    (y * g.permute(0, 3, 1, 2)).sum().backward()
    return x.grad.permute(0, 2, 3, 1).numpy()


def dgrad_weights_ref(w_taps, scale=None):
    """The packing of ops.conv3x3_dgrad_weights in numpy: flipped in both spatial axes, transposed, scale folded."""
    w = np.asarray(w_taps, np.float64)
    if scale is not None:
        w = w * np.asarray(scale, np.float64).reshape(1, 1, -1)
    return np.ascontiguousarray(w[::-1].transpose(0, 2, 1))


def conv_taps(x_img, w_taps):
    """The forward convention of dz_conv2d_forward: y[b, y, x, c] = sum x_img[b, y + ky, x + kx, ci] * w[ky * 3 + kx, ci, c]."""
    x_img, w_taps = np.asarray(x_img, np.float64), np.asarray(w_taps, np.float64)
    b, hp, wp, _ = x_img.shape
    h, w = hp - 2, wp - 2
    out = np.zeros((b, h, w, w_taps.shape[2]))
    for t in range(9):
        out += x_img[:, t // 3:t // 3 + h, t % 3:t % 3 + w, :] @ w_taps[t]
    return out


def bordered(x, value=0.0):
    x = np.asarray(x)
    out = np.full((x.shape[0], x.shape[1] + 2, x.shape[2] + 2, x.shape[3]), value, x.dtype)
    out[:, 1:-1, 1:-1, :] = x
    return out


def final_backward_ref(grad_head, w2, hidden_img, g_cout, g_ooff, absolute=False):
    """-> (g_hidden dense (B, H, W, groups * c), sums, d_w2 (groups, 9, c, 16), d_bias (groups, 16)) float64."""
    grad_head, w2, hidden_img = np.asarray(grad_head, np.float64), np.asarray(w2, np.float64), np.asarray(hidden_img, np.float64)
    b, hp, wp, ctot = hidden_img.shape
    h, w = hp - 2, wp - 2
    groups, c = w2.shape[0], w2.shape[2]
    gh = grad_head.reshape(b, h, w, 12)
    d_bias = np.zeros((groups, 16))
    g_hidden = np.zeros((b, h, w, ctot))
    for q in range(groups):
        gq = gh[..., g_ooff[q]:g_ooff[q] + g_cout[q]]
        wq = w2[q, :, :, :g_cout[q]]
        if absolute:
            gq, wq = np.abs(gq), np.abs(wq)
        d_bias[q, :g_cout[q]] = gq.sum(axis=(0, 1, 2))
        pad = bordered(gq)
        # hidden pixel (y, x) feeds output pixel (y - ky + 1, x - kx + 1) through tap (ky, kx)
        for ky in range(3):
            for kx in range(3):
                g_hidden[..., q * c:(q + 1) * c] += pad[:, 2 - ky:2 - ky + h, 2 - kx:2 - kx + w, :] @ wq[ky * 3 + kx].T
    g_hidden = np.where(hidden_img[:, 1:-1, 1:-1, :] > 0, g_hidden, 0.0)
    d_w2 = wgrad_ref(hidden_img, gh, groups, g_cout, g_ooff, absolute=absolute)
    return g_hidden, g_hidden.sum(axis=(0, 1, 2)), d_w2, d_bias


# ---- the module in float64 --------------------------------------------------------------------------------------
def module64(head):
    m = copy.deepcopy(head).cpu().double().eval()
    m.zero_grad()
    return m


def head_cols(head, index):
    names = head.class_names_each_head[index]
    return {n: (o, len(names) if n == 'hm' else c) for n, (o, c) in head.COLS.items()}


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def module_backward(head64, x, grad_heads, masks=None):
    """head64: module64(head).  x (B, Cin, H, W) float64; grad_heads: per head (B, H * W, 12) float64 (NaN in unread columns allowed);
    masks: None (real ReLU) or (shared (B, C, H, W), [hidden per head: {branch: (B, C, H, W)}]) of 0 / 1 float64.
    -> (grads by state_dict name, grad_input (B, Cin, H, W), masks of this run's own ReLUs in the same structure)."""
    head64.zero_grad()
    x = x.clone().requires_grad_(True)
    b, _, h, w = x.shape

    def run(seq, inp, mask):
        z = seq[1](seq[0](inp))
        own = (z > 0).to(z.dtype).detach()
        return (torch.relu(z) if mask is None else z * mask), own

    shared, own_shared = run(head64.shared_conv, x, None if masks is None else masks[0])
    own_hidden = []
    loss = 0.0
    for i, sep in enumerate(head64.heads_list):
        cols = head_cols(head64, i)
        gh = grad_heads[i].reshape(b, h, w, 12)
        own = {}
        for name in ORDER:
            fc = getattr(sep, name)
            hid, own[name] = run(fc[0], shared, None if masks is None else masks[1][i][name])
            o, n = cols[name]
            loss = loss + (fc[1](hid) * _nchw(gh[..., o:o + n])).sum()
        own_hidden.append(own)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in head64.named_parameters()}
    return grads, x.grad.clone(), (own_shared, own_hidden)


def graph_backward(head64, x, grad_heads, masks, absolute=False):
    """The same graph on leaf tensors: z = conv(x, w) + off, off = conv bias - running mean, y = (z * (gamma * rstd) + beta) * mask.
    absolute: x, w, off, gamma, the output layer's weights and the incoming gradients by their absolute values, masks kept - the
    gradients are then, per element, the sums of the absolute values of all monomials (the gradient at a conv bias is the one at off).
    -> (grads by state_dict name, grad_input)."""
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    leaves = {}

    def leaf(name, t):
        leaves[name] = ab(t.detach().clone()).requires_grad_(True)
        return leaves[name]

    def layer(prefix, conv, bn, inp, mask):
        wt = leaf(prefix + '.0.weight', conv.weight)
        bias = conv.bias.detach() if conv.bias is not None else torch.zeros_like(bn.running_mean)
        off = leaf(prefix + '.0.off', bias - bn.running_mean)
        gam = leaf(prefix + '.1.weight', bn.weight)
        bet = leaf(prefix + '.1.bias', bn.bias)
        rstd = 1.0 / torch.sqrt(bn.running_var + bn.eps)
        z = F.conv2d(inp, wt, padding=1) + off.reshape(1, -1, 1, 1)
        return (z * (gam * rstd).reshape(1, -1, 1, 1) + bet.reshape(1, -1, 1, 1)) * mask

    xl = leaf('input', x)
    b, _, h, w = x.shape
    shared = layer('shared_conv', head64.shared_conv[0], head64.shared_conv[1], xl, masks[0])
    loss = 0.0
    for i, sep in enumerate(head64.heads_list):
        cols = head_cols(head64, i)
        gh = grad_heads[i].reshape(b, h, w, 12)
        for name in ORDER:
            fc = getattr(sep, name)
            prefix = 'heads_list.%d.%s' % (i, name)
            hid = layer(prefix + '.0', fc[0][0], fc[0][1], shared, masks[1][i][name])
            w2 = leaf(prefix + '.1.weight', fc[1].weight)
            b2 = leaf(prefix + '.1.bias', fc[1].bias)
            o, n = cols[name]
            out = F.conv2d(hid, w2, padding=1) + b2.reshape(1, -1, 1, 1)
            loss = loss + (out * ab(_nchw(gh[..., o:o + n]))).sum()
    loss.backward()
    grads = {}
    for name, prm in head64.named_parameters():
        src = name[:-len('.bias')] + '.off' if name.endswith('.0.bias') and name[:-len('.bias')] + '.off' in leaves else name
        grads[name] = leaves[src].grad.clone()
    return grads, leaves['input'].grad.clone()


def masks_from_device(shared_img, hidden_imgs, c):
    """The device forward's stored activations (bordered, channel-last) -> the mask structure of module_backward, float64 on the CPU."""
    def m(img):
        return (img[:, 1:-1, 1:-1, :] > 0).permute(0, 3, 1, 2).cpu().double()
    return m(shared_img), [{name: m(img)[:, k * c:(k + 1) * c] for k, name in enumerate(ORDER)} for img in hidden_imgs]


def mask_mismatch(a, b):
    """(cells that differ, cells) over the whole structure."""
    diff = int((a[0] != b[0]).sum())
    total = a[0].numel()
    for ha, hb in zip(a[1], b[1]):
        for name in ORDER:
            diff += int((ha[name] != hb[name]).sum())
            total += ha[name].numel()
    return diff, total


# ---- float64 stand-ins for the device backend ---------------------------------------------------------------------
class NumpyBackend:
    """head_backward.DeviceBackend in numpy float64 on CPU tensors (the layouts of the device ops)."""

    @staticmethod
    def _t(a):
        return torch.from_numpy(np.ascontiguousarray(a))

    @classmethod
    def forward_layer(cls, x_img, w, scale, shift):
        y = conv_taps(x_img.numpy(), w.numpy()) * scale.double().numpy() + shift.double().numpy()
        return cls._t(bordered(np.maximum(y, 0.0)))

    @classmethod
    def relu_grad(cls, g_y, y_img):
        g, s = relu_grad_ref(g_y.numpy(), y_img.numpy())
        return cls._t(bordered(g)), cls._t(s)

    @classmethod
    def wgrad(cls, x_img, g_img, cin, cout):
        return cls._t(wgrad_ref(x_img.numpy(), g_img.numpy()[:, 1:-1, 1:-1, :]))

    @classmethod
    def dgrad(cls, g_img, w, scale):
        return cls._t(dgrad_ref(g_img.numpy()[:, 1:-1, 1:-1, :], w.numpy(), None if scale is None else scale.numpy()))

    @classmethod
    def final_backward(cls, grad_head, w2, hidden_img, g_cout, g_ooff):
        g, s, dw, db = final_backward_ref(grad_head.numpy(), w2.numpy(), hidden_img.numpy(), g_cout, g_ooff)
        return cls._t(bordered(g)), cls._t(s), cls._t(dw), cls._t(db)


# ---- fixtures ---------------------------------------------------------------------------------------------------
NAMES = ['Vehicle', 'Pedestrian', 'Cyclist']
RANGE_S, VOXEL = [-9.2, -7.6, -2.0, 9.2, 7.6, 4.0], [0.1, 0.1, 0.15]
W_S, H_S, STRIDE = 23, 19, 8
CIN = 32
ZERO_GAMMA, NEG_GAMMA = ('heads_list.0.dim.0.1', 5), ('heads_list.0.rot.0.1', 9)       # (BatchNorm, channel)


def small_head32(each_head, seed, nmax=64, iou_weight=1):
    """A CenterHead on the 23 x 19 map of the head-loss tests with 32 input channels: seeded, non-trivial BatchNorm statistics and
    affine values, one hidden channel with gamma = 0 and one with gamma < 0 (and a negative gamma in the shared layer)."""
    from detzero_amd.config import centerpoint_1sweep_cfg
    from detzero_amd.det_modules import CenterHead
    cfg = centerpoint_1sweep_cfg()
    cfg.MODEL.DENSE_HEAD.CLASS_NAMES_EACH_HEAD = each_head
    cfg.MODEL.DENSE_HEAD.IOU_WEIGHT = iou_weight
    cfg.MODEL.DENSE_HEAD.TARGET_ASSIGNER_CONFIG.NUM_MAX_OBJS = nmax
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    head = CenterHead(cfg.MODEL.DENSE_HEAD, CIN, 3, NAMES, np.array([W_S * STRIDE, H_S * STRIDE, 40]), RANGE_S, VOXEL)
    mods = dict(head.named_modules())
    with torch.no_grad():
        for name, m in mods.items():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(torch.randn(n, generator=gen) * 0.3)
                m.running_var.copy_(torch.rand(n, generator=gen) + 0.5)
                m.weight.copy_(torch.rand(n, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(n, generator=gen) * 0.3)
            elif isinstance(m, torch.nn.Conv2d) and m.bias is not None and not name.endswith('hm.1'):
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.2)
        mods[ZERO_GAMMA[0]].weight[ZERO_GAMMA[1]] = 0.0
        mods[ZERO_GAMMA[0]].bias[ZERO_GAMMA[1]] = 0.25             # (its ReLU is open everywhere: the channel's gradients are not all zero)
        mods[NEG_GAMMA[0]].weight[NEG_GAMMA[1]] *= -1.0
        mods['shared_conv.1'].weight[3] *= -1.0
    head.predict_boxes_when_training = False            # (no RoI outputs: the head is run on its own)
    return head.eval()


def seeded_input(seed, batch=2):
    """(B, CIN, H, W) float32 features."""
    return torch.randn((batch, CIN, H_S, W_S), generator=torch.Generator().manual_seed(1000 + seed))


def seeded_grad_heads(head, seed, batch=2, nan_unread=True):
    """One (B, H * W, 12) float32 gradient per head, NaN in the columns the head does not have."""
    gen = torch.Generator().manual_seed(2000 + seed)
    out = []
    for names in head.class_names_each_head:
        g = torch.randn((batch, H_S * W_S, 12), generator=gen)
        if nan_unread and len(names) < 3:
            g[..., 9 + len(names):] = float('nan')
        out.append(g)
    return out


EACH_HEAD = {'one_head': [NAMES], 'two_heads': [['Vehicle'], ['Pedestrian', 'Cyclist']]}
# seeds at which the ReLU masks of the float32 and the float64 torch forward agree in every cell (found on the CPU; checked by
# tests/test_head_backward_cpu.py)
SEEDS = {'one_head': 0, 'two_heads': 0}
