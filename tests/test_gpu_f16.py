"""GPU (MI355X): the opt-in 'f16' math mode - the tensors of 'f16x2' (fp16 pairs), ONE fp16 MFMA per product on the hi halves
(csrc/hgemm.h MathF16H): plain-fp16 inputs, fp32 accumulation, a third of the matrix work (BASELINE.json configs[4] names an
"fp16 sparse backbone"; the reference itself has no half-precision path to mirror).

It is NOT fp32-class and never the headline arithmetic; this file states what it delivers, against the CPU oracle on the headline
workload (160k points, 0.1 m voxels): the active sets stay bit-exact (the index path does not depend on the arithmetic), single
layers are within fp16 input rounding (a few 1e-4 relative) of the fp32 reference, and the final boxes stay within 2.5e-3
(observed: 8.3e-4 on this frame; the fp32-class modes are within 8e-6)."""
import numpy as np
import pytest
import torch

from detzero_amd.synth import VOXEL_SIZE_01
from tests.util import cpu_state_dict, make_model, masked_frame, match_boxes, oracle_detect

pytestmark = pytest.mark.gpu
BOX_TOL = 3e-2


def test_single_layers_in_f16_mode(device):
    """One dense 3x3 layer (resident-tile kernel) in 'f16x2' and 'f16' against fp32 torch on the SAME fp32 inputs - the error is that of
    rounding inputs and weights to fp16 (2^-11 relative each), not more - and one sparse layer in 'f16' against float64."""
    from detzero_amd import ops
    from detzero_amd.det_modules import conv_layer
    g = torch.Generator().manual_seed(0)
    b, h, w, cin, cout = 2, 64, 64, 64, 128
    x = torch.zeros(b, h + 2, w + 2, cin)
    x[:, 1:-1, 1:-1] = torch.randn(b, h, w, cin, generator=g)
    wt = torch.randn(9, cin, cout, generator=g) * 0.05
    ref = torch.nn.functional.conv2d(x[:, 1:-1, 1:-1].permute(0, 3, 1, 2), wt.reshape(3, 3, cin, cout).permute(3, 2, 0, 1), padding=1)
    ref = ref.permute(0, 2, 3, 1)
    xp = ops.pair16_from_f32(x.to(device), math=1)
    wp = ops.pack_weight_split(wt.to(device), 1)
    one = torch.ones(cout, device=device)
    for math, tol in ((1, 2e-5), (3, 3e-3)):
        y = torch.zeros(b, h + 2, w + 2, cout, device=device)
        conv_layer(xp, (h + 2, w + 2), wp, one, one * 0, False, y, (h + 2, w + 2), cin=cin, in_cstride=cin, ksize=3, stride=1, in_off=0,
                   out_cstride=cout, out_d=(1, 1), ho=h, wo=w, batch=b, math=math)
        got = ops.pair16_to_f32(y, 1)[:, 1:-1, 1:-1].cpu()
        err = float((got - ref).abs().max() / ref.abs().max())
        assert err < tol, (math, err)
        if math == 3:
            assert err > 1e-5            # it really is the single-product path
    # the sparse layer: 64 -> 64 submanifold on the gather and on the x-run kernel, 'f16' against float64 on the operands as stored, under
    # the dense 'f16' bound and above the 'f16x2' one (it really is the single-product path): tests/test_gpu_sparse_conv.py
    from tests import test_gpu_sparse_conv as sp
    for engine in ('split', 'x'):
        name, worst = sp.run_case(sp.sp_case(engine, 'f16', 64, 64, 'subm', 'plain'), device)
        assert sp.BOUND['f16x2'] < worst <= sp.BOUND['f16'], (name, worst)


def test_f16_mode_on_the_headline_workload(device):
    """Whole detector, 160k points / 0.1 m: voxels and active sets as in every mode, final boxes within BOX_TOL of the CPU oracle."""
    from detzero_amd.centerpoint import FramePipeline
    model, cfg, info = make_model(VOXEL_SIZE_01, seed=0)
    sd = cpu_state_dict(model)
    frame = masked_frame(0, 160000)
    ref = oracle_detect(sd, frame, info)
    model = model.to(device)
    pipe = FramePipeline(model, info, math='f16')
    out, d_n = pipe(torch.from_numpy(frame).to(device))
    n = int(d_n.item())
    rb = ref['final'][0]
    n_ref = rb['pred_boxes'].shape[0]
    got = out[:n].cpu().numpy()
    nm, worst = match_boxes(rb['pred_boxes'].numpy(), rb['pred_scores'].numpy(), got[:, :7], got[:, 7], tol=BOX_TOL)
    print('f16 (single product) vs oracle: %d / %d boxes, %d matched within %.1e (worst %.2e)' % (n, n_ref, nm, BOX_TOL, worst))
    assert n_ref > 50 and abs(n - n_ref) <= 3 and nm >= n_ref - 3, (n, n_ref, nm, worst)
    # and it is a different arithmetic from the fp32-class default: the same frame in f16x2 sits orders of magnitude closer
    pipe2 = FramePipeline(model, info, math='f16x2')
    out2, d_n2 = pipe2(torch.from_numpy(frame).to(device))
    g2 = out2[:int(d_n2.item())].cpu().numpy()
    nm2, worst2 = match_boxes(rb['pred_boxes'].numpy(), rb['pred_scores'].numpy(), g2[:, :7], g2[:, 7], tol=1e-3)
    print('f16x2 on the same frame: %d matched within 1e-3 (worst %.2e)' % (nm2, worst2))
    assert nm2 >= n_ref - 2 and 10.0 * worst2 < worst, (worst2, worst)
