"""GPU (MI355X): the split-precision engine (csrc/hgemm.h; 'f16x2' / 'bf16x2' math modes) against the same
oracles and reference goldens as the fp32-MFMA path, with the tolerances the north star states (boxes within
1e-3); conversions and data movers are checked bit-exactly against the torch packer."""
import os

import numpy as np
import pytest
import torch

from detzero_amd.synth import VOXEL_SIZE_01, VOXEL_SIZE_02
from tests.util import cpu_state_dict, make_model, masked_frame, match_boxes, oracle_detect

pytestmark = pytest.mark.gpu
MODES = [('f16x2', 1), ('bf16x2', 2)]
# per-product relative error of a pair: 2^-22 (fp16) / 2^-16 (bf16); tolerances leave ~10x room
TOL = {1: 2e-4, 2: 2e-3}


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device).contiguous()


@pytest.mark.parametrize('name,mid', MODES)
def test_pair16_conversions(device, name, mid):
    from detzero_amd import ops
    gen = torch.Generator().manual_seed(mid)
    x = torch.randn((1000, 40), generator=gen) * torch.logspace(-6, 3, 40)[None, :]
    x[0, :8] = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 1e-8, 70000.0, -1e5, 1.0])
    xd = x.to(device)
    dev = ops.pair16_from_f32(xd, 40, mid)
    host = ops.pair16_pack(x, mid)
    if mid == 1:
        # beyond the fp16 range the device saturates hi AND lo (sum up to 131008); the host packer only clamps
        ok = x.abs() <= 65504
        assert torch.equal(ops.pair16_unpack(dev.cpu(), mid)[ok], ops.pair16_unpack(host, mid)[ok])
        assert float(ops.pair16_unpack(dev.cpu(), mid)[0, 5]) == 70000.0
    else:
        assert torch.equal(dev.cpu().view(torch.int32), host.view(torch.int32))
    back = ops.pair16_to_f32(dev, mid).cpu()
    assert torch.equal(back, ops.pair16_unpack(dev.cpu(), mid))
    ok = x.abs() <= 65504
    # fp16 pair: 22 significant bits down to the subnormal quantum of lo (6e-8); bf16 pair: 16 bits, full range
    bound = (2.0 ** -21) * x.abs() + 6e-8 if mid == 1 else (2.0 ** -15) * x.abs()
    assert bool(((back - x).abs() <= bound)[ok].all())
    # zero-padded channels: 13 -> 16
    y = ops.pair16_to_f32(ops.pair16_from_f32(xd[:, :13].contiguous(), 16, mid), mid).cpu()
    assert float(y[:, 13:].abs().max()) == 0 and torch.allclose(y[:, :13], x[:, :13], rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize('name,mid', MODES)
@pytest.mark.parametrize('cin,cout,kvol', [(16, 16, 27), (16, 32, 27), (32, 32, 27), (32, 64, 27), (64, 64, 27),
                                           (64, 128, 27), (128, 128, 27), (128, 128, 3)])
def test_spconv_split_vs_oracle(device, cin, cout, kvol, name, mid):
    from detzero_amd import ops
    from oracle import sparse as osp
    rng = np.random.default_rng(cin * 1000 + cout + kvol)
    shape = [9, 40, 40]
    n = 3000
    lin = rng.choice(shape[0] * shape[1] * shape[2], size=n, replace=False)
    coords = np.stack([np.zeros(n, np.int64), lin // 1600, (lin // 40) % 40, lin % 40], 1).astype(np.int32)
    coords = coords[osp.canonical_order(coords, shape)]
    feats = rng.standard_normal((n, cin)).astype(np.float32)
    if kvol == 27:
        k, s, p = (3, 3, 3), (1, 1, 1), (1, 1, 1)
        oc = coords
    else:
        k, s, p = (3, 1, 1), (2, 1, 1), (0, 0, 0)
        oc, _ = osp.conv_out_coords(coords, shape, k, s, p)
    w = (rng.standard_normal((kvol, cin, cout)) / np.sqrt(cin * 8)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = rng.standard_normal(cout).astype(np.float32) * 0.1
    res = rng.standard_normal((oc.shape[0], cout)).astype(np.float32)
    rb = osp.build_rulebook(coords, shape, oc, k, s, p)
    ref = osp.sparse_conv(torch.from_numpy(feats), rb, torch.from_numpy(w), oc.shape[0])
    ref = torch.relu(ref * torch.from_numpy(scale) + torch.from_numpy(shift) + torch.from_numpy(res))

    lvl = ops.SparseLevel(1, shape, n, device)
    lvl.build_from_coords(_t(coords, device), want_rank=False)
    out_lvl = lvl if kvol == 27 else lvl.downsample(k, s, p)
    nbr = lvl.neighbors_to(out_lvl, k, s, p)
    res_pad = np.zeros((out_lvl.cap, cout), np.float32); res_pad[:oc.shape[0]] = res
    ws = ops.pack_weight_split(_t(w, device), mid)
    assert tuple(ws.shape) == (kvol, max(cout, 32), cin)
    out = ops.spconv_forward(ops.pair16_from_f32(_t(feats, device), cin, mid), nbr, out_lvl, ws, _t(scale, device), _t(shift, device),
                             ops.pair16_from_f32(_t(res_pad, device), cout, mid), relu=True, math=mid)
    got = ops.pair16_to_f32(out, mid)[:oc.shape[0]].cpu()
    torch.testing.assert_close(got, ref, rtol=TOL[mid], atol=TOL[mid])


@pytest.mark.parametrize('name,mid', MODES)
def test_packed_neighbour_tables(device, name, mid):
    """The packed 27-tap rulebook (one word per (tz, ty) row of the window: rank below the centre + three presence bits) holds the
    same triples as the plain table - on a dense grid whose rows straddle bitmap words, for submanifold and strided windows, and on
    a level whose prefix words are only valid where the bitmap has bits (dz_voxelize_to_level) - and the small-channel
    convolutions give the same bits from either form, with and without a residual."""
    from detzero_amd import ops
    from detzero_amd.synth import POINT_CLOUD_RANGE, VOXEL_SIZE_02, synth_waymo_frame
    rng = np.random.default_rng(5 + mid)
    shape, batch = [5, 9, 70], 2
    cells = shape[0] * shape[1] * shape[2]
    lin = np.nonzero(rng.random(batch * cells) < 0.5)[0]
    lin = np.unique(np.concatenate([lin, [0, 31, 32, batch * cells - 1]]))
    coords = np.stack([lin // cells, (lin % cells) // (shape[1] * shape[2]), (lin // shape[2]) % shape[1], lin % shape[2]], 1).astype(np.int32)
    lvl = ops.SparseLevel(batch, shape, coords.shape[0] + 3, device)
    lvl.build_from_coords(_t(coords, device), want_rank=False)
    K3, S1, P1 = (3, 3, 3), (1, 1, 1), (1, 1, 1)
    cases = [(lvl, lvl, K3, S1, P1)]
    for s, p in (((2, 2, 2), (1, 1, 1)), ((2, 2, 2), (0, 1, 1))):
        cases.append((lvl, lvl.downsample(K3, s, p), K3, s, p))
    grid = [int(round((POINT_CLOUD_RANGE[3 + i] - POINT_CLOUD_RANGE[i]) / VOXEL_SIZE_02[i])) for i in range(3)]
    lvl1, _ = ops.voxelize_to_level(_t(np.concatenate([synth_waymo_frame(3, 20000), synth_waymo_frame(4, 20000)], 0), device), 2,
                                    POINT_CLOUD_RANGE, VOXEL_SIZE_02, 5, 200000, [grid[2] + 1, grid[1], grid[0]], 16, math=mid, xy_range_mask=True)
    assert lvl1.prefix_partial
    cases.append((lvl1, lvl1, K3, S1, P1))
    cases.append((lvl1, lvl1.downsample(K3, (2, 2, 2), (1, 1, 1)), K3, (2, 2, 2), (1, 1, 1)))
    for src, dst, k, s, p in cases:
        plain = src.neighbors_to(dst, k, s, p)
        packed = src.neighbors_to(dst, k, s, p, packed=True)
        assert packed.packed and tuple(packed.shape) == (9, plain.shape[1]) and packed.kvol == 27
        m = dst.num_active()
        assert torch.equal(ops.unpack_table(packed)[:, :m], plain.words[:, :m])
        assert torch.equal(packed.tile_masks, plain.tile_masks)
        assert ops.table_pairs(packed, m) == ops.table_pairs(plain, m) == int((plain.words[:, :m] >= 0).sum().item())
        for cin, cout in ((16, 16), (16, 32), (32, 32)):
            w = ops.pack_weight_split(_t((rng.standard_normal((27, cin, cout)) / np.sqrt(cin * 8)).astype(np.float32), device), mid)
            scale, shift = _t(rng.uniform(0.5, 1.5, cout).astype(np.float32), device), _t(rng.standard_normal(cout).astype(np.float32) * 0.1, device)
            x = ops.pair16_from_f32(_t(rng.standard_normal((src.cap, cin)).astype(np.float32), device), cin, mid)
            res = ops.pair16_from_f32(_t(rng.standard_normal((dst.cap, cout)).astype(np.float32), device), cout, mid)
            for r in (None, res):
                a = ops.spconv_forward(x, plain, dst, w, scale, shift, r, relu=True, in_level=src, math=mid)
                b = ops.spconv_forward(x, packed, dst, w, scale, shift, r, relu=True, in_level=src, math=mid)
                assert torch.equal(a[:m].view(torch.int32), b[:m].view(torch.int32)), (cin, cout, s, r is not None)
    # windows the packed form does not cover come back plain
    odd = lvl.neighbors_to(lvl.downsample((3, 1, 1), (2, 1, 1), (0, 0, 0)), (3, 1, 1), (2, 1, 1), (0, 0, 0), packed=True)
    assert not getattr(odd, 'packed', False) and odd.shape[0] == 3
    with pytest.raises(Exception):
        ops.spconv_forward(ops.pair16_to_f32(x, mid)[:, :16].contiguous(), packed, dst, torch.zeros((27, 16, 16), device=x.device),
                           None, None, math=0)


def test_sparse_to_bev_split(device):
    from detzero_amd import ops
    from oracle import sparse as osp
    rng = np.random.default_rng(3)
    shape = [2, 30, 31]
    n = 500
    lin = rng.choice(2 * shape[0] * shape[1] * shape[2], size=n, replace=False)
    cells = shape[0] * shape[1] * shape[2]
    coords = np.stack([lin // cells, (lin % cells) // (30 * 31), (lin // 31) % 30, lin % 31], 1).astype(np.int32)
    coords = coords[osp.canonical_order(coords, shape)]
    feats = rng.standard_normal((n, 128)).astype(np.float32)
    lvl = ops.SparseLevel(2, shape, n, device)
    lvl.build_from_coords(_t(coords, device), want_rank=False)
    fp = ops.pair16_from_f32(_t(feats, device), 128, 1)
    bev = ops.sparse_to_bev(fp, lvl, 128, pad=1, math=1)
    plain = ops.pair16_to_f32(bev, 1)
    ref = osp.to_bev(ops.pair16_to_f32(fp, 1).cpu(), coords, shape, 2)         # the halves are moved, not re-rounded
    assert torch.equal(plain[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).cpu(), ref)
    assert float(plain[:, 0].abs().max()) == 0 and float(plain[:, :, -1].abs().max()) == 0
    # the two-slab level goes through the dense writer (every byte of the image, zeros included, from the level's index): the
    # same bits as zero-fill + scatter, into a buffer that held garbage, and in the brick key layout
    dirty = torch.full_like(bev, float('nan'))
    assert torch.equal(ops.sparse_to_bev(fp, lvl, 128, pad=1, out=dirty, math=1).view(torch.int32), bev.view(torch.int32))
    ops.BEV_DENSE = False
    try:
        scat = ops.sparse_to_bev(fp, lvl, 128, pad=1, math=1)
    finally:
        ops.BEV_DENSE = True
    assert torch.equal(scat.view(torch.int32), bev.view(torch.int32))
    lvl_b = ops.SparseLevel(2, shape, n, device, layout=1)
    rank_b = lvl_b.build_from_coords(_t(coords, device))
    fp_b = torch.empty_like(fp)
    fp_b[rank_b.long()] = fp                                                    # rows in the brick order
    assert torch.equal(ops.sparse_to_bev(fp_b, lvl_b, 128, pad=1, math=1).view(torch.int32), bev.view(torch.int32))
    # a level that overflowed its row capacity (calibrated capacities): the bitmap holds all n sites, the feature buffer only the first
    # `cap` rows - the dense writer treats the dropped ranks as empty cells, like the scatter form, and reads nothing past the buffer
    # (the rows behind the capacity are a poisoned guard region here)
    cap = 300
    lvl_o = ops.SparseLevel(2, shape, cap, device)
    lvl_o.build_from_coords(_t(coords, device), want_rank=False)
    assert int(lvl_o.d_m.item()) == n > cap
    guard = torch.full((cap + 64, 128), float('nan'), device=device)
    guard[:cap] = fp[:cap]
    over = ops.sparse_to_bev(guard[:cap], lvl_o, 128, pad=1, math=1)
    assert not torch.isnan(ops.pair16_to_f32(over, 1)).any()
    ops.BEV_DENSE = False
    try:
        over_s = ops.sparse_to_bev(guard[:cap], lvl_o, 128, pad=1, math=1)
    finally:
        ops.BEV_DENSE = True
    assert torch.equal(over.view(torch.int32), over_s.view(torch.int32))


@pytest.mark.parametrize('name,mid', MODES)
def test_bev_backbone_and_head_goldens_split(device, golden_dir, name, mid):
    """The reference's own BaseBEVBackbone / CenterHead outputs (tests/golden/det_golden.npz) in the split modes."""
    from detzero_amd.config import AttrDict
    from detzero_amd.det_modules import BaseBEVBackbone
    from tests.test_gpu_kernels import _golden_head
    g = np.load(os.path.join(golden_dir, 'det_golden.npz'))
    cfg = AttrDict({'LAYER_NUMS': [2, 2], 'LAYER_STRIDES': [1, 2], 'NUM_FILTERS': [32, 64], 'UPSAMPLE_STRIDES': [1, 2],
                    'NUM_UPSAMPLE_FILTERS': [32, 32]})
    bb = BaseBEVBackbone(cfg, 32)
    sd = {k[len('bev_backbone2d.'):]: torch.from_numpy(g[k]) for k in g.files if k.startswith('bev_backbone2d.')}
    bb.load_state_dict(sd, strict=True)
    bb = bb.to(device).eval().set_math(name)
    out = bb({'spatial_features': _t(g['bev_in'], device)})['spatial_features_2d']
    torch.testing.assert_close(out.cpu(), torch.from_numpy(g['bev_out']), rtol=TOL[mid], atol=TOL[mid])
    # the 2 x 2 phases of the ConvTranspose2d deblock as ONE launch (dz_conv2d_desc.phase_groups, the default) against one launch
    # per phase: the same products in the same order -> the same bits, on a batch large enough for several pixel tiles per phase
    from detzero_amd import det_modules
    x = torch.randn((3, 32, 24, 40), generator=torch.Generator().manual_seed(7)).to(device)
    assert det_modules.FUSED_DEBLOCK_PHASES
    fused = bb({'spatial_features': x})['spatial_features_2d'].clone()
    det_modules.FUSED_DEBLOCK_PHASES = False
    try:
        single = bb({'spatial_features': x})['spatial_features_2d']
    finally:
        det_modules.FUSED_DEBLOCK_PHASES = True
    assert torch.equal(fused, single) and float(fused[:, 32:].abs().max()) > 0

    head = _golden_head(g, device).set_math(name)
    dd = head({'spatial_features_2d': _t(g['head_in'], device), 'batch_size': 2})
    pred = head.forward_ret_dict['pred_dicts'][0]
    for nm_ in ('center', 'center_z', 'dim', 'rot', 'iou', 'hm'):
        torch.testing.assert_close(pred[nm_].cpu(), torch.from_numpy(g['head_pred_' + nm_]), rtol=TOL[mid], atol=TOL[mid])
    for i, fb in enumerate(dd['final_box_dicts']):
        ref_b, ref_s = g['head_boxes_%d' % i], g['head_scores_%d' % i]
        nm, worst = match_boxes(ref_b, ref_s, fb['pred_boxes'].cpu().numpy(), fb['pred_scores'].cpu().numpy(), tol=1e-3)
        assert abs(fb['pred_boxes'].shape[0] - ref_b.shape[0]) <= 1 and nm >= ref_b.shape[0] - 1, (nm, ref_b.shape[0], worst)


@pytest.mark.parametrize('name,mid', MODES)
def test_sparse_input_convolution_equals_the_dense_image(device, name, mid):
    """HeightCompression fused into the first BEV convolution (dz_conv2d_desc.in_rowidx + dz_bev_row_index, round 5): the 3 x 3
    convolution reading a two-slab level's rows through the row-index image against the same kernel on the materialised z-major
    image - bit for bit (same products, same order); tiles at the image edge, empty tiles, a row capacity the level overflows."""
    from detzero_amd import ops
    from detzero_amd.det_modules import conv_layer
    rng = np.random.default_rng(5 + mid)
    b, shape, c, cout = 16, [2, 61, 90], 128, 128
    cells = shape[0] * shape[1] * shape[2]
    lin = np.unique(np.concatenate([i * cells + np.nonzero(rng.random(cells) < (0.3 if i % 3 else 0.002))[0] for i in range(b)]))
    coords = np.stack([lin // cells, (lin % cells) // (shape[1] * shape[2]), (lin // shape[2]) % shape[1], lin % shape[2]], 1).astype(np.int32)
    n = coords.shape[0]
    for cap in (n + 5, n - 300):                      # the second: an overflowed level - ranks past the rows read as empty cells
        lvl = ops.SparseLevel(b, shape, cap, device)
        lvl.build_from_coords(_t(coords, device), want_rank=False)
        rows = ops.pair16_from_f32(_t(rng.standard_normal((cap, c)).astype(np.float32), device), c, mid)
        idx = ops.bev_row_index(lvl, cap, pad=1)
        assert tuple(idx.shape) == (b, shape[1] + 2, shape[2] + 2, 2)
        # the index image against the coordinates themselves
        want = np.full((b, shape[1] + 2, shape[2] + 2, 2), -1, np.int64)
        keep = np.arange(n) < cap
        want[coords[keep, 0], coords[keep, 2] + 1, coords[keep, 3] + 1, coords[keep, 1]] = np.arange(n)[keep]
        assert np.array_equal(idx.cpu().numpy(), want)
        # z-major dense image from the same rows (raw 32-bit words: a pair16 row is its channels' words)
        img = torch.zeros((b, shape[1] + 2, shape[2] + 2, 2 * c), dtype=torch.float32, device=device).view(torch.int32)
        ii = idx.long()
        for z in range(2):
            sel = ii[..., z] >= 0
            img[..., z * c:(z + 1) * c][sel] = rows.view(torch.int32)[ii[..., z][sel]]
        img = img.view(torch.float32)
        w = ops.pack_weight_split(_t((rng.standard_normal((9, 2 * c, cout)) / 48).astype(np.float32), device), mid)
        scale, shift = _t(rng.uniform(0.5, 1.5, cout).astype(np.float32), device), _t((rng.standard_normal(cout) * 0.1).astype(np.float32), device)
        outs = []
        for sparse in (False, True):
            out = torch.zeros((b, shape[1] + 2, shape[2] + 2, cout), dtype=torch.float32, device=device)
            conv_layer(rows if sparse else img, (shape[1] + 2, shape[2] + 2), w, scale, shift, True, out, (shape[1] + 2, shape[2] + 2), cin=2 * c,
                       in_cstride=2 * c, ksize=3, stride=1, in_off=0, out_cstride=cout, out_d=(1, 1), ho=shape[1], wo=shape[2], batch=b, math=mid,
                       in_rowidx=idx if sparse else None, in_row_channels=c, in_rows=cap)
            outs.append(out)
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)) and float(ops.pair16_to_f32(outs[1], mid).abs().max()) > 0.1
        # ... and with the empty pixel tiles left out of the launch and filled with their constant result (the detector's route)
        lists = ops.bev_tile_list(idx, shape[1], shape[2], 6)
        # list l against the definition: a tile is skippable at layer l iff every one of its pixels is at least l + 1 pixels (Chebyshev)
        # away from any pixel holding a row
        from scipy.ndimage import distance_transform_cdt
        occ = (idx.cpu().numpy()[:, 1:-1, 1:-1, :] >= 0).any(-1)
        dist = np.stack([distance_transform_cdt(~o, metric='chessboard') if o.any() else np.full(o.shape, 99) for o in occ])
        tyn, txn = (shape[1] + 7) // 8, (shape[2] + 31) // 32
        for layer in range(1, 7):
            lst = lists[layer - 1].cpu().numpy()
            want_skip = np.array([dist[bb, ty * 8:ty * 8 + 8, tx * 32:tx * 32 + 32].min() >= layer + 1 for bb in range(b) for ty in range(tyn) for tx in range(txn)])
            assert lst[0] == (~want_skip).sum() and lst[1] == want_skip.sum(), layer
            assert np.array_equal(lst[2:2 + lst[0]], np.nonzero(~want_skip)[0]) and np.array_equal(lst[2 + lst[0]:2 + lst[0] + lst[1]], np.nonzero(want_skip)[0])
        tiles = lists[0]
        n_occ, n_emp = (int(v) for v in tiles[:2].tolist())
        ntile = b * ((shape[1] + 7) // 8) * ((shape[2] + 31) // 32)
        assert n_occ + n_emp == ntile and n_emp > ntile // 20 and n_occ > ntile // 2
        ids = tiles[2:2 + ntile].cpu().numpy()
        assert np.array_equal(np.sort(ids), np.arange(ntile)) and (np.diff(ids[:n_occ]) > 0).all() and (np.diff(ids[n_occ:]) > 0).all()
        out = torch.full((b, shape[1] + 2, shape[2] + 2, cout), float('nan'), dtype=torch.float32, device=device)
        out[:, 0], out[:, -1], out[:, :, 0], out[:, :, -1] = 0, 0, 0, 0
        conv_layer(rows, (shape[1] + 2, shape[2] + 2), w, scale, shift, True, out, (shape[1] + 2, shape[2] + 2), cin=2 * c, in_cstride=2 * c, ksize=3,
                   stride=1, in_off=0, out_cstride=cout, out_d=(1, 1), ho=shape[1], wo=shape[2], batch=b, math=mid, in_rowidx=idx, in_row_channels=c,
                   in_rows=cap, in_tiles=tiles)
        ops.bev_fill_empty_tiles(tiles, b, shape[1], shape[2], shift, True, cout, out, mid)
        assert torch.equal(out.view(torch.int32), outs[1].view(torch.int32))


@pytest.fixture(scope='module')
def small(device):
    model, cfg, info = make_model(VOXEL_SIZE_02, seed=0)
    sd = cpu_state_dict(model)
    pts = masked_frame(0, 20000)
    ref = oracle_detect(sd, pts, info)
    return model.to(device), cfg, info, pts, ref


@pytest.mark.parametrize('name,mid', MODES)
def test_end_to_end_split_boxes_within_1e3(small, device, name, mid):
    """north star: boxes within 1e-3 of the reference-semantics path - in the split modes, through the module
    path (fp32 tensors at every reference batch_dict key) and through the batched FramePipeline."""
    from detzero_amd.centerpoint import FramePipeline, set_math
    from tests.test_gpu_e2e import _batch_dict
    model, cfg, info, pts, ref = small
    try:
        set_math(model, name)
        bd = _batch_dict(model, cfg, info, pts, device)
        pred_dicts, _ = model(bd)
        rb = ref['final'][0]
        got = pred_dicts[0]
        n_ref = rb['pred_boxes'].shape[0]
        nm, worst = match_boxes(rb['pred_boxes'].numpy(), rb['pred_scores'].numpy(), got['pred_boxes'].cpu().numpy(),
                                got['pred_scores'].cpu().numpy(), tol=1e-3)
        assert abs(got['pred_boxes'].shape[0] - n_ref) <= 2 and nm >= n_ref - 2, (got['pred_boxes'].shape[0], n_ref, nm, worst)
        # intermediate tensors handed to PyTorch callers are plain fp32 and close to the oracle's
        torch.testing.assert_close(bd['spatial_features_2d'].cpu(), ref['f2d'], rtol=2e-3, atol=2e-3)
        t = bd['multi_scale_3d_features']['x_conv3']
        torch.testing.assert_close(t.features.cpu(), ref['backbone']['x_conv3'][0], rtol=2e-3, atol=2e-3)
        # batched pipeline, two frames
        pipe = FramePipeline(model, info)
        out, cnt = pipe([torch.from_numpy(pts).to(device), torch.from_numpy(masked_frame(11, 9000)).to(device)])
        n0 = int(cnt[0].item())
        b = out[0, :n0].cpu().numpy()
        nm, worst = match_boxes(rb['pred_boxes'].numpy(), rb['pred_scores'].numpy(), b[:, :7], b[:, 7], tol=1e-3)
        assert abs(n0 - n_ref) <= 2 and nm >= n_ref - 2, (n0, n_ref, nm, worst)
    finally:
        set_math(model, 'f32')


def test_full_size_split_equals_f32_pipeline(device):
    """BASELINE configs[1] (160k points, 0.1 m voxels): the f16x2 pipeline reproduces the fp32-MFMA pipeline's
    boxes within 1e-3 (the oracle needs minutes at this size; the fp32 pipeline is pinned to it at the small size)."""
    from detzero_amd.centerpoint import FramePipeline, set_math
    model, cfg, info = make_model(VOXEL_SIZE_01, seed=1)
    model = model.to(device)
    tp = torch.from_numpy(masked_frame(0, 160000)).to(device)
    o32, n32 = FramePipeline(model, info, math='f32')(tp)
    n32 = int(n32.item())
    a = o32[:n32].cpu().numpy()
    # the detector's boxes depend on the frame (gain='preserve'): fp16 pairs reproduce the fp32 engine within the north star's 1e-3, the
    # 16-bit bf16 pairs do not (opt-in mode; checked at 1e-2)
    for name, tol in (('f16x2', 1e-3), ('bf16x2', 1e-2)):
        o, n = FramePipeline(model, info, math=name)(tp)
        n = int(n.item())
        b = o[:n].cpu().numpy()
        nm, worst = match_boxes(a[:, :7], a[:, 7], b[:, :7], b[:, 7], tol=tol)
        print('full-size %s vs f32 engine: %d / %d boxes, %d matched within %.0e (worst %.2e)' % (name, n, n32, nm, tol, worst))
        assert n32 > 50 and abs(n - n32) <= 2 and nm >= n32 - 2, (name, n, n32, nm, worst)
    set_math(model, 'f32')


@pytest.mark.parametrize('name,mid', MODES)
@pytest.mark.parametrize('cin,cout,h,w,out_f32', [(64, 128, 188, 188, False), (32, 64, 122, 200, False), (64, 64, 201, 97, True)])
def test_conv3x3_resident_tile_kernel_vs_torch(device, name, mid, cin, cout, h, w, out_f32):
    """conv3x3_h.hip (image-tile-resident input, 512-thread workgroups): ragged image sizes, channel offsets inside wider
    buffers, both channel-tile widths, pair16 and fp32 outputs - against torch's fp32 conv2d."""
    import ctypes
    import torch.nn.functional as F
    from detzero_amd import lib as L, ops
    from detzero_amd.det_modules import conv_layer
    b = 4
    gen = torch.Generator().manual_seed(cin + cout + h)
    x = torch.randn((b, cin, h, w), generator=gen)
    wt = torch.randn((cout, cin, 3, 3), generator=gen) / (3.0 * cin ** 0.5)
    scale = torch.rand((cout,), generator=gen) + 0.5
    shift = torch.randn((cout,), generator=gen) * 0.1
    ref = torch.relu(F.conv2d(x, wt, None, padding=1) * scale[None, :, None, None] + shift[None, :, None, None])
    # input lives at channel offset 8 of a wider zero-bordered channel-last buffer, output at offset 16 of another
    cs_in, cs_out = cin + 24, cout + 32
    xin = torch.zeros((b, h + 2, w + 2, cs_in))
    xin[:, 1:-1, 1:-1, 8:8 + cin] = x.permute(0, 2, 3, 1)
    xin[..., :8] = 7.0; xin[..., 8 + cin:] = -3.0                       # neighbours in the buffer must not leak in
    xin_d = ops.pair16_from_f32(xin.to(device), cs_in, mid)
    w_taps = wt.permute(2, 3, 1, 0).reshape(9, cin, cout).contiguous().to(device)
    w_split = ops.pack_weight_split(w_taps, mid)
    out = torch.zeros((b, h + 2, w + 2, cs_out), dtype=torch.float32, device=device)
    kw = dict(cin=cin, in_cstride=cs_in, in_coff=8, ksize=3, stride=1, in_off=0, out_cstride=cs_out, out_coff=16, out_d=(1, 1),
              ho=h, wo=w, batch=b, g_cout=[cout])
    d = L.Conv2dDesc()          # the kernel the dispatcher must pick for this shape
    d.batch, d.ho, d.wo, d.kh, d.kw, d.stride, d.groups, d.cin, d.cout_pad = b, h, w, 3, 3, 1, 1, cin, cout
    # (fp32 output: the resident-tile kernel writes it at 32-channel tiles only - this 64-channel layer runs on k_conv2d_h)
    want = 'k_conv2d_h<' if out_f32 else 'k_conv3x3_h<'
    assert L.load().dz_conv2d_variant_split(ctypes.byref(d), 1 if out_f32 else 0).decode().startswith(want)
    conv_layer(xin_d, (h + 2, w + 2), w_split, scale.to(device), shift.to(device), True, out, (h + 2, w + 2), math=mid,
               out_f32=out_f32, **kw)
    plain = out if out_f32 else ops.pair16_to_f32(out, mid)
    got = plain[:, 1:-1, 1:-1, 16:16 + cout].permute(0, 3, 1, 2).cpu()
    torch.testing.assert_close(got, ref, rtol=TOL[mid], atol=TOL[mid])
    assert float(plain[..., :16].abs().max()) == 0 and float(plain[..., 16 + cout:].abs().max()) == 0      # nothing outside its channels
    assert float(plain[:, 0].abs().max()) == 0 and float(plain[:, :, -1].abs().max()) == 0                 # border untouched


def test_full_size_batch_split_equals_f32_pipeline(device):
    """4 full-size frames in one pass (the dense layers then run on the resident-tile 3x3 kernel): f16x2 boxes within
    1e-3 of the fp32-MFMA engine, frame by frame."""
    from detzero_amd.centerpoint import FramePipeline, set_math
    model, cfg, info = make_model(VOXEL_SIZE_01, seed=1)
    model = model.to(device)
    frames = [torch.from_numpy(masked_frame(i, 160000)).to(device) for i in range(4)]
    o32, n32 = FramePipeline(model, info, math='f32')(frames)
    o16, n16 = FramePipeline(model, info, math='f16x2')(frames)
    for i in range(4):
        a, b = o32[i, :int(n32[i])].cpu().numpy(), o16[i, :int(n16[i])].cpu().numpy()
        nm, worst = match_boxes(a[:, :7], a[:, 7], b[:, :7], b[:, 7], tol=1e-3)
        assert a.shape[0] > 50 and abs(a.shape[0] - b.shape[0]) <= 2 and nm >= a.shape[0] - 2, (i, a.shape, b.shape, nm, worst)
    set_math(model, 'f32')


# ------------------------------------------------------------------------------------------------ range safety of the fp16 pairs
def _scaled_model(device, gain, homogeneous=False):
    """Seed-0 detector whose first BatchNorm gain is multiplied by `gain`: every later layer is positively homogeneous up to
    its shifts, so all activations scale by ~gain (real checkpoints are not normalised to O(1) like the synthetic ones).
    homogeneous: every BatchNorm shift and hidden conv bias zeroed (the network is then EXACTLY homogeneous: all hidden activations are
    gain x those of the gain-1 network) and the output layers' weights divided by gain - the boxes stay those of the gain-1 network,
    so a detection can be compared at any activation scale."""
    model, cfg, info = make_model(VOXEL_SIZE_02, seed=0)
    with torch.no_grad():
        if homogeneous:
            for mod in model.modules():
                if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                    mod.bias.zero_()
                    mod.running_mean.zero_()
            for name, mod in model.named_modules():
                if getattr(mod, 'bias', None) is not None and not isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                    out_layer = name.startswith('dense_head.heads_list') and name.split('.')[-1] == '1'
                    if not out_layer:
                        mod.bias.zero_()
            for hl in model.dense_head.heads_list:
                for head in ('center', 'center_z', 'dim', 'rot', 'iou', 'hm'):
                    getattr(hl, head)[1].weight.div_(gain)
                hl.hm[1].bias.fill_(-4.0)            # (no shifts: the far field of the dense stage is zero, the bias alone is the floor)
        model.backbone3d.conv_input[1].weight.mul_(gain)
        model.backbone3d.conv_input[1].bias.mul_(gain)
    return model.to(device), info


def _stage_features(model, info, pts, math):
    from detzero_amd import ops
    from detzero_amd.centerpoint import FramePipeline
    pipe = FramePipeline(model, info, math=math)
    res = pipe.backbone_stage(pipe.prepare([pts]))
    mid = ops.math_id(math)
    out = {}
    for name, (feats, lvl) in res.items():
        m = lvl.num_active()
        out[name] = ops.level_rows_f32(feats[:m], lvl, mid).clone()        # (pair16 decoded, the level's power-of-two pre-scale removed)
    return out


def _boxes(model, info, pts, math):
    from detzero_amd.centerpoint import FramePipeline
    o, n = FramePipeline(model, info, math=math)(pts)
    return o[:int(n.item())].cpu().numpy()


@pytest.mark.parametrize('gain', [1.0, 3.0e4, 1.0e6, 2.0 ** -10, 2.0 ** -20], ids=['1', '3e4', '1e6', '2^-10', '2^-20'])
def test_select_math_keeps_fp16_pairs_at_any_activation_scale(device, gain):
    """Round-5 review, item 2a: instead of falling back to bf16 pairs (16 bits) when a checkpoint's activations leave [2^-6, 3e4],
    select_math installs an exact per-stage power-of-two pre-scale.  On a detector whose hidden activations are `gain` x those of the
    gain-1 detector (and whose boxes are the same): f16x2 is retained, every sparse stage stays within 2e-5 of its peak of the exact-fp32
    engine, and the final boxes within the north star's 1e-3 - at activations of 1e8 (fp16 tops out at 65504) as at 1e-6."""
    from detzero_amd.centerpoint import F16_PAIR_TARGET_PEAK, select_math, set_math
    model, info = _scaled_model(device, gain, homogeneous=True)
    pts = torch.from_numpy(masked_frame(0, 20000)).to(device)
    mode, rng = select_math(model, info, [pts])
    assert mode == 'f16x2', (mode, rng)
    for k, e in model.prescale.items():
        assert F16_PAIR_TARGET_PEAK / 2 < rng[k] * 2.0 ** e <= F16_PAIR_TARGET_PEAK, (k, rng[k], e)
    ref = _stage_features(model, info, pts, 'f32')
    got = _stage_features(model, info, pts, 'f16x2')
    worst = 0.0
    for name in ref:
        scale = float(ref[name].abs().max())
        err = float((got[name] - ref[name]).abs().max()) / scale
        worst = max(worst, err)
        assert err < 2e-5, (name, err, scale)
    a, b = _boxes(model, info, pts, 'f32'), _boxes(model, info, pts, 'f16x2')
    nm, wbox = match_boxes(a[:, :7], a[:, 7], b[:, :7], b[:, 7], tol=1e-3)
    print('gain %.3g: peaks %s -> exponents %s; stages within %.2e of their peak; %d / %d boxes of the f32 engine matched within 1e-3 (worst %.2e)'
          % (gain, {k: float('%.3g' % v) for k, v in rng.items()}, model.prescale, worst, nm, a.shape[0], wbox))
    assert a.shape[0] > 50 and abs(a.shape[0] - b.shape[0]) <= 2 and nm >= a.shape[0] - 2, (a.shape, b.shape, nm, wbox)
    set_math(model, 'f32')


@pytest.mark.parametrize('gain', [3.0e4, 2.0 ** -20], ids=['3e4', '2^-20'])
def test_unscaled_fp16_pairs_fail_where_the_prescale_holds(device, gain):
    """What the pre-scale prevents: the same detectors on fp16 pairs WITHOUT it - saturated at gain 3e4 (stage errors of the order of the
    activations themselves), and at gain 2^-20 far less accurate than with it (the lo halves are subnormal: an absolute quantum of 2^-24
    against activations of 1e-5)."""
    from detzero_amd.centerpoint import select_math, set_math, set_prescale
    model, info = _scaled_model(device, gain, homogeneous=True)
    pts = torch.from_numpy(masked_frame(0, 20000)).to(device)
    select_math(model, info, [pts])
    ref = _stage_features(model, info, pts, 'f32')
    good = _stage_features(model, info, pts, 'f16x2')
    set_prescale(model, None)
    bad = _stage_features(model, info, pts, 'f16x2')
    rel = lambda t: max(float((t[n] - ref[n]).abs().max()) / float(ref[n].abs().max()) for n in ref)      # noqa: E731
    print('gain %.3g: worst stage error relative to its peak: %.2e with the pre-scale, %.2e without' % (gain, rel(good), rel(bad)))
    assert rel(good) < 2e-5 and rel(bad) > 50.0 * rel(good)
    if gain > 1:
        assert rel(bad) > 1e-2
    set_math(model, 'f32')


@pytest.mark.parametrize('gain', [300.0, 3.0e4])
def test_prescale_on_a_network_with_shifts(device, gain):
    """The gain on the first BatchNorm only, every shift in place (not homogeneous: the later stages grow by less than `gain`, each
    stage gets its own exponent): stage features of f16x2 + pre-scale within 2e-5 of each stage's peak of the fp32 engine."""
    from detzero_amd.centerpoint import select_math, set_math
    model, info = _scaled_model(device, gain)
    pts = torch.from_numpy(masked_frame(0, 20000)).to(device)
    mode, rng = select_math(model, info, [pts])
    assert mode == 'f16x2' and max(rng.values()) > 1e3
    ref = _stage_features(model, info, pts, 'f32')
    got = _stage_features(model, info, pts, mode)
    for name in ref:
        scale = float(ref[name].abs().max())
        err = float((got[name] - ref[name]).abs().max()) / scale
        assert err < 2e-5, (name, err, scale)
    set_math(model, 'f32')


@pytest.mark.parametrize('name,mid', MODES)
@pytest.mark.parametrize('cin,cout,groups,length,relu,shift_rows', [(128, 512, 6, 4096, True, False), (128, 256, 37, 256, True, False),
                                                                   (32, 128, 5, 384, False, True), (128, 512, 3, 9600, True, True)])
def test_linear_with_fused_group_max(device, name, mid, cin, cout, groups, length, relu, shift_rows):
    """dz_linear_forward_split(group_max): the max over each object's points taken in the layer's epilogue (integer atomics on the
    fp32 bits) equals dz_group_max over the layer's fp32 output BIT FOR BIT - with and without ReLU (negative maxima), with the
    per-object addend of the PointNet concat, for the GRM (4096), PRM query (256) and PRM memory (9600) group lengths."""
    from detzero_amd import ops
    rng = np.random.default_rng(cin + cout + groups)
    rows = groups * length
    x = ops.pair16_from_f32(_t(rng.standard_normal((rows, cin)).astype(np.float32), device), cin, mid)
    w = ops.pack_weight_split(_t((rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32), device), mid)
    scale = _t(rng.uniform(0.5, 1.5, w.shape[0]).astype(np.float32), device)
    shift = _t((rng.standard_normal(w.shape[0]) - (0.0 if relu else 12.0)).astype(np.float32), device)       # relu off: every maximum negative
    gs = _t(rng.standard_normal((groups, w.shape[0])).astype(np.float32), device) if shift_rows else None
    full = ops.linear_split(x, w, scale, shift, relu, cout, mid, out_f32=True, group_shift=gs, group_rows=length)
    want = ops.group_max(full, groups, length)
    got = ops.linear_split(x, w, scale, shift, relu, cout, mid, group_shift=gs, group_rows=length, group_max=True)
    assert tuple(got.shape) == (groups, cout) and torch.equal(got, want)
    if not relu:
        assert float(want.max()) < 0


@pytest.mark.gpu
@pytest.mark.parametrize('name,mid', [('f16x2', 1), ('bf16x2', 2)])
@pytest.mark.parametrize('cin,c3,groups,length', [(29, 256, 5, 4096), (30, 512, 37, 256), (32, 512, 3, 9600), (8, 128, 200, 32)])
def test_fused_pointnet_encoder(device, name, mid, cin, c3, groups, length):
    """dz_pointnet3_forward (three point-wise layers + max over an object's points in one kernel, the activations in registers;
    geometry_transformer.py:34-67, position_transformer.py:43-124) against (a) the same layers run one launch each through
    dz_linear_forward_split + dz_group_max and (b) float64 on the host.  The tapped second layer must be the layer-by-layer rows."""
    from detzero_amd import ops
    rng = np.random.default_rng(cin * 7 + c3 + groups)
    rows = groups * length
    xf = rng.standard_normal((rows, cin)).astype(np.float32)
    dims = [(cin, 128), (128, 128), (128, c3)]
    ws = [(rng.standard_normal(d) / np.sqrt(d[0])).astype(np.float32) for d in dims]
    ss = [rng.uniform(0.5, 1.5, d[1]).astype(np.float32) for d in dims]
    bs = [(0.3 * rng.standard_normal(d[1])).astype(np.float32) for d in dims]
    x = ops.pair16_from_f32(_t(xf, device), 32, mid)
    trip = []
    for w, s, b in zip(ws, ss, bs):
        wp = np.zeros(((w.shape[0] + 31) // 32 * 32, w.shape[1]), np.float32)
        wp[:w.shape[0]] = w
        trip.append((ops.pack_weight_split(_t(wp, device), mid), _t(s, device), _t(b, device)))
    got, tap = ops.pointnet3(x, trip, length, mid, want_tap=True)
    got2, none = ops.pointnet3(x, trip, length, mid)
    assert none is None and torch.equal(got, got2)
    # fp32 rows split inside the kernel: the same bits as the converted input
    cp = 16 if cin <= 16 else 32
    xpad = np.zeros((rows, cp), np.float32)
    xpad[:, :cin] = xf
    got3, tap3 = ops.pointnet3(_t(xpad, device), trip, length, mid, want_tap=True, x_f32=True)
    assert torch.equal(got3, got) and torch.equal(tap3, tap)
    h = x
    for li, (w, s, b) in enumerate(trip):
        h = ops.linear_split(h, w, s, b, True, w.shape[0], mid, out_f32=li == 2)
        if li == 1:
            tap_want = h
    want = ops.group_max(h, groups, length)
    tw, tg = ops.pair16_to_f32(tap_want, mid), ops.pair16_to_f32(tap, mid)
    e_tap = float((tw - tg).abs().max())
    e_pool = float((want - got).abs().max())
    ref = xf.astype(np.float64)
    for w, s, b in zip(ws, ss, bs):
        ref = np.maximum(ref @ w.astype(np.float64) * s + b, 0.0)
    ref = ref.reshape(groups, length, c3).max(1)
    e_ref = float(np.abs(got.cpu().numpy() - ref).max())
    tol = 2e-5 if mid == 1 else 2e-4
    print('pointnet3 %s cin %d c3 %d: |tap - layered| %.2e, |pool - layered| %.2e, |pool - f64| %.2e' % (name, cin, c3, e_tap, e_pool, e_ref))
    assert tuple(got.shape) == (groups, c3)
    assert e_tap <= tol and e_pool <= tol and e_ref <= 10 * tol


@pytest.mark.gpu
@pytest.mark.parametrize('name,mid', [('f16x2', 1), ('bf16x2', 2)])
@pytest.mark.parametrize('groups,length,kv', [(3, 4096, False), (2, 9600, True), (37, 32, True), (1, 160, False)])
def test_fused_memory_chain(device, name, mid, groups, length, kv):
    """dz_mlp_chain_forward (128 -> 512 with the per-object addend -> 256, then the key / value projections, one kernel, the 512-wide
    hidden layer never leaving the registers; geometry_transformer.py:56-67, position_transformer.py:60-72, multi_head_attention.py:
    199-236) against the same layers run one dz_linear_forward_split each: the same products in the same order -> the same bits."""
    from detzero_amd import ops
    rng = np.random.default_rng(groups * 31 + length)
    rows = groups * length
    x = ops.pair16_from_f32(_t(np.maximum(rng.standard_normal((rows, 128)), 0).astype(np.float32), device), 128, mid)
    dims = [(128, 512), (512, 256), (256, 256), (256, 256)]
    ws = [ops.pack_weight_split(_t((rng.standard_normal(d) / np.sqrt(d[0])).astype(np.float32), device), mid) for d in dims]
    sc = [_t(rng.uniform(0.5, 1.5, d[1]).astype(np.float32), device) for d in dims[:2]]
    sh = [_t((0.3 * rng.standard_normal(d[1])).astype(np.float32), device) for d in dims]
    gs = _t(rng.standard_normal((groups, 512)).astype(np.float32), device)
    one = torch.ones(256, device=device)
    res = ops.mlp_chain(x, (ws[0], sc[0], sh[0]), (ws[1], sc[1], sh[1]), gs, length, mid, kv=(ws[2], sh[2], ws[3], sh[3]) if kv else None)
    mem = res[0] if kv else res
    h = ops.linear_split(x, ws[0], sc[0], sh[0], True, 512, mid, group_shift=gs, group_rows=length)
    want = ops.linear_split(h, ws[1], sc[1], sh[1], True, 256, mid, out_f32=True)
    assert tuple(mem.shape) == (rows, 256) and torch.equal(mem, want), float((mem - want).abs().max())
    if kv:
        mp = ops.pair16_from_f32(want, 256, mid)
        for got, w, b in ((res[1], ws[2], sh[2]), (res[2], ws[3], sh[3])):
            assert torch.equal(got, ops.linear_split(mp, w, one, b, False, 256, mid, out_f32=True))
    # and against float64 on the host (the split arithmetic itself)
    xf = ops.pair16_to_f32(x, mid).cpu().numpy().astype(np.float64)[:64]
    wf = [ops.pair16_to_f32(w, mid).cpu().numpy().astype(np.float64) for w in ws[:2]]
    hh = np.maximum((xf @ wf[0].T + gs.cpu().numpy()[np.arange(64) // length]) * sc[0].cpu().numpy() + sh[0].cpu().numpy(), 0)
    mm = np.maximum((hh @ wf[1].T) * sc[1].cpu().numpy() + sh[1].cpu().numpy(), 0)
    err = float(np.abs(mem[:64].cpu().numpy() - mm).max())
    print('memory chain %s %d x %d: bit-identical to the layered path; |mem - f64| %.2e' % (name, groups, length, err))
    assert err <= (3e-5 if mid == 1 else 2e-4)                     # observed 2.9e-6 / 2.0e-5
