"""GPU (MI355X): the head's regression branches at the top-K cells only (csrc/head_cand.hip, FramePipeline.head_at_candidates).

The kernel keeps the dense kernels' accumulation order per output value (32-channel chunks outermost, nine taps inside, two 16-deep
MFMA steps, lo.hi + hi.lo + hi.hi), the same MFMA shape and lane -> k assignment and the same roundings of the hidden layer, so the
criterion at both levels is bit identity with the full-map route (`torch.equal`):
  kernel level    columns 0:8 of CenterHead.run_head on the same shared map at the listed cells; every other word of a
                  sentinel-filled head map untouched;
  pipeline level  counts and boxes of FramePipeline with and without `head_at_candidates`.
Served modes: f16x2, bf16x2 and f16 (one pair16 template) and f32 (v_mfma_f32_16x16x4_f32 in k_conv2d's order: taps outermost).
Heads whose shared width is not 64 keep the full-map route."""
import contextlib

import pytest
import torch

from detzero_amd import ops
from detzero_amd.synth import VOXEL_SIZE_02
from tests.util import masked_frame

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
MODES = ['f16x2', 'f32', 'bf16x2', 'f16']


def _detector(channels=64, names=('Vehicle', 'Pedestrian', 'Cyclist'), seed=0):
    """tests.util.make_model's small detector (0.2 m voxels, randomised BatchNorm, variance-preserving weights) with the head's shared
    width and class list open."""
    import torch.nn as nn
    from detzero_amd.centerpoint import SyntheticDatasetInfo, build_network
    from detzero_amd.config import centerpoint_1sweep_cfg
    from detzero_amd.synth_weights import variance_preserving_init
    cfg = centerpoint_1sweep_cfg(tuple(VOXEL_SIZE_02))
    cfg.CLASS_NAMES = list(names)
    cfg.MODEL.DENSE_HEAD.CLASS_NAMES_EACH_HEAD = [list(names)]
    cfg.MODEL.DENSE_HEAD.SHARED_CONV_CHANNEL = channels
    info = SyntheticDatasetInfo(cfg, num_point_features=5)
    torch.manual_seed(seed)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), info).eval()
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=gen) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=gen) + 0.5)
                m.weight.data.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                m.bias.data.copy_(torch.randn(m.bias.shape, generator=gen) * 0.1)
        variance_preserving_init(model, seed)
    return model, info


@pytest.fixture(scope='module')
def det(device):
    model, info = _detector()
    return model.to(device), info


@pytest.fixture(scope='module')
def frames(device):
    return [torch.from_numpy(masked_frame(20 + i, 9000 + 500 * i)).to(device) for i in range(5)]


def _shared_map(b, h, w, mode, device, seed=1):
    g = torch.Generator().manual_seed(seed)
    img = torch.zeros((b, h + 2, w + 2, 64))
    img[:, 1:-1, 1:-1] = torch.rand((b, h, w, 64), generator=g) * 2.0          # (the shared conv ends in a ReLU: values >= 0)
    return ops.pair16_from_f32(img.to(device), math=ops.math_id(mode)) if ops.math_id(mode) else img.to(device)


@contextlib.contextmanager
def _iou_weight(head, value):
    """The head with another IOU_WEIGHT (0: the score ignores the iou branch, which then is not computed densely either)."""
    saved = head.iou_weight
    head.iou_weight = value
    head.invalidate()
    try:
        yield head
    finally:
        head.iou_weight = saved
        head.invalidate()


def _pack_candidates(flat, scores):
    """Candidate words as dz_centerhead_select writes them: score bits << 32 | ~(cls * HW + pix)."""
    bits = scores.float().contiguous().view(torch.int32).to(torch.int64)
    return (bits << 32) | (0xFFFFFFFF - flat.to(torch.int64))


# ------------------------------------------------------------------------------------------------ kernel level
H, W, K = 12, 20, 128


def _cells():
    """Per frame: (list of (cls, y, x) in list order, count).  Entries past the count are valid cells that must be left alone."""
    f0 = [(0, 0, 0), (1, 0, W - 1), (2, H - 1, 0), (0, H - 1, W - 1),                                  # the four corners
          (0, 0, 7), (1, H - 1, 9), (2, 5, 0), (0, 6, W - 1),                                         # a cell on each edge
          (0, 5, 5), (1, 6, 11), (2, 3, 17), (0, 10, 2),                                              # interior
          (1, 5, 5), (2, 5, 5),                                                                       # the pixel (5, 5) again, other classes
          (0, 1, 1), (0, 2, 2)]                                                                       # beyond the count (14)
    f1 = [(0, 4, 4), (1, 7, 13), (2, 0, 0)]                                                            # count 0
    g = torch.Generator().manual_seed(7)
    pix = torch.randperm(H * W, generator=g)[:80].tolist()                                             # 70 counted: three blocks, the last ragged
    f2 = [(i % 3, p // W, p % W) for i, p in enumerate(pix)]
    return [(f0, 14), (f1, 0), (f2, 70)]


def _cand_tensors(cells, device):
    cand = torch.zeros((len(cells), ops.CAND_STRIDE), dtype=torch.int64)
    for b, (lst, _) in enumerate(cells):
        flat = torch.tensor([c * H * W + y * W + x for c, y, x in lst], dtype=torch.int64)
        score = torch.linspace(0.9, 0.1, len(lst))
        cand[b, :len(lst)] = _pack_candidates(flat, score)
    ncand = torch.tensor([n for _, n in cells], dtype=torch.int32)
    return cand.to(device), ncand.to(device)


@pytest.mark.parametrize('mode', MODES)
def test_listed_cells_equal_the_full_map_and_nothing_else_is_written(det, device, mode):
    model, _ = det
    head = model.dense_head.set_math(mode)
    assert head.at_candidates_ok()
    shared = _shared_map(3, H, W, mode, device)
    full, h, w = head.run_head(shared, 3)
    assert (h, w) == (H, W)
    cells = _cells()
    cand, ncand = _cand_tensors(cells, device)
    got = torch.full((3, H * W, 12), SENTINEL, dtype=torch.float32, device=device)
    head.regress_at_candidates(shared, got, cand, ncand, K)
    torch.cuda.synchronize()
    listed = torch.zeros((3, H * W), dtype=torch.bool)
    for b, (lst, n) in enumerate(cells):
        for _, y, x in lst[:n]:
            listed[b, y * W + x] = True
    listed = listed.to(device)
    assert int(listed.sum()) == 12 + 70
    assert torch.isfinite(full[..., :8]).all()
    assert torch.equal(got[..., :8][listed], full[..., :8][listed])
    assert bool((got[..., :8][~listed] == SENTINEL).all())
    assert bool((got[..., 8:] == SENTINEL).all())


def test_more_candidates_than_cells(det, device):
    """4 x 4 map, K = 64 > ncls * HW = 48: the selection lists every (class, cell) pair, every cell several times."""
    model, _ = det
    head = model.dense_head.set_math('f16x2')
    shared = _shared_map(2, 4, 4, 'f16x2', device, seed=3)
    full, h, w = head.run_head(shared, 2)
    ws, cand, ncand = ops.centerhead_select(full, 4, 4, 3, 64, use_iou=True)
    assert ncand.tolist() == [48, 48]
    got = torch.full_like(full, SENTINEL)
    head.regress_at_candidates(shared, got, cand, ncand, 64)
    assert torch.equal(got[..., :8], full[..., :8])
    assert bool((got[..., 8:] == SENTINEL).all())


@pytest.mark.parametrize('iou_weight', [1, 0])
def test_score_head_writes_the_selection_columns_only(det, device, iou_weight):
    """run_score_head: columns 8:12 as run_head writes them, bit for bit (channel / group slices of the same layers); with
    IOU_WEIGHT = 0 the hm branch alone (64 -> 64, one group): columns 9:12, column 8 is not written."""
    model, _ = det
    with _iou_weight(model.dense_head.set_math('f16x2'), iou_weight) as head:
        shared = _shared_map(3, H, W, 'f16x2', device)
        full, _, _ = head.run_head(shared, 3)
        part, h, w = head.run_score_head(shared, 3)
        first = 8 if iou_weight else 9
        assert head.plan()['heads'][0]['first_score_group'] == first - 4
        assert (h, w) == (H, W) and torch.equal(part[..., first:], full[..., first:])


# ------------------------------------------------------------------------------------------------ pipeline level
def _pipes(model, info, mode='f16x2'):
    from detzero_amd.centerpoint import FramePipeline
    new = FramePipeline(model, info, math=mode)
    old = FramePipeline(model, info, math=mode)
    old.head_at_candidates = False
    assert new.head_at_candidates
    return new, old


def _same(a, b):
    (out, cnt), (out2, cnt2) = a, b
    assert torch.equal(cnt, cnt2)
    for i in range(cnt.shape[0]):
        n = int(cnt[i])
        assert torch.equal(out[i, :n], out2[i, :n])
    return cnt


def _count_calls(monkeypatch):
    calls = []
    real = ops.head_at_candidates
    monkeypatch.setattr(ops, 'head_at_candidates', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize('mode,group,iou_weight', [('f16x2', 16, 1), ('f16x2', 2, 1), ('f32', 2, 1), ('f16x2', 2, 0)])
def test_pipeline_equals_full_map_route(det, frames, device, monkeypatch, mode, group, iou_weight):
    """One group, and dense_group = 2 over 5 frames (a ragged last group: the shared maps of all groups in one image); IOU_WEIGHT = 0:
    the selection must not read column 8, which no layer writes then."""
    model, info = det
    calls = _count_calls(monkeypatch)
    with _iou_weight(model.dense_head, iou_weight):
        new, old = _pipes(model, info, mode)
        new.dense_group = old.dense_group = group
        got = new(frames)
        assert len(calls) == 1
        ref = old(frames)
        assert len(calls) == 1                     # (the knob selects the full-map route)
        cnt = _same(got, ref)
        assert int(cnt.min()) > 0


def test_post_stage_refuses_a_copy_of_the_partial_map(det, frames, device):
    """Columns 0:8 of dense_stage's map exist only at the cells post_stage fills: a copy of it is not decodable and is refused."""
    from detzero_amd.lib import DetZeroHipError
    model, info = det
    new, _ = _pipes(model, info)
    head, h, w = new.dense_stage(new.backbone_stage(new.prepare(frames[:1])), 1)
    with pytest.raises(DetZeroHipError, match='head_at_candidates'):
        new.post_stage(head.clone(), h, w)
    out, cnt = new.post_stage(head, h, w)
    assert int(cnt.min()) > 0


def test_pipeline_graph_replayed_on_other_inputs(det, frames, device):
    model, info = det
    new, old = _pipes(model, info)
    n = min(f.shape[0] for f in frames[:4])
    a = torch.stack([f[:n] for f in frames[:2]])
    b = torch.stack([f[:n] for f in frames[2:4]])
    static = a.clone()
    new(static)                                # eager first: packed weights, workspace images
    torch.cuda.synchronize()
    cap = new.capture(static)
    for inp in (a, b, a):
        static.copy_(inp)
        cap.replay()
        torch.cuda.synchronize()
        cnt = _same((cap.boxes, cap.counts), old(inp))
        assert int(cnt.min()) > 0


def test_single_class_head(frames, device, monkeypatch):
    model, info = _detector(names=('Vehicle',))
    calls = _count_calls(monkeypatch)
    new, old = _pipes(model.to(device), info)
    cnt = _same(new(frames[:2]), old(frames[:2]))
    assert len(calls) == 1 and int(cnt.sum()) > 0


def test_other_shared_width_keeps_the_full_map_route(frames, device, monkeypatch):
    calls = _count_calls(monkeypatch)
    model32, info32 = _detector(channels=32)
    assert not model32.dense_head.set_math('f16x2').at_candidates_ok()
    new, old = _pipes(model32.to(device), info32)
    _same(new(frames[:1]), old(frames[:1]))
    assert not calls
