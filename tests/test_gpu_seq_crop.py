"""GPU: the sequence crop (dz_seq_crop_count / dz_seq_crop_fill, ops.seq_crop, object_crop.crop_sequence) against the per-frame oracle
(oracle.crop.crop_frame_objects) and the existing one-frame crop on the device (object_crop.crop_objects): rows, order and offsets bit
for bit, for payloads of 8 words (the float64 point rows) and of 1 word, on the shapes of tests/seq_crop_cases.py - one point, 63 / 64 /
65 boxes around the LDS staging round, points at the chunk's edges, frames without boxes or points, no frame, a point kept once per
identical box, nothing kept, and one 5 x 40 x 6000 sequence.  Then ranks, PackedTracks.from_crop, the frame groups, determinism and
the wrapper's refusals."""
import numpy as np
import pytest
import torch

from detzero_amd import object_crop, object_features as OF, ops
from detzero_amd.lib import DetZeroHipError
from tests import seq_crop_cases as C

ALL = list(C.SHAPES)


def prepared(name):
    return [(object_crop.prepare_frame_points(raw, pose), boxes) for raw, pose, boxes in C.sequence(name)]


def bits(t):
    return t.contiguous().cpu().numpy().tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ALL)
def test_rows_order_and_offsets_match_oracle_and_frame_crop(device, name):
    assert ops.seq_crop_chunk_points() == C.CHUNK
    frames = prepared(name)
    res = object_crop.crop_sequence(frames, device=device, want_index=True)               # 8 payload words: (x, y, z, tanh i) float64
    want = C.expected(name)
    assert res.rows.dtype == torch.float64 and res.offsets.dtype == torch.int32 and res.n_groups <= 1
    got = res.to_lists()
    assert len(got) == len(want) == res.num_boxes and res.total == sum(w.shape[0] for w in want)
    np.testing.assert_array_equal(res.offsets.cpu().numpy(), np.concatenate([[0], np.cumsum([w.shape[0] for w in want])]).astype(np.int32))
    for g, w in zip(got, want):
        assert C.same_bytes(g, w)
    # the existing one-frame crop on the device
    k = 0
    for pts, boxes in frames:
        if boxes.shape[0]:
            for o in object_crop.crop_objects(pts, object_crop.enlarge_boxes(boxes, 1.1, False), device):
                assert C.same_bytes(o, got[k])
                k += 1
    assert k == len(got)
    # source rows: ascending within a segment, and the rows are those points
    allpts = np.concatenate([p for p, _ in frames]) if frames else np.zeros((0, 4))
    index = res.index.cpu().numpy()
    assert C.same_bytes(allpts[index], res.rows.cpu().numpy())
    for idx in res.index_lists():
        assert (np.diff(idx) > 0).all()
    # 1 payload word through the wrapper itself, with the index
    m = allpts.shape[0]
    n_box = [b.shape[0] for _, b in frames]
    plan = ops.seq_crop_plan(np.concatenate([[0], np.cumsum([p.shape[0] for p, _ in frames])]).astype(np.int64),
                             np.concatenate([[0], np.cumsum(n_box)]).astype(np.int64), None, m, sum(n_box))
    word = np.random.default_rng(1).integers(-2 ** 31, 2 ** 31, (m, 1), dtype=np.int64).astype(np.int32)
    boxes = np.concatenate([object_crop.enlarge_boxes(b, 1.1, False) for _, b in frames]) if frames else np.zeros((0, 7))
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(device).contiguous()
    out, idx, seg_off, total = ops.seq_crop(up(allpts[:, :3], torch.float32), up(boxes, torch.float32), up(word, torch.int32), plan, want_index=True)
    assert total == res.total and out.shape == (total, 1)
    assert np.array_equal(idx.cpu().numpy(), index) and np.array_equal(out.cpu().numpy(), word[index])
    assert bits(seg_off) == bits(res.offsets)
    print('  %s: %d boxes, %d points, %d rows kept' % (name, len(want), m, res.total))


@pytest.mark.gpu
def test_crop_on_bev_and_scale(device):
    frames = prepared('boxes63_64_65')
    for scale, bev in ((1.0, False), (1.3, True)):
        got = object_crop.crop_sequence(frames, enlarge_scale=scale, crop_on_bev=bev, device=device).to_lists()
        for g, w in zip(got, C.expected('boxes63_64_65', scale, bev)):
            assert C.same_bytes(g, w)


@pytest.mark.gpu
def test_ranks_permute_the_segments(device):
    name = 'tracks6'
    frames = prepared(name)
    want = C.expected(name)
    nb = len(want)
    obj_rank, _ = C.object_major([t for t, _ in C.SHAPES[name][0]])
    shuffled = np.random.default_rng(3).permutation(nb)
    for rank in (np.arange(nb), np.arange(nb)[::-1].copy(), obj_rank, shuffled, shuffled.astype(np.int32)):
        res = object_crop.crop_sequence(frames, order=rank, device=device)
        got = res.to_lists()
        assert res.total == sum(w.shape[0] for w in want)
        for b in range(nb):
            assert C.same_bytes(got[rank[b]], want[b])


@pytest.mark.gpu
def test_packed_tracks_from_crop(device):
    """PackedTracks.from_crop(object-major crop) == PackedTracks(host tracks) tensor for tensor, and the GRM / PRM inputs made of them
    are bit-equal under one DeviceDraw seed."""
    name = 'tracks6'
    frames, spec = prepared(name), [t for t, _ in C.SHAPES[name][0]]
    want = C.expected(name)
    rank, per_obj = C.object_major(spec)
    start = np.concatenate([[0], np.cumsum(spec)])
    rng = np.random.default_rng(11)
    tracks = []
    for k, n in enumerate(per_obj):
        fs = [f for f, t in enumerate(spec) if t > k]
        assert len(fs) == n
        tracks.append({'boxes_global': np.stack([frames[f][1][k] for f in fs]), 'score': rng.uniform(0.1, 1, n),
                       'pts': [want[start[f] + k] for f in fs], 'name': ('Vehicle', 'Pedestrian', 'Cyclist')[k % 3]})
    host = OF.PackedTracks(tracks, device)
    crop = object_crop.crop_sequence(frames, order=rank, device=device)
    dev = OF.PackedTracks.from_crop(crop, [t['boxes_global'] for t in tracks], [t['score'] for t in tracks], [t['name'] for t in tracks])
    assert (dev.batch, dev.counts, dev.box_num, dev.obj_box_start, dev.classes) == (host.batch, host.counts, host.box_num, host.obj_box_start, host.classes)
    for k in ('pts', 'box_offsets', 'traj', 'score', 'obj_box_offsets', 'obj_cls'):
        a, b = getattr(dev, k), getattr(host, k)
        assert a.dtype == b.dtype and a.shape == b.shape and bits(a) == bits(b), k
    assert np.array_equal(dev.traj_host, host.traj_host) and all(np.array_equal(a, b) for a, b in zip(dev.scores, host.scores))
    for fn in (OF.grm_features, OF.prm_features):
        a, b = fn(dev, rng=OF.DeviceDraw(7)), fn(host, rng=OF.DeviceDraw(7))
        assert a.keys() == b.keys()
        for k in a:
            if torch.is_tensor(a[k]):
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and bits(a[k]) == bits(b[k]), (fn.__name__, k)
            else:
                assert a[k] == b[k], (fn.__name__, k)


@pytest.mark.gpu
def test_frame_groups_give_the_same_bytes(device):
    name = '5x40x6000'
    frames = prepared(name)
    rank = np.random.default_rng(5).permutation(200)
    per_frame = 6000 * 44 + 40 * 24 * 16
    for order in ('frame', rank):
        one = object_crop.crop_sequence(frames, order=order, device=device, want_index=True)
        cut = object_crop.crop_sequence(frames, order=order, device=device, want_index=True, budget_bytes=2 * per_frame + 1000)
        assert one.n_groups == 1 and cut.n_groups == 3
        assert bits(one.rows) == bits(cut.rows) and bits(one.offsets) == bits(cut.offsets) and bits(one.index) == bits(cut.index)


@pytest.mark.gpu
def test_two_runs_give_the_same_bytes(device):
    frames = prepared('5x40x6000')
    a = object_crop.crop_sequence(frames, device=device, want_index=True)
    b = object_crop.crop_sequence(frames, device=device, want_index=True)
    assert a.total > 0 and bits(a.rows) == bits(b.rows) and bits(a.offsets) == bits(b.offsets) and bits(a.index) == bits(b.index)


@pytest.mark.gpu
def test_wrapper_refusals_launch_nothing(device, monkeypatch):
    from detzero_amd import lib as L
    lib = L.load()
    calls = []
    frames = prepared('frame_without_boxes')
    pts = np.concatenate([p for p, _ in frames])
    m = pts.shape[0]
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(device).contiguous()
    xyz, boxes, payload = up(pts[:, :3], torch.float32), up(np.concatenate([b for _, b in frames]), torch.float32), up(pts, torch.float64)

    class Spy:
        def __getattr__(self, k):
            if k in ('dz_seq_crop_count', 'dz_seq_crop_fill'):
                calls.append(k)
            return getattr(lib, k)
    monkeypatch.setattr(L, 'load', lambda: Spy())
    good_p, good_b = [0, 300, 600, m], [0, 4, 4, 8]
    for what, p_off, b_off, rank in (('rank repeats an index', good_p, good_b, [0, 1, 2, 3, 4, 5, 6, 6]),
                                     ('offsets descend', [0, 600, 300, m], good_b, None), ('box offsets descend', good_p, [0, 4, 3, 8], None),
                                     ('offsets do not end at M', [0, 300, 600, m - 1], good_b, None),
                                     ('offsets do not end at B', good_p, [0, 4, 4, 7], None)):
        with pytest.raises(DetZeroHipError):
            ops.seq_crop(xyz, boxes, payload, ops.seq_crop_plan(p_off, b_off, rank, m, 8))
    plan = ops.seq_crop_plan(good_p, good_b, None, m, 8)
    for bad in ((xyz[:-1].contiguous(), boxes, payload), (xyz, boxes[:-1].contiguous(), payload), (xyz, boxes, payload[:-1].contiguous()),
                (xyz.double(), boxes, payload), (xyz, boxes, payload.view(torch.int16)[:, :5].contiguous()), (xyz.cpu(), boxes, payload)):
        with pytest.raises(DetZeroHipError):
            ops.seq_crop(*bad, plan)
    with pytest.raises(DetZeroHipError):
        ops.seq_crop(xyz, boxes, payload, (good_p, good_b))
    with pytest.raises(DetZeroHipError):
        object_crop.crop_sequence(frames, order=np.zeros(8, dtype=np.int64), device=device)
    assert calls == []
    out, _, seg_off, total = ops.seq_crop(xyz, boxes, payload, plan)                           # and the accepted call does launch
    assert calls == ['dz_seq_crop_count', 'dz_seq_crop_fill'] and total == int(seg_off[-1]) > 0
