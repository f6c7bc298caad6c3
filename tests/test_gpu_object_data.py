"""GPU: the object-data stage end to end on the fixture of the reference's outputs (tests/golden/object_data_golden.npz) with the device
ops: every discrete field and every kept index set of every pickle exactly, the rows equal to the host-prepared rows at those indices;
pack_sequence against PackedTracks of the written pickles; the IoU labels within the 3-D IoU bound of tests/test_gpu_traj_pair.py."""
import logging
import os
import pickle

import numpy as np
import pytest
import torch

from detzero_amd import object_data, object_features as OF, refine_combine
from tests.test_object_data import check_against_reference, load_golden, run_prepare

IOU3D_BOUND = 2e-5            # DESIGN.md 7k / tests/test_gpu_traj_pair.py: float32 3-D IoU of two implementations of the same formulas


@pytest.fixture(scope='module')
def gold():
    return load_golden()


@pytest.mark.gpu
@pytest.mark.parametrize('split,bev', [('val', False), ('val', True), ('test', False), ('test', True)])
def test_prepare_on_the_device_equals_the_reference(device, gold, tmp_path, split, bev):
    out, prep = run_prepare(gold, split, bev, tmp_path, device=device)
    assert check_against_reference(gold, split, bev, out, prep) > 1000


@pytest.mark.gpu
def test_frame_groups_do_not_change_the_files(device, gold, tmp_path):
    points = {e['name']: e['points'] for e in gold['sequences']}
    files = []
    for budget in (256 << 20, 1):
        root = tmp_path / str(budget)
        prep = object_data.WaymoObjectDataPrepare(gold['class_names'], root_path=str(root), split='val', points_loader=lambda s, f: points[s][f],
                                                  device=device, budget_bytes=budget)
        e = gold['sequences'][0]
        prep.prepare_data_worker({e['name']: e['assign']})
        files.append([open(os.path.join(str(root), 'refining', cn, '%s.pkl' % e['name']), 'rb').read() for cn in gold['class_names']])
    assert files[0] == files[1]


@pytest.mark.gpu
def test_pack_sequence_equals_packed_tracks_of_the_pickles(device, gold, tmp_path):
    out, _ = run_prepare(gold, 'test', False, tmp_path, device=device)
    e = gold['sequences'][0]
    packed, infos = object_data.pack_sequence(e['name'], e['tracks'], gold['class_names'], split='test',
                                              points_loader=lambda s, f: e['points'][f], device=device)
    tracks = [o for cn in gold['class_names'] for o in out[cn][e['name']].values()]
    host = OF.PackedTracks(tracks, device)
    assert [(o['name'], o['obj_id']) for o in infos] == [(o['name'], o['obj_id']) for o in tracks] and all('pts' in o and not o['pts'] for o in infos)
    assert (packed.batch, packed.counts, packed.box_num, packed.classes) == (host.batch, host.counts, host.box_num, host.classes)
    for k in ('pts', 'box_offsets', 'traj', 'score', 'obj_box_offsets', 'obj_cls'):
        a, b = getattr(packed, k), getattr(host, k)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), k
    a, b = OF.prm_features(packed, rng=OF.DeviceDraw(3)), OF.prm_features(host, rng=OF.DeviceDraw(3))
    assert all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k]))


@pytest.mark.gpu
def test_iou_labels_on_the_device(device, gold, tmp_path):
    worst, n = 0.0, 0
    for cn in gold['class_names']:
        geo, pos = os.path.join(str(tmp_path), '%s_geometry_train.pkl' % cn), os.path.join(str(tmp_path), '%s_position_train.pkl' % cn)
        for path, kind in ((geo, 'geo'), (pos, 'pos')):
            with open(path, 'wb') as f:
                pickle.dump(gold['refine'][cn][kind], f)
        refine_combine.generate_refine_boxes_iou(cn, geo, pos, str(tmp_path), logging.getLogger('test'))
        with open(os.path.join(str(tmp_path), '%s_iou_train.pkl' % cn), 'rb') as f:
            mine = pickle.load(f)
        want = gold['iou'][cn]
        assert list(mine.keys()) == list(want.keys())
        for seq in want:
            assert list(mine[seq].keys()) == list(want[seq].keys())
            for obj in want[seq]:
                a, b = mine[seq][obj], want[seq][obj]
                assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
                worst = max(worst, float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))))
                n += len(a)
    print('  IoU labels: %d boxes, largest difference to the reference %.3e (bound %.0e)' % (n, worst, IOU3D_BOUND))
    assert n > 100 and worst <= IOU3D_BOUND
