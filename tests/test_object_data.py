"""CPU: the object-data stage (object_data.WaymoObjectDataPrepare) and the refining stage's other end (refine_combine) against the
reference's own outputs (tests/golden/object_data_golden.npz, made by gen_object_data_golden.py from daemon/prepare_object_data.py,
combine_output.py and generate_iou_gt.py).  The orchestration runs on the numpy ops of tests/crop_ref.py; every pickle must equal the
reference's: key order, Python and numpy types, dtypes, shapes, values, and the kept point index sets."""
import copy
import logging
import os
import pickle
from collections import defaultdict

import numpy as np
import pytest

from detzero_amd import object_data, refine_combine
from detzero_amd.object_crop import prepare_frame_points
from tests.crop_ref import NumpyCropOps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'object_data_golden.npz')
LOG = logging.getLogger('test_object_data')


def load_golden():
    return pickle.loads(np.load(GOLDEN)['pickle'].tobytes())


@pytest.fixture(scope='module')
def gold():
    return load_golden()


def strict_diff(a, b, path=''):
    """Path of the first difference between two nested results, or None: same types (Python and numpy), same key order, same dtypes and
    shapes, same values."""
    if type(a) is not type(b):
        return '%s: type %s against %s' % (path, type(a).__name__, type(b).__name__)
    if isinstance(a, dict):
        if list(a.keys()) != list(b.keys()) or [type(k) for k in a] != [type(k) for k in b]:
            return '%s: keys %r against %r' % (path, list(a.keys()), list(b.keys()))
        return next((d for d in (strict_diff(a[k], b[k], '%s/%s' % (path, k)) for k in a) if d), None)
    if isinstance(a, (list, tuple)):
        if len(a) != len(b):
            return '%s: length %d against %d' % (path, len(a), len(b))
        return next((d for d in (strict_diff(x, y, '%s[%d]' % (path, i)) for i, (x, y) in enumerate(zip(a, b))) if d), None)
    if isinstance(a, np.ndarray):
        if a.dtype != b.dtype or a.shape != b.shape:
            return '%s: %s %s against %s %s' % (path, a.dtype, a.shape, b.dtype, b.shape)
        if a.dtype == object:
            return next((d for d in (strict_diff(x, y, '%s[%d]' % (path, i)) for i, (x, y) in enumerate(zip(a.ravel(), b.ravel()))) if d), None)
        return None if a.tobytes() == b.tobytes() else '%s: values' % path
    if isinstance(a, np.generic):
        return None if a.dtype == b.dtype and a == b else '%s: %r against %r' % (path, a, b)
    return None if a == b else '%s: %r against %r' % (path, a, b)


def run_prepare(gold, split, bev, tmp, class_names=None, crop_ops=None, device=None, rename=None):
    """The prepare stage on the fixture's sequences -> ({class: {seq: pickle content}}, the prepare object)."""
    cns = gold['class_names'] if class_names is None else class_names
    points = {(rename or {}).get(e['name'], e['name']): e['points'] for e in gold['sequences']}
    prep = object_data.WaymoObjectDataPrepare(cns, root_path=str(tmp), split=split, enlarge_scale=gold['enlarge_scale'], crop_on_bev=bev, workers=4,
                                              points_loader=lambda seq, frm: points[seq][frm], crop_ops=crop_ops, device=device, keep_index=True)
    out = defaultdict(dict)
    for e in gold['sequences']:
        seq = (rename or {}).get(e['name'], e['name'])
        prep.prepare_data_worker({seq: copy.deepcopy(e['assign'] if split == 'val' else e['tracks'])})
        for cn in ([cns] if isinstance(cns, str) else cns):
            with open(os.path.join(str(tmp), 'refining', cn, '%s.pkl' % seq), 'rb') as f:
                out[cn][seq] = pickle.load(f)
    return out, prep


def check_against_reference(gold, split, bev, out, prep):
    """Every discrete field, every kept index set, and the rows = the host-prepared points at those indices."""
    want = gold['prepare'][(split, bev)]
    poses = {e['name']: {str(f).zfill(4): tk['pose'][i] for tk in e['tracks'].values() for i, f in enumerate(tk['sample_idx'])} for e in gold['sequences']}
    n_rows = 0
    for cn in gold['class_names']:
        for e in gold['sequences']:
            seq = e['name']
            mine, ref = out[cn][seq], want[cn][seq]
            assert list(mine.keys()) == list(ref.keys()) and [type(k) for k in mine] == [type(k) for k in ref], (cn, seq)
            for obj_id in ref:
                a = {k: v for k, v in mine[obj_id].items() if k != 'pts'}
                b = {k: v for k, v in ref[obj_id].items() if k != 'pts'}
                assert list(mine[obj_id].keys()) == list(ref[obj_id].keys())
                d = strict_diff(a, b, '%s/%s/%s' % (cn, seq, obj_id))
                assert d is None, d
                assert isinstance(mine[obj_id]['pts'], list) and len(mine[obj_id]['pts']) == len(ref[obj_id]['pts'])
                for frm, rows, idx, got_idx in zip(ref[obj_id]['sample_idx'], mine[obj_id]['pts'], ref[obj_id]['pts'], prep.pts_index[(cn, seq)][obj_id]):
                    assert np.array_equal(got_idx, idx), (cn, seq, obj_id, frm)
                    prepared = prepare_frame_points(e['points'][frm], poses[seq][frm])
                    assert rows.dtype == np.float64 and rows.shape == (len(idx), 4) and rows.tobytes() == prepared[idx].tobytes(), (cn, seq, obj_id, frm)
                    n_rows += len(idx)
    return n_rows


@pytest.mark.parametrize('split,bev', [('val', False), ('val', True), ('test', False), ('test', True)])
def test_pickles_equal_the_reference(gold, tmp_path, split, bev):
    ops_ = NumpyCropOps()
    out, prep = run_prepare(gold, split, bev, tmp_path, crop_ops=ops_)
    assert check_against_reference(gold, split, bev, out, prep) > 1000
    assert ops_.calls == len(gold['sequences'])                       # one crop per sequence for the three classes


def test_fixture_covers_the_quirks(gold):
    k = gold['kinds']
    assert k['two_classes'] >= 1 and k['unlabelled'] >= 1 and k['unmatched_frames'] >= 1 and k['extra_frame_objects'] >= 1 and k['empty_crops'] >= 1
    assert gold['min_face_gap'] > 1e-4 and gold['min_iou'] > 1e-3
    ref = gold['prepare'][('val', False)]
    e = gold['sequences'][0]
    both = ref['Vehicle'][e['name']][e['class_change']], ref['Pedestrian'][e['name']][e['class_change']]
    assert len(both[0]['sample_idx']) == len(both[1]['sample_idx']) and both[0]['name'] == both[1]['name'] == 'Vehicle'      # (sic)
    some = next(iter(ref['Vehicle'][e['name']].values()))
    assert isinstance(some['state'], np.ndarray) and some['state'].shape == () and some['state'].dtype.kind == 'U'               # (sic)
    unl = [o for d in ref.values() for s in d.values() for o in s.values() if not o['matched_tracklet']][0]
    assert unl['gt_obj_id'] is None and unl['gt_name'] is None and bool(np.all(unl['matched'])) and not np.any(unl['gt_boxes_global'])
    test_obj = next(iter(gold['prepare'][('test', False)]['Vehicle'][e['name']].values()))
    assert test_obj['matched_tracklet'] is False and test_obj['gt_obj_id'] is None


def test_one_class_at_a_time_and_existing_files_are_kept(gold, tmp_path):
    """The reference's form - one class per object - writes the same file; a file that exists is not written again."""
    out, _ = run_prepare(gold, 'val', False, tmp_path, class_names='Pedestrian', crop_ops=NumpyCropOps())
    want = gold['prepare'][('val', False)]['Pedestrian']
    for seq, content in out['Pedestrian'].items():
        assert list(content.keys()) == list(want[seq].keys())
    path = os.path.join(str(tmp_path), 'refining', 'Pedestrian', '%s.pkl' % gold['sequences'][0]['name'])
    with open(path, 'wb') as f:
        f.write(b'kept')
    ops_ = NumpyCropOps()
    prep = object_data.WaymoObjectDataPrepare('Pedestrian', root_path=str(tmp_path), split='val', points_loader=lambda s, f: 1 / 0, crop_ops=ops_)
    assert prep.save_path == os.path.dirname(path)
    e = gold['sequences'][0]
    prep.prepare_data_worker({e['name']: copy.deepcopy(e['assign'])})
    assert open(path, 'rb').read() == b'kept' and ops_.calls == 0


def test_init_infos_from_tracking_reads_the_pickle(gold, tmp_path):
    track_path = os.path.join(str(tmp_path), 'tracking_val.pkl')
    with open(track_path, 'wb') as f:
        pickle.dump({e['name']: e['assign'] for e in gold['sequences']}, f)
    points = {e['name']: e['points'] for e in gold['sequences']}
    prep = object_data.WaymoObjectDataPrepare(gold['class_names'], root_path=str(tmp_path), split='val', track_data_path=track_path,
                                              points_loader=lambda seq, frm: points[seq][frm], crop_ops=NumpyCropOps())
    prep.init_infos_from_tracking()
    for cn in gold['class_names']:
        assert sorted(os.listdir(os.path.join(str(tmp_path), 'refining', cn))) == sorted('%s.pkl' % e['name'] for e in gold['sequences'])


def test_default_loader_reads_the_processed_frames(gold, tmp_path):
    e = gold['sequences'][0]
    folder = os.path.join(str(tmp_path), 'waymo_processed_data', 'segment-%s' % e['name'])
    os.makedirs(folder)
    for frm, pts in e['points'].items():
        np.save(os.path.join(folder, '%s.npy' % frm), pts)
    prep = object_data.WaymoObjectDataPrepare('Cyclist', root_path=str(tmp_path), split='test', crop_ops=NumpyCropOps())
    prep.prepare_data_worker({e['name']: copy.deepcopy(e['tracks'])})
    with open(os.path.join(prep.save_path, '%s.pkl' % e['name']), 'rb') as f:
        mine = pickle.load(f)
    assert list(mine.keys()) == list(gold['prepare'][('test', False)]['Cyclist'][e['name']].keys())


def test_round_trip_through_the_refine_dataset(gold, tmp_path):
    """The written files load through refine_dataset.DatasetTemplate.init_infos; the matched_tracklet filter keeps the labelled tracks."""
    from detzero_amd.config import AttrDict
    from detzero_amd.refine_dataset import DatasetTemplate
    rename = {e['name']: '1020365_76_00%d' % i for i, e in enumerate(gold['sequences'])}       # names that survive the reference's str.strip
    run_prepare(gold, 'val', False, tmp_path, crop_ops=NumpyCropOps(), rename=rename)
    os.makedirs(os.path.join(str(tmp_path), 'ImageSets'))
    with open(os.path.join(str(tmp_path), 'ImageSets', 'val.txt'), 'w') as f:
        f.write(''.join('segment-%s_with_camera_labels.tfrecord\n' % s for s in rename.values()))
    ref = gold['prepare'][('val', False)]
    every = {(seq, int(k)) for d in ref.values() for seq, objs in d.items() for k in objs}
    labelled = {(seq, int(k)) for d in ref.values() for seq, objs in d.items() for k, o in objs.items() if o['matched_tracklet']}
    assert 0 < len(labelled) < len(every)
    for save, want in ((False, labelled), (True, every)):
        cfg = AttrDict({'DATA_SPLIT': {'test': 'val'}, 'save_to_file': save})
        ds = DatasetTemplate(cfg, gold['class_names'], training=False, root_path=str(tmp_path))
        assert len(ds) == len(want)
        assert ds.box_num == sum(len(t['boxes_global']) for t in ds.track_infos) > 0
        assert all(len(t['pts']) == len(t['boxes_global']) == len(t['refine_iou']) for t in ds.track_infos)


def test_cli_checks_the_split_against_the_path():
    with pytest.raises(ValueError, match='does not match the dataset split'):
        object_data.main(['--split', 'val', '--track_data_path', '/data/tracking_test.pkl'])
    with pytest.raises(ValueError, match='training split'):
        refine_combine.main(['iou', '--geo_path', 'Vehicle_geometry_val.pkl', '--pos_path', 'Vehicle_position_train.pkl'])
    with pytest.raises(ValueError, match='training split'):
        refine_combine.generate_refine_boxes_iou('Vehicle', 'geo_train.pkl', 'pos_val.pkl', '.', LOG)


# ------------------------------------------------------------------------------------------------------------- the other end
def write_results(gold, tmp, split='val'):
    os.makedirs(os.path.join(str(tmp), 'result'), exist_ok=True)
    for cn in gold['class_names']:
        for kind, word in (('geo', 'geometry'), ('pos', 'position'), ('conf', 'confidence')):
            with open(os.path.join(str(tmp), 'result', '%s_%s_%s.pkl' % (cn, word, split)), 'wb') as f:
                pickle.dump(gold['refine'][cn][kind], f)
    drop = os.path.join(str(tmp), 'drop.pkl')
    with open(drop, 'wb') as f:
        pickle.dump(gold['drop'], f)
    return drop


@pytest.mark.parametrize('variant', ['conf_drop', 'plain'])
def test_combine_final_is_exact(gold, tmp_path, variant):
    drop = write_results(gold, tmp_path)
    conf = variant == 'conf_drop'
    refine_combine.combine_final(str(tmp_path), gold['class_names'], LOG, split='val', combine_conf_res=conf, combine_drop_path=drop if conf else None)
    for name, want in gold['combine'][variant].items():
        with open(os.path.join(str(tmp_path), 'result', name), 'rb') as f:
            mine = pickle.load(f)
        d = strict_diff(mine, want, name)
        assert d is None, d
    assert len(gold['combine'][variant]) >= 4


def test_combine_final_needs_its_inputs_and_honours_the_switches(gold, tmp_path):
    with pytest.raises(FileNotFoundError):
        refine_combine.combine_final(str(tmp_path), gold['class_names'], LOG)
    write_results(gold, tmp_path)
    refine_combine.combine_final(str(tmp_path), ['Vehicle'], LOG, combine_conf_res=False, track_save=False, frame_save=True)
    assert not os.path.exists(os.path.join(str(tmp_path), 'result', 'Vehicle_final.pkl'))
    assert os.path.exists(os.path.join(str(tmp_path), 'result', 'Vehicle_final_frame.pkl'))


def test_convert_frame_format_and_combine_det(gold, tmp_path):
    drop = write_results(gold, tmp_path)
    tracks = gold['combine']['conf_drop']['%s_final.pkl' % gold['class_names'][-1]]
    frames = []
    for seq in tracks:
        frames.extend(refine_combine.convert_frame_format(copy.deepcopy(tracks[seq])))
    merged = refine_combine.combine_det(copy.deepcopy(frames), drop)
    d = strict_diff(merged, gold['combine']['conf_drop']['%s_final_frame.pkl' % gold['class_names'][-1]], 'frames')
    assert d is None, d
    assert sum(len(f['score']) for f in merged) == sum(len(f['score']) for f in frames) + sum(len(r['score']) for s in gold['drop'].values() for r in s.values())
    # tracks that carry global boxes only: the lidar boxes come through the inverse of the frame's pose, one box at a time
    from detzero_amd.track_adapter import transform_boxes3d
    e = gold['sequences'][0]
    tk = {k: dict(v, sequence_name=e['name']) for k, v in list(e['tracks'].items())[:3]}
    for rec in refine_combine.convert_frame_format(tk):
        assert rec['boxes_global'].shape == (len(rec['obj_ids']), 9) and rec['boxes_lidar'].dtype == np.float32
        for i in range(len(rec['obj_ids'])):
            want = transform_boxes3d(rec['boxes_global'][i][None, :], rec['pose'], inverse=True).reshape(-1).astype(np.float32)
            assert rec['boxes_lidar'][i].tobytes() == want.tobytes()


def test_iou_labels_on_the_numpy_ops(gold, tmp_path):
    """generate_refine_boxes_iou's orchestration (one paired call per sequence, split per object) with the float32 numpy IoU the
    fixture was made with: the reference's file exactly."""
    from tests import track_ref
    calls = []

    def paired(a, b):
        calls.append(len(a))
        return np.diag(track_ref.iou3d(a, b))
    for cn in gold['class_names']:
        geo, pos = os.path.join(str(tmp_path), '%s_geometry_train.pkl' % cn), os.path.join(str(tmp_path), '%s_position_train.pkl' % cn)
        for path, kind in ((geo, 'geo'), (pos, 'pos')):
            with open(path, 'wb') as f:
                pickle.dump(gold['refine'][cn][kind], f)
        refine_combine.generate_refine_boxes_iou(cn, geo, pos, str(tmp_path), LOG, paired_iou=paired)
        with open(os.path.join(str(tmp_path), '%s_iou_train.pkl' % cn), 'rb') as f:
            mine = pickle.load(f)
        d = strict_diff(mine, gold['iou'][cn], cn)
        assert d is None, d
    assert len(calls) == sum(len(gold['refine'][cn]['geo']) for cn in gold['class_names'])
