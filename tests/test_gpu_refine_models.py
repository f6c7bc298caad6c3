"""The refining stage's model layer on the device (detzero_amd/refine_models.py, refine_dataset.py, the detzero_refine shim).

Golden parity: GeometryRefineModel / PositionRefineModel / ConfidenceRefineModel.generate_recall_record on the inputs of
tests/golden/refine_model_golden.npz (recorded from the reference's own classes by gen_refine_model_golden.py) give every
entry of the reference's recall dicts, as integers.  The fixture keeps every pair's IoU at least 1e-3 away from the
thresholds, a condition on the inputs (asserted by the generator), so that libm / device differences of the overlap
cannot move a count; the worst |device IoU - stored CPU IoU| is printed.
"""
import json
import os
import pickle
import random

import numpy as np
import pytest
import torch
import torch.nn as nn

from detzero_amd.config import AttrDict
from detzero_amd.synth import synth_state_dict
from tests.test_refine_models import CRM_MODEL, GRM_MODEL, PRM_MODEL, _Dataset, fixture_batches, gen

gpu = pytest.mark.gpu
MODELS = {'grm': GRM_MODEL, 'prm': PRM_MODEL, 'crm': CRM_MODEL}
DATASETS = {'grm': ('WaymoGeometryDataset', ['xyz', 'intensity', 'p2s', 'score']), 'prm': ('WaymoPositionDataset', ['xyz', 'intensity', 'p2co', 'score']),
            'crm': ('WaymoConfidenceDataset', ['xyz', 'intensity', 'p2co', 'score'])}


@pytest.fixture(scope='module')
def g(golden_dir):
    return np.load(os.path.join(golden_dir, 'refine_model_golden.npz'))


@pytest.fixture(scope='module')
def recall(g):
    return json.loads(str(g['recall_json']))


def _model(tag, thresholds=None, tta=False):
    from detzero_amd.refine_models import build_network
    cfg = AttrDict(MODELS[tag])
    if thresholds is not None:
        cfg.POST_PROCESSING.RECALL_THRESH_LIST = list(thresholds)
    return build_network(cfg, _Dataset(tta))


def _labels(tracks):
    return {'state': [t['state'] for t in tracks], 'matched': [t['matched'] for t in tracks],
            'matched_tracklet': [t['matched_tracklet'] for t in tracks]}


def grm_inputs(g, bi, tracks, device):
    data = {'geo_trajectory': [t['boxes_global'] for t in tracks], 'gt_geo_trajectory': [t['gt_boxes_global'] for t in tracks],
            'gt_geo_query_boxes': g['grm_b%d_gt_geo_query_boxes' % bi], **_labels(tracks)}
    return data, torch.from_numpy(g['grm_b%d_box_preds' % bi]).to(device)


def prm_inputs(g, bi, tracks, device):
    data = {'pos_trajectory': torch.from_numpy(g['prm_b%d_pos_trajectory' % bi]).to(device),
            'gt_pos_trajectory': torch.from_numpy(g['prm_b%d_gt_pos_trajectory' % bi]).to(device),
            'box_num': [len(t['matched']) for t in tracks], **_labels(tracks)}
    return data, torch.from_numpy(g['prm_b%d_box_preds' % bi]).to(device)


def crm_inputs(g, bi, tracks, device):
    data = {'batch_size': len(tracks), 'box_num': [len(t['matched']) for t in tracks], **_labels(tracks)}
    for k in ('conf_score', 'pred_score', 'iou'):
        data[k] = torch.from_numpy(g['crm_b%d_%s' % (bi, k)]).to(device)
    return data


def _same_crm(got, want):
    assert set(got) == set(want)
    for k, v in want.items():
        if isinstance(v, list):
            assert [float(x) for x in got[k]] == v, k
        else:
            assert type(got[k]) is int and got[k] == v, k


@gpu
def test_recall_records_match_the_reference(device, g, recall):
    from detzero_amd import iou3d_nms_utils
    from detzero_amd.refine_models import ConfidenceRefineModel, PositionRefineModel
    grm = _model('grm').eval()
    worst = {'grm': 0.0, 'prm': 0.0}
    for bi, (_, tracks) in enumerate(fixture_batches(g)):
        data, preds = grm_inputs(g, bi, tracks, device)
        got = grm.generate_recall_record(preds, {}, data, recall['thresholds']['grm'])
        assert got == recall['recall']['grm'][bi] and all(type(v) is int for v in got.values()), ('grm', bi)
        pdata, ppreds = prm_inputs(g, bi, tracks, device)
        for case in ('prm', 'prm3'):
            got = PositionRefineModel.generate_recall_record(ppreds, {}, dict(pdata), recall['thresholds'][case])
            assert got == recall['recall'][case][bi] and all(type(v) is int for v in got.values()), (case, bi)
        _same_crm(ConfidenceRefineModel.generate_recall_record(None, {}, crm_inputs(g, bi, tracks, device), [0.7]), recall['recall']['crm'][bi])
        # device IoU against the stored CPU IoU, pair by pair
        for i, t in enumerate(tracks):
            if not t['matched_tracklet']:
                continue
            m, n = torch.from_numpy(t['matched']).to(device), len(t['matched'])
            gt = torch.from_numpy(t['gt_boxes_global'][:, :7]).float().to(device)[m]
            tin = torch.from_numpy(t['boxes_global'][:, :7]).float().to(device)
            tout = tin.clone()
            tout[:, 3:6] = preds[i, 3:6]
            for s, boxes in enumerate((tin, tout)):
                d = iou3d_nms_utils.boxes_iou3d_paired_gpu(boxes[m], gt).cpu().numpy() - g['grm_b%d_iou' % bi][s, i, :n][t['matched']]
                worst['grm'] = max(worst['grm'], float(np.abs(d).max()))
            gt = pdata['gt_pos_trajectory'][i, :n][m]
            for s, boxes in enumerate((pdata['pos_trajectory'][i, :n], ppreds[i, :n])):
                d = iou3d_nms_utils.boxes_iou3d_paired_gpu(boxes[m], gt).cpu().numpy() - g['prm_b%d_iou' % bi][s, i, :n][t['matched']]
                worst['prm'] = max(worst['prm'], float(np.abs(d).max()))
    print('\n[refine_models] worst |device IoU - stored CPU IoU|: GRM (global frame, km from the origin) %.3e, PRM (object frame) %.3e'
          % (worst['grm'], worst['prm']))
    assert max(worst.values()) < 1e-3          # the fixture's exclusion band: beyond it a count could move


@gpu
def test_recall_record_refuses_a_matched_track_without_matched_box(device, g):
    from detzero_amd.lib import DetZeroHipError
    from detzero_amd.refine_models import PositionRefineModel
    _, tracks = fixture_batches(g)[0]
    data, preds = prm_inputs(g, 0, tracks, device)
    data['matched'] = [m.copy() for m in data['matched']]
    data['matched'][1][:] = False
    with pytest.raises(DetZeroHipError, match='track 1'):
        PositionRefineModel.generate_recall_record(preds, {}, data, [0.7])


def _write_dataset(root, tracks):
    (root / 'ImageSets').mkdir()
    (root / 'ImageSets' / 'val.txt').write_text('segment-synthetic_with_camera_labels.tfrecord\n')
    (root / 'refining' / 'Vehicle').mkdir(parents=True)
    name = 'segment-synthetic_with_camera_labels.tfrecord'.strip('segment-').strip('_with_camera_labels.tfrecord') + '.pkl'
    with open(root / 'refining' / 'Vehicle' / name, 'wb') as f:
        pickle.dump({t['obj_id']: {k: v for k, v in t.items() if k != 'refine_iou'} for t in tracks}, f)


def _loader(tag, root, batch_size, length=0):
    from detzero_amd import shim
    shim.install()
    from detzero_refine.datasets import build_dataloader
    name, enc = DATASETS[tag]
    cfg = AttrDict({'DATASET': name, 'DATA_PATH': 'unused', 'DATA_SPLIT': {'train': 'train', 'test': 'val'}, 'ENCODING': enc,
                    'save_to_file': True})           # keeps the false-positive tracks: the fixture's batches hold them
    return build_dataloader(cfg, ['Vehicle'], batch_size, False, root_path=str(root), workers=0, logger=None, training=False, length=length)


@gpu
@pytest.mark.parametrize('tag', ['grm', 'prm', 'crm'])
def test_network_round_trip(device, g, tag, tmp_path):
    """build_network on the vehicle config's MODEL block: the reference's state_dict manifest, one forward on a small batch from
    the loader, the reference's pred_dicts keys, a recall dict exactly when the batch carries ground truth."""
    from detzero_amd.refine_models import load_data_to_gpu
    model = _model(tag)
    mine = {k: str(tuple(v.shape)) for k, v in model.state_dict().items()}
    assert mine == dict(zip(g[tag + '_keys'].tolist(), g[tag + '_shapes'].tolist()))
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=3), strict=True)
    model = model.to(device).eval()
    _write_dataset(tmp_path, gen.tracks_from_fixture(g))
    ds, loader, _ = _loader(tag, tmp_path, 4, length=4)
    batch = next(iter(loader))
    load_data_to_gpu(batch)
    labelled = dict(batch)
    pred, rec, extra = model(labelled)
    b = 4
    want = {'grm': {'pred_boxes': (b, 7), 'pose': None, 'geo_trajectory': None},
            'prm': {'pred_boxes': (b, 200, 7), 'pose': None, 'pos_init_box': (b, 7), 'gt_pos_trajectory': (b, 200, 7)},
            'crm': {'pred_score': (b, 200)}}[tag]
    assert set(pred) == set(want) and extra == {}
    for k, shape in want.items():
        if shape is not None:
            assert isinstance(pred[k], np.ndarray) and pred[k].shape == shape and np.all(np.isfinite(pred[k])), k
    assert pred['pred_score' if tag == 'crm' else 'pred_boxes'].dtype == np.float32
    assert rec and rec['Track num'] == 3 and rec['Box num'] > 0 and 'Box level input 0.7' in rec
    gt_keys = {'grm': ['gt_geo_trajectory', 'gt_geo_query_boxes'], 'prm': ['gt_pos_trajectory'], 'crm': ['iou']}[tag]
    plain = {k: v for k, v in batch.items() if k not in gt_keys}
    pred2, rec2, _ = model(plain)
    assert rec2 == {} and set(pred2) == set(want) - set(gt_keys)
    # the write-back accepts what the model returned
    annos = ds.generate_prediction_dicts(batch, pred, {})
    assert sorted(annos['segment-synthetic']) == ['obj00', 'obj01', 'obj02', 'obj03']


class _FixtureReg(nn.Module):
    """Stands in for the regression network in the loader loop: the fixture's recall dicts were recorded with synthetic
    predictions (and, for CRM, synthetic IoU labels - the test-mode dataset has none), which it writes into the batch."""

    def __init__(self, g, tag, device):
        super().__init__()
        self.g, self.tag, self.device, self.bi = g, tag, device, 0

    def forward(self, data_dict):
        if self.tag == 'crm':
            for k in ('pred_score', 'iou'):
                data_dict[k] = torch.from_numpy(self.g['crm_b%d_%s' % (self.bi, k)]).to(self.device)
        else:
            data_dict['batch_box_preds'] = torch.from_numpy(self.g['%s_b%d_box_preds' % (self.tag, self.bi)]).to(self.device)
        self.bi += 1
        return data_dict


def statistics_info(thresholds, ret_dict, metric):
    """refining/tools/eval_utils.py:15-57, restated: what the evaluation loop adds up per batch."""
    for cur_th in thresholds:
        for level, short in (('Box', 'box'), ('Track', 'track')):
            for scope in ('', ' (static)', ' (dynamic)'):
                for side in ('input', 'output'):
                    key = 'Num@%s %s%s %s' % (short, side, scope, str(cur_th))
                    metric[key] = metric.get(key, 0) + ret_dict['%s level %s%s %s' % (level, side, scope, str(cur_th))]
    for key, src in (('Box num', 'Box num'), ('Track num', 'Track num'), ('static_num', 'static'), ('dynamic_num', 'dynamic'),
                     ('matched_up', 'matched_up'), ('matched_down', 'matched_down'), ('unmatched_down', 'unmatched_down'),
                     ('unmatched_up', 'unmatched_up')):
        metric[key] = metric.get(key, 0) + ret_dict.get(src, 0)
    for key in ('gt_score', 'pred_score', 'ori_score'):
        metric.setdefault(key, []).extend(ret_dict.get(key, []))


@gpu
@pytest.mark.parametrize('tag', ['grm', 'prm', 'crm'])
def test_loader_end_to_end(device, g, recall, tag, tmp_path):
    from detzero_amd import object_features
    from detzero_amd.refine_models import load_data_to_gpu
    tracks = gen.tracks_from_fixture(g)
    _write_dataset(tmp_path, tracks)
    ds, loader, sampler = _loader(tag, tmp_path, int(g['batch_size']))
    assert sampler is None and loader.dataset is ds and len(ds) == len(tracks) and len(loader) == 3 and ds.tta is False
    random.seed(11)
    batches = list(loader)
    assert [b['batch_size'] for b in batches] == [4, 4, 1]
    # the model inputs are object_features' on the same tracks with the same draws
    random.seed(11)
    feats = {'grm': object_features.grm_features, 'prm': object_features.prm_features, 'crm': object_features.crm_features}[tag]
    for (start, chunk), batch in zip(fixture_batches(g), batches):
        ref = feats(chunk, encoding=tuple(DATASETS[tag][1]), rng=random, device=device)
        for k, v in ref.items():
            if torch.is_tensor(v):
                assert batch[k].is_cuda and torch.equal(batch[k], v), k
            elif isinstance(v, np.ndarray):
                np.testing.assert_array_equal(batch[k], v)
            elif k != 'obj_cls':
                assert batch[k] == v, k
    # bookkeeping and ground-truth keys: the reference's collated ones
    for bi, ((start, chunk), batch) in enumerate(zip(fixture_batches(g), batches)):
        assert batch['sequence_name'] == ['segment-synthetic'] * len(chunk) and batch['obj_id'] == [t['obj_id'] for t in chunk]
        assert batch['state'] == [t['state'] for t in chunk] and batch['matched_tracklet'] == [t['matched_tracklet'] for t in chunk]
        for i, t in enumerate(chunk):
            np.testing.assert_array_equal(batch['frame'][i], t['sample_idx'])
        if tag == 'grm':
            # (the fixture holds what load_data_to_gpu made of it: float32)
            np.testing.assert_array_equal(batch['gt_geo_query_boxes'].astype(np.float32), g['grm_b%d_gt_geo_query_boxes' % bi].astype(np.float32))
            for i, t in enumerate(chunk):
                np.testing.assert_array_equal(batch['geo_trajectory'][i], t['boxes_global'])
                np.testing.assert_array_equal(batch['gt_geo_trajectory'][i], t['gt_boxes_global'])
                np.testing.assert_array_equal(batch['geo_score'][i], t['score'])
                np.testing.assert_array_equal(batch['matched'][i], t['matched'])
            assert batch['obj_cls'].tolist() == [1] * len(chunk)
        elif tag == 'prm':
            np.testing.assert_array_equal(batch['gt_pos_trajectory'].astype(np.float32), g['prm_b%d_gt_pos_trajectory' % bi])
            # (float32 of coordinates below 128 m in the object frame: 2 ulp = 1.5e-5)
            np.testing.assert_allclose(batch['pos_trajectory'].cpu().numpy(), g['prm_b%d_pos_trajectory' % bi], rtol=0, atol=1.6e-5)
            assert batch['box_num'] == [len(t['matched']) for t in chunk]
        else:
            np.testing.assert_array_equal(batch['conf_score'].astype(np.float32), g['crm_b%d_conf_score' % bi])
            assert batch['iou'].shape == (len(chunk), 200) and set(np.unique(batch['iou'])) <= {0.0, -1.0}
    # the evaluation loop's totals
    model = _model(tag).eval()
    model.reg = _FixtureReg(g, tag, device)
    thr = MODELS[tag]['POST_PROCESSING']['RECALL_THRESH_LIST']
    metric, want = {}, {}
    for bi, batch in enumerate(batches):
        load_data_to_gpu(batch)
        pred_dicts, ret_dict, _ = model(batch)
        statistics_info(thr, ret_dict, metric)
        statistics_info(thr, recall['recall'][tag][bi], want)
    for k, v in want.items():
        assert ([float(x) for x in metric[k]] == v) if isinstance(v, list) else (metric[k] == v and type(metric[k]) is int), k
    assert metric['Track num'] == 7 and metric['Box num'] == (sum(len(t['matched']) for t in tracks) if tag == 'crm' else 356)
