"""CPU: the refining stage's model layer (detzero_amd/refine_models.py) and its shim names - what needs no device.

The recall records' host logic is fed the reference's own per-pair IoUs (tests/golden/refine_model_golden.npz, recorded by
gen_refine_model_golden.py from the reference's classes) in place of the kernel's table and must reproduce every entry of
the reference's recall dicts; the refusals raise; the reference's refining/tools/eval_utils.py imports under the shim.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

from detzero_amd import shim
from detzero_amd.config import AttrDict
from detzero_amd.lib import DetZeroHipError

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import gen_refine_model_golden as gen          # noqa: E402  (track layout of the fixture; importing it does not touch the reference)

REF_TOOLS = '/root/reference/refining/tools'

GRM_MODEL = {'NAME': 'GeometryRefineModel', 'QUERY_POINT_DIMS': 11, 'MEMORY_POINT_DIMS': 4,
             'REGRESSION': {'NAME': 'GeometryTransformer', 'QUERY_ENCODER': [128, 128], 'MEMORY_ENCODER': [128, 128], 'REGRESSION_MLP': [512],
                            'EMBED_DIMS': 256, 'ANCHOR_SIZES': [[4.8, 1.8, 1.5], [10.0, 2.6, 3.2], [2.0, 1.0, 1.6]],
                            'DECODER': {'NAME': 'GeometryHead', 'num_classes': 3, 'num_heads': 8, 'num_decoder_layers': 1, 'auxiliary': True,
                                        'cross_only': False, 'memory_self_attn': False, 'hidden_channel': 256, 'ffn_channel': 256,
                                        'dropout': 0.1, 'bn_momentum': 0.1, 'activation': 'relu'}},
             'POST_PROCESSING': {'GENERATE_RECALL': True, 'RECALL_THRESH_LIST': [0.7]}}
PRM_MODEL = {'NAME': 'PositionRefineModel', 'QUERY_POINT_DIMS': 32, 'MEMORY_POINT_DIMS': 32,
             'REGRESSION': {'NAME': 'PositionTransformer', 'QUERY_ENCODER': [128, 128], 'MEMORY_ENCODER': [128, 128], 'REGRESSION_MLP': [512],
                            'DECODER': {'NAME': 'PositionHead', 'num_classes': 3, 'num_heads': 8, 'num_decoder_layers': 1, 'auxiliary': True,
                                        'cross_only': False, 'hidden_channel': 256, 'dropout': 0.1, 'bn_momentum': 0.1, 'activation': 'relu',
                                        'ffn_channel': 256, 'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2],
                                        'grid_size': [1440, 1440, 40], 'out_size_factor': 8},
                            'LOSS_CLS': {'type': 'CrossEntropyLoss', 'reduction': 'mean', 'ignore_index': -1}},
             'POST_PROCESSING': {'GENERATE_RECALL': True, 'RECALL_THRESH_LIST': [0.7]}}
CRM_MODEL = {'NAME': 'ConfidenceRefineModel', 'QUERY_POINT_DIMS': 32, 'MEMORY_POINT_DIMS': 32,
             'REGRESSION': {'NAME': 'ConfidencePointnet', 'ENCODER_MLP': [128, 128], 'REGRESSION_MLP': [512], 'SCORE_THRESH': [0.35, 0.7]},
             'POST_PROCESSING': {'GENERATE_RECALL': True, 'RECALL_THRESH_LIST': [0.7]}}


class _Dataset:
    def __init__(self, tta=False):
        self.tta = tta


@pytest.fixture(scope='module')
def g(golden_dir):
    return np.load(os.path.join(golden_dir, 'refine_model_golden.npz'))


def fixture_batches(g):
    """[(first track, tracks of the batch)] in the fixture's batching."""
    tracks, bs = gen.tracks_from_fixture(g), int(g['batch_size'])
    return [(s, tracks[s:s + bs]) for s in range(0, len(tracks), bs)]


def counts_from_ious(iou, matched, mth_tk, thresholds):
    """The kernel's table from stored IoUs: (2, B, T) -> (B, 2, n_thr + 1), `>` taken in float32."""
    counts = np.zeros((iou.shape[1], 2, len(thresholds) + 1), np.int64)
    for i, m in enumerate(matched):
        if not mth_tk[i]:
            continue
        m = np.asarray(m, dtype=bool)
        for s in range(2):
            v = iou[s, i, :len(m)][m].astype(np.float32)
            counts[i, s, 0] = m.sum()
            for k, th in enumerate(thresholds):
                counts[i, s, 1 + k] = (v > np.float32(th)).sum()
    return counts


def test_shim_names_import():
    shim.install()
    from detzero_refine import datasets, models
    assert callable(models.build_network) and callable(models.load_data_to_gpu) and callable(models.model_fn_decorator)
    assert sorted(models.__all__) == ['ConfidenceRefineModel', 'GeometryRefineModel', 'PositionRefineModel']
    assert callable(datasets.build_dataloader)
    assert {'WaymoGeometryDataset', 'WaymoPositionDataset', 'WaymoConfidenceDataset'} <= set(datasets.__all__)
    from detzero_utils.ops.iou3d_nms import iou3d_nms_utils
    assert callable(iou3d_nms_utils.boxes_iou3d_paired_gpu)


@pytest.mark.parametrize('case', ['grm', 'prm', 'prm3'])
def test_recall_host_logic_reproduces_the_reference(g, case):
    from detzero_amd.refine_models import recall_record_from_counts
    rec = json.loads(str(g['recall_json']))
    thr = rec['thresholds'][case]
    tag = 'grm' if case == 'grm' else 'prm'
    for bi, (_, tracks) in enumerate(fixture_batches(g)):
        matched, mth_tk = [t['matched'] for t in tracks], [t['matched_tracklet'] for t in tracks]
        counts = counts_from_ious(g['%s_b%d_iou' % (tag, bi)], matched, mth_tk, thr)
        got = recall_record_from_counts(counts, [t['state'] for t in tracks], mth_tk, thr, {}, case != 'grm', case)
        assert got == rec['recall'][case][bi], bi
        assert all(type(v) is int for v in got.values())
    # the track whose fraction is exactly 7 / 10: counted by PRM's `>=`, not by GRM's `>`
    first = rec['recall'][case][0]
    assert first['Track level input (dynamic) %s' % thr[-1]] == (1 if case == 'grm' else 2)


def test_recall_accumulates_into_a_given_dict(g):
    from detzero_amd.refine_models import recall_record_from_counts
    rec = json.loads(str(g['recall_json']))
    total = {}
    for bi, (_, tracks) in enumerate(fixture_batches(g)):
        matched, mth_tk = [t['matched'] for t in tracks], [t['matched_tracklet'] for t in tracks]
        counts = counts_from_ious(g['prm_b%d_iou' % bi], matched, mth_tk, [0.7])
        total = recall_record_from_counts(counts, [t['state'] for t in tracks], mth_tk, [0.7], total, True, 'prm')
    want = {k: sum(d[k] for d in rec['recall']['prm']) for k in rec['recall']['prm'][0]}
    assert total == want


def test_crm_recall_record_reproduces_the_reference(g):
    from detzero_amd.refine_models import ConfidenceRefineModel
    rec = json.loads(str(g['recall_json']))
    for bi, (_, tracks) in enumerate(fixture_batches(g)):
        data = {'batch_size': len(tracks), 'box_num': [len(t['matched']) for t in tracks], 'state': [t['state'] for t in tracks],
                'matched_tracklet': [t['matched_tracklet'] for t in tracks]}
        for k in ('conf_score', 'pred_score', 'iou'):
            data[k] = torch.from_numpy(g['crm_b%d_%s' % (bi, k)])
        got = ConfidenceRefineModel.generate_recall_record(None, {}, data, [0.7])
        want = rec['recall']['crm'][bi]
        assert set(got) == set(want)
        for k, v in want.items():
            if isinstance(v, list):
                assert [float(x) for x in got[k]] == v, k
            else:
                assert type(got[k]) is int and got[k] == v, k
        assert 'iou' in data and ConfidenceRefineModel.generate_recall_record(None, {}, {}, [0.7]) == {}


def test_matched_track_without_matched_box_is_named():
    from detzero_amd.refine_models import recall_record_from_counts
    counts = np.zeros((2, 2, 2), np.int64)
    counts[0, :, 0] = 3
    with pytest.raises(DetZeroHipError, match='track 1'):
        recall_record_from_counts(counts, ['static', 'dynamic'], [True, True], [0.7], {}, True, 'PositionRefineModel')


def test_state_dict_layout_and_refusals(g):
    from detzero_amd import refine_models as M
    for tag, cfg in (('grm', GRM_MODEL), ('prm', PRM_MODEL), ('crm', CRM_MODEL)):
        model = M.build_network(AttrDict(cfg), _Dataset())
        assert type(model).__name__ == cfg['NAME']
        mine = {k: str(tuple(v.shape)) for k, v in model.state_dict().items()}
        assert mine == dict(zip(g[tag + '_keys'].tolist(), g[tag + '_shapes'].tolist())), tag
        assert 'global_step' in mine and all(k == 'global_step' or k.startswith('reg.') for k in mine)
        assert model.mode == 'TRAIN' and model.eval().mode == 'TEST'
        # training
        model.train()
        with pytest.raises(DetZeroHipError, match='training'):
            model({'batch_size': 1})
        with pytest.raises(DetZeroHipError, match='training'):
            M.model_fn_decorator()(model, {})
        # test-time augmentation: the reference's own is `raise NotImplementedError`
        tta = M.build_network(AttrDict(cfg), _Dataset(tta=True)).eval()
        with pytest.raises(DetZeroHipError, match='NotImplementedError'):
            tta.post_processing({'batch_box_preds': torch.zeros(1, 7), 'batch_size': 1, 'pred_score': torch.zeros(1, 200)})
    with pytest.raises(DetZeroHipError):
        M.build_network(AttrDict({'NAME': 'NoSuchModel'}), _Dataset())
    cfg = AttrDict(GRM_MODEL)
    cfg.POST_PROCESSING.CENTER_ALIGN = True
    model = M.build_network(cfg, _Dataset()).eval()
    with pytest.raises(DetZeroHipError, match='CENTER_ALIGN'):
        model.generate_recall_record(torch.zeros(1, 7), {}, {'gt_geo_trajectory': [np.zeros((1, 7))]}, [0.7])


def test_load_data_to_gpu_leaves_non_arrays_alone():
    from detzero_amd.refine_models import load_data_to_gpu
    t = torch.zeros(2)
    batch = {'sequence_name': np.array(['a']), 'frame': [np.arange(2)], 'box_num': [2], 'pos_trajectory': t}
    load_data_to_gpu(batch)          # nothing here is uploaded: no device needed
    assert batch['pos_trajectory'] is t and isinstance(batch['sequence_name'], np.ndarray) and batch['box_num'] == [2]


def test_dataloader_refusals(tmp_path):
    from detzero_amd.refine_dataset import build_dataloader
    cfg = AttrDict({'DATASET': 'WaymoPositionDataset', 'DATA_PATH': str(tmp_path), 'DATA_SPLIT': {'train': 'train', 'test': 'val'}})
    with pytest.raises(DetZeroHipError, match='training'):
        build_dataloader(cfg, ['Vehicle'], 2, False, root_path=str(tmp_path), training=True)
    with pytest.raises(DetZeroHipError, match='distributed'):
        build_dataloader(cfg, ['Vehicle'], 2, True, root_path=str(tmp_path), training=False)
    with pytest.raises(DetZeroHipError):
        build_dataloader(AttrDict(cfg, DATASET='DatasetTemplate'), ['Vehicle'], 2, False, root_path=str(tmp_path), training=False)


def test_dataset_reads_split_and_filters_unmatched_tracks(g, tmp_path):
    """ImageSets/<split>.txt + refining/<Class>/<seq>.pkl; false-positive tracks only with save_to_file (dataset.py:109-113)."""
    import pickle
    from detzero_amd.refine_dataset import build_dataloader, gt_to_init_box_frame
    tracks = gen.tracks_from_fixture(g)
    (tmp_path / 'ImageSets').mkdir()
    (tmp_path / 'ImageSets' / 'val.txt').write_text('segment-synthetic_with_camera_labels.tfrecord\nsegment-absent_with_camera_labels.tfrecord\n')
    (tmp_path / 'refining' / 'Vehicle').mkdir(parents=True)
    name = 'segment-synthetic_with_camera_labels.tfrecord'.strip('segment-').strip('_with_camera_labels.tfrecord') + '.pkl'
    with open(tmp_path / 'refining' / 'Vehicle' / name, 'wb') as f:
        pickle.dump({t['obj_id']: {k: v for k, v in t.items() if k != 'refine_iou'} for t in tracks}, f)
    cfg = AttrDict({'DATASET': 'WaymoPositionDataset', 'DATA_PATH': 'unused', 'DATA_SPLIT': {'train': 'train', 'test': 'val'},
                    'ENCODING': ['xyz', 'intensity', 'p2co', 'score'], 'TTA': False})
    ds, loader, sampler = build_dataloader(cfg, ['Vehicle'], 4, False, root_path=str(tmp_path), workers=0, training=False)
    assert sampler is None and loader.dataset is ds and ds.tta is False
    assert len(ds) == sum(t['matched_tracklet'] for t in tracks) == 7 and len(loader) == 2
    assert ds.box_num == sum(len(t['matched']) for t in tracks if t['matched_tracklet'])
    cfg.save_to_file = True
    ds, loader, _ = build_dataloader(cfg, ['Vehicle'], 4, False, root_path=str(tmp_path), training=False, length=5)
    assert len(ds) == 9 and [t['obj_id'] for t in ds.track_infos] == [t['obj_id'] for t in tracks] and len(loader) == 2
    # the ground-truth trajectory in the frame of the middle box equals the reference's collated one
    for bi, (s, chunk) in enumerate(fixture_batches(g)):
        for i, t in enumerate(chunk):
            n = len(t['matched'])
            got = gt_to_init_box_frame(t['boxes_global'], t['gt_boxes_global'])
            np.testing.assert_array_equal(got.astype(np.float32), g['prm_b%d_gt_pos_trajectory' % bi][i, :n])


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF_TOOLS, 'eval_utils.py')), reason='needs the reference tree')
def test_reference_eval_utils_imports_under_the_shim():
    shim.install()
    spec = importlib.util.spec_from_file_location('refining_eval_utils', os.path.join(REF_TOOLS, 'eval_utils.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from detzero_amd import refine_models
    assert mod.load_data_to_gpu is refine_models.load_data_to_gpu
    assert callable(mod.eval_one_epoch) and callable(mod.statistics_info)
