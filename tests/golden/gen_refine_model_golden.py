"""Golden records for the refining stage's model layer (recall records of GRM / PRM / CRM, ground-truth keys of the data
layer, state-dict manifests) from the REFERENCE's own classes, CPU.

    python tests/golden/gen_refine_model_golden.py      (build container only; needs /root/reference)

Runs GeometryRefineModel / PositionRefineModel / ConfidenceRefineModel.generate_recall_record
(refining/detzero_refine/models/{geometry,position,confidence}_refine_model.py) as they are, on batches made by the
reference's own WaymoGeometryDataset / WaymoPositionDataset / WaymoConfidenceDataset.extract_track_feature and
DatasetTemplate.collate_batch (constructors bypassed as in gen_refine_feat_golden.py) followed by load_data_to_gpu.
Stand-ins: `torch.Tensor.cuda` is the identity, `torch.cuda.FloatTensor` the CPU constructor, and the CUDA extension call
`iou3d_nms_cuda.boxes_overlap_bev_gpu` under the reference's own iou3d_nms_utils.boxes_iou3d_gpu is the oracle's overlap
routine (oracle.cref.boxes_overlap_bev).  The three vehicle configs' MODEL blocks are built with the reference's
build_network for the state-dict manifests.

Tracks (`make_tracks`): seeded synthetic ones - detzero_amd.synth.synth_boxes moved to global coordinates of a few thousand
metres, one size per object, ground truth = the track plus seeded perturbations (tight / loose / far), mixed `matched` masks,
both states, two `matched_tracklet = False` tracks, lengths 1, 2, 10, 37 and 200.  Track 0 has 10 matched boxes of which exactly 7
pass 0.7 on both sides: its fraction is 7 / 10, the case that separates GRM's `> 0.7` from PRM's `>= 0.7`.
Stored: the tracks (no points: the recall records do not depend on them), per batch the collated ground-truth keys, the
synthetic `box_preds`, the per-pair CPU IoUs and every recall-dict entry after int() / float().  No reference text.

Asserted before writing: no stored IoU within 1e-3 of a threshold or of 0.7; per threshold at least 10 % of the counted pairs
on each side; track 0 as described; no matched track without a matched box.
"""
import importlib
import json
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

ORIGIN = np.array([3120.0, -2260.0, 35.0])
LENGTHS = [10, 1, 2, 10, 200, 200, 10, 2, 37]
UNMATCHED_TRACKS = (3, 7)
BATCH_SIZE = 4
CASES = {'grm': [0.7], 'prm': [0.7], 'prm3': [0.3, 0.5, 0.7], 'crm': [0.7]}
BAND = 1e-3
PRED_SEED = 7050          # seeds the synthetic predictions; chosen so that the conditions asserted in main() hold


def perturb(rng, boxes, kinds):
    """tight (0): centimetres; loose (1): a third of the length along x, some heading; far (2): more than a box away."""
    out = boxes.copy()
    n = len(boxes)
    out[:, :3] += rng.normal(0, 1, (n, 3)) * np.array([0.04, 0.04, 0.02])
    out[:, 3:6] *= rng.uniform(0.97, 1.03, (n, 3))
    loose, far = kinds == 1, kinds == 2
    out[loose, 0] += 0.3 * boxes[loose, 3] * rng.choice([-1, 1], loose.sum())
    out[loose, 6] += rng.normal(0, 0.12, loose.sum())
    out[far, :2] += 1.5 * boxes[far, 3:5]
    return out


def make_tracks():
    """The track records as the crop step stores them (daemon/prepare_object_data.py), without points."""
    from detzero_amd.synth import synth_boxes
    tracks = []
    for t, n in enumerate(LENGTHS):
        rng = np.random.default_rng(4200 + t)
        boxes = synth_boxes(300 + t, n, xy_range=60.0, near_duplicates=0.0).astype(np.float64)
        size = np.array([4.6, 2.0, 1.7]) * rng.uniform(0.9, 1.2, 3)
        boxes[:, 3:6] = size * rng.uniform(0.98, 1.02, (n, 3))
        boxes[:, :3] += ORIGIN
        kinds = rng.choice([0, 0, 1, 2], n)
        matched = rng.random(n) < 0.8
        if t == 0:
            kinds, matched = np.array([0, 0, 1, 0, 0, 2, 0, 1, 0, 0]), np.ones(n, dtype=bool)
        matched[rng.integers(0, n)] = True
        gt = perturb(rng, boxes, kinds)
        gt[:, 3:6] = size                      # one ground-truth size per object
        tracks.append({
            'boxes_global': boxes, 'gt_boxes_global': gt, 'score': rng.uniform(0.05, 0.99, n), 'sample_idx': np.arange(n) + 3 * t,
            'pose': np.tile(np.eye(4), (n, 1, 1)), 'matched': matched, 'matched_tracklet': t not in UNMATCHED_TRACKS,
            'state': 'dynamic' if t % 2 == 0 else 'static', 'sequence_name': 'segment-synthetic', 'obj_id': 'obj%02d' % t,
            'name': 'Vehicle', 'kinds': kinds})
    return tracks


def track_points(track, seed):
    """A few points per box (global frame, [x, y, z, intensity]): the recall records do not depend on them, the model inputs do."""
    rng = np.random.default_rng(seed)
    pts = []
    for box in track['boxes_global']:
        n = int(rng.integers(0, 12))
        pts.append(np.concatenate([box[:3] + rng.uniform(-0.5, 0.5, (n, 3)) * box[3:6], rng.uniform(0, 1, (n, 1))], axis=1))
    return pts


def tracks_from_fixture(g):
    """The same records rebuilt from the stored arrays (tests write them to pickles)."""
    tracks, at = [], 0
    for t, n in enumerate(g['track_len'].tolist()):
        tr = {'boxes_global': g['boxes_global'][at:at + n].copy(), 'gt_boxes_global': g['gt_boxes_global'][at:at + n].copy(),
              'score': g['score'][at:at + n].copy(), 'sample_idx': g['sample_idx'][at:at + n].copy(), 'pose': np.tile(np.eye(4), (n, 1, 1)),
              'matched': g['matched'][at:at + n].copy(), 'matched_tracklet': bool(g['matched_tracklet'][t]), 'state': str(g['state'][t]),
              'sequence_name': 'segment-synthetic', 'obj_id': 'obj%02d' % t, 'name': 'Vehicle'}
        tr['pts'] = track_points(tr, 900 + t)
        tr['refine_iou'] = np.zeros(n)
        tracks.append(tr)
        at += n
    return tracks


def import_reference():
    import gen_refine_feat_golden as feat
    from oracle import cref
    REF = feat.REF
    Geo, Pos, Base = feat.import_reference()
    conf = importlib.import_module('detzero_refine.datasets.waymo.waymo_confidence_dataset')
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.cuda.FloatTensor = torch.FloatTensor

    def overlap_stub(a, b, out):
        out.copy_(torch.from_numpy(cref.boxes_overlap_bev(a.numpy().astype(np.float32), b.numpy().astype(np.float32))))
        return 1
    feat._pkg('detzero_utils.ops.iou3d_nms', REF + '/utils/detzero_utils/ops/iou3d_nms')
    ext = types.ModuleType('detzero_utils.ops.iou3d_nms.iou3d_nms_cuda')
    ext.boxes_overlap_bev_gpu = overlap_stub
    sys.modules[ext.__name__] = ext
    sys.modules['detzero_utils.ops.iou3d_nms'].iou3d_nms_cuda = ext
    feat._pkg('detzero_refine.models', REF + '/refining/detzero_refine/models')
    mods = feat._pkg('detzero_refine.models.modules', REF + '/refining/detzero_refine/models/modules')
    importlib.import_module('detzero_utils.model_utils')
    mods.GeometryTransformer = importlib.import_module('detzero_refine.models.modules.geometry_transformer').GeometryTransformer
    mods.PositionTransformer = importlib.import_module('detzero_refine.models.modules.position_transformer').PositionTransformer
    mods.ConfidencePointnet = importlib.import_module('detzero_refine.models.modules.confidence_pointnet').ConfidencePointnet
    models = {k: importlib.import_module('detzero_refine.models.%s_refine_model' % k) for k in ('geometry', 'position', 'confidence')}
    # models/__init__.py:16-30 by path (the package object above is a path-only stand-in)
    spec = importlib.util.spec_from_file_location('detzero_refine.models', REF + '/refining/detzero_refine/models/__init__.py',
                                                  submodule_search_locations=[REF + '/refining/detzero_refine/models'])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules['detzero_refine.models'] = pkg
    spec.loader.exec_module(pkg)
    return feat, {'grm': Geo, 'prm': Pos, 'crm': conf.WaymoConfidenceDataset}, Base, models, pkg


class Recorder:
    """Wraps the reference's boxes_iou3d_gpu: keeps the diagonal of every matrix it returns."""

    def __init__(self, fn):
        self.fn, self.diags = fn, []

    def __call__(self, a, b):
        m = self.fn(a, b)
        self.diags.append(m.diag().numpy().copy())
        return m


def place(diags, matched, mth_tk, t_cap):
    """The recorded (input, output) diagonals of the matched tracks -> two (B, t_cap) arrays, zero outside the counted rows."""
    out = np.zeros((2, len(matched), t_cap), np.float32)
    it = iter(diags)
    for i, m in enumerate(matched):
        if not mth_tk[i]:
            continue
        for s in range(2):
            out[s, i, :len(m)][np.asarray(m, dtype=bool)] = next(it)
    assert next(it, None) is None
    return out


def plain(rec):
    res = {}
    for k, v in rec.items():
        if isinstance(v, list):
            res[k] = [float(x) for x in v]
        else:
            assert float(v) == int(v), (k, v)
            res[k] = int(v)
    return res


def main():
    import importlib.util  # noqa: F401
    import yaml
    from detzero_amd.config import AttrDict
    feat, ds_cls, Base, models, ref_models = import_reference()
    tracks = make_tracks()
    out = {'track_len': np.array(LENGTHS), 'matched_tracklet': np.array([t['matched_tracklet'] for t in tracks]),
           'state': np.array([t['state'] for t in tracks]), 'batch_size': np.array(BATCH_SIZE)}
    for k in ('boxes_global', 'gt_boxes_global', 'score', 'sample_idx', 'matched'):
        out[k] = np.concatenate([t[k] for t in tracks], axis=0)
    full = tracks_from_fixture(out)
    for t in full:
        assert (not t['matched_tracklet']) or t['matched'].sum() > 0, 'a matched track without a matched box'

    recalls = {c: [] for c in CASES}
    ious = {c: [] for c in CASES}
    enc = {'grm': ['xyz', 'intensity', 'p2s', 'score'], 'prm': ['xyz', 'intensity', 'p2co', 'score'], 'crm': ['xyz', 'intensity', 'p2co', 'score']}
    for bi, start in enumerate(range(0, len(full), BATCH_SIZE)):
        chunk = full[start:start + BATCH_SIZE]
        rng = np.random.default_rng(PRED_SEED + bi)
        batches = {}
        for tag in ('grm', 'prm', 'crm'):
            items = []
            for t in chunk:
                kw = {'grm': dict(query_num=3, query_pts_num=256, memory_pts_num=4096), 'prm': dict(query_num=200, query_pts_num=256, memory_pts_num=48),
                      'crm': dict(query_num=200, query_pts_num=256)}[tag]
                ds = feat.bare(ds_cls[tag], encoding=enc[tag], **kw)      # a fresh object per track: GRM's lowers its query_num for good
                random.seed(5000 + start)
                info = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in t.items()}
                info['pts'] = [p.copy() for p in t['pts']]
                items.append(ds.extract_track_feature(info))
            batch = Base.collate_batch(items)
            ref_models.load_data_to_gpu(batch)
            batches[tag] = batch
        # ---- GRM: one predicted size per object
        b = batches['grm']
        gt_size = np.stack([t['gt_boxes_global'][0, 3:6] for t in chunk])
        preds = np.zeros((len(chunk), 7), np.float32)
        preds[:, 3:6] = gt_size * np.where(rng.random((len(chunk), 1)) < 0.4, 0.86, 1.0) * rng.uniform(0.97, 1.03, (len(chunk), 3))
        if bi == 0:
            preds[0, 3:6] = gt_size[0] * 1.004
        rec = Recorder(models['geometry'].iou3d_nms_utils.boxes_iou3d_gpu)
        models['geometry'].iou3d_nms_utils = types.SimpleNamespace(boxes_iou3d_gpu=rec)
        self_ = types.SimpleNamespace(model_cfg=AttrDict({'POST_PROCESSING': {'GENERATE_RECALL': True, 'RECALL_THRESH_LIST': CASES['grm']}}))
        r = models['geometry'].GeometryRefineModel.generate_recall_record(self_, torch.from_numpy(preds), {}, b, CASES['grm'])
        models['geometry'].iou3d_nms_utils = types.SimpleNamespace(boxes_iou3d_gpu=rec.fn)
        recalls['grm'].append(plain(r))
        t_cap = max(len(t['matched']) for t in chunk)
        io = place(rec.diags, b['matched'], b['matched_tracklet'], t_cap)
        ious['grm'].append(io)
        out['grm_b%d_box_preds' % bi] = preds
        out['grm_b%d_iou' % bi] = io
        out['grm_b%d_gt_geo_query_boxes' % bi] = b['gt_geo_query_boxes'].numpy().astype(np.float64)
        # ---- PRM: per-box predictions in the init-box frame
        b = batches['prm']
        gt_local = b['gt_pos_trajectory'].numpy().astype(np.float64)
        preds = np.zeros_like(gt_local)
        for i, t in enumerate(chunk):
            n = len(t['matched'])
            kinds = rng.choice([0, 0, 0, 1, 2], n)
            if bi == 0 and i == 0:
                kinds = np.array([0, 0, 2, 0, 0, 1, 0, 2, 0, 0])
            preds[i, :n] = perturb(rng, gt_local[i, :n], kinds)
        preds = preds.astype(np.float32)
        out['prm_b%d_box_preds' % bi] = preds
        out['prm_b%d_pos_trajectory' % bi] = b['pos_trajectory'].numpy()
        out['prm_b%d_gt_pos_trajectory' % bi] = b['gt_pos_trajectory'].numpy()
        for case in ('prm', 'prm3'):
            rec = Recorder(models['position'].iou3d_nms_utils.boxes_iou3d_gpu)
            models['position'].iou3d_nms_utils = types.SimpleNamespace(boxes_iou3d_gpu=rec)
            r = models['position'].PositionRefineModel.generate_recall_record(torch.from_numpy(preds), {}, b, CASES[case])
            models['position'].iou3d_nms_utils = types.SimpleNamespace(boxes_iou3d_gpu=rec.fn)
            recalls[case].append(plain(r))
            io = place(rec.diags, b['matched'], b['matched_tracklet'], 200)
            ious[case].append(io)
        out['prm_b%d_iou' % bi] = io
        # ---- CRM: host record on a few values per box
        b = batches['crm']
        nb = len(chunk)
        b['pred_score'] = torch.from_numpy(rng.uniform(0, 1, (nb, 200)).astype(np.float32))
        b['iou'] = torch.from_numpy(np.where(b['conf_score'].numpy() >= 0, rng.choice([0.2, 0.55, 0.7, 0.9], (nb, 200)), -1.0).astype(np.float32))
        r = models['confidence'].ConfidenceRefineModel.generate_recall_record(None, {}, b, CASES['crm'])
        recalls['crm'].append(plain(r))
        for k in ('pred_score', 'iou', 'conf_score'):
            out['crm_b%d_%s' % (bi, k)] = b[k].numpy()

    # ---- conditions on the inputs
    for case, thr in CASES.items():
        if case == 'crm':
            continue
        at, vals = 0, [[], []]
        for bi, io in enumerate(ious[case]):
            for i in range(io.shape[1]):
                t = full[at + i]
                if t['matched_tracklet']:
                    for s in range(2):
                        vals[s].append(io[s, i, :len(t['matched'])][t['matched']])
            at += io.shape[1]
        for s in range(2):
            v = np.concatenate(vals[s])
            for th in set(thr) | {0.7}:
                assert np.abs(v - np.float32(th)).min() >= BAND, (case, s, th, np.abs(v - np.float32(th)).min())
            for th in thr:
                frac = (v > np.float32(th)).mean()
                assert 0.1 <= frac <= 0.9, (case, s, th, frac)
            print(case, RECALL_SIDE[s], 'pairs', v.size, 'above', {th: int((v > np.float32(th)).sum()) for th in thr})
        if case in ('grm', 'prm'):
            io = ious[case][0]
            assert full[0]['matched'].all() and len(full[0]['matched']) == 10
            assert (io[0, 0, :10] > np.float32(0.7)).sum() == 7 and (io[1, 0, :10] > np.float32(0.7)).sum() == 7, (case, io[:, 0, :10])
    out['recall_json'] = np.array(json.dumps({'thresholds': CASES, 'recall': recalls}))

    # ---- state-dict manifests of the three vehicle configs, from the reference's build_network
    for tag in ('grm', 'prm', 'crm'):
        cfg = yaml.safe_load(open(feat.REF + '/refining/tools/cfgs/ref_model_cfgs/vehicle_%s_model.yaml' % tag))
        model = ref_models.build_network(AttrDict(cfg['MODEL']), types.SimpleNamespace(tta=False))
        out[tag + '_keys'] = np.array(list(model.state_dict().keys()))
        out[tag + '_shapes'] = np.array([str(tuple(v.shape)) for v in model.state_dict().values()])
    path = os.path.join(HERE, 'refine_model_golden.npz')
    np.savez_compressed(path, **out)
    print('saved %d arrays, %d KiB' % (len(out), os.path.getsize(path) // 1024))


RECALL_SIDE = ('input', 'output')

if __name__ == '__main__':
    main()
