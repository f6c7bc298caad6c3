"""Golden vectors for the tracker with FILTER.NAME AB3DMOT, from the REFERENCE's own classes, CPU.

    python tests/golden/gen_track_ab3dmot_golden.py      (build container only; needs /root/reference)

The pin is the reference's ``AB3DMOT`` (kalman_filter/ab3dmot.py) and ``TrackManager`` (track_manager.py), imported by path, OVER THE
STAND-IN ``KalmanFilter`` BELOW: filterpy is not installed where this runs, so ``filterpy.kalman.KalmanFilter`` is a class written
here from the filter's equations (x (dim_x, 1) float64; P, Q, R, F identity, H zero; predict: x = F x, P = F P F^T + Q; update:
y = z - H x, S = H P H^T + R, K = P H^T inv(S) with np.linalg.inv, x += K y, P = (I - K H) P (I - K H)^T + K R K^T).  The other
stand-ins are those of gen_track_model_golden.py (np.int / np.bool for numpy 2, .cuda() a no-op, the iou3d imports backed by the
oracle's C restatement, easydict from the shim's fall-back).

Two runs on one seeded sequence (detzero_amd.synth.synth_track_sequence, edited as described at ``sequence``):
  r0  the MODEL values of tools/cfgs/tk_model_cfgs/waymo_ab3dmot.yaml as shipped: one stage, no merge, no reverse, BIRTH_AGE 3,
      DEATH_AGE 2.  (The file's DATA_CONFIG part has a mis-indented THRESHOLD line that no YAML parser accepts, so the text is read
      from its ``MODEL:`` line on.)
  r1  the same with the two-stage association and TRACK_MERGE of waymo_detzero_track.yaml.
The detections are float64 arrays holding float32-representable values, so rounding on upload is not a difference.  The frame ids
differ from the ordinals; some are below BIRTH_AGE.  The generator ASSERTS the scripted events in the reference's own results (a gap
of one frame survived, a gap of two frames ending a track and a new id taking over, an empty frame, headings crossing +-pi, the
obtuse-angle flip, the >= 3 pi / 2 branch, a measurement wrapped), and - as gen_track_model_golden.py - that no affinity or merge
ratio sits within its gap of a threshold and no assignment moves under a +-1e-4 perturbation of the costs; it walks the seeds until
the conditions hold and stores the gaps.  ``solve_diff`` = the largest difference between the reference's boxes and the numpy
restatement (tests/track_ab3dmot_ref.py) run with a Cholesky solve instead of inv: the unit of the sequence-level tolerance.
"""
import copy
import importlib
import json
import math
import os
import sys

import numpy as np
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_track_model_golden as base  # noqa: E402  (sets the numpy aliases and the import paths)

REF = base.REF
GAP = base.GAP
N_FRAMES, N_OBJECTS = 20, 12
EVENTS = {'missing': {1: [8], 3: [9, 10]}, 'dup': {5: 6}, 'false_pos': [(1, 1), (7, 2)], 'empty': [13], 'low': {6: [5, 11]}}
CROSS, FLIP, FLIP_FRAME = 0, 2, 7          # objects: heading walks across +pi; one detection turned by pi


class KalmanFilter:
    """Stand-in for filterpy.kalman.KalmanFilter, written from the equations (see the module docstring)."""

    def __init__(self, dim_x, dim_z):
        self.dim_x, self.dim_z = dim_x, dim_z
        self.x = np.zeros((dim_x, 1))
        self.P, self.Q, self.F = np.eye(dim_x), np.eye(dim_x), np.eye(dim_x)
        self.H, self.R = np.zeros((dim_z, dim_x)), np.eye(dim_z)

    def predict(self):
        self.x = np.dot(self.F, self.x)
        self.P = np.dot(np.dot(self.F, self.P), self.F.T) + self.Q

    def update(self, z):
        z = np.asarray(z, dtype=np.float64).reshape(self.dim_z, 1)
        y = z - np.dot(self.H, self.x)
        pht = np.dot(self.P, self.H.T)
        s = np.dot(self.H, pht) + self.R
        k = np.dot(pht, np.linalg.inv(s))
        self.x = self.x + np.dot(k, y)
        i_kh = np.eye(self.dim_x) - np.dot(k, self.H)
        self.P = np.dot(np.dot(i_kh, self.P), i_kh.T) + np.dot(np.dot(k, self.R), k.T)


def import_reference():
    tk, _ = base.import_reference()
    sys.modules['filterpy.kalman'].KalmanFilter = KalmanFilter
    ab = importlib.import_module('detzero_track.models.tracking_modules.kalman_filter.ab3dmot')
    ab.KalmanFilter = KalmanFilter
    return tk, ab


def count_branches(ab, original, counts):
    """Wrap AB3DMOT.update (``original``) so that the branches an update takes are counted (the conditions restated on copies)."""

    def update(self, bbox, name, score, num_points, two_stage=False):
        th, new = float(self.kf.x[6, 0]), float(bbox[6])
        wrap = lambda v: v - np.pi * 2 if v >= np.pi else (v + np.pi * 2 if v < -np.pi else v)
        counts['z_wrap'] += int(wrap(new) != new)
        th, new = wrap(th), wrap(new)
        if np.pi / 2.0 < abs(new - th) < np.pi * 3 / 2.0:
            counts['flip'] += 1
            th += np.pi
            if th > np.pi:
                th -= np.pi * 2
            if th < -np.pi:
                th += np.pi * 2
        counts['wide'] += int(abs(new - th) >= np.pi * 3 / 2.0)
        counts['second_stage'] += int(bool(two_stage))
        return original(self, bbox, name, score, num_points, two_stage=two_stage)
    ab.AB3DMOT.update = update


def sequence(seed):
    """The seeded sequence with: float64 boxes of float32 values; object CROSS's heading walking from pi - 0.05 upwards by 0.012 a
    frame, unwrapped (so above pi) up to frame 11 and wrapped from frame 12 on; object FLIP's detection of frame FLIP_FRAME turned
    by pi; the frame keys 1, 2, 4, 5, 7, 8, ... instead of the ordinals.  -> ({key: frame}, the objects' noise-free centres)."""
    from detzero_amd.synth import synth_track_ground_truth, synth_track_sequence
    seq = synth_track_sequence(seed, N_FRAMES, N_OBJECTS, origin=(2100.0, -900.0, 20.0), events=EVENTS, sequence_name='seq_ab3dmot')
    gt = synth_track_ground_truth(seed, N_FRAMES, N_OBJECTS, origin=(2100.0, -900.0, 20.0), events=EVENTS)
    out = {}
    for f in range(N_FRAMES):
        fr = seq[str(f)]
        boxes = fr['boxes_global'].astype(np.float32)
        centres = gt[str(f)]['annos']['gt_boxes_global'][:, :3]
        for obj, heading in ((CROSS, math.pi - 0.05 + 0.012 * f - (2 * math.pi if f >= 12 else 0.0)), (FLIP, None)):
            if len(boxes) == 0:
                continue
            near = np.flatnonzero(np.linalg.norm(boxes[:, :2] - centres[obj, :2], axis=1) < 0.3)
            for j in near:
                if heading is not None:
                    boxes[j, 6] = heading
                elif f == FLIP_FRAME:
                    boxes[j, 6] = boxes[j, 6] + math.pi if boxes[j, 6] < 0 else boxes[j, 6] - math.pi
        key = str(f + 1 + f // 2)
        out[key] = {'boxes_global': boxes.astype(np.float64), 'name': fr['name'], 'score': fr['score'], 'num_points': fr['num_points'],
                    'pose': fr['pose']}
    return out


def models():
    with open(REF + '/tracking/tools/cfgs/tk_model_cfgs/waymo_ab3dmot.yaml') as f:
        text = f.read()
    shipped = yaml.safe_load(text[text.index('MODEL:'):])['MODEL']
    with open(REF + '/tracking/tools/cfgs/tk_model_cfgs/waymo_detzero_track.yaml') as f:
        detzero = yaml.safe_load(f)['MODEL']['TRACKING']
    second = copy.deepcopy(shipped)
    second['TRACKING']['DATA_ASSOCIATION']['STAGE'] = copy.deepcopy(detzero['DATA_ASSOCIATION']['STAGE'])
    second['TRACKING']['TRACK_MERGE'] = copy.deepcopy(detzero['TRACK_MERGE'])
    return [shipped, second]


def run_mine(model, seq, solve, gaps=None):
    from tests import track_ab3dmot_ref
    from detzero_amd.config import AttrDict
    from detzero_amd.track_models import TrackManager
    ops = track_ab3dmot_ref.NumpyAb3dTrackOps(solve=solve, gaps=gaps)
    return TrackManager(AttrDict(model).TRACKING, ops_factory=lambda: ops).forward(copy.deepcopy(seq)), ops


def events_present(ref_raw, seq, counts, birth_age):
    keys = sorted(seq.keys(), key=int)
    last = keys[-1]
    hits = [''.join(str(int(h)) for h in t['hit']) for t in ref_raw.values()]
    if not any('101' in h for h in hits):
        return 'no gap of one frame survived'
    died = [t for t in ref_raw.values() if t['hit'][-1] == 0 and str(t['sample_idx'][-1]) != last and int(np.sum(t['hit'])) >= birth_age]
    born = [t for t in ref_raw.values() if int(t['sample_idx'][0]) >= birth_age]
    if not any(int(b['sample_idx'][0]) > int(d['sample_idx'][-1]) and np.linalg.norm(b['boxes_global'][0, :2] - d['boxes_global'][-1, :2]) < 5.0
               for d in died for b in born):
        return 'no track ended by a gap of two frames with a new id taking over'
    if not any(len(fr['score']) == 0 for fr in seq.values()):
        return 'no empty frame'
    if not any(int(t['sample_idx'][0]) < birth_age for t in ref_raw.values()) or not any(int(k) < birth_age for k in keys):
        return 'no row logged through the frame-id half of the output rule'
    if [int(k) for k in keys] == list(range(len(keys))):
        return 'frame ids equal the ordinals'
    for key in ('flip', 'wide', 'z_wrap'):
        if counts[key] == 0:
            return 'no update through the %s branch' % key
    return None


def try_seed(seed, tk, ab, original, all_models):
    from easydict import EasyDict
    rng = np.random.default_rng(seed)
    seq = sequence(seed)
    out, gaps_all = {}, {'affinity': 1.0, 'merge': 1.0, 'score': 1.0}
    for ri, model in enumerate(all_models):
        counts = {'flip': 0, 'wide': 0, 'z_wrap': 0, 'second_stage': 0}
        count_branches(ab, original, counts)
        cfg = EasyDict(copy.deepcopy(model))
        ref_raw = tk.TrackManager(cfg.TRACKING).forward(copy.deepcopy(seq))
        why = events_present(ref_raw, seq, counts, model['TRACKING']['TRACK_AGE']['BIRTH_AGE'])
        if why:
            return None, 'run %d: %s' % (ri, why)
        if ri == 1 and counts['second_stage'] == 0:
            return None, 'run 1: no second-stage match'
        gaps = {}
        mine, ops = run_mine(model, seq, 'cholesky', gaps)
        if list(mine.keys()) != list(ref_raw.keys()):
            return None, 'run %d: track ids differ from the restatement' % ri
        if ri == 1 and len(gaps.get('merge', [])) == 0:
            return None, 'run 1: the merge saw no pair'
        for key in ('affinity', 'merge'):
            if gaps.get(key):
                gaps_all[key] = min(gaps_all[key], min(gaps[key]))
        stage = model['TRACKING']['DATA_ASSOCIATION']['STAGE']
        if 'SECOND_STAGE' in stage:
            for fr in seq.values():
                if len(fr['score']):
                    gaps_all['score'] = min(gaps_all['score'], float(np.min(np.abs(fr['score'] - stage['SECOND_STAGE']['SCORE_THRESHOLD'][0]))))
        if not base.assignments_stable(ops.costs, rng):
            return None, 'run %d: an assignment moves under a 1e-4 perturbation' % ri
        solve_diff = 0.0
        for tid, t in ref_raw.items():
            if not np.array_equal(t['hit'], mine[tid]['hit']) or not np.array_equal(t['sample_idx'], mine[tid]['sample_idx']):
                return None, 'run %d: rows differ from the restatement' % ri
            solve_diff = max(solve_diff, float(np.max(np.abs(t['boxes_global'].astype(np.float64) - mine[tid]['boxes_global']))))
        p = 'r%d_' % ri
        keys = sorted(seq.keys(), key=int)
        out[p + 'frame_ids'] = np.array([int(k) for k in keys], dtype=np.int64)
        for k in keys:
            for key in ('boxes_global', 'name', 'score', 'num_points', 'pose'):
                out['%sf%s_%s' % (p, k, key)] = seq[k][key]
        out[p + 'raw_ids'] = np.array(list(ref_raw.keys()), dtype=np.int64)
        out[p + 'raw_len'] = np.array([len(t['hit']) for t in ref_raw.values()], dtype=np.int64)
        out[p + 'raw_box_dtype'] = np.array([str(t['boxes_global'].dtype) for t in ref_raw.values()])
        for key in ('boxes_global', 'name', 'score', 'sample_idx', 'hit', 'num_points', 'obj_ids', 'pose'):
            parts = [np.asarray(t[key]) for t in ref_raw.values()]
            if key == 'boxes_global':
                parts = [q.astype(np.float64) for q in parts]
            out['%sraw_%s' % (p, key)] = np.concatenate(parts, axis=0)
        out[p + 'solve_diff'] = np.array(solve_diff)
        out[p + 'model'] = np.array(json.dumps(model))
        out[p + 'branches'] = np.array(json.dumps(counts))
    for key, val in gaps_all.items():
        if val < GAP:
            return None, '%s gap %.2e' % (key, val)
        out['gap_' + key] = np.array(val)
    return out, 'ok'


def main():
    tk, ab = import_reference()
    original = ab.AB3DMOT.update
    all_models = models()
    for seed in range(300, 400):
        out, why = try_seed(seed, tk, ab, original, all_models)
        print('seed %d: %s' % (seed, why))
        if out is not None:
            out['seed'] = np.array(seed)
            path = os.path.join(HERE, 'track_ab3dmot_golden.npz')
            np.savez_compressed(path, **out)
            print('saved %d arrays, %d KiB' % (len(out), os.path.getsize(path) // 1024))
            print({k: (float(v) if v.dtype.kind == 'f' else str(v)) for k, v in out.items()
                   if k.startswith('gap_') or k.endswith('solve_diff') or k.endswith('branches')})
            return
    raise SystemExit('no seed met the conditions')


if __name__ == '__main__':
    main()
