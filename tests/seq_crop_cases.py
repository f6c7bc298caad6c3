"""Test infrastructure: seeded sequences for the sequence crop (frames of raw lidar points with a pose, global boxes) and their
expected crops from the per-frame oracle.  Shared by tests/test_seq_crop.py (CPU) and tests/test_gpu_seq_crop.py."""
import functools

import numpy as np

from oracle import crop as ocrop

CHUNK = 256          # asserted against dz_seq_crop_chunk_points() by the tests that sit on its edges

# name -> (per-frame (boxes, kept points), family)
SHAPES = {
    '1x1x1': ([(1, 1)], 'all'),
    'boxes63_64_65': ([(63, 300), (64, 300), (65, 300)], 'random'),
    'chunk_edges': ([(5, CHUNK - 1), (5, CHUNK), (5, CHUNK + 1)], 'random'),
    'pts255_256_257': ([(5, 255), (5, 256), (5, 257)], 'random'),
    'frame_without_boxes': ([(4, 300), (0, 300), (4, 300)], 'random'),
    'frame_without_points': ([(4, 300), (4, 0), (4, 300)], 'random'),
    'no_frame': ([], 'random'),
    'three_identical_boxes': ([(3, 300)], 'same'),
    'nothing_inside': ([(5, 300), (6, 700)], 'nothing'),
    '5x40x6000': ([(40, 6000)] * 5, 'random'),
    'tracks6': ([(10, 2000), (9, 2000), (10, 1500), (8, 2000), (10, 2100), (10, 2000)], 'random'),
}


@functools.lru_cache(maxsize=None)
def sequence(name, seed=0):
    """-> list of frames (raw (N,6) float64 [x,y,z,intensity,elongation,NLZ] in the lidar frame, pose (4,4), boxes_global (T,7))."""
    spec, family = SHAPES[name]
    rng = np.random.default_rng(9000 + seed)
    frames = []
    for f, (t, m) in enumerate(spec):
        yaw = rng.uniform(-np.pi, np.pi)
        pose = np.eye(4)
        pose[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
        pose[:3, 3] = rng.uniform([-500, -500, -5], [500, 500, 5])
        boxes = np.empty((t, 7))
        boxes[:, :2] = pose[:2, 3] + rng.uniform(-30, 30, (t, 2))
        boxes[:, 2] = pose[2, 3] + rng.uniform(-1, 1, t)
        boxes[:, 3:6] = rng.uniform([2, 1, 1], [8, 4, 3], (t, 3))
        boxes[:, 6] = rng.uniform(-np.pi, np.pi, t)
        if family == 'same' and t:
            boxes[:] = boxes[0]
        if family == 'all':
            boxes[:, 3:6] = [200, 200, 50]
        n_flag = m // 8 + 1                                              # returns inside a no-label zone: dropped by the preparation
        n = m + n_flag
        glob = pose[:3, 3] + rng.uniform([-35, -35, -2], [35, 35, 2], (n, 3))
        if t:
            owner = rng.integers(0, t, n)
            local = rng.uniform(-0.6, 0.6, (n, 3)) * boxes[owner, 3:6]      # enlarged half size = 0.55: on both sides of the faces
            c, s = np.cos(boxes[owner, 6]), np.sin(boxes[owner, 6])
            seeded = np.stack([local[:, 0] * c - local[:, 1] * s, local[:, 0] * s + local[:, 1] * c, local[:, 2]], 1) + boxes[owner, :3]
            half = rng.random(n) < 0.5
            glob[half] = seeded[half]
        if family == 'nothing':
            boxes[:, 0] += 1000
        raw = np.empty((n, 6))
        raw[:, :3] = (glob - pose[:3, 3]) @ pose[:3, :3]                 # the lidar-frame point whose global image is `glob`
        raw[:, 3] = rng.uniform(0, 3, n)
        raw[:, 4] = rng.uniform(0, 1, n)
        raw[:, 5] = -1
        raw[rng.permutation(n)[:n_flag], 5] = 1
        assert int((raw[:, 5] == -1).sum()) == m
        frames.append((raw, pose, boxes))
    return frames


@functools.lru_cache(maxsize=None)
def expected(name, enlarge_scale=1.1, crop_on_bev=False, seed=0):
    """Per-frame oracle crop, flattened in (frame, box) order: list of B (n,4) float64 arrays."""
    out = []
    for raw, pose, boxes in sequence(name, seed):
        if boxes.shape[0]:
            out += ocrop.crop_frame_objects(raw, pose, boxes, enlarge_scale, crop_on_bev)
    return out


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def object_major(spec):
    """Boxes of a (T_f) list, box k of a frame = object k: (rank, boxes per object) for the (object, frame) order."""
    keys = [(k, f) for f, t in enumerate(spec) for k in range(t)]
    order = sorted(range(len(keys)), key=lambda i: keys[i])
    rank = np.empty(len(keys), dtype=np.int64)
    rank[order] = np.arange(len(keys))
    n_obj = max([t for t in spec], default=0)
    return rank, [sum(1 for t in spec if t > k) for k in range(n_obj)]
