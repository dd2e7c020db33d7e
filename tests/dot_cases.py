"""Scenes of the dot-product matcher tests (CPU reference test and GPU test share them, so that what the CPU test shows about a
scene — its acceptance band, its gaps — holds for the scene the GPU runs)."""
from __future__ import annotations

import numpy as np

from eacham_amd import synth

MIN_SCORE = 0.5  # true correspondences of unit_float_descriptors score ~0.98, unrelated rows |s| < ~0.5 at these dims

# name -> (dim, rows per frame, shared rows, seed): sizes that are not multiples of 32 and unequal within every pair; the seeds are
# picked so that every row's best and second-best similarity are more than 1e-4 apart (asserted by tests/test_match_dot_reference.py)
SCENES = {
    "d64": (64, [237, 150, 301, 97], 80, 101),
    "d128": (128, [205, 333, 97, 161], 80, 1442),
    "d256": (256, [130, 75, 201], 60, 223),
    "d100": (100, [237, 150, 301, 97], 80, 784),   # a dim that is not a multiple of 32
}


def float_frames(dim, sizes, shared, seed, noise=0.15):
    """Float-mode descriptors of eacham_amd/synth.py: every frame holds noisy copies of the same `shared` unit rows (true
    correspondences) + unrelated rows, in an order of its own."""
    base = synth.unit_float_descriptors(max(shared, 1), dim, seed, 99)
    frames = []
    for f, n in enumerate(sizes):
        d = synth.unit_float_descriptors(max(n, shared), dim, seed, f, shared=base[:shared], noise=noise)
        d = d[synth.rng_permutation(seed, 700 + f, d.shape[0])][:n]
        frames.append(np.ascontiguousarray(d, np.float32))
    return frames


def scene(name):
    dim, sizes, shared, seed = SCENES[name]
    return float_frames(dim, sizes, shared, seed)


def ordered_pairs(n):
    return np.array([(i, j) for i in range(n) for j in range(n) if i != j], np.int32)


def negative_pair(n=70, dim=64, seed=7):
    """A pair whose true similarities are ALL negative: unit rows around one common direction, and the negated frame plus
    noise as the train frame. A zero (padding) row would beat every real one."""
    c = synth.rng_normal(seed, 1, (1, dim))
    c /= np.linalg.norm(c)
    a = c * np.sqrt(dim) + 0.5 * synth.rng_normal(seed, 2, (n, dim))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = -(a * np.sqrt(dim) + 0.15 * synth.rng_normal(seed, 3, (n, dim)))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    b = b[synth.rng_permutation(seed, 4, n)]
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


def multi_launch_batch(rows=2000):
    """Pairs per launch of run_match_f32's planner for frames of `rows` rows (eacham_amd/csrc/matcher_f32.hip, plan_match_f32):
    tiles = rows / 32 rounded up to a multiple of 4; per_pair = row results + column partials + match list + count;
    batch = 1 GiB / per_pair."""
    tiles = ((rows + 31) // 32 + 3) // 4 * 4
    row_stride = 32 * tiles
    per_pair = row_stride * 16 + tiles * row_stride * 16 + row_stride * 8 + 4
    return (1 << 30) // per_pair
