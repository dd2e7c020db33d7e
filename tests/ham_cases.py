"""Scenes of the Hamming matcher tests (the CPU reference test and the GPU test share them, so that what the CPU test shows
about a scene — matches in both directions, ties, rows on the boundary of the ratio test — holds for the scene the GPU runs)."""
from __future__ import annotations

import functools

import numpy as np

from eacham_amd import synth

import ham_reference as R

RATIO = 0.8
FLIP = 0.08   # probability that an observation flips a bit of its landmark

# name -> (bytes per row, rows per frame, landmarks, seed). Sizes that are no multiple of 32 and unequal within every pair. The
# seeds are picked so that every scene is non-vacuous (tests/test_match_hamming_reference.py asserts it).
SCENES = {
    "b8": (8, [300, 257, 65, 33], 120, 11),      # KS 2: the bound form
    "b16": (16, [300, 201, 97], 120, 12),        # KS 4: the bound form
    "b32": (32, [300, 257, 130], 120, 13),       # KS 8: the screen
    "b17": (17, [237, 150, 65], 90, 14),         # 136 bits, padded to 256
    "b1": (1, [12, 14, 9], 5, 74),               # 8 bits padded to 16: ties everywhere
    "rows": (16, [0, 1, 2, 31, 33, 65, 257, 300], 40, 16),
}


def _bytes(seed, stream, shape):
    w = synth.rng_u64(seed, stream, np.arange(int(np.prod(shape)), dtype=np.uint64))
    return (w >> np.uint64(56)).astype(np.uint8).reshape(shape)


def _flips(seed, stream, shape, p):
    """Random masks with every bit set with probability p."""
    u = synth.rng_uniform(seed, stream, (*shape, 8)) < p
    return np.packbits(u, axis=-1).reshape(shape)


def _mask(nbytes, nbits):
    """A row with its first nbits bits set (nbits <= 8 nbytes)."""
    bits = np.zeros(8 * nbytes, np.uint8)
    bits[:nbits] = 1
    return np.packbits(bits)


def binary_frames(nbytes, sizes, landmarks, seed, flip=FLIP, inject=True):
    """Every frame observes some of the same `landmarks` base rows, each bit flipped with probability `flip`, and adds
    distractors; the rows are shuffled. The first two frames with eight rows or more get, in the place of distractors: a
    duplicated observation in the second (a tied minimum for the row of the first that observes the same landmark) and a row X
    in the first with rows at 4 and 5 bits from it in the second (5 h0 = 4 h1, the ratio test's boundary, wherever nothing else
    of the second frame lies nearer: always at 8 bytes or more, by the choice of the seed at 1 byte)."""
    base = _bytes(seed, 1, (max(landmarks, 1), nbytes))
    big = [f for f, n in enumerate(sizes) if n >= 8][:2] if inject else []
    frames = []
    for f, n in enumerate(sizes):
        k = min(landmarks, (2 * n) // 3)
        who = synth.rng_permutation(seed, 100 + f, landmarks)[:k]
        obs = base[who] ^ _flips(seed, 200 + f, (k, nbytes), flip)
        rows = np.concatenate([obs, _bytes(seed, 300 + f, (n - k, nbytes))])
        if len(big) == 2 and n - k >= 3:
            x = _bytes(seed, 400, (nbytes,))
            if f == big[0]:
                rows[k] = x
            elif f == big[1]:
                rows[k] = x ^ _mask(nbytes, 4)
                rows[k + 1] = x ^ (_mask(nbytes, 5) if nbytes > 1 else np.array([0x1F], np.uint8))
                rows[k + 2] = rows[0]                 # a duplicate of the first observation
        frames.append(np.ascontiguousarray(rows[synth.rng_permutation(seed, 500 + f, n)], np.uint8))
    return frames


def scene(name):
    nbytes, sizes, landmarks, seed = SCENES[name]
    return binary_frames(nbytes, sizes, landmarks, seed)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The scene's frames with their distance matrices: computed once, shared by the tests that need them."""
    return R.Scene(scene(name))


def ordered_pairs(n):
    return np.array([(i, j) for i in range(n) for j in range(n) if i != j], np.int32)


def properties(name):
    """What makes a scene non-vacuous, over its ordered pairs: (pairs with matches at RATIO whose reverse has matches too, rows
    whose minimum is tied between two train rows with h0 > 0, rows with 5 h0 = 4 h1 and h0 > 0)."""
    ref = reference(name)
    both = ties = boundary = 0
    for a, b in ordered_pairs(len(ref.descs)):
        D = ref.D(a, b)
        if D.shape[0] == 0 or D.shape[1] < 2:
            continue
        fwd, bwd = R.directed_from(D, RATIO), R.directed_from(np.ascontiguousarray(D.T), RATIO)
        both += len(fwd[0]) > 0 and len(bwd[0]) > 0
        _, h0, h1 = R.top2(D)
        ties += int(((h0 == h1) & (h0 > 0)).sum())
        boundary += int(((5 * h0 == 4 * h1) & (h0 > 0)).sum())
    return both, ties, boundary


def boundary_frames(nbytes=32):
    """Hand-built rows on the boundary of the ratio test. Query row i is a random anchor (the anchors lie ~4 nbytes bits apart);
    the train frame holds, per query, two rows at the chosen distances (h0, h1) from it. (4,5), (8,10), (40,50): 5 h0 = 4 h1,
    which Hamming fails and the square-root route (bits as floats under L2 with sqrt(0.8)) lets pass; (0,0), (3,3): ties, fail;
    (0,3), (3,4): pass.
    Returns (query, train, cases, expect) with expect[i] = the train index query i must match, or -1."""
    cases = [(4, 5), (8, 10), (40, 50), (0, 0), (3, 3), (0, 3), (3, 4)]
    nbits = 8 * nbytes
    anchors = _bytes(991, 1, (len(cases), nbytes))     # random anchors: ~nbits / 2 apart from each other
    q, t, expect = [], [], []
    for i, (h0, h1) in enumerate(cases):
        x = anchors[i]
        q.append(x)
        m1 = np.zeros(nbits, np.uint8)
        m1[:h0] = 1
        m2 = np.zeros(nbits, np.uint8)
        m2[nbits - h1:] = 1
        expect.append(len(t) if 5 * h0 < 4 * h1 else -1)
        t.append(x ^ np.packbits(m1))
        t.append(x ^ np.packbits(m2))
    return np.array(q, np.uint8), np.array(t, np.uint8), cases, np.array(expect, np.int64)
