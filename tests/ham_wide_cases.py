"""Scenes of the wide Hamming matcher tests (rows of 33..64 bytes; tests/ham_cases.py holds the narrow ones). The CPU reference test
and the GPU test share them, so that what the CPU test shows about a scene holds for the scene the GPU runs."""
from __future__ import annotations

import functools

import numpy as np

import ham_cases as HC
import ham_reference as R

RATIO = HC.RATIO
SEED = 21

# name -> (bytes per row, rows per frame, landmarks). Sizes that are no multiple of 32 and unequal within every pair.
SCENES = {
    "w64": (64, [300, 257, 130], 120),                       # BRISK / FREAK: KS 8, no padding bit
    "w61": (61, [237, 150, 65], 90),                         # AKAZE's MLDB, 486 bits stored in 61 bytes: KS 8 with 24 padding bits
    "w48": (48, [130, 97, 65, 33], 60),                      # KS 6
    "w33": (33, [300, 201, 97], 120),                        # the first width the narrow kind refuses: KS 5, 56 padding bits
    "rows64": (64, [0, 1, 2, 31, 33, 65, 257, 300], 40),     # empty, one-row and two-row frames on either side
}


def scene(name):
    nbytes, sizes, landmarks = SCENES[name]
    return HC.binary_frames(nbytes, sizes, landmarks, SEED)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The scene's frames with their distance matrices: computed once, shared by the tests that need them."""
    return R.Scene(scene(name))


def properties(name):
    """(pairs with matches in both directions, rows with a tied minimum and h0 > 0, rows with 5 h0 = 4 h1 and h0 > 0, directed
    matches at RATIO), over the scene's ordered pairs."""
    ref = reference(name)
    both = ties = boundary = matches = 0
    for a, b in HC.ordered_pairs(len(ref.descs)):
        D = ref.D(a, b)
        if D.shape[0] == 0 or D.shape[1] < 2:
            continue
        fwd, bwd = R.directed_from(D, RATIO), R.directed_from(np.ascontiguousarray(D.T), RATIO)
        both += len(fwd[0]) > 0 and len(bwd[0]) > 0
        matches += len(fwd[0])
        _, h0, h1 = R.top2(D)
        ties += int(((h0 == h1) & (h0 > 0)).sum())
        boundary += int(((5 * h0 == 4 * h1) & (h0 > 0)).sum())
    return both, ties, boundary, matches


def pair_at(nbytes, x, h0, h1):
    """Two rows at h0 and h1 bits from x: the first h0 bits flipped, the last h1 bits flipped (boundary_frames' construction)."""
    nbits = 8 * nbytes
    m1, m2 = np.zeros(nbits, np.uint8), np.zeros(nbits, np.uint8)
    m1[:h0] = 1
    m2[nbits - h1:] = 1
    return x ^ np.packbits(m1), x ^ np.packbits(m2)
