"""CPU: the scenes of the wide Hamming tests are non-vacuous, the key arithmetic of the FP4 sweep (eacham_amd/csrc/matcher_ham_wide.hip)
restated in numpy float32 is exact and ordered, and the library exports the wide entry points."""
import numpy as np
import pytest

from eacham_amd import capi
import ham_cases as HC
import ham_reference as R
import ham_wide_cases as W

# (pairs with matches in both directions, tied minima with h0 > 0, rows with 5 h0 = 4 h1, directed matches at 0.8)
TABLE = {"w64": (6, 100, 1, 586), "w61": (6, 64, 1, 354), "w48": (12, 56, 1, 410), "w33": (6, 115, 1, 498), "rows64": (28, 255, 1, 520)}


@pytest.mark.parametrize("name", sorted(W.SCENES))
def test_scenes_are_not_vacuous(name):
    props = W.properties(name)
    assert all(v > 0 for v in props), props
    assert props == TABLE[name]


def test_wide_scenes_hold_distances_above_256():
    """What the 0 / 255 embedding of the narrow kind cannot hold."""
    assert W.reference("w64").D(0, 1).max() == 306
    assert W.reference("w61").D(0, 1).max() == 290


def test_w64_edges_under_the_reference_thresholds():
    st = W.reference("w64").match_all_pairs([[0, 1], [0, 2], [1, 2]], W.RATIO, 30, 30)[5]
    assert st.tolist() == [[119, 123, 119, 1], [86, 86, 86, 1], [87, 85, 85, 1]]


def test_keys_are_exact_and_ordered_in_float32():
    """key = 2^14 h + idx for every h in 0..512 and idx at the ends and the middle of the 14-bit field: exact in float32, decoded by
    a shift and a mask, and ordered as (h, idx)."""
    h = np.arange(513, dtype=np.int64)[:, None]
    idx = np.array([0, 1, 8191, 8192, 16383], np.int64)[None, :]
    exact = (h << 14) + idx
    key = (np.float32(16384.0) * h.astype(np.float32) + idx.astype(np.float32)).astype(np.float32)
    assert np.array_equal(key.astype(np.int64), exact) and exact.max() == (1 << 23) + (1 << 14) - 1
    assert np.array_equal(key.astype(np.int64) >> 14, np.broadcast_to(h, exact.shape))
    assert np.array_equal(key.astype(np.int64) & 16383, np.broadcast_to(idx, exact.shape))
    flat = key.ravel()                                   # row-major = (h, idx) lexicographic
    assert (np.diff(flat) > 0).all()
    assert key.max() < np.float32(2.0 ** 24) <= np.float32(2.0 ** 25)   # padding rows (2^25) never win


@pytest.mark.parametrize("nbytes", [1, 33, 61, 64])
def test_partial_sums_stay_integers_below_2_24(nbytes):
    """The chain of a row in float32, in two orders: C-init 2^13 D + idx, then -2^13 per agreeing bit and +2^13 per differing bit.
    Every partial sum is an integer in [0, 2^24) and the end is the key, whatever the order."""
    D = 8 * nbytes
    a, b = HC._bytes(5, 1, (4, nbytes)), HC._bytes(5, 2, (4, nbytes))
    a[1], b[1] = 0, 255                                  # h = D
    b[2] = a[2]                                          # h = 0
    for idx in (0, 8191, 16383):
        for x, y in zip(a, b):
            diff = np.unpackbits(x ^ y).astype(np.float32)
            prod = (np.float32(2.0) * diff - np.float32(1.0)) * np.float32(8192.0)
            c0 = np.float32(8192.0 * D + idx)
            for order in (np.arange(D), np.argsort(-diff, kind="stable")):   # as stored; every +2^13 first (the largest partial sums)
                part = c0 + np.cumsum(prod[order], dtype=np.float32)
                assert part.dtype == np.float32
                assert (part >= 0).all() and (part < np.float32(2.0 ** 24)).all() and (part == np.rint(part)).all()
                assert int(part[-1]) == (int(R.distances(x[None], y[None])[0, 0]) << 14) + idx


def test_library_exports_the_wide_entry_points():
    L = capi.lib()
    for name in ("eacham_upload_descriptors_bits_wide", "eacham_upload_descriptors_bits_wide_dev", "eacham_match_debug_hamming_wide_pair",
                 "eacham_match_debug_hamming_wide"):
        assert hasattr(L, name), name
