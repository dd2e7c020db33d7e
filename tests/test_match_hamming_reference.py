"""CPU: the reference of the Hamming matcher (tests/ham_reference.py), the embedding and the predicate the device relies on, and
the scenes the GPU test runs (tests/ham_cases.py)."""
import numpy as np
import pytest

import ham_cases as HC
import ham_reference as R


def test_table_popcount_against_unpackbits():
    rows = HC._bytes(5, 9, (300, 32))
    assert np.array_equal(R.popcount(rows), np.unpackbits(rows, axis=1).sum(axis=1))
    assert np.array_equal(R.POPCOUNT, np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1))
    a, b = rows[:70], rows[70:200]
    want = (np.unpackbits(a, axis=1)[:, None, :] != np.unpackbits(b, axis=1)[None, :, :]).sum(axis=2)
    assert np.array_equal(R.distances(a, b), want)


@pytest.mark.parametrize("nbytes", [1, 8, 17, 32])
def test_squared_l2_of_the_embedding_is_65025_hamming(nbytes):
    a, b = HC._bytes(6, nbytes, (40, nbytes)), HC._bytes(7, nbytes, (55, nbytes))
    ea, eb = R.embed(a).astype(np.int64), R.embed(b).astype(np.int64)
    d2 = ((ea[:, None, :] - eb[None, :, :]) ** 2).sum(axis=2)
    assert np.array_equal(d2, 65025 * R.distances(a, b).astype(np.int64))
    assert d2.max() <= 256 * 255 * 255 < 1 << 24


def test_predicate_table():
    """All h0, h1 <= 256: at ratio 0.8 the fp32 quotient compared as double is 5 h0 < 4 h1; the same quotient comes out of the
    squared distances 65025 h the kernels hold (both exact in fp32); the square-root route disagrees exactly on 5 h0 = 4 h1."""
    h0, h1 = np.meshgrid(np.arange(257), np.arange(257), indexing="ij")
    got = R.ratio_pass(h0, h1, 0.8)
    assert np.array_equal(got, 5 * h0 < 4 * h1)
    assert not R.ratio_pass(0, 0, 0.8) and R.ratio_pass(0, 3, 0.8) and not R.ratio_pass(3, 3, 0.8) and not R.ratio_pass(4, 5, 0.8)
    with np.errstate(divide="ignore", invalid="ignore"):
        q_h = h0.astype(np.float32) / h1.astype(np.float32)
        q_d2 = (65025 * h0).astype(np.float32) / (65025 * h1).astype(np.float32)
    assert np.array_equal(q_h.view(np.uint32)[h1 > 0], q_d2.view(np.uint32)[h1 > 0])
    with np.errstate(divide="ignore", invalid="ignore"):
        root = (np.sqrt((65025 * h0).astype(np.float32)) / np.sqrt((65025 * h1).astype(np.float32))).astype(np.float64) < np.sqrt(0.8)
    wrong = np.argwhere((root != got) & (h0 <= h1) & (h1 > 0))
    assert len(wrong) and all(5 * a == 4 * b for a, b in wrong) and [4, 5] in wrong.tolist() and [8, 10] in wrong.tolist()


@pytest.mark.parametrize("name", sorted(HC.SCENES))
def test_every_scene_is_non_vacuous(name):
    both, ties, boundary = HC.properties(name)
    assert both > 0, "no pair with matches in both directions"
    assert ties > 0, "no tied minimum for the lower index to decide"
    assert boundary > 0, "no row with 5 h0 = 4 h1"
    ref = HC.reference(name)
    ordered = HC.ordered_pairs(len(ref.descs))
    # a tie is visible in a result: the directed form at a ratio above 1 keeps tied rows, with the lower train index
    loose, tight = ref.match_pairs_directed(ordered, 1.25), ref.match_pairs_directed(ordered, HC.RATIO)
    assert loose[0].sum() > tight[0].sum() > 0
    rows = sum(ref.descs[a].shape[0] for a, _ in ordered)
    assert tight[0].sum() < rows                                   # the ratio test cuts both ways


def test_boundary_frames_and_forms():
    q, t, cases, expect = HC.boundary_frames()
    D = R.distances(q, t)
    _, h0, h1 = R.top2(D)
    assert [(int(a), int(b)) for a, b in zip(h0, h1)] == cases
    gq, gt, gd = R.match_directed(q, t, 0.8)
    assert gq.tolist() == [5, 6] and gt.tolist() == expect[[5, 6]].tolist() and gd.tolist() == [0, 3]
    # forms: an empty and a one-row train frame give nothing; CSR offsets are the running sum
    descs = [q, t, t[:1], t[:0]]
    c, o, *_ = R.match_pairs_directed(descs, [[0, 1], [0, 2], [0, 3], [3, 0]], 0.8)
    assert c.tolist() == [2, 0, 0, 0] and o.tolist() == [0, 2, 2, 2, 2]
    c, o, mq, mt, md, st = R.match_all_pairs(descs, [[0, 1], [1, 0]], 0.8, 0, -1)
    assert st[0, 3] == 1 and c[0] == c[1] > 0
    assert sorted(zip(mq[o[0]:o[1]].tolist(), mt[o[0]:o[1]].tolist())) == sorted(zip(mt[o[1]:o[2]].tolist(), mq[o[1]:o[2]].tolist()))
    assert R.match_all_pairs(descs, [[0, 1]], 0.8, 3, -1)[0].tolist() == [0]        # |m12| = 2 < min_dir
