"""CPU: the reference of the dot-product matcher (tests/cpp/dot_reference.c via tests/dot_reference.py) held against a float64
numpy evaluation and hand-made cases; the scenes the GPU test uses are checked here for their acceptance band; the header
declares the three dot-product entry points and the built library exports them."""
import os
import re

import numpy as np
import pytest

import dot_cases as DC
import dot_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["eacham_match_pair_dot", "eacham_match_pairs_directed_dot", "eacham_match_all_pairs_dot"]


def _np_directed(A, B, min_score):
    S = A.astype(np.float64) @ B.astype(np.float64).T
    best = S.argmax(axis=1)                      # first maximum = lower index
    keep = S[np.arange(len(A)), best] > min_score
    return np.flatnonzero(keep), best[keep], S


@pytest.mark.parametrize("name", sorted(DC.SCENES))
def test_reference_indices_against_float64(name):
    descs = DC.scene(name)
    for a, b in DC.ordered_pairs(len(descs)):
        A, B = descs[a], descs[b]
        q64, t64, S = _np_directed(A, B, DC.MIN_SCORE)
        top2 = np.sort(S, axis=1)[:, -2:]
        gap = top2[:, 1] - top2[:, 0]
        assert gap.min() > 1e-4, (name, a, b, gap.min())                       # rounding cannot decide the argmax
        assert np.abs(top2[:, 1] - DC.MIN_SCORE).min() > 1e-4                    # ... nor the threshold
        q, t, s = R.match_directed(A, B, DC.MIN_SCORE)
        assert np.array_equal(q, q64) and np.array_equal(t, t64)
        assert np.abs(s - S[q64, t64]).max() <= A.shape[1] * 2.0 ** -24           # dim roundings of at most half an ulp of a partial sum <= sum|a_k b_k| <= 1 (unit rows)
        best, sc = R.argmax(A, B)
        assert np.array_equal(best, S.argmax(axis=1))
        # mutual form: m21 from the transposed problem
        qb, tb, _ = _np_directed(B, A, DC.MIN_SCORE)
        m21 = dict(zip(qb.tolist(), tb.tolist()))
        mut = [(i, j) for i, j in zip(q64.tolist(), t64.tolist()) if m21.get(j) == i]
        qm, tm, sm, st = R.match_mutual(A, B, DC.MIN_SCORE, 0, -1)
        assert list(zip(qm.tolist(), tm.tolist())) == mut
        assert st.tolist() == [len(q64), len(qb), len(mut), 1]
        assert np.array_equal(sm, s[np.isin(q, qm)])


@pytest.mark.parametrize("name", sorted(DC.SCENES))
def test_scenes_exercise_both_branches_of_the_threshold(name):
    """What the GPU test asserts on the reference's output, shown here for the same scenes: 10 % .. 90 % of the rows accepted."""
    descs = DC.scene(name)
    pairs = DC.ordered_pairs(len(descs))
    counts, *_ = R.match_pairs_directed(descs, pairs, DC.MIN_SCORE)
    rows = sum(descs[a].shape[0] for a, _ in pairs)
    assert 0.10 * rows <= counts.sum() <= 0.90 * rows, (counts.sum(), rows)


def test_thresholds_of_the_mutual_form():
    descs = DC.scene("d64")
    A, B = descs[0], descs[1]
    q, t, s, st = R.match_mutual(A, B, DC.MIN_SCORE, 0, -1)
    m = int(st[2])
    assert m > 10 and len(q) == m
    assert len(R.match_mutual(A, B, DC.MIN_SCORE, 0, m)[0]) == 0           # |mutual| > min_mutual is strict
    assert len(R.match_mutual(A, B, DC.MIN_SCORE, 0, m - 1)[0]) == m
    assert len(R.match_mutual(A, B, DC.MIN_SCORE, int(min(st[0], st[1])) + 1, -1)[0]) == 0   # a direction below min_dir
    assert len(R.match_mutual(A, B, DC.MIN_SCORE, int(min(st[0], st[1])), -1)[0]) == m
    assert R.match_mutual(A, B, DC.MIN_SCORE, 0, m)[3].tolist() == [st[0], st[1], m, 0]     # stats are reported either way


def test_duplicate_train_rows_resolve_to_the_lower_index():
    A = np.array([[1, 0, 0, 0], [0, 1, 0, 0]], np.float32)
    B = np.array([[0, 1, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0]], np.float32)
    q, t, s = R.match_directed(A, B, 0.5)
    assert q.tolist() == [0, 1] and t.tolist() == [1, 0] and s.tolist() == [1.0, 1.0]
    # by column the duplicates tie too: rows 1 and 2 of B both choose row 0 of A, only (0, 1) is mutual
    qm, tm, _, st = R.match_mutual(A, B, 0.5, 0, -1)
    assert list(zip(qm.tolist(), tm.tolist())) == [(0, 1), (1, 0)] and st.tolist() == [2, 4, 2, 1]


def test_similarity_equal_to_min_score_is_rejected():
    A = np.array([[0.5, 0.0], [1.0, 0.0]], np.float32)
    B = np.array([[1.0, 0.0]], np.float32)
    q, t, s = R.match_directed(A, B, 0.5)             # row 0 scores exactly 0.5: strict '>' rejects it
    assert q.tolist() == [1] and t.tolist() == [0] and s.tolist() == [1.0]
    q, _, _ = R.match_directed(A, B, np.nextafter(np.float32(0.5), np.float32(0)))
    assert q.tolist() == [0, 1]


def test_one_row_and_zero_row_train_frames():
    A = DC.scene("d64")[0]
    one = A[5:6].copy()
    q, t, s = R.match_directed(A, one, 0.9)           # legal, unlike the L2 form: no second neighbour is needed
    assert q.tolist() == [5] and t.tolist() == [0]
    q, t, s = R.match_directed(A, one, -2.0)
    assert len(q) == len(A) and not t.any()
    empty = np.zeros((0, A.shape[1]), np.float32)
    assert len(R.match_directed(A, empty, -2.0)[0]) == 0
    assert len(R.match_directed(empty, A, -2.0)[0]) == 0
    qm, _, _, st = R.match_mutual(A, empty, -2.0, 0, -1)
    assert len(qm) == 0 and st.tolist() == [0, 0, 0, 1]


def test_nan_and_minus_infinity_never_win_and_never_pass():
    A = np.array([[1.0, 0.0], [np.nan, 0.0]], np.float32)
    B = np.array([[np.nan, 0.0], [0.25, 0.0], [-np.inf, 0.0]], np.float32)
    q, t, s = R.match_directed(A, B, -np.inf)
    assert q.tolist() == [0] and t.tolist() == [1] and s.tolist() == [0.25]
    assert len(R.match_directed(A, B, np.nan)[0]) == 0


def test_padding_scene_is_all_negative():
    a, b = DC.negative_pair()
    S = a.astype(np.float64) @ b.astype(np.float64).T
    assert a.shape[0] == 70 and S.max() < -0.1          # a zero row would beat every real one
    q, t, s = R.match_directed(a, b, -2.0)
    assert np.array_equal(q, np.arange(70)) and t.max() < 70 and s.max() < 0


def test_header_declares_and_library_exports_the_dot_entry_points():
    text = open(os.path.join(ROOT, "include", "eacham_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(eacham_[a-z0-9_]+)\s*\(", text))
    assert all(s in declared for s in ENTRY_POINTS), sorted(set(ENTRY_POINTS) - declared)
    from eacham_amd import capi
    L = capi.lib()
    assert all(hasattr(L, s) for s in ENTRY_POINTS)
    from eacham_amd import matcher
    for m in ("match_pair_dot", "match_pairs_directed_dot", "match_all_pairs_dot"):
        assert hasattr(matcher.HipContext, m)
