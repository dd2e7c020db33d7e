"""CPU: the reference of guided matching (tests/guided_reference.py) held to what it must reduce to, and the preconditions of
the cases (tests/guided_cases.py) asserted on the reference alone, so that no GPU case is vacuous."""
import numpy as np
import pytest

import guided_cases as GCS
import guided_reference as GR
import np_reference as NR


def test_no_gate_no_cross_check_is_the_directed_match():
    """max_error = +inf, cross_check = 0 on frames with >= 2 train rows: np_reference.directed."""
    for name in ("twins128", "rows128", "parity", "planar"):
        c = GCS.case_by_name(name)
        for p, (f1, f2) in enumerate(c["pairs"].tolist()):
            if len(c["descs"][f2]) < 2 or not np.all(np.isfinite(c["models"][p])):
                continue
            assert np.all(np.isfinite(GR.errors(c["kind"], c["xys"][f1], c["xys"][f2], c["models"][p], c["K"]))), "a NaN error would gate"
            q, t, d2, stats = GR.guided_pair(c["kind"], c["descs"][f1], c["descs"][f2], c["xys"][f1], c["xys"][f2], c["models"][p], c["K"],
                                             np.inf, 0.8, 0, False)
            wq, wt = NR.directed(c["descs"][f1], c["descs"][f2], 0.8)
            assert np.array_equal(q, wq) and np.array_equal(t, wt), (name, p)
            D = NR.sq_dists(c["descs"][f1], c["descs"][f2])
            assert np.array_equal(d2, D[q.astype(int), t.astype(int)]) and stats.tolist() == [len(wq), 0, len(wq)]


def test_transposed_problem_gives_the_transposed_result():
    """(f2, f1, F') cross-checked = the transposed matches of (f1, f2, F)."""
    c = GCS.twins(128)
    F = c["models"][0]
    for max_error in (4, 0, np.inf):
        q, t, d2, st = GR.guided_pair("fundamental", c["descs"][0], c["descs"][1], c["xys"][0], c["xys"][1], F, None, max_error)
        q2, t2, d22, st2 = GR.guided_pair("fundamental", c["descs"][1], c["descs"][0], c["xys"][1], c["xys"][0], F.reshape(3, 3).T.reshape(9), None, max_error)
        order = np.argsort(t, kind="stable")
        assert np.array_equal(q2, t[order]) and np.array_equal(t2, q[order]) and np.array_equal(d22, d2[order])
        assert st2.tolist() == [st[1], st[0], st[2]]


def test_twins_case_is_not_vacuous():
    c = GCS.twins(128)
    mask = GR.admissible("fundamental", c["xys"][0], c["xys"][1], c["models"][0], None, 4)
    per_row = mask.sum(1)
    assert (per_row == 0).any() and (per_row == 1).any() and (per_row >= 2).any()
    counts, _, q, t, _, stats = GCS.reference("twins128", 0)
    assert counts[0] >= 50, "the gate brings the matches back"
    assert NR.mutual(c["descs"][0], c["descs"][1], 0.8, 0, -1)[2][2] <= 5, "blind mutual matching finds next to nothing"
    truth = c["truth"]
    assert (truth[q.astype(int)] == t.astype(int)).mean() > 0.9


def test_zero_threshold_and_planar_and_essential_cases_find_something():
    assert GCS.reference("planar", 0)[0][0] >= 20
    assert GCS.reference("twinsE_K", 0)[0][0] >= 50
    assert np.array_equal(GCS.reference("twinsE_K", 0)[0], GCS.reference("twinsE_norm", 0)[0]) or GCS.reference("twinsE_norm", 0)[0][0] >= 50
    assert GCS.reference("large_train", 0)[0][0] >= 30
    assert GCS.reference("large_train", 0)[3].max() >= 4096, "a partner beyond the 4 096th train row"


@pytest.mark.parametrize("name", ["twins128", "planar", "multi_pair", "twinsE_K"])
def test_max_d2_cases_cut_some_matches_and_keep_others(name):
    ks = GCS.calls(name)
    for i in (len(ks) - 2, len(ks) - 1):
        assert ks[i]["max_d2"] > 0
        base = 0 if ks[i]["cross_check"] else [j for j, k in enumerate(ks) if not k["cross_check"] and k["max_d2"] == 0 and k["max_error"] == ks[i]["max_error"] and k["ratio"] == ks[i]["ratio"]][0]
        full, cut = GCS.reference(name, base)[0].sum(), GCS.reference(name, i)[0].sum()
        assert 0 < cut < full, (name, i, cut, full)
        assert GCS.reference(name, i)[4].max() <= ks[i]["max_d2"]


def test_duplicated_train_rows():
    c = GCS.duplicates()
    counts, offsets, q, t, d2, stats = GCS.reference("duplicates", 0)      # no cross-check
    got = dict(zip(q[:counts[0]].tolist(), t[:counts[0]].tolist()))
    assert got == c["expect_m12"]
    assert d2[q[:counts[0]].tolist().index(3)] == 0
    counts1 = GCS.reference("duplicates", 2)[0]                            # ratio = 1: equal distances still fail
    assert counts1[0] == counts[0]


def test_dead_models_and_empty_frames_give_empty_pairs():
    c = GCS.multi_pair()
    counts, _, _, _, _, stats = GCS.reference("multi_pair", 0)
    for p, ((f1, f2), M) in enumerate(zip(c["pairs"].tolist(), c["models"])):
        if not np.any(M != 0) or np.all(np.isnan(M)) or 4 in (f1, f2):
            assert counts[p] == 0 and not stats[p].any(), p
    assert counts[-1] > 30 and counts[0] > 30
    lone = [p for p, pr in enumerate(c["pairs"].tolist()) if pr == [0, 5]][0]
    cnt_dir = GCS.reference("multi_pair", 1)[0]      # 4 px^2, no cross-check
    assert cnt_dir[lone] >= 1, "a train frame of one row: its lone admissible row matches"


def test_row_count_case_reaches_the_small_frames():
    c = GCS.row_counts(128)
    counts = GCS.reference("rows128", 1)[0]      # max_error 400, no cross-check
    sizes = [len(d) for d in c["descs"]]
    for p, (f1, f2) in enumerate(c["pairs"].tolist()):
        if sizes[f1] == 0 or sizes[f2] == 0:
            assert counts[p] == 0
    assert sum(counts[p] > 0 for p, (f1, f2) in enumerate(c["pairs"].tolist()) if sizes[f2] == 1) >= 1
