"""CPU: the yardstick of eacham_two_view_batch — per problem ONE call of the single-pair entry point with all of the problem's
candidates, then the host rules in numpy (tests/two_view_batch_cases.py: compose) — run over the CPU oracle's two_view_points and
held against sequential statements of the reference: tests/estimator_reference.py's recover_pose followed by the per-match loop of
ReconstructionManager.cpp:153-177 for the POSES rule, a literal match-by-match loop of :98-144 for the SOLUTIONS rule.
tests/test_two_view_batch_gpu.py runs the same compose over the device library's eacham_two_view_points and holds
eacham_two_view_batch to it byte for byte, so a GPU mismatch can be traced to one side."""
import numpy as np
import pytest

import estimator_reference as ER
import oracle_api as O
import two_view_batch_cases as TC


def oracle_compose(case):
    return TC.compose(O.two_view_points, case)


def K9(K4):
    return np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]])


def one(uv1, uv2, K4, T, i, max_err, min_angle, strict):
    """TriangulatePoint and the keep test of ONE match under ONE transform."""
    pts, keep, _ = O.two_view_points(uv1[i:i + 1], uv2[i:i + 1], K4, T.reshape(1, 16), max_err, min_angle, strict)
    return pts[0, 0], bool(keep[0, 0])


def sequential_solutions(case, p):
    """ReconstructionManager.cpp:98-144, statement for statement: (winner or -1, its matches as (index, point))."""
    uv1, uv2, Ts = case["uv1"][p], case["uv2"][p], case["transforms"][p]
    best_matches, best_num = [], -1
    for i in range(len(Ts)):
        matches = []
        for m in range(len(uv1)):
            point3d, kept = one(uv1, uv2, case["K"], Ts[i], m, case["max_err"], case["min_angle"], True)
            if kept:
                matches.append((m, point3d))
        if len(matches) > len(best_matches):
            best_matches, best_num = matches, i
    if len(best_matches) > case["min_solution_matches"]:
        return best_num, best_matches
    return -1, []


def as_matches(rec):
    return [(int(i), rec["points"][i]) for i in np.flatnonzero(rec["keep"])]


def same_matches(a, b):
    return len(a) == len(b) and all(i == j and np.array_equal(x.view(np.uint64), y.view(np.uint64)) for (i, x), (j, y) in zip(a, b))


@pytest.mark.parametrize("name", ["mixed", "twins", "solutions_only"])
def test_solutions_rule_is_the_sequential_loop(name):
    case = TC.CASES[name]()
    got = oracle_compose(case)
    seen = 0
    for p, g in enumerate(got):
        if case["rules"][p] != "solutions":
            continue
        seen += 1
        winner, matches = sequential_solutions(case, p)
        assert g["winner"] == winner and g["good"] == 0 and not g["pose_mask"].any(), p
        assert g["kept"] == len(matches) and same_matches(as_matches(g), matches), p
    assert seen


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name", ["single", "mixed", "twins"])
def test_poses_rule_is_recover_pose_then_the_match_loop(name, masked):
    case = TC.CASES[name]()
    if masked:
        case = TC.random_mask(case)
    got = oracle_compose(case)
    for p, g in enumerate(got):
        if case["rules"][p] != "poses":
            continue
        uv1, uv2, Ts = case["uv1"][p], case["uv2"][p], case["transforms"][p]
        # cv::recoverPose over the problem's own candidates, one at a time as estimator_reference.recover_pose runs them
        best, votes = None, []
        for k, T in enumerate(Ts):
            r = pose_vote(case, p, T)
            votes.append(r["good"])
            if best is None or r["good"] > best["good"]:
                best = dict(r, winner=k)
        assert g["winner"] == best["winner"] and g["good"] == best["good"] and list(g["cand_counts"]) == votes, p
        assert np.array_equal(g["pose_mask"], best["mask"]), p
        # :153-177 for the winner
        matches = []
        for m in range(len(uv1)):
            point3d, kept = one(uv1, uv2, case["K"], Ts[best["winner"]], m, case["max_err"], case["min_angle"], False)
            if kept:
                matches.append((m, point3d))
        assert g["kept"] == len(matches) and same_matches(as_matches(g), matches), p


def pose_vote(case, p, T):
    """estimator_reference.recover_pose's vote for ONE candidate: its loop body, through recover_pose itself when the candidate list
    is cv::recoverPose's own (test_poses_over_recover_pose_candidates below), restated here for an arbitrary candidate."""
    uv1, uv2 = case["uv1"][p], case["uv2"][p]
    keep = np.ones(len(uv1), bool) if case["in_mask"] is None else case["in_mask"][p].astype(bool)
    pts, _, _ = O.two_view_points(uv1, uv2, case["K"], T.reshape(1, 16), float(np.finfo(np.float32).max), 0.0, False)
    X, M = pts[0], T.reshape(4, 4)
    z1 = X[:, 2]
    z2 = ((M[2, 0] * X[:, 0] + M[2, 1] * X[:, 1]) + M[2, 2] * X[:, 2]) + M[2, 3]
    with np.errstate(invalid="ignore"):
        good = keep & (z1 > 0) & (z1 < case["dist"]) & (z2 > 0) & (z2 < case["dist"])
    return {"good": int(good.sum()), "mask": good.astype(np.uint8)}


@pytest.mark.parametrize("masked", [False, True])
def test_poses_over_recover_pose_candidates(masked):
    """The candidates in cv::recoverPose's own order: compose must give estimator_reference.recover_pose, field for field."""
    import score_cases as SC
    for seed, n in ((3, 70), (4, 257)):
        c = SC.two_view_case(n=n, n_models=1, seed=seed, outliers=0.25, facing=True)
        E = c["E"][0]
        mask = (np.random.default_rng(seed).random(n) < 0.6).astype(np.uint8) if masked else None
        ref = ER.recover_pose(E, c["uv1"], c["uv2"], K9(c["K"]), TC.DIST, mask)
        R1, R2, t = ER.decompose_essential(E)
        Ts = []
        for R, tt in ((R1, t), (R2, t), (R1, -t), (R2, -t)):
            M = np.eye(4)
            M[:3, :3], M[:3, 3] = R, tt
            Ts.append(M.reshape(16))
        case = TC._case([(c["uv1"], c["uv2"], np.array(Ts))], ["poses"], in_mask=None if mask is None else [mask])
        g = oracle_compose(case)[0]
        assert g["winner"] == ref["winner"] and g["good"] == ref["good"] and list(g["cand_counts"]) == ref["votes"]
        assert np.array_equal(g["pose_mask"], ref["mask"]) and ref["good"] > n // 3


def test_the_cases_hold_what_they_are_for():
    """Checked here, through the oracle, before the GPU test relies on it."""
    mix = oracle_compose(TC.mixed())
    rules = TC.mixed()["rules"]
    assert [len(u) for u in TC.mixed()["uv1"]] == TC.MIXED_SIZES and sorted({len(t) for t in TC.mixed()["transforms"]}) == [1, 2, 3, 4]
    assert any(m["winner"] > 0 for m in mix) and any(m["winner"] == 0 for m in mix)
    assert any(m["winner"] >= 0 and r == "solutions" for m, r in zip(mix, rules)) and any(m["winner"] < 0 and r == "solutions" for m, r in zip(mix, rules))
    emp_case = TC.empties()
    emp = oracle_compose(emp_case)
    assert [e["winner"] for e in emp][:1] == [0] and emp[0]["good"] == 0                              # POSES, candidates, no points
    assert [e["winner"] >= 0 for e in emp] == [True, True, False, False, True, False, True, False]
    assert [len(e["cand_counts"]) for e in emp] == [3, 4, 0, 0, 2, 2, 3, 0]
    for t in oracle_compose(TC.twins()):
        cc = t["cand_counts"]
        assert np.array_equal(cc[:4], cc[4:]) and 0 <= t["winner"] < 4 and cc[t["winner"]] == cc.max() > 0
    off = oracle_compose(TC.masked_out())
    assert all(o["winner"] == 0 and o["good"] == 0 and not o["pose_mask"].any() and o["kept"] > 0 for o in off)
    sol = oracle_compose(TC.solutions_only())
    for p, s in enumerate(sol):
        top = int(s["cand_counts"].max())
        assert s["winner"] >= 0 and top > TC.MIN_SOLUTION
        assert oracle_compose(TC.solutions_only(top))[p]["winner"] == -1                             # not strictly above: none
        assert oracle_compose(TC.solutions_only(top - 1))[p]["winner"] == s["winner"]
    deg = oracle_compose(TC.degenerate())
    assert not np.isfinite(deg[3]["points"]).all() or deg[3]["winner"] < 0
    assert all(d["winner"] >= 0 for d in deg[:3])
    with_mask, without = oracle_compose(TC.random_mask(TC.mixed())), mix
    assert any(a["good"] < b["good"] for a, b in zip(with_mask, without))
    for m, r in zip(mix, rules):                                                                    # t-flipped candidates: fewer votes than the winner
        if r == "poses" and len(m["cand_counts"]) >= 2:
            assert m["cand_counts"].min() < m["cand_counts"].max()
