"""CPU: tests/golden/tri_hard_golden.npz (hard geometry, judged at 60 digits) pinned from three sides.

  * the fixture is what tests/tri_hard_cases.py and tests/tri_mp_reference.py give (needs mpmath), and meets the generator's own
    conditions: size, undecided caps;
  * oracle/tri_oracle.c obeys the rules of tests/tri_hard_rules.py on it, and its own distance to the reference is still the
    `oracle_ratio` that the fixture's constant was derived from;
  * tests/np_reference.py's LAPACK statement obeys them too: every decided verdict, and the point rule with one documented
    difference, in three groups named below (LAPACK_NORMWISE).
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import np_reference as R
import oracle_api as O
import tri_hard_rules as HR
import two_view_batch_cases as TC

GROUPS, ORACLE_RATIO = HR.load()
C = 8.0 * ORACLE_RATIO
TRACKS = [n for n, g in GROUPS.items() if g["kind"] == "tracks"]
TWOVIEW = [n for n, g in GROUPS.items() if g["kind"] == "twoview"]
LAUNCH_SIZES = (255, 256, 257)


def scalars(g):
    return float(g["max_err"]), float(g["min_angle"])


def oracle_tracks(g):
    return O.tri_tracks(g["T"], g["ptr"], g["frame"], g["uv"], g["K"], *scalars(g))


def batch_case(g, rule):
    P = HR.problems(g)
    return {"uv1": [p[0] for p in P], "uv2": [p[1] for p in P], "transforms": [p[2] for p in P], "rules": [rule] * len(P), "in_mask": None,
            "K": g["K"], "max_err": scalars(g)[0], "min_angle": scalars(g)[1], "dist": float(g["dist"]),
            "min_solution_matches": int(g["min_solution_matches"])}


def as_batch(records):
    """tests/two_view_batch_cases.compose records -> the fields of eacham_amd.twoview.TwoViewBatch."""
    return SimpleNamespace(**{k: [r[k] for r in records] for k in ("winner", "good", "kept", "cand_counts", "points", "keep", "pose_mask")})


def test_fixture_meets_the_generators_conditions():
    assert os.path.getsize(HR.GOLD) <= 64 * 1024
    assert 0.0 < ORACLE_RATIO < 16.0
    kinds = set()
    for name, g in GROUPS.items():
        share = HR.undecided_share(g)
        assert share <= 0.10, (name, share)
        assert bool(g["ladder"]) or share == 0.0, (name, share)
        kinds.add(g["kind"])
    assert kinds == {"tracks", "reproj", "twoview"}
    assert any(HR.undecided_share(g) > 0 for g in GROUPS.values())          # the ladders do reach under the resolution
    assert any((~g["defined"]).any() for g in GROUPS.values() if "defined" in g)
    seen = set()
    for n in TRACKS:
        seen |= set(np.unique(GROUPS[n]["status"]).tolist())
    assert seen == {0, 1, 2, 3}


def test_fixture_is_the_reference_on_the_cases():
    """The reference, evaluated again on the fixture's inputs, gives the fixture's arrays back exactly (mpmath is software
    arithmetic: the same on every machine); the inputs are what tests/tri_hard_cases.py builds, to within the few hundred ulps
    by which numpy's own sin / cos / SVD may round differently from one CPU to the next (1e-13: a tenth of the finest rung of
    the ladders, so an edit of the cases that moves a rung asks for a new fixture)."""
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_tri_hard_golden as gen
    import tri_hard_cases as HC
    groups, ratio, _ = gen.build(oracle_ratio=ORACLE_RATIO, cases={n: HR.as_case(g) for n, g in GROUPS.items()})
    assert ratio == ORACLE_RATIO and list(groups) == list(GROUPS)
    for name, g in groups.items():
        assert set(g) == set(GROUPS[name]), name
        for k, v in g.items():
            if k == "kind":
                assert str(v) == GROUPS[name]["kind"]
                continue
            have = GROUPS[name][k]
            assert have.dtype == np.asarray(v).dtype and have.shape == np.asarray(v).shape, (name, k)
            assert np.array_equal(have, v, equal_nan=have.dtype.kind == "f"), (name, k)
    fresh = HC.groups()
    assert list(fresh) == list(GROUPS)
    for name, case in fresh.items():
        flat = HR.flatten(case, {})
        for k in HR.INPUTS[case["kind"]] + ("ladder",):
            assert flat[k].shape == GROUPS[name][k].shape and np.allclose(flat[k], GROUPS[name][k], rtol=1e-13, atol=1e-13), (name, k)


def test_oracle_tracks_obey_the_rules():
    top = {}
    for name in TRACKS:
        g = GROUPS[name]
        top[name] = HR.check_tracks(name, g, oracle_tracks(g), C)
        for t in np.flatnonzero(np.isfinite(g["angle"])):                    # pair tracks: TriangulationAngle of the reference's point
            a, b = g["ptr"][t], g["ptr"][t] + 1
            T = g["T"].reshape(-1, 4, 4)
            ang = O.tri_angle(T[g["frame"][a]], T[g["frame"][b]], g["points"][t])
            assert abs(ang - g["angle"][t]) <= g["angle_tol"][t], (name, t, ang, g["angle"][t])
    print("oracle point ratios", top)
    # the constant was derived from this build's twin: still within the three bits either way
    assert ORACLE_RATIO / 8 <= max(top.values()) <= C


@pytest.mark.parametrize("n", LAUNCH_SIZES)
def test_oracle_on_the_tiled_calls(n):
    g = HR.tiled(GROUPS["launch_pool"], n)
    assert len(g["ptr"]) - 1 == n and g["ptr"][-1] == len(g["frame"])
    HR.check_tracks(f"launch_{n}", g, oracle_tracks(g), C)


def test_oracle_reprojection_errors():
    g = GROUPS["reprojection"]
    with np.errstate(all="ignore"):
        err = O.reprojection_errors(g["T"], g["frame"], g["X"], g["uv"], g["K"])
    assert HR.check_reprojection("reprojection", g, err) <= 1.0
    assert (~np.isfinite(g["err"])).sum() >= 4 and g["err"][np.isfinite(g["err"])].min() < 1e-6 and g["err"][np.isfinite(g["err"])].max() > 1e6


@pytest.mark.parametrize("name", TWOVIEW)
def test_oracle_two_view_obeys_the_rules(name):
    g = GROUPS[name]
    for p, (u1, u2, Ts) in enumerate(HR.problems(g)):
        for strict in (True, False):
            HR.check_two_view_points(name, g, p, O.two_view_points(u1, u2, g["K"], Ts, *scalars(g), strict), C)
    for rule in HR.RULES:
        HR.check_batch(name, g, rule, as_batch(TC.compose(O.two_view_points, batch_case(g, rule))), C)


def test_the_track_cases_hold_what_they_are_for():
    g = GROUPS["selection"]
    m, ptr = np.diff(g["ptr"]), g["ptr"]
    mask = lambda t: g["masks"][ptr[t]:ptr[t + 1]].tolist()   # noqa: E731
    # every pair under the angle gate at m >= 3: no winner, status 0, mask 0, a defined (last pair's) point
    fail = [t for t in range(len(m)) if m[t] >= 3 and g["status"][t] == 0 and not any(mask(t)) and g["defined"][t]]
    assert len(fail) >= 4 and {int(m[t]) for t in fail} == {3, 4}
    # m = 3: all three inliers (status 3) and two of three (`best > 2` fails)
    assert any(m[t] == 3 and g["status"][t] == 3 for t in range(len(m))) and any(m[t] == 3 and mask(t) == [1, 1, 0] and g["status"][t] == 0 for t in range(len(m)))
    # ties: three inliers each way (the first pair's mask stays, ransac true, not full) and two each way
    assert sum(mask(t) == [1, 1, 1, 0, 0, 0] and g["status"][t] == 1 for t in range(len(m))) >= 4
    assert sum(mask(t) == [1, 1, 0, 0] and g["status"][t] == 0 for t in range(len(m))) >= 4
    # the last pair without baseline while an earlier pair wins: every observation an inlier, the point (and bit 1) anything
    last = [t for t in range(len(m)) if not g["defined"][t] and m[t] == 4]
    assert len(last) >= 4 and all(g["bits"][t] == 2 and g["status"][t] & 2 and all(mask(t)) for t in last)
    # a frame twice inside a good track
    assert any(m[t] == 5 and len(set(g["frame"][ptr[t]:ptr[t + 1]].tolist())) == 4 and g["status"][t] == 3 for t in range(len(m)))
    z = GROUPS["zero_baseline"]
    T, fr = z["T"], z["frame"].reshape(-1, 2)
    same_slot = [t for t in range(len(fr)) if fr[t, 0] == fr[t, 1] and not z["defined"][t]]
    two_slots = [t for t in range(len(fr)) if fr[t, 0] != fr[t, 1] and np.array_equal(T[fr[t, 0]], T[fr[t, 1]]) and not z["defined"][t]]
    assert len(same_slot) >= 2 and len(two_slots) >= 2                        # one frame twice; two frame slots with equal transforms
    assert any(fr[t, 0] == fr[t, 1] and z["defined"][t] for t in range(len(fr)))   # one frame, two pixels: defined, never accepted
    assert not z["status"][same_slot + two_slots].any()
    s = GROUPS["shift_scale"]
    centre = np.abs(s["points"]).max(1)
    assert (centre > 5e5).sum() >= 3 and (centre < 1e-2).sum() >= 8 and (centre[s["decided"]] > 500).sum() >= 8


def test_the_two_view_cases_hold_what_they_are_for():
    g = GROUPS["two_view_shapes"]
    assert np.diff(g["point_ptr"]).tolist() == [1, 63, 64, 65, 257, 0, 40, 30]
    # the true pose wins wherever it is, a tie keeps the first, under `solutions` small problems have no winner
    assert g["poses_winner"].tolist() == [1, 0, 1, 0, 1, 0, 0, 1] and g["solutions_winner"].tolist() == [-1, 0, 1, 0, 1, -1, 0, 1]
    assert (g["poses_good"][[1, 2, 3, 4, 6, 7]] > 20).all() and g["poses_good"][5] == 0
    pairs = GROUPS["two_view_pairs"]
    assert not pairs["defined"].all() and (pairs["kappa"][pairs["defined"]] > 1e7).any()
    assert (GROUPS["depth_over_baseline"]["kappa"] > 1e8).any()
    lad = GROUPS["two_view_ladders"]                                           # every gate of the two-view kernels within 1e-9 of its threshold
    assert bool(lad["ladder"]) and 0 < HR.undecided_share(lad) <= 0.10 and (lad["margin"] < 1e4).sum() >= 16
    assert (lad["solutions_winner"] == 0).all() and (lad["poses_winner"] == 0).all()
    deg = GROUPS["two_view_degenerate"]
    assert (~deg["defined"]).sum() >= 6 and HR.undecided_share(deg) == 0.0


# The LAPACK statement is held to the same rule and the same constant C as the oracle, except in the groups named here, where
# the rule as written does not describe a norm-wise backward stable SVD:
#   * sub-unit scenes. Such an SVD returns the UNIT null vector (X, 1) / |(X, 1)| to within ||E|| / gap in norm, so a point much
#     nearer to the origin than one unit inherits that error absolutely, not relative to itself as the one-sided Jacobi of the
#     oracle and the kernels (column-wise relative accuracy) does: there the rule's max|X_ref| is max(max|X_ref|, 1);
#   * and there, and at depths of 1e5 baselines and more, its constant: Householder bidiagonalisation of an m x n matrix is
#     backward stable with ||E|| <= m n u sigma_1 (Higham, Accuracy and Stability, gamma_mn), the null vector moves by at most
#     sqrt(3) ||E|| / gap (its couplings to the other three right singular vectors), and dehomogenising carries that to
#     |dX| <= 2 |dv| max(|X|, 1) / w: in the rule's units of 2^-52 kappa that is sqrt(3) m n.
C_LAPACK = np.sqrt(3.0) * 16
LAPACK_NORMWISE = ("shift_scale", "two_view_pairs", "two_view_degenerate")


def lapack_ratio(X, g, name, sl=slice(None)):
    """(per-item ratio, the constant it is held to)"""
    ref, kappa, defined = g["points"][sl], g["kappa"][sl], g["defined"][sl]
    if name not in LAPACK_NORMWISE:
        return HR.point_ratio(X, ref, kappa, defined), C
    with np.errstate(all="ignore"):
        r = np.abs(np.asarray(X, np.float64).reshape(-1, 3) - ref).max(1) / (np.maximum(np.abs(ref).max(1), 1.0) * 2.0 ** -52 * kappa)
    r[np.isnan(r)] = np.inf
    r[~defined] = np.nan
    return r, C_LAPACK


def test_lapack_statement_obeys_the_rules_on_tracks():
    top = {}
    for name in TRACKS:
        g = GROUPS[name]
        T, ptr = g["T"].reshape(-1, 4, 4), g["ptr"]
        oracle = oracle_tracks(g)
        pts, status, masks = np.zeros_like(g["points"]), np.zeros_like(g["status"]), np.zeros_like(g["masks"])
        for t in range(len(ptr) - 1):
            a, b = ptr[t], ptr[t + 1]
            with np.errstate(all="ignore"):
                ok, X, mask = R.tri_ransac([T[f] for f in g["frame"][a:b]], list(g["uv"][a:b]), g["K"], *scalars(g))
            pts[t], masks[a:b] = X, [int(x) for x in mask] if mask else 0
            status[t] = int(ok) | (2 if len(mask) > 0 and all(mask) else 0)
        ratio, bound = lapack_ratio(pts, g, name)
        assert not (ratio > bound).any(), (name, np.flatnonzero(ratio > bound), ratio[ratio > bound])
        top[name] = HR.worst(ratio)
        free = dict(g, defined=np.zeros_like(g["defined"]))                  # (points judged above)
        HR.check_tracks(name, free, (pts, status, masks), C, other=oracle)
    print("LAPACK point ratios", top)


@pytest.mark.parametrize("name", TWOVIEW)
def test_lapack_statement_obeys_the_rules_on_two_views(name):
    g = GROUPS[name]
    for p, (u1, u2, Ts) in enumerate(HR.problems(g)):
        sl, nt, n = HR.items(g, p)
        if n == 0:
            continue
        with np.errstate(all="ignore"):
            got = [R.two_view(u1, u2, g["K"], T, *scalars(g), True) for T in Ts]
        pts, keep = np.array([x[0] for x in got]), np.array([x[1] for x in got]).astype(np.uint8)
        ratio, bound = lapack_ratio(pts, g, name, sl)
        assert not (ratio > bound).any(), (name, p, np.flatnonzero(ratio > bound), ratio[ratio > bound])
        det = g["det_keep"][sl]
        assert np.array_equal(keep.reshape(-1)[det], g["keep"][sl][det]), (name, p)
