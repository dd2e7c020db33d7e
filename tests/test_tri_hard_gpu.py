"""GPU: the triangulation kernels (eacham_amd/csrc/triangulate.hip) on hard geometry, judged by the 60-digit reference that
tests/golden/tri_hard_golden.npz holds (tests/tri_hard_cases.py, tests/tri_mp_reference.py) under the rules of
tests/tri_hard_rules.py: points within C 2^-52 kappa of the reference, every decided verdict equal to it, an item that hangs on
an undecided decision equal to the oracle's, an undefined item never accepted and without effect on its neighbours. Reads only
the fixture: no mpmath here. Every entry point, every call twice on the same context with the same bytes."""
import numpy as np
import pytest

import oracle_api as O
import tri_hard_rules as HR
import two_view_batch_cases as TC
from eacham_amd import triangulate as tri
from eacham_amd import twoview

pytestmark = pytest.mark.gpu

GROUPS, ORACLE_RATIO = HR.load()
C = 8.0 * ORACLE_RATIO
TRACKS = [n for n, g in GROUPS.items() if g["kind"] == "tracks"]
TWOVIEW = [n for n, g in GROUPS.items() if g["kind"] == "twoview"]
REPEATS = 8                                     # copies of every group in the one large call


def scalars(g):
    return float(g["max_err"]), float(g["min_angle"])


def same(a, b):
    return all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(a, b))


def tracks_twice(ctx, g):
    args = (g["T"], g["ptr"], g["frame"], g["uv"], g["K"], *scalars(g))
    got = tri.triangulate_tracks(ctx, *args)
    assert same(got, tri.triangulate_tracks(ctx, *args)), "a repeat of the call returns other bytes"
    return got


def oracle_tracks(g):
    return O.tri_tracks(g["T"], g["ptr"], g["frame"], g["uv"], g["K"], *scalars(g))


def test_tracks_in_one_large_call(hip_ctx):
    """Every group with the common intrinsics, eight times over, as ONE call of a few thousand tracks: each copy of each
    group obeys the rules wherever it lies in the launch, and all copies return the same bytes."""
    names = [n for n in TRACKS if np.array_equal(GROUPS[n]["K"], GROUPS[TRACKS[0]]["K"])]
    assert len(names) >= len(TRACKS) - 1
    big, first = HR.concat([GROUPS[n] for n in names] * REPEATS)
    assert 2000 < len(big["ptr"]) - 1 < 8000
    pts, status, masks = tracks_twice(hip_ctx, big)
    opts, ostatus, omasks = oracle_tracks(big)
    top, ptr = {}, big["ptr"]
    for k, name in enumerate(names * REPEATS):
        a, b = first[k], first[k + 1]
        part = (pts[a:b], status[a:b], masks[ptr[a]:ptr[b]])
        r = HR.check_tracks(f"{name} (copy {k // len(names)})", GROUPS[name], part, C, other=(opts[a:b], ostatus[a:b], omasks[ptr[a]:ptr[b]]))
        top[name] = max(top.get(name, 0.0), r)
        if k >= len(names):
            a0, b0 = first[k % len(names)], first[k % len(names) + 1]
            assert same(part, (pts[a0:b0], status[a0:b0], masks[ptr[a0]:ptr[b0]])), f"{name}: copy {k // len(names)} differs from the first"
    print("GPU point ratios (x 2^-52 kappa), allowed", C, top)


@pytest.mark.parametrize("name", TRACKS)
def test_tracks_group_alone(hip_ctx, name):
    g = GROUPS[name]
    print(name, "GPU point ratio", HR.check_tracks(name, g, tracks_twice(hip_ctx, g), C, other=oracle_tracks(g)))


@pytest.mark.parametrize("n", (255, 256, 257))
def test_track_counts_around_a_workgroup(hip_ctx, n):
    g = HR.tiled(GROUPS["launch_pool"], n)
    HR.check_tracks(f"launch_{n}", g, tracks_twice(hip_ctx, g), C, other=oracle_tracks(g))


@pytest.mark.parametrize("name", ["zero_baseline", "on_baseline", "selection", "launch_pool"])
def test_undefined_tracks_leave_their_neighbours_alone(hip_ctx, name):
    """Never accepted (the reference's status 0 / mask 0, checked above), and the well-posed tracks before and after them return
    the bytes they return in a call without them."""
    g = GROUPS[name]
    posed = np.flatnonzero(g["defined"] & (g["bits"] == 3))
    assert 0 < len(posed) < len(g["defined"])
    pts, status, masks = tracks_twice(hip_ctx, g)
    rest = HR.take(g, posed)
    rpts, rstatus, rmasks = tracks_twice(hip_ctx, rest)
    obs = np.concatenate([np.arange(g["ptr"][t], g["ptr"][t + 1]) for t in posed])
    assert same((pts[posed], status[posed], masks[obs]), (rpts, rstatus, rmasks))
    lost = np.flatnonzero(~g["defined"] & (np.diff(g["ptr"]) == 2))
    assert not status[lost].any() and not any(masks[g["ptr"][t]:g["ptr"][t + 1]].any() for t in lost)


@pytest.mark.parametrize("name", TRACKS)
def test_single_track_mirror(hip_ctx, name):
    """TriangulatePointRansac on the group's longest track."""
    g = GROUPS[name]
    t = int(np.argmax(np.diff(g["ptr"])))
    one = HR.take(g, [t])
    T = one["T"].reshape(-1, 4, 4)
    data = [tri.EstimatorData(p, T[f], one["K"]) for f, p in zip(one["frame"], one["uv"])]
    ok, X, inl = tri.TriangulatePointRansac(hip_ctx, data, *scalars(one))
    ok2, X2, inl2 = tri.TriangulatePointRansac(hip_ctx, data, *scalars(one))
    assert ok == ok2 and inl == inl2 and X.tobytes() == X2.tobytes(), "a repeat of the call returns other bytes"
    got = (np.array([X]), np.array([int(ok) | (2 if inl and all(inl) else 0)], np.int32), np.array(inl, np.uint8))
    HR.check_tracks(f"{name}[{t}]", one, got, C, other=oracle_tracks(one))


def test_reprojection_errors(hip_ctx):
    g = GROUPS["reprojection"]
    args = (g["T"], g["frame"], g["X"], g["uv"], g["K"])
    err = tri.reprojection_errors(hip_ctx, *args)
    assert err.tobytes() == tri.reprojection_errors(hip_ctx, *args).tobytes()
    print("reprojection: worst error in units of (float ulp + carried bound)", HR.check_reprojection("reprojection", g, err))
    big = (g["T"], np.tile(g["frame"], 100), np.tile(g["X"], (100, 1)), np.tile(g["uv"], (100, 1)), g["K"])   # a few thousand items
    assert tri.reprojection_errors(hip_ctx, *big).tobytes() == np.tile(err, 100).tobytes()


@pytest.mark.parametrize("name", TWOVIEW)
def test_two_view_points(hip_ctx, name):
    g, top = GROUPS[name], 0.0
    for p, (u1, u2, Ts) in enumerate(HR.problems(g)):
        for strict in (True, False):
            args = (u1, u2, g["K"], Ts, *scalars(g), strict)
            got = tri.two_view_points(hip_ctx, *args)
            assert same(got, tri.two_view_points(hip_ctx, *args))
            top = max(top, HR.check_two_view_points(name, g, p, got, C, other=O.two_view_points(*args) if len(u1) else None))
    print(name, "GPU point ratio", top)


def batch_case(g, rule, problems=None):
    P = HR.problems(g) if problems is None else problems
    return {"uv1": [p[0] for p in P], "uv2": [p[1] for p in P], "transforms": [p[2] for p in P], "rules": [rule] * len(P), "in_mask": None,
            "K": g["K"], "max_err": scalars(g)[0], "min_angle": scalars(g)[1], "dist": float(g["dist"]),
            "min_solution_matches": int(g["min_solution_matches"])}


def run_batch(ctx, case):
    return twoview.two_view_batch(ctx, case["uv1"], case["uv2"], case["K"], case["rules"], case["transforms"], case["max_err"], case["min_angle"],
                                  case["in_mask"], case["dist"], case["min_solution_matches"])


def batch_bytes(b):
    return b"".join(np.ascontiguousarray(x).tobytes() for x in (b.winner, b.good, b.kept, *b.cand_counts, *b.points, *b.keep, *b.pose_mask))


@pytest.mark.parametrize("rule", HR.RULES)
@pytest.mark.parametrize("name", TWOVIEW)
def test_two_view_batch(hip_ctx, name, rule):
    g = GROUPS[name]
    case = batch_case(g, rule)
    got = run_batch(hip_ctx, case)
    assert batch_bytes(got) == batch_bytes(run_batch(hip_ctx, case))
    top = HR.check_batch(name, g, rule, got, C, other=TC.compose(O.two_view_points, case))
    print(name, rule, "GPU point ratio", top)


def test_undefined_candidates_leave_the_others_alone(hip_ctx):
    """two_view_pairs' last problem: the same pixels in both images, candidates identity / a pose / identity. The identity has no
    baseline: no keep, no vote, and the pose between them returns the bytes it returns alone."""
    g = GROUPS["two_view_pairs"]
    p = len(g["point_ptr"]) - 2
    u1, u2, Ts = HR.problems(g)[p]
    sl, nt, n = HR.items(g, p)
    assert not g["defined"][sl].reshape(nt, n)[[0, 2]].any() and g["defined"][sl].reshape(nt, n)[1].all()
    for strict in (True, False):
        pts, keep, counts = tri.two_view_points(hip_ctx, u1, u2, g["K"], Ts, *scalars(g), strict)
        apts, akeep, acounts = tri.two_view_points(hip_ctx, u1, u2, g["K"], Ts[1:2], *scalars(g), strict)
        assert not keep[[0, 2]].any() and counts[0] == counts[2] == 0
        assert same((pts[1], keep[1], counts[1:2]), (apts[0], akeep[0], acounts))
    others = HR.problems(g)[:p]
    for rule in HR.RULES:
        # the problem between two ordinary ones, with and without its undefined candidates: the pose's count, and for every
        # problem (this one's winner is the pose either way, or none) the same points, keep, pose_mask, good and kept
        got = run_batch(hip_ctx, batch_case(g, rule, [others[0], (u1, u2, Ts), others[1]]))
        alone = run_batch(hip_ctx, batch_case(g, rule, [others[0], (u1, u2, Ts[1:2]), others[1]]))
        assert got.cand_counts[1][0] == got.cand_counts[1][2] == 0 and got.cand_counts[1][1] == alone.cand_counts[1][0]
        assert int(got.winner[1]) == {0: 1, -1: -1}[int(alone.winner[1])]
        assert same((got.good, got.kept, *got.points, *got.keep, *got.pose_mask), (alone.good, alone.kept, *alone.points, *alone.keep, *alone.pose_mask))
        assert same((got.winner[[0, 2]], got.cand_counts[0], got.cand_counts[2]), (alone.winner[[0, 2]], alone.cand_counts[0], alone.cand_counts[2]))
