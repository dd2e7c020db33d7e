"""GPU: eacham_two_view_batch (eacham_amd/csrc/triangulate.hip) against the per-problem composition of the entry point that
already exists and is already held to the oracle — eacham_two_view_points on the same context with all of the problem's
candidates, then the host rules in numpy (tests/two_view_batch_cases.py: compose; tests/test_two_view_batch_reference.py holds
that composition to the sequential statements of the reference on the CPU) — EVERY output byte for byte: winner, good, kept,
the per-candidate counts, the winner's points (compared as bytes: NaN / inf must match too), keep, pose_mask. The cases are the
smallest shapes at which the segmented kernels can still go wrong."""
import ctypes as C

import numpy as np
import pytest

from eacham_amd import capi, triangulate as tri, twoview
import two_view_batch_cases as TC

pytestmark = pytest.mark.gpu


def device_compose(ctx, case):
    return TC.compose(lambda *a: tri.two_view_points(ctx, *a), case)


def run(ctx, case):
    return ctx.two_view_batch(case["uv1"], case["uv2"], case["K"], case["rules"], case["transforms"], case["max_err"], case["min_angle"],
                              case["in_mask"], case["dist"], case["min_solution_matches"])


def same_bytes(a, b, dtype):
    return np.ascontiguousarray(a, dtype=dtype).tobytes() == np.ascontiguousarray(b, dtype=dtype).tobytes()


def assert_same(got, want, label=""):
    """got: TwoViewBatch, want: the composition's records. Exact, output by output, every problem's own slice."""
    assert len(want) == len(got.winner) == len(got.points) == len(got.cand_counts)
    for p, w in enumerate(want):
        at = f"{label} problem {p}"
        assert (int(got.winner[p]), int(got.good[p]), int(got.kept[p])) == (w["winner"], w["good"], w["kept"]), at
        assert np.array_equal(got.cand_counts[p], w["cand_counts"]), at
        assert same_bytes(got.points[p], w["points"], np.float64), at
        assert same_bytes(got.keep[p], w["keep"], np.uint8) and same_bytes(got.pose_mask[p], w["pose_mask"], np.uint8), at


def assert_none(got, p):
    assert got.winner[p] == -1 and got.good[p] == 0 and got.kept[p] == 0
    assert not got.keep[p].any() and not got.pose_mask[p].any() and got.points[p].tobytes() == bytes(got.points[p].nbytes)


@pytest.mark.parametrize("name", list(TC.CASES))
def test_every_output_equals_the_composition_of_the_existing_call(hip_ctx, name):
    case = TC.CASES[name]()
    want = device_compose(hip_ctx, case)
    got = run(hip_ctx, case)
    assert_same(got, want, name)
    if name == "empties":                      # the "none" record, and the neighbours where they belong
        assert [int(w) >= 0 for w in got.winner] == [True, True, False, False, True, False, True, False]
        assert got.winner[0] == 0 and got.good[0] == 0 and got.kept[0] == 0 and len(got.cand_counts[0]) == 3
        for p in (2, 3, 5, 7):
            assert_none(got, p)
    if name == "twins":
        for p in range(2):
            assert np.array_equal(got.cand_counts[p][:4], got.cand_counts[p][4:]) and 0 <= got.winner[p] < 4
    if name == "masked_out":
        assert all(got.winner[p] == 0 and got.good[p] == 0 and got.kept[p] > 0 and not got.pose_mask[p].any() for p in range(2))
    if name == "degenerate":
        assert not np.isfinite(np.concatenate([w["points"] for w in want])).all() or want[3]["winner"] < 0
    if name == "mixed":                        # the t-flipped candidates lose the vote
        assert any(w > 0 for w in got.winner) and all(c.min() < c.max() for c, r in zip(got.cand_counts, case["rules"]) if r == "poses" and len(c) > 1)


def test_problem_order_only_reorders_the_results(hip_ctx):
    case = TC.mixed()
    fwd, rev = run(hip_ctx, case), run(hip_ctx, TC.reverse(case))
    P = len(case["uv1"])
    for p in range(P):
        q = P - 1 - p
        assert (fwd.winner[p], fwd.good[p], fwd.kept[p]) == (rev.winner[q], rev.good[q], rev.kept[q])
        assert np.array_equal(fwd.cand_counts[p], rev.cand_counts[q]) and same_bytes(fwd.points[p], rev.points[q], np.float64)
        assert np.array_equal(fwd.keep[p], rev.keep[q]) and np.array_equal(fwd.pose_mask[p], rev.pose_mask[q])


def test_no_problems_is_not_an_error(hip_ctx):
    got = run(hip_ctx, TC._case([], []))
    assert len(got.winner) == 0 and got.points == [] and got.cand_counts == []


def test_solution_acceptance_threshold(hip_ctx):
    """min_solution_matches at the best count the composition observed: none; one below it: accepted."""
    want = device_compose(hip_ctx, TC.solutions_only())
    tops = [int(w["cand_counts"].max()) for w in want]
    assert all(w["winner"] >= 0 for w in want) and tops[0] != tops[1]
    for p, top in enumerate(tops):
        at = run(hip_ctx, TC.solutions_only(top))
        assert_none(at, p)
        assert np.array_equal(at.cand_counts[p], want[p]["cand_counts"])           # still written
        assert_same(at, device_compose(hip_ctx, TC.solutions_only(top)), f"at {top}")
        below = run(hip_ctx, TC.solutions_only(top - 1))
        assert below.winner[p] == want[p]["winner"] and below.kept[p] == top
        assert_same(below, device_compose(hip_ctx, TC.solutions_only(top - 1)), f"below {top}")


def test_random_in_mask_against_null(hip_ctx):
    case = TC.mixed()
    masked = TC.random_mask(case)
    ones = dict(case, in_mask=[np.ones(len(u), np.uint8) for u in case["uv1"]])
    a, b, c = run(hip_ctx, case), run(hip_ctx, ones), run(hip_ctx, masked)
    assert_same(c, device_compose(hip_ctx, masked), "masked")
    for p, rule in enumerate(case["rules"]):
        assert a.good[p] == b.good[p] and np.array_equal(a.pose_mask[p], b.pose_mask[p]) and np.array_equal(a.cand_counts[p], b.cand_counts[p])
        if rule == "poses":
            assert not (c.pose_mask[p] & ~masked["in_mask"][p]).any() and c.good[p] <= a.good[p]
        else:                                                                        # the SOLUTIONS rule does not read it
            assert np.array_equal(a.keep[p], c.keep[p]) and a.winner[p] == c.winner[p]
    assert any(c.good[p] < a.good[p] for p in range(len(case["rules"])))


SENTINEL = 0x5A


def test_error_paths_leave_the_outputs_and_the_context_alone(hip_ctx):
    case = TC.mixed()
    pp, a, b, tp, T, _ = twoview.pack(case["uv1"], case["uv2"], case["transforms"])
    rule = np.array([twoview.RULES[r] for r in case["rules"]], np.int32)
    want = run(hip_ctx, case)

    def outputs():
        P, NP, NT = len(pp) - 1, int(pp[-1]), int(tp[-1])
        return tuple(np.full(shape, SENTINEL, dt) for shape, dt in (((P,), np.int32), ((P,), np.int32), ((P,), np.int32), ((NT,), np.int32),
                                                                    ((NP, 3), np.float64), ((NP,), np.uint8), ((NP,), np.uint8)))

    def refused(code, word, **change):
        args = dict(point_ptr=pp, uv1=a, uv2=b, K=case["K"], rule=rule, transform_ptr=tp, transforms=T, in_mask=None, n_problems=None)
        args.update(change)
        out = outputs()
        with pytest.raises(capi.EachamError) as e:
            twoview.two_view_batch_raw(hip_ctx, args["point_ptr"], args["uv1"], args["uv2"], args["K"], args["rule"], args["transform_ptr"],
                                       args["transforms"], args["in_mask"], case["max_err"], case["min_angle"], case["dist"],
                                       case["min_solution_matches"], n_problems=args["n_problems"], out=out)
        assert e.value.code == code and word in str(e.value), str(e.value)
        for o, fresh in zip(out, outputs()):
            assert o.tobytes() == fresh.tobytes()                                    # untouched
        again = run(hip_ctx, case)                                                   # and the context still works
        assert np.array_equal(again.winner, want.winner) and all(same_bytes(x, y, np.float64) for x, y in zip(again.points, want.points))

    bad = rule.copy()
    bad[5] = 2
    refused(capi.ERR_INVALID, "problem 5", rule=bad)                                 # an unknown rule
    refused(capi.ERR_INVALID, "negative", n_problems=-1)                             # a negative size
    for name, table in (("point_ptr", pp), ("transform_ptr", tp)):
        refused(capi.ERR_INVALID, "null offset table", **{name: None}, n_problems=len(pp) - 1)
        shifted = table.copy()
        shifted[0] = 1
        refused(capi.ERR_INVALID, "start at 0", **{name: shifted})
        dec = table.copy()
        dec[3] = dec[2] - 1
        refused(capi.ERR_INVALID, "problem 2", **{name: dec})                        # a table that decreases
    for name in ("uv1", "uv2", "K", "rule", "transforms"):                           # a null required array
        refused(capi.ERR_INVALID, "null", **{name: None})
    huge = pp.copy()
    huge[-1] = 1 << 31                                                               # more items than one call takes
    refused(capi.ERR_CAPACITY, "2^31", point_ptr=huge)
    items = np.array([0, (1 << 31) - 1], np.int64)                                   # points and candidates fit, their product does not
    refused(capi.ERR_CAPACITY, "2^31", point_ptr=items, transform_ptr=np.array([0, 4], np.int64), rule=rule[:1], n_problems=1)


def test_a_null_output_is_refused(hip_ctx):
    case = TC.single()
    pp, a, b, tp, T, _ = twoview.pack(case["uv1"], case["uv2"], case["transforms"])
    rule = np.zeros(1, np.int32)
    vp = lambda x: C.c_void_p(x.ctypes.data)   # noqa: E731
    K4 = np.ascontiguousarray(case["K"], np.float64)
    i32, pts, byt = np.zeros(1, np.int32), np.zeros((70, 3)), np.zeros(70, np.uint8)
    rc = capi.lib().eacham_two_view_batch(hip_ctx.handle, 1, vp(pp), vp(a), vp(b), vp(K4), vp(rule), vp(tp), vp(T), None, 4.0, 0.01, 50.0, 20,
                                          vp(i32), vp(i32), vp(i32), vp(np.zeros(4, np.int32)), None, vp(byt), vp(byt))
    assert rc == capi.ERR_INVALID
