"""GPU: eacham_ransac_batch (eacham_amd/csrc/ransac_batch.hip), EVERY output byte for byte — model doubles, inlier count, mask bytes,
the winner triple, n_candidates, n_used — against
  (a) tests/ransac_reference.py: the sequential loop on the CPU oracle, one sample and one candidate at a time, no budget table;
  (b) the same loop over the device library's existing calls (eacham_solve_minimal, the inlier counts of eacham_score_hypotheses),
      so that a mismatch can be traced to one side;
for every case of tests/ransac_cases.py x {homography, essential, fundamental}, with K and with pre-normalised points, and for
stage1 in {0 (the default), 1, 3, the boundary case's value, more than every S}: the two passes must not show in any output."""
import ctypes as C
import functools

import numpy as np
import pytest

from eacham_amd import capi, lmeds, ransac, score
import ransac_cases as RC
import ransac_reference as RR

pytestmark = pytest.mark.gpu

VARIANTS = ["homography", "essential", "fundamental", "homography_noK", "essential_noK", "fundamental_noK"]
STAGES = [0, 1, 3, RC.BOUNDARY_STAGE1, 1 << 20]
NAMES = list(RC.CASES)


@functools.lru_cache(maxsize=None)
def reference(name, variant):
    """Computed once per (case, variant), shared by the tests below, never written to."""
    return RR.ransac_case(RC.build(name, variant))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def run(ctx, case, stage1=0):
    return ransac.ransac_batch(ctx, case["kind"], case["uv1"], case["uv2"], case["samples"], case["threshold"], case["confidence"], stage1, case["K"])


def device_loop(ctx, case):
    solve = lambda kind, a, b, s, K: score.solve_minimal(ctx, RR.SOLVER[kind], a, b, s, K)                      # noqa: E731
    count = lambda kind, a, b, models, K, thr: score.score_hypotheses(ctx, kind, a, b, models, K, float(thr))[:2]  # noqa: E731
    return [RR.ransac_loop(solve, count, case["kind"], a, b, case["K"], s, case["threshold"], case["confidence"])
            for a, b, s in zip(case["uv1"], case["uv2"], case["samples"])]


def assert_same(got, want, label=""):
    assert len(want) == len(got.inliers) == len(got.masks)
    for p, w in enumerate(want):
        at = f"{label} problem {p}"
        assert tuple(int(x) for x in got.winner[p]) == tuple(w["winner"]), at
        assert int(got.n_used[p]) == w["n_used"], at
        assert int(got.n_candidates[p]) == w["candidates"], at
        assert np.array_equal(bits(got.models[p]), bits(w["model"])), at
        assert int(got.inliers[p]) == w["inliers"], at
        assert np.array_equal(got.masks[p], w["mask"]) and int(got.masks[p].sum()) == w["inliers"], at


def same_outputs(x, y):
    return (np.array_equal(bits(x.models), bits(y.models)) and np.array_equal(x.inliers, y.inliers) and np.array_equal(x.winner, y.winner)
            and np.array_equal(x.n_candidates, y.n_candidates) and np.array_equal(x.n_used, y.n_used)
            and all(np.array_equal(a, b) for a, b in zip(x.masks, y.masks)))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", NAMES)
def test_every_output_equals_the_sequential_reference_for_every_stage1(hip_ctx, name, variant):
    case = RC.build(name, variant)
    want = reference(name, variant)
    for stage1 in STAGES:
        assert_same(run(hip_ctx, case, stage1), want, f"{name}/{variant}/stage1={stage1}")
    if name == "empties":
        got = run(hip_ctx, case)
        for p in (1, 2):
            assert got.winner[p].tolist() == [-1, -1, -1] and not got.models[p].any() and not got.masks[p].any() and got.inliers[p] == 0 and got.n_used[p] == 0
    if name == "early_stop":
        assert all(4 * w["n_used"] < len(s) for w, s in zip(want, case["samples"]))
    if name == "boundary":
        assert [w["winner"][1] for w in want] == [RC.BOUNDARY_STAGE1 - 1, RC.BOUNDARY_STAGE1]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", NAMES)
def test_every_output_equals_the_loop_over_the_existing_calls(hip_ctx, name, variant):
    case = RC.build(name, variant)
    assert_same(run(hip_ctx, case), device_loop(hip_ctx, case), f"{name}/{variant}")


@pytest.mark.parametrize("variant", ["essential", "essential_noK"])
def test_a_later_root_of_the_records_own_sample_wins_past_the_budget(hip_ctx, variant):
    case = RC.build("multi_root", variant)
    want = reference("multi_root", variant)
    if variant == "essential":
        assert want[0]["winner"][2] > 0 and want[0]["n_used"] == want[0]["winner"][1] + 1
    for stage1 in STAGES + [want[0]["winner"][1], want[0]["winner"][1] + 1]:
        assert_same(run(hip_ctx, case, stage1), want, f"{variant}/stage1={stage1}")
    assert_same(run(hip_ctx, case), device_loop(hip_ctx, case), variant)


@pytest.mark.parametrize("variant", ["homography", "essential", "fundamental"])
def test_problem_order_only_reorders_the_results(hip_ctx, variant):
    case = RC.build("mixed", variant)
    for stage1 in (0, 3):
        fwd, rev = run(hip_ctx, case, stage1), run(hip_ctx, RC.reverse(case), stage1)
        P = len(case["uv1"])
        for p in range(P):
            q = P - 1 - p
            assert np.array_equal(bits(fwd.models[p]), bits(rev.models[q])) and fwd.inliers[p] == rev.inliers[q] and np.array_equal(fwd.masks[p], rev.masks[q])
            assert np.array_equal(fwd.winner[p], rev.winner[q]) and fwd.n_candidates[p] == rev.n_candidates[q] and fwd.n_used[p] == rev.n_used[q]


def test_the_debug_read_out_counts_the_samples_handed_to_the_solver(hip_ctx):
    """eacham_ransac_debug_last: a single pass solves every sample, two passes pass 1 in full and pass 2 up to the budget after it."""
    case = RC.build("early_stop", "essential")
    S = [len(s) for s in case["samples"]]
    want = reference("early_stop", "essential")
    run(hip_ctx, case, 1 << 20)
    solved, table_ms = ransac.debug_last(hip_ctx)
    assert solved == sum(S) and table_ms >= 0.0
    stage1 = max(w["n_used"] for w in want) + 1          # every problem's loop has ended inside pass 1: its budget is below stage1
    run(hip_ctx, case, stage1)
    assert ransac.debug_last(hip_ctx)[0] == len(S) * stage1
    run(hip_ctx, case, 1)                                 # after one sample a budget is still large: pass 2 takes more than the loop consumes
    assert sum(w["n_used"] for w in want) <= ransac.debug_last(hip_ctx)[0] <= sum(S)


def test_outputs_are_optional(hip_ctx):
    case = RC.build("single", "homography")
    pp, a, b, sp, idx = lmeds.pack("homography", case["uv1"], case["uv2"], case["samples"])
    used = np.zeros(1, np.int32)
    vp = C.c_void_p
    hip_ctx._check(capi.lib().eacham_ransac_batch(hip_ctx.handle, capi.SOLVE_HOMOGRAPHY4, 1, vp(pp.ctypes.data), vp(a.ctypes.data), vp(b.ctypes.data), None,
                                                  vp(sp.ctypes.data), vp(idx.ctypes.data), case["threshold"], case["confidence"], 3, None, None, None, None,
                                                  None, vp(used.ctypes.data)))
    assert used[0] == run(hip_ctx, case).n_used[0] > 0


def test_the_documented_errors_are_errors_and_leave_the_context_usable(hip_ctx):
    case = RC.build("mixed", "homography")
    pp, a, b, sp, idx = lmeds.pack("homography", case["uv1"], case["uv2"], case["samples"])
    thr, conf = case["threshold"], case["confidence"]
    want = run(hip_ctx, case)

    def fails(word, *, pp=pp, sp=sp, idx=idx, thr=thr, conf=conf, stage1=0, kind="homography"):
        with pytest.raises(capi.EachamError) as e:
            ransac.ransac_batch_raw(hip_ctx, kind, pp, a, b, sp, idx, thr, conf, stage1)
        assert e.value.code == capi.ERR_INVALID and word in str(e.value), str(e.value)
        assert same_outputs(run(hip_ctx, case), want)

    fails("threshold", thr=float("nan"))
    fails("threshold", thr=-1.0)
    for c in (0.0, 1.0, 1.5, -0.1, float("nan")):
        fails("confidence", conf=c)
    fails("stage1", stage1=-1)
    fails("kind", kind=7)
    bad = pp.copy()
    bad[2] = bad[1] - 1
    fails("monotone", pp=bad)
    out = idx.copy()
    out[int(sp[3]) + 1, 2] = len(case["uv1"][3])                            # one past the end of problem 3's points
    fails("problem 3", idx=out)
    out = idx.copy()
    out[int(sp[1]), 0] = -1
    fails("problem 1", idx=out)
