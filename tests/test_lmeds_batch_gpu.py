"""GPU: eacham_lmeds_batch (eacham_amd/csrc/lmeds_batch.hip) against the per-problem composition of the entry points that
already exist and are already held to the oracles — eacham_solve_minimal on problem p, host compaction, eacham_score_hypotheses
for the medians, first smallest non-NaN, sigma in Python float64, eacham_score_hypotheses for the errors
(tests/test_lmeds_batch_reference.py: compose) — EVERY output bit for bit: model doubles, median, threshold, inliers, mask bytes,
the winner triple, n_candidates. The cases (tests/lmeds_batch_cases.py) are the smallest shapes at which the segmented kernels can
still go wrong; each runs for the homography, for the essential matrix with K and for the essential matrix with K = NULL.
The error-row path (a problem above SC_MAX_LDS points) runs at the real SC_MAX_LDS: with 3 samples it is 3 / at most 30
candidates over 16 385 points, milliseconds."""
import numpy as np
import pytest

from eacham_amd import capi, lmeds, score
import lmeds_batch_cases as LC
import test_lmeds_batch_reference as REF

pytestmark = pytest.mark.gpu

VARIANTS = ["homography", "essential", "essential_noK"]


def build(name, variant):
    kind = variant.split("_")[0]
    case = LC.multi_root() if name == "multi_root" else LC.CASES[name](kind)
    return LC.normalised(case) if variant.endswith("noK") else case


def device_compose(ctx, case):
    return REF.compose(lambda *a: score.solve_minimal(ctx, *a), lambda *a: score.score_hypotheses(ctx, *a), case)


def assert_same(got, want, label=""):
    """got: LmedsBatch, want: the composition's records. Exact, output by output, every problem's own slice."""
    assert len(want) == len(got.medians) == len(got.masks)
    for p, w in enumerate(want):
        at = f"{label} problem {p}"
        assert tuple(int(x) for x in got.winner[p]) == w["winner"], at
        assert int(got.n_candidates[p]) == w["candidates"], at
        assert np.array_equal(REF.bits(got.models[p], np.float64), REF.bits(w["model"], np.float64)), at
        assert REF.bits(got.medians[p], np.float32) == REF.bits(w["median"], np.float32) or (np.isnan(got.medians[p]) and np.isnan(w["median"])), at
        assert REF.bits(got.thresholds[p], np.float32) == REF.bits(w["threshold"], np.float32), at
        assert int(got.inliers[p]) == w["inliers"], at
        assert np.array_equal(got.masks[p], w["mask"]), at


def run(ctx, case):
    return ctx.lmeds_batch(case["kind"], case["uv1"], case["uv2"], case["samples"], case["K"])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(LC.CASES))
def test_every_output_equals_the_composition_of_the_existing_calls(hip_ctx, name, variant):
    case = build(name, variant)
    want = device_compose(hip_ctx, case)
    got = run(hip_ctx, case)
    assert_same(got, want, f"{name}/{variant}")
    if name == "empties":                      # the "none" record, and the neighbours where they belong
        assert [w["winner"][0] >= 0 for w in want] == [True, False, False, True]
        for p in (1, 2):
            assert np.isnan(got.medians[p]) and not got.models[p].any() and not got.masks[p].any() and got.inliers[p] == 0
    if name == "degenerate":
        assert want[0]["roots"][1] == 0 and want[0]["winner"][0] >= 0 and got.n_candidates[1] == 0 and got.winner[1].tolist() == [-1, -1, -1]
    if name == "ties":
        for p, w in enumerate(want):
            rows = case["samples"][p]
            assert w["winner"][1] == min(s for s in range(len(rows)) if np.array_equal(rows[s], rows[w["winner"][1]]))
    if name == "key_paths":
        assert len(case["uv1"][0]) > LC.SC_MAX_LDS > len(case["uv1"][1]) and want[0]["winner"][0] >= 0 and want[1]["winner"][0] >= 0


@pytest.mark.parametrize("variant", ["essential", "essential_noK"])
def test_essential_samples_with_several_roots(hip_ctx, variant):
    case = build("multi_root", variant)
    want = device_compose(hip_ctx, case)
    assert max(int(w["roots"].max()) for w in want) >= 2
    assert any(w["winner"][2] > 0 for w in want) and any(w["winner"][2] == 0 for w in want)
    assert_same(run(hip_ctx, case), want, variant)


@pytest.mark.parametrize("variant", VARIANTS)
def test_problem_order_only_reorders_the_results(hip_ctx, variant):
    case = build("mixed", variant)
    fwd, rev = run(hip_ctx, case), run(hip_ctx, LC.reverse(case))
    P = len(case["uv1"])
    for p in range(P):
        q = P - 1 - p
        assert np.array_equal(REF.bits(fwd.models[p], np.float64), REF.bits(rev.models[q], np.float64))
        assert REF.bits(fwd.medians[p], np.float32) == REF.bits(rev.medians[q], np.float32)
        assert REF.bits(fwd.thresholds[p], np.float32) == REF.bits(rev.thresholds[q], np.float32)
        assert fwd.inliers[p] == rev.inliers[q] and np.array_equal(fwd.masks[p], rev.masks[q])
        assert np.array_equal(fwd.winner[p], rev.winner[q]) and fwd.n_candidates[p] == rev.n_candidates[q]


def test_outputs_are_optional(hip_ctx):
    """Every output may be NULL: only the medians are asked for."""
    import ctypes as C
    case = build("single", "homography")
    pp, a, b, sp, idx = lmeds.pack("homography", case["uv1"], case["uv2"], case["samples"])
    med = np.zeros(1, np.float32)
    vp = C.c_void_p
    hip_ctx._check(capi.lib().eacham_lmeds_batch(hip_ctx.handle, capi.SOLVE_HOMOGRAPHY4, 1, vp(pp.ctypes.data), vp(a.ctypes.data), vp(b.ctypes.data),
                                                 None, vp(sp.ctypes.data), vp(idx.ctypes.data), None, vp(med.ctypes.data), None, None, None, None, None))
    assert REF.bits(med[0], np.float32) == REF.bits(run(hip_ctx, case).medians[0], np.float32)


def test_error_paths_leave_the_context_usable(hip_ctx):
    case = build("mixed", "homography")
    pp, a, b, sp, idx = lmeds.pack("homography", case["uv1"], case["uv2"], case["samples"])
    want = run(hip_ctx, case)

    def still_works():
        again = run(hip_ctx, case)
        assert np.array_equal(again.winner, want.winner) and np.array_equal(REF.bits(again.models, np.float64), REF.bits(want.models, np.float64))

    bad = pp.copy()
    bad[2] = bad[1] - 1                                                     # a non-monotone point_ptr
    with pytest.raises(capi.EachamError) as e:
        lmeds.lmeds_batch_raw(hip_ctx, "homography", bad, a, b, sp, idx)
    assert e.value.code == capi.ERR_INVALID and "monotone" in str(e.value)
    still_works()
    out = idx.copy()
    out[int(sp[3]) + 1, 2] = len(case["uv1"][3])                            # one past the end of problem 3's points
    with pytest.raises(capi.EachamError) as e:
        lmeds.lmeds_batch_raw(hip_ctx, "homography", pp, a, b, sp, out)
    assert e.value.code == capi.ERR_INVALID and "problem 3" in str(e.value)
    still_works()
    out = idx.copy()
    out[int(sp[1]), 0] = -1
    with pytest.raises(capi.EachamError) as e:
        lmeds.lmeds_batch_raw(hip_ctx, "homography", pp, a, b, sp, out)
    assert e.value.code == capi.ERR_INVALID and "problem 1" in str(e.value)
    still_works()
    with pytest.raises(capi.EachamError) as e:                              # a bad kind
        lmeds._call(hip_ctx, 7, pp, a, b, sp, idx, None)
    assert e.value.code == capi.ERR_INVALID and "kind" in str(e.value)
    still_works()
