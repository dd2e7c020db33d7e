"""GPU: eacham_pnp_hypotheses_batch / eacham_pnp_refit_batch (eacham_amd/csrc/pnp_batch.hip) against the per-problem composition
of the entry points that already exist and are already held to the oracles — eacham_solve_pnp on the problem's rows and
eacham_score_hypotheses(kind PNP); one model with its errors, the host compaction, eacham_solve_pnp on one row of inliers
(tests/test_pnp_batch_reference.py: compose_hypotheses, compose_refit, round_ransac) — on the same context, EVERY output compared
as bytes. The cases (tests/pnp_batch_cases.py) are the smallest shapes at which the segmented kernels can still go wrong."""
import ctypes as C

import numpy as np
import pytest

from eacham_amd import capi, pnp, score
import pnp_batch_cases as PC
import test_pnp_batch_reference as REF

pytestmark = pytest.mark.gpu

bits = REF.bits


def device_calls(ctx):
    solve = lambda X, uv, K, rows: score.solve_pnp(ctx, X, uv, K, rows)   # noqa: E731
    scr = lambda kind, X, uv, models, K, thr: score.score_hypotheses(ctx, kind, X, uv, models, K, thr)   # noqa: E731
    return solve, scr


def assert_same_hypotheses(got, want, label=""):
    assert len(want) == len(got.n_models)
    for p, (models, ok, cnt) in enumerate(want):
        at = f"{label} problem {p}"
        assert np.array_equal(got.n_models[p], ok), at
        assert np.array_equal(got.inlier_counts[p], cnt), at
        if got.models is not None:
            assert np.array_equal(bits(got.models[p]), bits(models)), at


def assert_same_refit(got, want, label=""):
    assert len(want) == len(got.masks)
    for p, w in enumerate(want):
        at = f"{label} problem {p}"
        assert np.array_equal(got.masks[p], w["mask"]) and int(got.n_inliers[p]) == w["n_inliers"] == int(got.masks[p].sum()), at
        assert int(got.refit_ok[p]) == w["refit_ok"] and np.array_equal(bits(got.refit[p]), bits(w["refit"])), at


@pytest.mark.parametrize("name", list(PC.HYP_CASES))
def test_a_round_equals_the_composition_of_the_existing_calls(hip_ctx, name):
    c = PC.HYP_CASES[name]()
    want = REF.compose_hypotheses(*device_calls(hip_ctx), c["X"], c["uv"], c["K"], c["samples"], PC.THR)
    got = hip_ctx.pnp_hypotheses_batch(c["X"], c["uv"], c["K"], c["samples"], PC.THR)
    assert_same_hypotheses(got, want, name)
    if name == "mixed":
        assert not got.n_models[0].any() and not got.models[0].any() and all(g.any() for g in got.n_models[1:])
    if name == "structure":
        assert got.n_models[0].tolist() == [1, 0, 1] and not got.models[0][1].any() and got.inlier_counts[0][1] == 0
        assert got.n_models[1].all() and not got.n_models[2].any() and not got.inlier_counts[2].any()
    if name == "trip_edges":                     # some model of each problem counts every point but the camera centre, the last included
        assert [int(c.max()) for c in got.inlier_counts] == [62, 63, 64, 254, 255, 256]
    if name == "empties":
        assert len(got.n_models[1]) == 0 and got.n_models[0].any() and got.n_models[2].any()


def test_a_larger_sample_size(hip_ctx):
    """m = 64, the upper end of the class (rows of 64 distinct indices), and m = 7."""
    base = PC.problem(200, 0, 33)
    for m in (7, 64):
        rng = np.random.default_rng(m)
        rows = [np.array([rng.choice(len(x), size=m, replace=False) for _ in range(5)], dtype=np.int32) for x in (base[0], base[0][:90])]
        X, uv = [base[0], base[0][:90]], [base[1], base[1][:90]]
        solve, scr = device_calls(hip_ctx)
        got = hip_ctx.pnp_hypotheses_batch(X, uv, PC.K, rows, PC.THR)
        for p in range(2):
            models, ok = solve(X[p], uv[p], PC.K, rows[p])
            _, cnt, _ = scr("pnp", X[p], uv[p], models, PC.K, PC.THR)
            assert ok.all() and np.array_equal(bits(got.models[p]), bits(models)) and np.array_equal(got.n_models[p], ok)
            assert np.array_equal(got.inlier_counts[p], cnt)


def test_models_null_works(hip_ctx):
    c = PC.mixed()
    full = hip_ctx.pnp_hypotheses_batch(c["X"], c["uv"], c["K"], c["samples"], PC.THR)
    lean = hip_ctx.pnp_hypotheses_batch(c["X"], c["uv"], c["K"], c["samples"], PC.THR, want_models=False)
    assert lean.models is None
    for p in range(len(c["X"])):
        assert np.array_equal(full.n_models[p], lean.n_models[p]) and np.array_equal(full.inlier_counts[p], lean.inlier_counts[p])


def test_the_refit_equals_the_composition_of_the_existing_calls(hip_ctx):
    c = PC.refit_case()
    want = REF.compose_refit(*device_calls(hip_ctx), c["X"], c["uv"], c["K"], c["models"], c["has_model"], PC.THR)
    got = hip_ctx.pnp_refit_batch(c["X"], c["uv"], c["K"], c["models"], c["has_model"], PC.THR)
    assert_same_refit(got, want)
    p, line = c["collinear"]
    assert np.array_equal(np.nonzero(got.masks[p])[0], line) and got.n_inliers[p] == 10 and got.refit_ok[p] == 0 and not got.refit[p].any()
    assert got.refit_ok.tolist() == [1, 1, 0, 0, 0, 1, 1] and got.n_inliers[0] > 64 >= got.n_inliers[1] >= 5
    assert not got.masks[2].any() and got.n_inliers[2] == 0 and got.n_inliers[4] < 5
    e = PC.refit_edges()                                                         # 63 .. 65 and 255 .. 257 points
    want = REF.compose_refit(*device_calls(hip_ctx), e["X"], e["uv"], e["K"], e["models"], e["has_model"], PC.THR)
    assert_same_refit(hip_ctx.pnp_refit_batch(e["X"], e["uv"], e["K"], e["models"], e["has_model"], PC.THR), want, "trip edges")
    assert [w["n_inliers"] for w in want] == [62, 63, 64, 254, 255, 256] and all(w["refit_ok"] and w["mask"][-1] for w in want)


@pytest.mark.parametrize("count", [5, 63, 64, 65, 129])
def test_the_refit_on_both_sides_of_the_64_row_boundary(hip_ctx, count):
    """Inlier sets of exactly `count` rows: the true pose, every pixel beyond the first `count` good ones pushed 50 px away."""
    X, uv, _, T = PC.problem(200, 0, 97, outliers=0.0)
    good = np.nonzero(np.sum((PC.project(X, T) - uv) ** 2, 1) < 8.0)[0]
    uv = uv.copy()
    uv[np.setdiff1d(np.arange(len(uv)), good[:count])] += 50.0
    want = REF.compose_refit(*device_calls(hip_ctx), [X], [uv], PC.K, [T], [1], PC.THR)
    assert want[0]["n_inliers"] == count and want[0]["refit_ok"]
    assert_same_refit(hip_ctx.pnp_refit_batch([X], [uv], PC.K, [T], [1], PC.THR), want, f"{count} inliers")


@pytest.mark.parametrize("name", list(PC.RANSAC_CASES))
def test_the_round_loop_equals_the_per_problem_loop(hip_ctx, name):
    c = PC.RANSAC_CASES[name]()
    solve, scr = device_calls(hip_ctx)
    want = [REF.round_ransac(solve, scr, x, u, c["K"], s, c["max_iters"]) for x, u, s in zip(c["X"], c["uv"], c["samples"])]
    got, turns = pnp.pnp_ransac_batch(hip_ctx, c["X"], c["uv"], c["K"], c["samples"], c["max_iters"])
    for p, w in enumerate(want):
        REF.assert_same_run(got[p], w, f"{name} problem {p}")
    assert turns == max(w["rounds"] for w in want) + 1            # rounds + 1 host turns for the whole list


def test_problem_order_only_reorders_the_results(hip_ctx):
    c = PC.mixed()
    fwd = hip_ctx.pnp_hypotheses_batch(c["X"], c["uv"], c["K"], c["samples"], PC.THR)
    r = PC.reverse(c)
    rev = hip_ctx.pnp_hypotheses_batch(r["X"], r["uv"], r["K"], r["samples"], PC.THR)
    P = len(c["X"])
    for p in range(P):
        q = P - 1 - p
        assert np.array_equal(bits(fwd.models[p]), bits(rev.models[q])) and np.array_equal(fwd.n_models[p], rev.n_models[q])
        assert np.array_equal(fwd.inlier_counts[p], rev.inlier_counts[q])
    c = PC.refit_case()
    r = PC.reverse(c)
    fwd = hip_ctx.pnp_refit_batch(c["X"], c["uv"], c["K"], c["models"], c["has_model"], PC.THR)
    rev = hip_ctx.pnp_refit_batch(r["X"], r["uv"], r["K"], r["models"], r["has_model"], PC.THR)
    P = len(c["X"])
    for p in range(P):
        q = P - 1 - p
        assert np.array_equal(fwd.masks[p], rev.masks[q]) and fwd.n_inliers[p] == rev.n_inliers[q] and fwd.refit_ok[p] == rev.refit_ok[q]
        assert np.array_equal(bits(fwd.refit[p]), bits(rev.refit[q]))


def test_error_paths_leave_the_context_usable(hip_ctx):
    c = PC.mixed()
    pp, X, uv = pnp.pack_points(c["X"], c["uv"])
    rows = [np.asarray(s, np.int32).reshape(-1, 5) for s in c["samples"]]
    sp, idx = pnp._ptr([len(r) for r in rows]), np.concatenate(rows)
    want = hip_ctx.pnp_hypotheses_batch(c["X"], c["uv"], c["K"], c["samples"], PC.THR)
    f = PC.refit_case()
    fpp, fX, fuv = pnp.pack_points(f["X"], f["uv"])
    fwant = hip_ctx.pnp_refit_batch(f["X"], f["uv"], f["K"], f["models"], f["has_model"], PC.THR)

    def hyp(point_ptr=pp, Xa=X, uva=uv, K=PC.K, sample_ptr=sp, m=5, sample_idx=idx, n_problems=None):
        return pnp.pnp_hypotheses_batch_raw(hip_ctx, point_ptr, Xa, uva, K, sample_ptr, m, sample_idx, PC.THR, n_problems=n_problems)

    def refit(point_ptr=fpp, Xa=fX, uva=fuv, K=PC.K, models=f["models"], has=f["has_model"], n_problems=None):
        return pnp.pnp_refit_batch_raw(hip_ctx, point_ptr, Xa, uva, K, models, has, PC.THR, n_problems=n_problems)

    def fails(call, code, *words, **kw):
        with pytest.raises(capi.EachamError) as e:
            call(**kw)
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)
        again = hyp()                                                            # the next call succeeds, same bits
        for p in range(len(rows)):
            assert np.array_equal(bits(again.models[p]), bits(want.models[p])) and np.array_equal(again.inlier_counts[p], want.inlier_counts[p])
        again = refit()
        assert np.array_equal(bits(again.refit), bits(fwant.refit)) and np.array_equal(again.n_inliers, fwant.n_inliers)

    def changed(t, k, v):
        t = t.copy()
        t[k] = v
        return t

    for call, table in ((hyp, pp), (refit, fpp)):
        fails(call, capi.ERR_INVALID, "negative", n_problems=-1)
        fails(call, capi.ERR_INVALID, "null", point_ptr=None, n_problems=len(table) - 1)
        fails(call, capi.ERR_INVALID, "start at 0", point_ptr=changed(table, 0, 1))
        fails(call, capi.ERR_INVALID, "problem 1", "decreases", point_ptr=changed(table, 2, table[1] - 1))
        fails(call, capi.ERR_CAPACITY, "2^31", point_ptr=changed(table, len(table) - 1, 1 << 31))
        fails(call, capi.ERR_INVALID, "null array", K=None)
        fails(call, capi.ERR_INVALID, "null array", Xa=None)
    fails(refit, capi.ERR_INVALID, "null array", models=None)
    fails(refit, capi.ERR_INVALID, "null array", has=None)
    fails(hyp, capi.ERR_INVALID, "null", sample_ptr=None)
    fails(hyp, capi.ERR_INVALID, "problem 2", "decreases", sample_ptr=changed(sp, 3, sp[2] - 1))
    fails(hyp, capi.ERR_CAPACITY, "2^31", sample_ptr=changed(sp, len(sp) - 1, 1 << 31))
    fails(hyp, capi.ERR_INVALID, "null array", sample_idx=None)
    fails(hyp, capi.ERR_INVALID, "sample_size", m=4)
    fails(hyp, capi.ERR_INVALID, "sample_size", m=65)
    out = idx.copy()
    out[int(sp[3]) + 1, 2] = len(c["X"][3])                                      # one past the end of problem 3's points
    fails(hyp, capi.ERR_INVALID, "problem 3", sample_idx=out)
    out = idx.copy()
    out[int(sp[1]), 0] = -1
    fails(hyp, capi.ERR_INVALID, "problem 1", sample_idx=out)
    with pytest.raises(capi.EachamError) as e:                                   # the two per-sample results are required
        hip_ctx._check(capi.lib().eacham_pnp_hypotheses_batch(
            hip_ctx.handle, len(pp) - 1, C.c_void_p(pp.ctypes.data), C.c_void_p(X.ctypes.data), C.c_void_p(uv.ctypes.data),
            C.c_void_p(PC.K.ctypes.data), C.c_void_p(sp.ctypes.data), 5, C.c_void_p(idx.ctypes.data), PC.THR, None, None, None))
    assert e.value.code == capi.ERR_INVALID
