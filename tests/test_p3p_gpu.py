"""GPU: eacham_solve_p3p / eacham_pnp_hypotheses_batch_p3p (eacham_amd/csrc/p3p.hip) against the CPU restatement
(tests/cpp/p3p_reference.c through tests/p3p_reference.py), EVERY output compared as bytes, on the samples of
tests/golden/p3p_golden.npz (where tests/test_p3p_reference.py holds the restatement to the 60-digit solution set) and on the problem
lists of tests/p3p_cases.py: the smallest shapes at which the lane-per-sample and the wave-per-sample kernel can still go wrong."""
import ctypes as C

import numpy as np
import pytest

from eacham_amd import capi, pnp, score
import p3p_cases as PC
import p3p_reference as R

pytestmark = pytest.mark.gpu


def bits(x, dtype=np.float64):
    return np.ascontiguousarray(x, dtype=dtype).view({4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize])


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(PC.GOLDEN))
    g["ref"] = R.solve_p3p(g["X"], g["uv"], g["K"], g["samples"])
    return g


def assert_same_solve(got, want, at=""):
    for k, (a, b) in enumerate(zip(got, want)):
        same = np.array_equal(a, b) if a.dtype == np.int32 else np.array_equal(bits(a), bits(b))
        assert same, f"{at}: output {('models', 'n_models', 'candidates', 'n_candidates')[k]} differs"


def test_the_solver_equals_the_restatement_on_every_golden_sample(hip_ctx, golden):
    g = golden
    got = hip_ctx.solve_p3p(g["X"], g["uv"], g["K"], g["samples"])
    assert_same_solve(got, g["ref"], "golden")
    assert got[1].sum() >= 300 and set(np.unique(got[3])) >= {1, 2, 4}     # (models nearly everywhere; 1, 2 and 4 candidates all occur)
    again = hip_ctx.solve_p3p(g["X"], g["uv"], g["K"], g["samples"])       # the same call twice
    assert_same_solve(again, got, "second call")


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_sample_counts_at_the_lane_wave_and_workgroup_boundaries(hip_ctx, golden, count):
    g = golden
    rows = g["samples"][:count]
    got = hip_ctx.solve_p3p(g["X"], g["uv"], g["K"], rows)
    assert_same_solve(got, [x[:count] for x in g["ref"]], f"{count} samples")
    twice = hip_ctx.solve_p3p(g["X"], g["uv"], g["K"], np.repeat(rows, 2, axis=0))   # every sample row given twice
    assert_same_solve([x[0::2] for x in twice], got, "first of a pair")
    assert_same_solve([x[1::2] for x in twice], got, "second of a pair")


def test_candidates_null_works(hip_ctx, golden):
    g = golden
    models, nm = hip_ctx.solve_p3p(g["X"], g["uv"], g["K"], g["samples"], want_candidates=False)
    assert np.array_equal(bits(models), bits(g["ref"][0])) and np.array_equal(nm, g["ref"][1])
    vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    idx = np.ascontiguousarray(g["samples"][:70])
    m2, n2, nc = np.zeros((70, 12)), np.zeros(70, np.int32), np.zeros(70, np.int32)
    hip_ctx._check(capi.lib().eacham_solve_p3p(hip_ctx.handle, len(g["X"]), vp(g["X"]), vp(g["uv"]), vp(g["K"]), 70, vp(idx), vp(m2), vp(n2), None, vp(nc)))
    assert np.array_equal(bits(m2), bits(g["ref"][0][:70])) and np.array_equal(nc, g["ref"][3][:70])     # only one of the two optional outputs


def test_degenerate_samples_give_no_model(hip_ctx):
    for name, (X, uv) in PC.degenerate().items():
        rows = np.array([[0, 1, 2, 3], [2, 1, 0, 3], [1, 2, 0, 0]], dtype=np.int32)
        got = hip_ctx.solve_p3p(X, uv, PC.K, rows)
        assert_same_solve(got, R.solve_p3p(X, uv, PC.K, rows), name)
        assert not got[1].any() and not got[0].any() and not got[2].any() and not got[3].any(), name


def device_compose(ctx, c, thr=PC.THR):
    count = lambda x, u, m, k, t: score.score_hypotheses(ctx, "pnp", x, u, m, k, t)[1]   # noqa: E731
    return R.compose_hypotheses(lambda x, u, k, rows: ctx.solve_p3p(x, u, k, rows), count, c["X"], c["uv"], c["K"], c["samples"], thr)


def assert_same_hypotheses(got, want, label=""):
    assert len(want) == len(got.n_models)
    for p, (models, ok, cnt) in enumerate(want):
        at = f"{label} problem {p}"
        assert np.array_equal(got.n_models[p], ok), at
        assert np.array_equal(got.inlier_counts[p], cnt), at
        if got.models is not None:
            assert np.array_equal(bits(got.models[p]), bits(models)), at


def test_a_round_equals_the_single_call_and_the_scorer(hip_ctx):
    c = PC.hyp_case()
    assert [len(u) for u in c["uv"]] == [3, 4, 5, 64, 65, 257, 600, 40, 30, 80, 65] and len(c["samples"][7]) == 0
    got = hip_ctx.pnp_hypotheses_batch_p3p(c["X"], c["uv"], c["K"], c["samples"], PC.THR)
    assert_same_hypotheses(got, device_compose(hip_ctx, c), "device composition")
    cpu = R.compose_hypotheses(R.solve_p3p, lambda x, u, m, k, t: R.score(x, u, m, k, t)[1], c["X"], c["uv"], c["K"], c["samples"], PC.THR)
    assert_same_hypotheses(got, cpu, "restatement")
    assert not got.n_models[0].any() and not got.models[0].any() and not got.inlier_counts[0].any()      # three points: not looked at
    assert got.n_models[1].tolist() == [1, 1, 0, 1] and got.inlier_counts[1].tolist() == [4, 4, 0, 4]    # four points; a duplicate among the three
    assert all(got.n_models[p].any() and got.inlier_counts[p].max() >= 4 for p in (2, 3, 4, 5, 6, 9))
    assert not got.n_models[8].any() and not got.inlier_counts[8].any() and not got.models[8].any()      # collinear: every sample degenerate
    for a, b in ((got.models, bits), (got.n_models, np.asarray), (got.inlier_counts, np.asarray)):       # the duplicated problem
        assert np.array_equal(b(a[4]), b(a[10]))
    lean = hip_ctx.pnp_hypotheses_batch_p3p(c["X"], c["uv"], c["K"], c["samples"], PC.THR, want_models=False)   # models = NULL
    assert lean.models is None
    for p in range(len(c["X"])):
        assert np.array_equal(lean.n_models[p], got.n_models[p]) and np.array_equal(lean.inlier_counts[p], got.inlier_counts[p])
    e = PC.trip_edges()                                                                                  # 63 .. 65 and 255 .. 257 points
    got = hip_ctx.pnp_hypotheses_batch_p3p(e["X"], e["uv"], e["K"], e["samples"], PC.THR)
    assert_same_hypotheses(got, device_compose(hip_ctx, e), "trip edges, device composition")
    cpu = R.compose_hypotheses(R.solve_p3p, lambda x, u, m, k, t: R.score(x, u, m, k, t)[1], e["X"], e["uv"], e["K"], e["samples"], PC.THR)
    assert_same_hypotheses(got, cpu, "trip edges, restatement")
    assert [int(g.max()) for g in got.inlier_counts] == [63, 64, 65, 255, 256, 257] == [len(u) for u in e["uv"]]


def test_the_ransac_loop_equals_the_loop_over_the_restatement(hip_ctx):
    c = PC.ransac_case()
    want, wturns = pnp.pnp_ransac_batch(None, c["X"], c["uv"], c["K"], c["samples"], c["max_iters"], hypotheses=R.hypotheses, refit=R.refit, solver="p3p")
    got, turns = pnp.pnp_ransac_batch(hip_ctx, c["X"], c["uv"], c["K"], c["samples"], c["max_iters"], solver="p3p")
    assert turns == wturns and turns >= 4
    for p, (g, w) in enumerate(zip(got, want)):
        assert g["ok"] == w["ok"] and g["iterations"] == w["iterations"] and g["winner"] == w["winner"], p
        if w["ok"]:
            assert np.array_equal(bits(g["model"]), bits(w["model"])) and np.array_equal(g["inliers"], w["inliers"]), p
            assert np.array_equal(bits(g["pose"]), bits(w["pose"])), p
    assert got[0]["ok"] and got[0]["iterations"] <= PC.CHUNK and got[1]["ok"] and got[1]["iterations"] > 2 * PC.CHUNK
    assert got[2]["ok"] and len(got[2]["inliers"]) == 4 and np.array_equal(bits(got[2]["pose"]), bits(got[2]["model"]))   # a winner and no refit
    assert not got[3]["ok"] and got[3]["iterations"] == 0


SENTINEL_F, SENTINEL_I = -7.25, -77


def test_error_returns_leave_the_outputs_untouched(hip_ctx):
    c = PC.hyp_case()
    pp, X, uv = pnp.pack_points(c["X"], c["uv"])
    rows = [np.asarray(s, np.int32).reshape(-1, 4) for s in c["samples"]]
    sp, idx = pnp._ptr([len(r) for r in rows]), np.ascontiguousarray(np.concatenate(rows))
    S, P = int(sp[-1]), len(pp) - 1
    K = PC.K
    L = capi.lib()
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731

    def changed(t, k, v):
        t = t.copy()
        t[k] = v
        return t

    def batch(code, *words, n_problems=P, point_ptr=pp, Xa=X, uva=uv, Ka=K, sample_ptr=sp, sample_idx=idx, null_out=False):
        m, n, cnt = np.full((S, 12), SENTINEL_F), np.full(S, SENTINEL_I, np.int32), np.full(S, SENTINEL_I, np.int32)
        rc = L.eacham_pnp_hypotheses_batch_p3p(hip_ctx.handle, n_problems, vp(point_ptr), vp(Xa), vp(uva), vp(Ka), vp(sample_ptr), vp(sample_idx),
                                               PC.THR, vp(m), None if null_out else vp(n), vp(cnt))
        msg = L.eacham_last_error(hip_ctx.handle).decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)
        assert (m == SENTINEL_F).all() and (n == SENTINEL_I).all() and (cnt == SENTINEL_I).all(), msg

    batch(capi.ERR_INVALID, "negative", n_problems=-1)
    batch(capi.ERR_INVALID, "null", point_ptr=None)
    batch(capi.ERR_INVALID, "start at 0", point_ptr=changed(pp, 0, 1))
    batch(capi.ERR_INVALID, "problem 1", "decreases", point_ptr=changed(pp, 2, pp[1] - 1))
    batch(capi.ERR_CAPACITY, "2^31", point_ptr=changed(pp, len(pp) - 1, 1 << 31))
    batch(capi.ERR_INVALID, "null", sample_ptr=None)
    batch(capi.ERR_INVALID, "problem 2", "decreases", sample_ptr=changed(sp, 3, sp[2] - 1))
    batch(capi.ERR_CAPACITY, "2^31", sample_ptr=changed(sp, len(sp) - 1, 1 << 31))
    batch(capi.ERR_INVALID, "null array", Ka=None)
    batch(capi.ERR_INVALID, "null array", Xa=None)
    batch(capi.ERR_INVALID, "null array", uva=None)
    batch(capi.ERR_INVALID, "null array", sample_idx=None)
    batch(capi.ERR_INVALID, "null array", null_out=True)
    out = idx.copy()
    out[int(sp[3]) + 1, 3] = len(c["X"][3])                     # one past the end of problem 3's points
    batch(capi.ERR_INVALID, "problem 3", sample_idx=out)
    out = idx.copy()
    out[int(sp[1]), 0] = -1
    batch(capi.ERR_INVALID, "problem 1", sample_idx=out)

    g = PC.scenes(70, 9)
    gX, guv, gS = g[0], g[1], np.ascontiguousarray(g[2])

    def single(code, *words, n_points=len(gX), n_samples=70, Xa=gX, uva=guv, Ka=K, sample_idx=gS, null_out=False):
        m, n = np.full((70, 12), SENTINEL_F), np.full(70, SENTINEL_I, np.int32)
        cand, nc = np.full((70, 4, 12), SENTINEL_F), np.full(70, SENTINEL_I, np.int32)
        rc = L.eacham_solve_p3p(hip_ctx.handle, n_points, vp(Xa), vp(uva), vp(Ka), n_samples, vp(sample_idx), None if null_out else vp(m), vp(n),
                                vp(cand), vp(nc))
        msg = L.eacham_last_error(hip_ctx.handle).decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)
        assert (m == SENTINEL_F).all() and (n == SENTINEL_I).all() and (cand == SENTINEL_F).all() and (nc == SENTINEL_I).all(), msg

    single(capi.ERR_INVALID, "negative size", n_samples=-1)
    single(capi.ERR_INVALID, "negative size", n_points=-1)
    for name in ("Xa", "uva", "Ka", "sample_idx"):
        single(capi.ERR_INVALID, "null argument", **{name: None})
    single(capi.ERR_INVALID, "null argument", null_out=True)
    single(capi.ERR_INVALID, "sample index", sample_idx=changed(gS, (5, 3), len(gX)))
    single(capi.ERR_INVALID, "sample index", sample_idx=changed(gS, (69, 0), -1))
    single(capi.ERR_INVALID, "sample index", n_points=len(gX) - 1)                # the last row's fourth index is now outside
    # the context is still usable, same bits
    assert_same_solve(hip_ctx.solve_p3p(gX, guv, K, gS), R.solve_p3p(gX, guv, K, gS), "after the errors")
    m, n = np.full((1, 12), SENTINEL_F), np.full(1, SENTINEL_I, np.int32)        # nothing to do: success, nothing written
    assert L.eacham_solve_p3p(hip_ctx.handle, len(gX), vp(gX), vp(guv), vp(K), 0, vp(gS), vp(m), vp(n), None, None) == capi.OK
    assert L.eacham_pnp_hypotheses_batch_p3p(hip_ctx.handle, 0, None, None, None, None, None, None, PC.THR, vp(m), vp(n), vp(n)) == capi.OK
    assert (m == SENTINEL_F).all() and (n == SENTINEL_I).all()


def test_the_epnp_round_gives_the_bytes_it_gave_before_a_p3p_call(hip_ctx, golden):
    import pnp_batch_cases as EC
    c = EC.mixed()
    before = hip_ctx.pnp_hypotheses_batch(c["X"], c["uv"], c["K"], c["samples"], EC.THR)
    hip_ctx.solve_p3p(golden["X"], golden["uv"], golden["K"], golden["samples"])
    h = PC.hyp_case()
    hip_ctx.pnp_hypotheses_batch_p3p(h["X"], h["uv"], h["K"], h["samples"], PC.THR)
    after = hip_ctx.pnp_hypotheses_batch(c["X"], c["uv"], c["K"], c["samples"], EC.THR)
    for p in range(len(c["X"])):
        assert np.array_equal(bits(before.models[p]), bits(after.models[p])) and np.array_equal(before.n_models[p], after.n_models[p])
        assert np.array_equal(before.inlier_counts[p], after.inlier_counts[p])
