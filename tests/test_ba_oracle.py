"""CPU: the bundle-adjustment oracle — Jacobians, chart, Schur vs dense, LM policy, numpy objective."""
import os

import numpy as np
import pytest

from eacham_amd import ba, synth
import np_reference as R
import oracle_api as O
from ba_helpers import schur_step_equals_dense_step

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")
GOLDEN = ["ba_golden.npz", "ba_golden_hard.npz", "ba_golden_policy.npz"]


def small_scene(seed=3, n_cams=6, n_lm=200, k=4, **kw):
    return synth.make_scene(n_cams, n_lm, k, seed=seed, **kw)


def test_reprojection_jacobians_match_finite_differences():
    sc = small_scene()
    K5 = np.array([960.0, 950.0, 0.3, 400.0, 410.0])  # non-zero skew exercises every column
    rng = np.random.default_rng(0)
    for i in range(5):
        T = sc["T_true"][i]
        p = sc["points_true"][i * 7]
        uv = np.array([123.0, -45.0])
        ok, r, Jp, Jl, Jk = O.ba_project(T, p, K5, uv)
        assert ok == 1
        h = 1e-6
        for k in range(6):  # pose: right perturbation in the [omega, v] chart
            e = np.zeros(6); e[k] = h
            rp = O.ba_project(O.ba_pose_retract(T, e), p, K5, uv)[1]
            rm = O.ba_project(O.ba_pose_retract(T, -e), p, K5, uv)[1]
            assert np.allclose((rp - rm) / (2 * h), Jp[:, k], rtol=1e-6, atol=1e-5)
        for k in range(3):
            e = np.zeros(3); e[k] = h
            d = (O.ba_project(T, p + e, K5, uv)[1] - O.ba_project(T, p - e, K5, uv)[1]) / (2 * h)
            assert np.allclose(d, Jl[:, k], rtol=1e-6, atol=1e-5)
        for k in range(5):
            e = np.zeros(5); e[k] = h * 100
            d = (O.ba_project(T, p, K5 + e, uv)[1] - O.ba_project(T, p, K5 - e, uv)[1]) / (2 * h * 100)
            assert np.allclose(d, Jk[:, k], rtol=1e-6, atol=1e-6)
        assert rng is not None


def test_cheirality_gives_zero_residual_and_jacobians():
    T = np.eye(4)
    ok, r, Jp, Jl, Jk = O.ba_project(T, np.array([0.1, 0.2, -1.0]), np.array([900.0, 900, 0, 400, 400]), np.array([1.0, 2.0]))
    assert ok == 0 and not r.any() and not Jp.any() and not Jl.any() and not Jk.any()
    ok, *_ = O.ba_project(T, np.array([0.1, 0.2, 0.0]), np.array([900.0, 900, 0, 400, 400]), np.array([1.0, 2.0]))
    assert ok == 0  # z <= 0 is a cheirality failure too


def test_pose_chart_is_consistent():
    sc = small_scene()
    rng = np.random.default_rng(1)
    for i in range(6):
        T = sc["T_true"][i]
        xi = rng.normal(0, 0.3, 6)
        T2 = O.ba_pose_retract(T, xi)
        R2 = T2[:3, :3]
        assert np.allclose(R2 @ R2.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(R2) - 1) < 1e-12
        assert np.allclose(O.ba_pose_local(T, T2), xi, atol=1e-12)  # Local(x, x (+) xi) == xi
        assert np.allclose(O.ba_pose_local(T, T), 0, atol=1e-15)


def test_graph_error_matches_numpy_statement():
    sc = small_scene(pixel_noise=3.0)
    A = ba.BaArrays.from_scene(sc)
    A.obs_uv[::17] += 40.0  # outliers: Huber branch
    assert np.isclose(O.ba_error(A), R.ba_error_np(A), rtol=1e-12)
    out = O.ba_solve(A, ba.OptimizerConfig("LM", 3, 1e-9, 10.0, False))
    assert np.isclose(out.final_error, R.ba_error_np(A, out.cam_T_wc, out.points, out.K), rtol=1e-10)
    assert np.isclose(out.initial_error, R.ba_error_np(A), rtol=1e-12)


@pytest.mark.parametrize("lam", [0.0, 1e-4, 1.0, 1e3])
def test_schur_complement_equals_dense_solve(lam):
    sc = small_scene(seed=9, n_cams=5, n_lm=60, k=3, pixel_noise=2.0)
    A = ba.BaArrays.from_scene(sc)
    A.obs_uv[::11] += 25.0
    schur_step_equals_dense_step(A, lam)   # (tests/test_ba_ragged_reference.py runs the same check on ragged problems)


def replay_lambda_policy(out, policy):
    """Replays the lambda schedule of a trace under one reading of decreaseLambda."""
    lam, factor, err = 1e-4, 2.0, out.initial_error
    for lam_i, new_err, lin, acc, outer in out.trace:
        assert np.isclose(lam_i, lam, rtol=1e-12)
        if acc:
            rho = (err - new_err) / lin
            assert rho > 1e-3
            lam = max(1e-16, lam * max(1 / 3, 1 - (2 * rho - 1) ** 3))
            factor = 2 * factor if policy == "double" else 2 * 2.0   # 2 * currentFactor | 2 * params.lambdaFactor
            err = new_err
        else:
            lam *= factor
            factor *= 2
    return err


@pytest.mark.parametrize("policy", ["reset", "double"])
def test_lm_follows_the_ceres_default_policy(policy):
    sc = small_scene(seed=5, n_cams=8, n_lm=300, k=4)
    A = ba.BaArrays.from_scene(sc)
    out = O.ba_solve(A, ba.OptimizerConfig.refine_ba(), lm_factor=policy)
    tr = out.trace
    assert out.status == 0 and tr.shape[0] == out.inner_iterations >= out.outer_iterations >= 2
    assert tr[0, 0] == 1e-4  # lambdaInitial
    err = replay_lambda_policy(out, policy)
    assert np.isclose(out.final_error, err, rtol=1e-12) and out.final_error < 0.1 * out.initial_error
    # converged: last accepted decrease below the tolerances or max_iter reached
    assert out.outer_iterations <= 100
    # truth is recovered up to noise
    assert np.abs(out.points - sc["points_true"]).max() < 0.05


def test_the_two_factor_policies_part_after_reject_accept_reject():
    """EACHAM_BA_LM_FACTOR_RESET (default: currentFactor = 2 * lambdaFactor after an accepted step) against
    _DOUBLE (2 * currentFactor): identical until a rejected step follows two accepted ones, different after."""
    sc = synth.make_scene(6, 90, 2, seed=1, rot_noise=0.5, trans_noise=0.5, point_noise=0.8)
    A = ba.BaArrays.from_scene(sc)
    a = O.ba_solve(A, ba.OptimizerConfig.refine_ba(), nthreads=1, lm_factor="reset")
    b = O.ba_solve(A, ba.OptimizerConfig.refine_ba(), nthreads=1, lm_factor="double")
    replay_lambda_policy(a, "reset")
    replay_lambda_policy(b, "double")
    k = int(np.argmax(~np.isclose(a.trace[:min(len(a.trace), len(b.trace)), 0], b.trace[:min(len(a.trace), len(b.trace)), 0])))
    assert k > 0 and a.trace[k - 1, 3] == 0                      # the first different lambda follows a rejected step ...
    assert (a.trace[:k - 1, 3] == 1).sum() >= 2                  # ... that came after at least two accepted ones
    assert np.allclose(a.trace[:k], b.trace[:k])
    assert a.trace[k, 0] < b.trace[k, 0]                         # RESET grows lambda by 4, DOUBLE by more
    assert (a.inner_iterations, a.final_error) != (b.inner_iterations, b.final_error)


@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_pcg_block_jacobi_step_equals_the_direct_step(lam):
    """The iterative solve the reference can configure (BundleAdjuster.cpp:192-200: PCG, block-Jacobi, 1e-10) against
    the direct Schur / Cholesky solve of the same damped system, one step: they differ by the PCG's own truncation."""
    A = ba.BaArrays.from_scene(small_scene(seed=9, n_cams=7, n_lm=150, k=4, pixel_noise=2.0))
    _, _, dc, dl, _, lin, ok = O.ba_step(A, lam, 0)
    _, _, dcp, dlp, _, linp, okp = O.ba_step(A, lam, 2)
    assert ok and okp
    # (the absolute part of the stopping rule, gamma <= 1e-10, leaves 2e-8 .. 2e-6 relative depending on lambda)
    assert np.abs(dcp - dc).max() < 1e-5 * np.abs(dc).max() and np.abs(dlp - dl).max() < 1e-5 * np.abs(dl).max()
    assert np.isclose(linp, lin, rtol=1e-8)


def test_lm_with_pcg_follows_the_direct_solve_on_ba_windows():
    """use_preconditioner selects the iterative solve (oracle and device alike); the direct solve is the limit it
    iterates towards. On windows of the kind RefineBA sees — a perturbed reconstruction, a local window of the TUM stand-in — the LM
    trajectories of the two solves take the same decisions and end within 1e-5 relative (measured 3e-7 / 2e-6)."""
    cases = [ba.BaArrays.from_scene(small_scene(seed=21, n_cams=12, n_lm=900, k=5)),
             ba.BaArrays.from_scene(synth.local_window(synth.make_scene(120, 7200, 10, seed=3), 60))]
    for A in cases:
        d = O.ba_solve(A, ba.OptimizerConfig("LM", 100, 1e-5, 10.0, False))
        p = O.ba_solve(A, ba.OptimizerConfig("LM", 100, 1e-5, 10.0, True))
        assert p.reserved >= 20 * p.inner_iterations and d.reserved == 0   # the PCG did iterate (tens of steps per solve)
        assert (d.outer_iterations, d.inner_iterations) == (p.outer_iterations, p.inner_iterations)
        assert np.array_equal(d.trace[:, 3], p.trace[:, 3]) and np.allclose(d.trace[:, :2], p.trace[:, :2], rtol=1e-6)
        assert np.abs(p.cam_T_wc - d.cam_T_wc).max() < 1e-5 * np.abs(d.cam_T_wc).max()
        assert np.abs(p.points - d.points).max() < 1e-5 * np.abs(d.points).max()
        assert np.isclose(p.final_error, d.final_error, rtol=1e-8)


def test_lm_with_pcg_on_a_far_off_start_is_a_different_trajectory():
    """Recorded, not hidden: from a far-off start (rejected steps, lambda swings over orders of magnitude) the LM
    trajectory amplifies the truncation error of a 1e-10 PCG — the iterative and the direct solve then take
    different decisions and may end in different local minima. Both reduce the error by orders of magnitude."""
    A = ba.BaArrays.from_scene(synth.make_scene(6, 90, 2, seed=1, rot_noise=0.5, trans_noise=0.5, point_noise=0.8))
    d = O.ba_solve(A, ba.OptimizerConfig("LM", 100, 1e-5, 10.0, False), nthreads=1)
    p = O.ba_solve(A, ba.OptimizerConfig("LM", 100, 1e-5, 10.0, True), nthreads=1)
    assert d.final_error < 0.01 * d.initial_error and p.final_error < 0.01 * p.initial_error
    assert abs(p.final_error - d.final_error) < 0.01 * d.final_error


def test_result_is_a_stationary_point_of_the_numpy_objective():
    sc = small_scene(seed=11, n_cams=5, n_lm=80, k=3)
    A = ba.BaArrays.from_scene(sc)
    out = O.ba_solve(A, ba.OptimizerConfig("LM", 100, 1e-12, 10.0, False))
    f0 = R.ba_error_np(A, out.cam_T_wc, out.points, out.K)
    h = 1e-5
    for j in range(0, 80, 9):
        for a in range(3):
            P = out.points.copy(); P[j, a] += h
            Pm = out.points.copy(); Pm[j, a] -= h
            gnum = (R.ba_error_np(A, out.cam_T_wc, P, out.K) - R.ba_error_np(A, out.cam_T_wc, Pm, out.K)) / (2 * h)
            assert abs(gnum) < 2e-3 * max(1.0, f0)
    for i in range(1, 5):
        for k in range(6):
            e = np.zeros(6); e[k] = h
            Tp = out.cam_T_wc.copy(); Tp[i] = O.ba_pose_retract(out.cam_T_wc[i], e)
            Tm = out.cam_T_wc.copy(); Tm[i] = O.ba_pose_retract(out.cam_T_wc[i], -e)
            gnum = (R.ba_error_np(A, Tp, out.points, out.K) - R.ba_error_np(A, Tm, out.points, out.K)) / (2 * h)
            assert abs(gnum) < 2e-2 * max(1.0, f0)


def test_fewer_than_50_landmarks_is_a_silent_no_op():
    sc = small_scene(n_cams=4, n_lm=49, k=3)
    A = ba.BaArrays.from_scene(sc)
    out = O.ba_solve(A, ba.OptimizerConfig.refine_ba())
    assert out.status == 1 and out.outer_iterations == 0
    assert np.array_equal(out.points, A.points) and np.array_equal(out.cam_T_wc.reshape(-1, 16), A.cam_T_wc.reshape(-1, 16))
    sc = small_scene(n_cams=4, n_lm=50, k=3)
    assert O.ba_solve(ba.BaArrays.from_scene(sc), ba.OptimizerConfig.refine_ba()).status == 0


@pytest.mark.parametrize("policy", ["reset", "double"])
@pytest.mark.parametrize("name", GOLDEN)
def test_golden_fixture(name, policy):
    g = np.load(os.path.join(GOLD_DIR, name))
    pre = "" if policy == "reset" else "double_"   # unprefixed keys: the default policy
    if "hard" in name or "policy" in name:
        assert (g[pre + "trace"][:, 3] == 0).sum() >= 1  # the fixture covers the increaseLambda branch
    if "policy" in name:
        assert g["trace"].shape != g["double_trace"].shape  # ... and this one tells the two policies apart
    A = ba.BaArrays(g["cam_T_wc"], g["cam_fixed"], g["points"], g["point_observers"], g["obs_cam"], g["obs_point"],
                    g["obs_uv"], g["K"])
    out = O.ba_solve(A, ba.OptimizerConfig("LM", int(g["max_iter"]), float(g["max_toler"]), 10.0, False), lm_factor=policy)
    assert out.outer_iterations == int(g[pre + "outer_iterations"]) and out.inner_iterations == int(g[pre + "inner_iterations"])
    assert np.allclose(out.trace, g[pre + "trace"], rtol=1e-7, atol=0)
    assert np.allclose(out.cam_T_wc, g[pre + "out_T_wc"], rtol=0, atol=1e-9)
    assert np.allclose(out.points, g[pre + "out_points"], rtol=0, atol=1e-9) and np.allclose(out.K, g[pre + "out_K"], rtol=1e-10)
    assert np.isclose(out.final_error, float(g[pre + "final_error"]), rtol=1e-9)


def test_dogleg_reaches_the_lm_optimum_and_adapts_the_region():
    """DoglegOptimizer restatement (GTSAM 4.1.1 DoglegOptimizerImpl::Iterate, ONE_STEP_PER_ITERATION)."""
    from eacham_amd import ba, synth
    sc = synth.make_scene(6, 90, 4, seed=12345)
    A = ba.BaArrays.from_scene(sc)
    lm = O.ba_solve(A, ba.OptimizerConfig.refine_ba(), nthreads=1)
    big = O.ba_solve(A, ba.OptimizerConfig("DogLeg", 100, 1e-5, 10.0, False), nthreads=1)
    small = O.ba_solve(A, ba.OptimizerConfig("DogLeg", 100, 1e-5, 0.05, False), nthreads=1)
    assert np.isclose(big.final_error, lm.final_error, rtol=1e-5) and np.isclose(small.final_error, lm.final_error, rtol=1e-5)
    assert small.outer_iterations > big.outer_iterations                 # a tiny region needs more steps ...
    r = small.trace[:, 0]
    assert r[0] == np.float32(0.05) and np.allclose(r[1:4] / r[0:3], 3.0)  # ... and grows by 3 |x_d| while rho >= 0.75
    assert (np.diff(small.trace[:, 1]) < 0).all()                         # monotone decrease of the error
    hard = synth.make_scene(6, 90, 2, seed=0, rot_noise=0.5, trans_noise=0.5, point_noise=0.8)
    H = ba.BaArrays.from_scene(hard)
    out = O.ba_solve(H, ba.OptimizerConfig("DogLeg", 100, 1e-5, 10.0, False), nthreads=1)
    rej = out.trace[:, 3] == 0
    assert rej.any() and np.allclose(out.trace[1:, 0][rej[:-1]] / out.trace[:-1, 0][rej[:-1]], 0.5)  # rho < 0 halves the region
