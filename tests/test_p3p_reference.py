"""CPU: the yardsticks of the P3P solver (eacham_solve_p3p / eacham_pnp_hypotheses_batch_p3p; include/eacham_hip.h states it).

  the restatement (tests/cpp/p3p_reference.c, what the kernels are held to as bytes) recovers the true pose of 3 000 seeded scenes
      within 1e-8 and the fourth point selects it — a Python port of the recipe gave a worst error of 2.3e-10 over 2 x 3 000 scenes,
      so the bound leaves about 40x;
  its candidates equal the 60-digit solution set (tests/golden/p3p_golden.npz, made by tests/golden/make_p3p_golden.py with mpmath)
      in number and within the file's bound = 8 x the restatement's own largest deviation, on every decided sample;
  numpy.roots finds as many real roots of the same quartic; degenerate samples give no model; planar scenes give the pose; 1 px of
      noise gives errors that scale with the noise; the chosen model's fourth-point error is the CPU oracle's PnP score, as bits;
  the round-wise RANSAC with m = 4 (eacham_amd.pnp.pnp_ransac_batch(solver="p3p") over the restatement) is the one-sample-at-a-time
      rule (replay(), below)."""
import numpy as np
import pytest

from eacham_amd import pnp
import oracle_api as O
import p3p_cases as PC
import p3p_reference as R

BOUND = 1e-8


def bits(x, dtype=np.float64):
    return np.ascontiguousarray(x, dtype=dtype).view({4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize])


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(PC.GOLDEN))
    g["ref"] = R.solve_p3p(g["X"], g["uv"], g["K"], g["samples"], want_quartic=True)
    return g


def candidate_distance(cand, count, T):
    """Per sample the smallest max-abs distance of a candidate from T (inf without candidates)."""
    d = np.abs(cand - np.asarray(T)[:, None, :]).max(2)
    d[np.arange(4)[None, :] >= count[:, None]] = np.inf
    return d.min(1)


def test_truth_recovery_on_3000_scenes():
    X, uv, S, T = PC.scenes(3000, 2024)
    models, nm, cand, nc = R.solve_p3p(X, uv, PC.K, S)
    among, chosen = candidate_distance(cand, nc, T), PC.pose_error(models, T)
    print(f"worst candidate distance {among.max():.3e}, worst chosen-pose error {chosen.max():.3e}, candidate counts {np.bincount(nc).tolist()}")
    assert nm.all() and (nc >= 1).all() and (nc <= 4).all()
    assert among.max() <= BOUND                       # the true pose is among the candidates
    assert chosen.max() <= BOUND                      # and the fourth point selects it
    assert not cand[np.arange(4)[None, :] >= nc[:, None]].any()   # the slots behind the count are zero


def test_solution_set_against_the_60_digit_reference(golden):
    g = golden
    _, _, cand, nc, _, _, _ = g["ref"]
    dec = g["decided"].astype(bool)
    assert len(dec) == 320 and g["kind"].tolist() == [0] * 256 + [1] * 32 + [2] * 32
    assert (~dec).sum() <= 0.02 * len(dec)
    assert float(g["bound"]) == 8 * float(g["deviation"]) and float(g["bound"]) <= BOUND
    assert np.array_equal(nc[dec], g["mp_count"][dec])
    worst = 0.0
    for s in np.nonzero(dec)[0]:
        want = g["mp_candidates"][g["mp_ptr"][s]:g["mp_ptr"][s + 1]]
        if len(want):
            worst = max(worst, float(np.abs(cand[s, :len(want)] - want).max()))
    print(f"worst deviation from the 60-digit candidates {worst:.3e}, bound {float(g['bound']):.3e}")
    assert worst <= float(g["bound"])
    exact = dec & (g["kind"] != 2)                    # exact pixels: the truth is one of the 60-digit candidates
    for s in np.nonzero(exact)[0]:
        want = g["mp_candidates"][g["mp_ptr"][s]:g["mp_ptr"][s + 1]]
        assert np.abs(want - g["T"][s]).max(1).min() <= 1e-9, s   # (the pixels are the projection rounded to double: ~1e-13 px)


def test_the_golden_file_is_what_its_generator_makes(golden):
    MP = pytest.importorskip("p3p_mp_reference")
    g = golden
    for s in (0, 1, 2, 255, 256, 287, 288, 319):
        cand, decided = MP.solve(g["X"][4 * s:4 * s + 4], g["uv"][4 * s:4 * s + 4], g["K"])
        assert decided == bool(g["decided"][s]) and len(cand) == g["mp_count"][s]
        assert np.array_equal(bits(cand), bits(g["mp_candidates"][g["mp_ptr"][s]:g["mp_ptr"][s + 1]]))
    X, uv, S, T = PC.scenes(256, 101)
    assert np.array_equal(bits(X), bits(g["X"][:1024])) and np.array_equal(bits(uv), bits(g["uv"][:1024])) and np.array_equal(bits(T), bits(g["T"][:256]))


def test_numpy_roots_finds_as_many_real_roots(golden):
    _, _, _, _, quartic, roots, nr = golden["ref"]
    for s in np.nonzero(golden["decided"])[0]:
        z = np.roots(quartic[s][::-1])
        real = z[np.abs(z.imag) <= 1e-7 * (1 + np.abs(z.real))].real
        assert len(real) == nr[s], s
        assert np.allclose(np.sort(real), roots[s, :nr[s]], rtol=1e-6, atol=1e-6), s
        assert np.all(np.diff(roots[s, :nr[s]]) >= 0)


@pytest.mark.parametrize("name", list(PC.degenerate()))
def test_degenerate_samples_give_no_model(name):
    X, uv = PC.degenerate()[name]
    for rows in ([0, 1, 2, 3], [2, 1, 0, 3], [1, 2, 0, 0]):
        models, nm, cand, nc = R.solve_p3p(X, uv, PC.K, [rows])
        assert nm[0] == 0 and nc[0] == 0 and not models.any() and not cand.any(), rows


def test_a_duplicate_fourth_index_is_fine():
    X, uv, S, T = PC.scenes(50, 5)
    S = S.copy()
    S[:, 3] = S[:, 1]
    models, nm, cand, nc = R.solve_p3p(X, uv, PC.K, S)
    assert nm.all() and candidate_distance(cand, nc, T).max() <= BOUND


def test_planar_scenes_give_the_pose(golden):
    g = golden
    models, nm = g["ref"][0], g["ref"][1]
    planar = (g["kind"] == 1) & g["decided"].astype(bool)
    assert planar.sum() >= 24 and nm[planar].all()
    X = g["X"].reshape(-1, 4, 3)[planar]
    assert all(np.linalg.matrix_rank(x - x.mean(0), tol=1e-9) == 2 for x in X)
    assert PC.pose_error(models[planar], g["T"][planar]).max() <= BOUND


def test_noise_gives_errors_that_scale_with_it():
    med = {}
    for noise in (0.1, 1.0):
        X, uv, S, T = PC.scenes(2000, 77, noise=noise)     # (the same scenes and the same unit noise, scaled)
        models, nm, cand, nc = R.solve_p3p(X, uv, PC.K, S)
        assert not np.isnan(models).any() and not np.isnan(cand).any()
        assert nm.mean() > 0.95                            # (noise can leave a sample without a positive-depth root)
        med[noise] = np.median(candidate_distance(cand, nc, T)[nm != 0])
    print(f"median distance of the nearest candidate: {med}")
    assert 5.0 <= med[1.0] / med[0.1] <= 20.0              # first order in the noise: ten times the noise, ten times the error
    assert med[1.0] < 0.05                                 # 1 px at f = 960 is 1e-3 rad; depths 2..8 over a baseline ~1


def test_the_fourth_point_error_is_the_oracles_score(golden):
    g = golden
    models, nm, cand, nc = g["ref"][:4]
    for s in range(len(nm)):
        X, uv = g["X"][4 * s:4 * s + 4], g["uv"][4 * s:4 * s + 4]
        err, cnt = R.score(X, uv, cand[s], g["K"], PC.THR)
        oerr, ocnt, _ = O.score_hypotheses("pnp", X, uv, cand[s], g["K"], PC.THR)
        assert np.array_equal(bits(err, np.float32), bits(oerr, np.float32)) and np.array_equal(cnt, ocnt)
        e3 = oerr[:nc[s], 3]
        if nm[s]:
            best = int(np.nanargmin(e3))                   # the first smallest (NaN never wins)
            assert np.array_equal(bits(models[s]), bits(cand[s, best]))
        else:
            assert len(e3) == 0 or np.isnan(e3).all()


# ---- the RANSAC rule with m = 4 -------------------------------------------------------------------------------------------

def replay(X, uv, K, samples, max_iters, reprojection_error=4.0, confidence=0.999):
    """cv::solvePnPRansac with SOLVEPNP_P3P for ONE problem, one sample at a time (RANSACPointSetRegistrator::run): a model with
    strictly more inliers (and at least 4) replaces the best and shrinks the budget."""
    n = len(uv)
    out = {"ok": False, "iterations": 0, "winner": -1, "rounds": 0}
    if n < 4 or max_iters <= 0 or not len(samples):
        return out
    thr = float(np.float32(reprojection_error) * np.float32(reprojection_error))
    budget, best, model, s = max_iters, -1, None, 0
    while s < budget:
        m, ok, _, _ = R.solve_p3p(X, uv, K, samples[s:s + 1])
        out["iterations"] = s + 1
        if ok[0]:
            cnt = int(R.score(X, uv, m, K, thr)[1][0])
            if cnt > max(best, 3):
                best, model, out["winner"] = cnt, m[0].copy(), s
                budget = pnp.ransac_update_num_iters(confidence, (n - best) / n, 4, budget)
        s += 1
    out["rounds"] = -(-out["iterations"] // PC.CHUNK)
    if model is None:
        return out
    err, _ = R.score(X, uv, model, K, thr)
    out.update(ok=True, model=model, inliers=np.nonzero(err[0] <= np.float32(thr))[0].astype(np.int32))
    return out


@pytest.fixture(scope="module")
def ransac_runs():
    c = PC.ransac_case()
    got, turns = pnp.pnp_ransac_batch(None, c["X"], c["uv"], c["K"], c["samples"], c["max_iters"], hypotheses=R.hypotheses, refit=R.refit,
                                      solver="p3p")
    want = [replay(x, u, c["K"], s, c["max_iters"]) for x, u, s in zip(c["X"], c["uv"], c["samples"])]
    return c, got, turns, want


def test_the_round_wise_ransac_is_the_sequential_rule(ransac_runs):
    c, got, turns, want = ransac_runs
    for p, (g, w) in enumerate(zip(got, want)):
        assert g["ok"] == w["ok"] and g["iterations"] == w["iterations"] and g["winner"] == w["winner"], p
        if w["ok"]:
            assert np.array_equal(g["inliers"], w["inliers"]) and np.array_equal(bits(g["model"]), bits(w["model"])), p
    assert turns == max(w["rounds"] for w in want) + 1


def test_the_ransac_case_holds_what_it_is_for(ransac_runs):
    c, got, _, want = ransac_runs
    assert want[0]["ok"] and want[0]["iterations"] <= PC.CHUNK and len(want[0]["inliers"]) > 64          # ends inside the first chunk
    assert want[1]["ok"] and want[1]["iterations"] > 2 * PC.CHUNK                                        # at least three rounds
    assert want[2]["ok"] and len(c["uv"][2]) == 4 and len(want[2]["inliers"]) == 4                        # four points: a winner
    assert np.array_equal(bits(got[2]["pose"]), bits(got[2]["model"]))                                    # ... and no refit
    assert not want[3]["ok"] and want[3]["iterations"] == 0                                               # three points: nothing
    assert want[4]["ok"]
    for p in (0, 4):                                                                                      # the refit (EPnP) is near the truth
        T = PC.problem(300, 0, 40)[3] if p == 0 else PC.problem(90, 0, 44, outliers=0.4, planar=True)[3]
        assert PC.pose_error(got[p]["pose"], T).max() < 0.05, p


def test_the_default_solver_is_unchanged():
    import pnp_batch_cases as EC
    import test_pnp_batch_reference as REF
    c = EC.ties()
    hyp = lambda X, uv, K, rows, thr, want: REF._as_batch(REF.compose_hypotheses(O.solve_pnp, REF.oracle_score, X, uv, K, rows, thr))   # noqa: E731
    ref = lambda X, uv, K, models, has, thr: REF._as_refit(REF.compose_refit(O.solve_pnp, REF.oracle_score, X, uv, K, models, has, thr))   # noqa: E731
    a, ta = pnp.pnp_ransac_batch(None, c["X"], c["uv"], c["K"], c["samples"], c["max_iters"], hypotheses=hyp, refit=ref)
    b, tb = pnp.pnp_ransac_batch(None, c["X"], c["uv"], c["K"], c["samples"], c["max_iters"], hypotheses=hyp, refit=ref, solver="epnp")
    assert ta == tb
    for x, y in zip(a, b):
        REF.assert_same_run(x, y)
    with pytest.raises(ValueError):
        pnp.pnp_ransac_batch(None, c["X"], c["uv"], c["K"], c["samples"], c["max_iters"], hypotheses=hyp, refit=ref, solver="ap3p")
