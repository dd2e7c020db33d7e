"""CPU: the yardsticks of eacham_pnp_hypotheses_batch / eacham_pnp_refit_batch and of the round loop over them — the per-problem
COMPOSITION of the calls that already exist, written once over whatever `solve` / `score` it is given:

  compose_hypotheses   solve_pnp on the problem's rows, then score_hypotheses(kind pnp) for the counts
  compose_refit        score_hypotheses with one model and its errors, the compaction err <= thr, solve_pnp on one row of inliers
  round_ransac         SolvePnPRansac's loop for ONE problem: chunks of 256 samples through the two above, the sequential rule
                       replayed over the chunk's counts in sample order

Here they run on the CPU oracle (oracle_api) and round_ransac is held against the sequential statement of
tests/estimator_reference.py (one sample at a time), which also ASSERTS what the cases of tests/pnp_batch_cases.py are for;
tests/test_pnp_batch_gpu.py runs the same functions over the device library's eacham_solve_pnp / eacham_score_hypotheses and
holds the batched entry points to them bit for bit."""
import numpy as np
import pytest

import estimator_reference as ER
import oracle_api as O
import pnp_batch_cases as PC

M = PC.M


def bits(x, dtype=np.float64):
    return np.ascontiguousarray(x, dtype=dtype).view({4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize])


def compose_hypotheses(solve, score, X, uv, K, samples, thr):
    """Per problem (models [s, 12], n_models [s], counts [s]). solve(X, uv, K, samples) -> (models, ok);
    score("pnp", X, uv, models, K, thr) -> (errors or None, counts, medians)."""
    out = []
    for x, u, rows in zip(X, uv, samples):
        rows = np.asarray(rows, np.int32).reshape(-1, M)
        s = len(rows)
        if s == 0 or len(u) < M:
            out.append((np.zeros((s, 12)), np.zeros(s, np.int32), np.zeros(s, np.int32)))
            continue
        models, ok = solve(x, u, K, rows)
        _, cnt, _ = score("pnp", x, u, models, K, thr)
        out.append((models, ok, np.where(ok != 0, cnt, 0).astype(np.int32)))
    return out


def compose_refit(solve, score, X, uv, K, models, has_model, thr):
    """Per problem a dict mask, n_inliers, refit, refit_ok."""
    out = []
    for p, (x, u) in enumerate(zip(X, uv)):
        rec = {"mask": np.zeros(len(u), np.uint8), "n_inliers": 0, "refit": np.zeros(12), "refit_ok": 0}
        if has_model[p]:
            err, _, _ = score("pnp", x, u, models[p], K, thr)
            rec["mask"] = (err[0] <= np.float32(thr)).astype(np.uint8)
            rows = np.nonzero(rec["mask"])[0].astype(np.int32)          # ascending point index
            rec["n_inliers"] = len(rows)
            if len(rows) >= 5:
                refit, rok = solve(x, u, K, rows[None])
                rec["refit"], rec["refit_ok"] = refit[0], int(rok[0])
        out.append(rec)
    return out


def round_ransac(solve, score, X, uv, K, samples, max_iters, reprojection_error=4.0, confidence=0.999):
    """SolvePnPRansac for one problem (include/eacham/PnPHip.hpp): same dict as estimator_reference.pnp_ransac, plus `rounds`."""
    X, uv = np.asarray(X, float).reshape(-1, 3), np.asarray(uv, float).reshape(-1, 2)
    n = len(uv)
    out = {"ok": False, "iterations": 0, "winner": -1, "rounds": 0}
    if n < M or max_iters <= 0:
        return out
    samples = np.asarray(samples, np.int32).reshape(-1, M)
    thr = float(np.float32(reprojection_error) * np.float32(reprojection_error))
    budget, best, model, first = max_iters, -1, None, 0
    while first < budget:
        rows = samples[first:min(first + PC.CHUNK, max_iters)]
        (models, ok, cnt), = compose_hypotheses(solve, score, [X], [uv], K, [rows], thr)
        out["rounds"] += 1
        for k in range(len(rows)):
            if first + k >= budget:
                break
            out["iterations"] = first + k + 1
            if ok[k] and cnt[k] > max(best, M - 1):
                best, model, out["winner"] = int(cnt[k]), models[k].copy(), first + k
                budget = ER.update_num_iters(confidence, (n - best) / n, M, budget)
        first += PC.CHUNK
    if model is None:
        return out
    rec, = compose_refit(solve, score, [X], [uv], K, [model], [1], thr)
    out.update(ok=True, model=model, inliers=np.nonzero(rec["mask"])[0].astype(np.int32), pose=rec["refit"] if rec["refit_ok"] else model)
    return out


def oracle_score(kind, a, b, models, K, thr):
    return O.score_hypotheses(kind, a, b, models, K, thr)


def assert_same_run(got, want, at=""):
    assert got["ok"] == want["ok"] and got["iterations"] == want["iterations"] and got["winner"] == want["winner"], at
    if want["ok"]:
        assert np.array_equal(bits(got["model"]), bits(want["model"])), at
        assert np.array_equal(got["inliers"], want["inliers"]), at
        assert np.array_equal(bits(got["pose"]), bits(want["pose"])), at


@pytest.fixture(scope="module")
def sequential():
    """estimator_reference.pnp_ransac over every problem of the RANSAC cases, once."""
    out = {}
    for name, make in PC.RANSAC_CASES.items():
        c = make()
        out[name] = (c, [ER.pnp_ransac(x, u, c["K"], s, c["max_iters"]) for x, u, s in zip(c["X"], c["uv"], c["samples"])])
    return out


@pytest.mark.parametrize("name", list(PC.RANSAC_CASES))
def test_the_round_wise_composition_is_the_sequential_ransac(sequential, name):
    c, want = sequential[name]
    for p, w in enumerate(want):
        got = round_ransac(O.solve_pnp, oracle_score, c["X"][p], c["uv"][p], c["K"], c["samples"][p], c["max_iters"])
        assert_same_run(got, w, f"{name} problem {p}")
        assert got["rounds"] == (0 if len(c["uv"][p]) < M else -(-w["iterations"] // PC.CHUNK))


def test_the_cases_hold_what_they_are_for(sequential):
    c, r = sequential["rounds"]
    assert r[0]["ok"] and r[0]["iterations"] <= PC.CHUNK and len(r[0]["inliers"]) > 64                 # done inside the first chunk
    assert r[1]["ok"] and r[1]["iterations"] > 2 * PC.CHUNK and 5 <= len(r[1]["inliers"]) <= 64         # at least three rounds
    assert not r[2]["ok"] and r[2]["iterations"] == 0                                                   # fewer than 5 points
    assert not r[3]["ok"] and r[3]["winner"] == -1 and r[3]["iterations"] == c["max_iters"]             # collinear: never a model
    assert r[4]["ok"] and np.linalg.matrix_rank(c["X"][4] - c["X"][4].mean(0), tol=1e-9) == 2           # coplanar
    c, r = sequential["ties"]
    for p, w in enumerate(r):
        rows = c["samples"][p]
        assert w["ok"] and w["winner"] % 2 == 0 and np.array_equal(rows[w["winner"]], rows[w["winner"] + 1])   # the twin came later and lost
    thr = PC.THR
    s = PC.structure()
    h = compose_hypotheses(O.solve_pnp, oracle_score, s["X"], s["uv"], s["K"], s["samples"], thr)
    assert h[0][1].tolist() == [1, 0, 1] and h[1][1].all() and not h[2][1].any() and h[3][1].all()
    assert max(int(x[2].max()) for x in (h[0], h[1], h[3])) >= 5
    m = PC.mixed()
    h = compose_hypotheses(O.solve_pnp, oracle_score, m["X"], m["uv"], m["K"], m["samples"], thr)
    assert [len(u) for u in m["uv"]] == [4, 5, 6, 64, 65, 257, 600] and not h[0][1].any() and all(x[1].any() for x in h[1:])
    f = PC.refit_case()
    rf = compose_refit(O.solve_pnp, oracle_score, f["X"], f["uv"], f["K"], f["models"], f["has_model"], thr)
    assert rf[0]["n_inliers"] > 64 and rf[0]["refit_ok"] and 5 <= rf[1]["n_inliers"] <= 64 and rf[1]["refit_ok"]
    assert rf[2]["n_inliers"] == 0 and not rf[2]["refit_ok"]
    p, line = f["collinear"]
    assert np.array_equal(np.nonzero(rf[p]["mask"])[0], line) and rf[p]["n_inliers"] == 10 and not rf[p]["refit_ok"] and not rf[p]["refit"].any()
    assert rf[4]["n_inliers"] < 5 and not rf[4]["refit_ok"]
    assert rf[5]["refit_ok"] and rf[5]["mask"][:PC.REFIT_BLOCK].any() and rf[5]["mask"][PC.REFIT_BLOCK:].any()
    assert rf[6]["refit_ok"] and rf[6]["n_inliers"] > 64
    e = PC.refit_edges()
    h = compose_hypotheses(O.solve_pnp, oracle_score, e["X"], e["uv"], e["K"], e["samples"], thr)
    rf = compose_refit(O.solve_pnp, oracle_score, e["X"], e["uv"], e["K"], e["models"], e["has_model"], thr)
    assert [len(u) for u in e["uv"]] == [63, 64, 65, 255, 256, 257] and [int(x[2].max()) for x in h] == [62, 63, 64, 254, 255, 256]
    assert [r["n_inliers"] for r in rf] == [62, 63, 64, 254, 255, 256] and all(r["refit_ok"] and r["mask"][-1] for r in rf)


def test_the_python_round_loop_is_the_same_rule():
    """eacham_amd.pnp.pnp_ransac_batch over the composed calls (no device): the whole list at once equals problem by problem."""
    from eacham_amd import pnp

    c = PC.ties()
    hyp = lambda X, uv, K, rows, thr, want: _as_batch(compose_hypotheses(O.solve_pnp, oracle_score, X, uv, K, rows, thr))   # noqa: E731
    ref = lambda X, uv, K, models, has, thr: _as_refit(compose_refit(O.solve_pnp, oracle_score, X, uv, K, models, has, thr))   # noqa: E731
    got, turns = pnp.pnp_ransac_batch(None, c["X"], c["uv"], c["K"], c["samples"], c["max_iters"], hypotheses=hyp, refit=ref)
    want = [round_ransac(O.solve_pnp, oracle_score, x, u, c["K"], s, c["max_iters"]) for x, u, s in zip(c["X"], c["uv"], c["samples"])]
    for p, w in enumerate(want):
        assert_same_run(got[p], w, f"problem {p}")
    assert turns == max(w["rounds"] for w in want) + 1


def _as_batch(recs):
    from eacham_amd import pnp
    return pnp.PnpHypotheses([r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs], None, None)


def _as_refit(recs):
    from eacham_amd import pnp
    return pnp.PnpRefit([r["mask"] for r in recs], np.array([r["n_inliers"] for r in recs]), np.array([r["refit"] for r in recs]),
                        np.array([r["refit_ok"] for r in recs]), None)
