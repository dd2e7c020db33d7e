"""CPU: the yardstick of eacham_lmeds_batch — the per-problem COMPOSITION of the calls that already exist (solve every sample,
compact the candidates, take the medians, first smallest non-NaN, sigma in float64, the winner's errors) — written once, over
whatever `solve` / `score` it is given. Here it runs on the CPU oracle (oracle_api) and is held against the sequential LMedS
statement of tests/estimator_reference.py; tests/test_lmeds_batch_gpu.py runs the same function over the device library's
eacham_solve_minimal / eacham_score_hypotheses and holds eacham_lmeds_batch to it bit for bit. A GPU mismatch can so be traced
to one side."""
import math

import numpy as np
import pytest

import estimator_reference as ER
import lmeds_batch_cases as LC
import oracle_api as O

SOLVER = {"homography": "homography4", "essential": "essential5"}


def none_record(n, candidates=0):
    return {"model": np.zeros(9), "median": np.float32(np.nan), "threshold": np.float32(0), "inliers": 0,
            "mask": np.zeros(n, np.uint8), "winner": (-1, -1, -1), "candidates": candidates}


def compose_one(solve, score, kind, uv1, uv2, samples, K):
    """One problem. solve(solver, a, b, samples, K) -> (models [s, max_models, 9], n_models [s]);
    score(kind, a, b, models, K, threshold) -> (errors [nm, n] float32, inlier counts, medians float32)."""
    m = LC.M[kind]
    n = len(uv1)
    samples = np.asarray(samples, np.int32).reshape(-1, m)
    if n < m or len(samples) == 0:
        return none_record(n)
    models, counts = solve(SOLVER[kind], uv1, uv2, samples, K)
    where = [(s, r) for s in range(len(samples)) for r in range(int(counts[s]))]          # sample order, then root order
    if not where:
        return none_record(n)
    cand = np.array([models[s, r] for s, r in where])
    _, _, med = score(kind, uv1, uv2, cand, K, 0.0)
    best = -1
    for k in range(len(where)):
        if not np.isnan(med[k]) and (best < 0 or med[k] < med[best]):                      # strictly smaller: the first one stays
            best = k
    if best < 0:
        return none_record(n, len(where))
    sigma = max(2.5 * 1.4826 * (1.0 + 5.0 / max(n - m, 1)) * math.sqrt(float(med[best])), 0.001)
    thr = np.float32(sigma * sigma)
    err, cnt, _ = score(kind, uv1, uv2, cand[best], K, float(thr))
    return {"model": cand[best].copy(), "median": med[best], "threshold": thr, "inliers": int(cnt[0]),
            "mask": (err[0] <= thr).astype(np.uint8), "winner": (best, where[best][0], where[best][1]), "candidates": len(where),
            "roots": np.asarray(counts).copy()}


def compose(solve, score, case):
    return [compose_one(solve, score, case["kind"], a, b, s, case["K"]) for a, b, s in zip(case["uv1"], case["uv2"], case["samples"])]


def oracle_compose(case):
    return compose(O.solve_minimal, O.score_hypotheses, case)


def bits(x, dtype):
    return np.ascontiguousarray(x, dtype=dtype).view({4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize])


@pytest.mark.parametrize("kind", ["homography", "essential"])
@pytest.mark.parametrize("name", ["mixed", "ties"])
def test_the_composition_is_the_sequential_lmeds(name, kind):
    case = LC.CASES[name](kind)
    got = oracle_compose(case)
    for p, g in enumerate(got):
        ref = ER.lmeds(kind, case["uv1"][p], case["uv2"][p], case["K"], case["samples"][p])
        assert ref["ok"] == (g["winner"][0] >= 0) and ref["candidates"] == g["candidates"], p
        if not ref["ok"]:
            continue
        assert g["winner"] == (ref["candidate"], ref["sample"], ref["root"]), p
        assert np.array_equal(bits(g["model"], np.float64), bits(ref["model"], np.float64))
        assert bits(g["median"], np.float32) == bits(ref["median"], np.float32) and bits(g["threshold"], np.float32) == bits(ref["threshold"], np.float32)
        assert g["inliers"] == ref["inliers"] == int(g["mask"].sum()) and np.array_equal(g["mask"], ref["mask"])


def test_the_cases_hold_what_they_are_for():
    """Checked here, through the oracle, before the GPU test relies on it."""
    for kind in ("homography", "essential"):
        deg = oracle_compose(LC.degenerate(kind))
        assert deg[0]["roots"][1] == 0 and deg[0]["winner"][0] >= 0 and deg[0]["roots"][0] > 0      # the coincident sample is skipped
        assert deg[1]["candidates"] == 0 and deg[1]["winner"] == (-1, -1, -1) and deg[2]["winner"][0] >= 0
        emp = oracle_compose(LC.empties(kind))
        assert [e["winner"][0] >= 0 for e in emp] == [True, False, False, True]
        tie = LC.ties(kind)
        for p, t in enumerate(oracle_compose(tie)):
            rows = tie["samples"][p]
            first = min(s for s in range(len(rows)) if np.array_equal(rows[s], rows[t["winner"][1]]))
            assert t["winner"][1] == first and sum(np.array_equal(r, rows[first]) for r in rows) == 2   # its twin came later and lost
        mix = oracle_compose(LC.mixed(kind))
        assert all(x["winner"][0] >= 0 for x in mix)
    multi = oracle_compose(LC.multi_root())
    assert max(int(x["roots"].max()) for x in multi) >= 2                                          # a sample with several roots
    assert any(x["winner"][2] > 0 for x in multi) and any(x["winner"][2] == 0 for x in multi)      # the winner is not always root 0
