"""A plain, sequential statement of eacham_ransac_batch per problem (test infrastructure): RANSACPointSetRegistrator::run one
sample at a time, one candidate at a time, no batches and no budget table. The arithmetic underneath is the CPU oracle's
(oracle_api.solve_minimal / score_hypotheses; tests/fundamental_reference.py for the fundamental kind), the budget is
estimator_reference.update_num_iters, the samples are handed in: every discrete decision below is fully determined.

    budget = S; best = -1
    for s = 0, 1, ... while s < budget:
        for every root r of sample s:
            cnt = #{i : err_i <= threshold};  if cnt > max(best, m - 1): record, budget = update_num_iters(confidence, (n - cnt) / n, m, budget)
"""
import numpy as np

import estimator_reference as ER
import fundamental_reference as FR
import oracle_api as O

M = {"homography": 4, "essential": 5, "fundamental": 7}
SOLVER = {"homography": "homography4", "essential": "essential5", "fundamental": "fundamental7"}


def solve(kind, uv1, uv2, samples, K):
    """(models [s, max_models, 9], n_models [s]) on the CPU."""
    if kind == "fundamental":
        return FR.solve_minimal(uv1, uv2, samples)
    return O.solve_minimal(SOLVER[kind], uv1, uv2, samples, K)


def score(kind, uv1, uv2, models, K, threshold):
    """(errors [nm, n] float32, inlier counts [nm]) on the CPU."""
    if kind == "fundamental":
        err, cnt, _ = FR.score_hypotheses(uv1, uv2, models, float(threshold))
    else:
        err, cnt, _ = O.score_hypotheses(kind, uv1, uv2, models, K, float(threshold))
    return err, cnt


def none_record(n, n_used, candidates=0):
    return {"model": np.zeros(9), "inliers": 0, "mask": np.zeros(n, np.uint8), "winner": (-1, -1, -1), "candidates": candidates, "n_used": n_used}


def ransac_loop(solve_fn, score_fn, kind, uv1, uv2, K, samples, threshold, confidence, trace=None):
    """The loop over whatever solve_fn(kind, uv1, uv2, samples, K) / score_fn(kind, uv1, uv2, models, K, threshold) it is given.
    trace: a list that receives (sample, root, count, budget before, budget after) of every record."""
    m = M[kind]
    uv1, uv2 = np.asarray(uv1, float).reshape(-1, 2), np.asarray(uv2, float).reshape(-1, 2)
    n = len(uv1)
    samples = np.asarray(samples, np.int32).reshape(-1, m)
    S = len(samples)
    if n < m:
        return none_record(n, 0)
    thr = np.float32(threshold)
    budget, best, win, seen, s = S, -1, None, 0, 0
    while s < budget:
        models, counts = solve_fn(kind, uv1, uv2, samples[s][None], K)
        for r in range(int(counts[0])):
            _, cnt = score_fn(kind, uv1, uv2, models[0, r], K, thr)
            c = int(cnt[0])
            if c > max(best, m - 1):                                   # strictly more: the earlier candidate stays
                before = budget
                best, win = c, (seen, s, r, models[0, r].copy())
                budget = ER.update_num_iters(confidence, (n - c) / n, m, budget)
                if trace is not None:
                    trace.append((s, r, c, before, budget))
            seen += 1
        s += 1
    if win is None:
        return none_record(n, S, seen)
    err, _ = score_fn(kind, uv1, uv2, win[3], K, thr)
    return {"model": win[3], "inliers": best, "mask": (err[0] <= thr).astype(np.uint8), "winner": win[:3], "candidates": seen, "n_used": s}


def ransac(kind, uv1, uv2, K, samples, threshold, confidence, trace=None):
    return ransac_loop(solve, score, kind, uv1, uv2, K, samples, threshold, confidence, trace)


def ransac_case(case, trace=None):
    """Every problem of a case of tests/ransac_cases.py."""
    out = []
    for p, (a, b, s) in enumerate(zip(case["uv1"], case["uv2"], case["samples"])):
        t = None if trace is None else []
        out.append(ransac(case["kind"], a, b, case["K"], s, case["threshold"], case["confidence"], t))
        if trace is not None:
            trace.append(t)
    return out
