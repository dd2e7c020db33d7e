"""Seeded problem lists for eacham_lmeds_batch (shared by tests/test_lmeds_batch_reference.py, CPU, and
tests/test_lmeds_batch_gpu.py): the smallest shapes at which the segmented kernels can still go wrong.

A case is a dict: uv1 / uv2 = one n_p x 2 array per problem, samples = one s_p x m index array per problem (indices into the
problem's own points), K = fx fy cx cy. kind "homography" scenes are planar, "essential" ones general."""
import numpy as np

import score_cases as SC

M = {"homography": 4, "essential": 5}
SC_BLOCK = 256        # eacham_amd/csrc/score_dev.hpp: threads of a scoring workgroup
SC_MAX_LDS = 16384    # ... and the largest problem whose keys live in LDS (beyond it: the error row)


def draw(n, m, count, seed):
    """count samples of m distinct indices out of n (n >= m)."""
    rng = np.random.default_rng(seed)
    return np.array([rng.choice(n, size=m, replace=False) for _ in range(count)], dtype=np.int32).reshape(count, m)


def problem(kind, n, count, seed):
    """(uv1, uv2, samples) of one pair: n matches (a quarter of them gross outliers), count random minimal samples."""
    c = SC.two_view_case(n=max(n, 8), n_models=1, seed=seed, outliers=0.25, planar=kind == "homography", facing=True)
    return c["uv1"][:n].copy(), c["uv2"][:n].copy(), draw(n, M[kind], count, seed + 1000) if n >= M[kind] else np.zeros((0, M[kind]), np.int32)


K = np.array(SC.two_view_case(n=8, n_models=1, seed=1)["K"], dtype=np.float64)


def _case(kind, probs):
    return {"kind": kind, "uv1": [p[0] for p in probs], "uv2": [p[1] for p in probs], "samples": [p[2] for p in probs], "K": K}


def single(kind):
    return _case(kind, [problem(kind, 64, 12, 11)])


def mixed(kind):
    """n = m (sigma's max(n - m, 1) branch), 6, 7 (odd), 64, one above SC_BLOCK (a second trip of the point loops)."""
    return _case(kind, [problem(kind, n, 6, 20 + k) for k, n in enumerate([M[kind], 6, 7, 64, SC_BLOCK + 1])])


def key_paths(kind):
    """One problem above SC_MAX_LDS (keys in the workgroup's error row) and one below it (keys in LDS) in the same call; the LDS
    size comes from the largest. 3 samples each: the large problem costs 3 / up to 30 candidates x 16 385 points."""
    return _case(kind, [problem(kind, SC_MAX_LDS + 1, 3, 31), problem(kind, 100, 3, 32)])


def sample_counts(kind):
    return _case(kind, [problem(kind, 60, c, 40 + k) for k, c in enumerate([3, 72, 89])])


def empties(kind):
    """no samples / fewer than m points (with samples that are then ignored) between two ordinary problems."""
    few = problem(kind, 3, 0, 52)
    few = (few[0], few[1], np.array([[0, 1, 2, 1, 0][:M[kind]], [2, 2, 1, 0, 1][:M[kind]]], dtype=np.int32))
    nosamples = problem(kind, 30, 0, 51)
    return _case(kind, [problem(kind, 40, 5, 50), nosamples, few, problem(kind, 41, 5, 53)])


def degenerate(kind):
    """Problem 0: a sample whose points coincide between two good ones; problem 1: only such samples; problem 2: ordinary."""
    m = M[kind]
    p0 = problem(kind, 50, 2, 60)
    p0 = (p0[0], p0[1], np.array([p0[2][0], [7] * m, p0[2][1]], dtype=np.int32))
    p1 = problem(kind, 50, 0, 61)
    p1 = (p1[0], p1[1], np.array([[3] * m, [9] * m], dtype=np.int32))
    return _case(kind, [p0, p1, problem(kind, 50, 4, 62)])


def ties(kind):
    """Every sample row appears twice: equal medians, the earlier candidate must win."""
    p = problem(kind, 80, 6, 70)
    q = problem(kind, 33, 4, 71)
    return _case(kind, [(p[0], p[1], np.concatenate([p[2], p[2]])), (q[0], q[1], np.repeat(q[2], 2, axis=0))])


def multi_root():
    """Essential only: five-point samples with several real roots; over these problems the winner is not always root 0."""
    return _case("essential", [problem("essential", 48, 10, 80 + k) for k in range(6)])


def reverse(case):
    return dict(case, uv1=case["uv1"][::-1], uv2=case["uv2"][::-1], samples=case["samples"][::-1])


def normalised(case):
    """The same problems with K-normalised points, for K = NULL."""
    f, c = case["K"][:2], case["K"][2:]
    return dict(case, uv1=[(u - c) / f for u in case["uv1"]], uv2=[(u - c) / f for u in case["uv2"]], K=None)


CASES = {"single": single, "mixed": mixed, "key_paths": key_paths, "sample_counts": sample_counts, "empties": empties,
         "degenerate": degenerate, "ties": ties}
