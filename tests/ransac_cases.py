"""Seeded problem lists for eacham_ransac_batch (shared by tests/test_ransac_reference.py, CPU, and the GPU tests): the smallest
shapes at which the segmented kernels and the rule can still go wrong, on tests/lmeds_batch_cases.py's problems (homography,
essential) and tests/fundamental_cases.py's scenes (fundamental).

A case is a dict: kind, uv1 / uv2 = one n_p x 2 array per problem, samples = one s_p x m index array per problem, K = fx fy cx cy,
threshold (squared, in the error's units: K-normalised for the essential kind), confidence."""
import functools

import numpy as np

import fundamental_cases as FC
import lmeds_batch_cases as LC
import score_cases as SC

M = {"homography": 4, "essential": 5, "fundamental": 7}
KINDS = ("homography", "essential", "fundamental")
CONFIDENCE = {"homography": 0.995, "essential": 0.999, "fundamental": 0.99}      # cv::findHomography / findEssentialMat / findFundamentalMat
PIXELS = {"homography": 3.0, "essential": 1.0, "fundamental": 3.0}               # ... and their thresholds
BOUNDARY_STAGE1 = 5


def K_of(kind):
    return FC.K4.copy() if kind == "fundamental" else LC.K.copy()


def threshold_of(kind, pixels=None):
    """The squared threshold as the adapters form it: pixels, for the essential kind divided by (fx + fy) / 2 first."""
    px = PIXELS[kind] if pixels is None else pixels
    if kind == "essential":
        K = K_of(kind)
        px = px / ((K[0] + K[1]) / 2)
    return float(np.float32(px * px))


def points(kind, n, seed, outliers=0.25):
    """(uv1, uv2, bad): n matches of one pair, a share of them gross outliers."""
    if kind == "fundamental":
        rng = np.random.default_rng(9000 + seed)
        c = FC.scene(7000 + seed, max(n, 8))
        uv1 = c["uv1"][:n] + 0.3 * rng.normal(size=(n, 2))
        uv2 = c["uv2"][:n] + 0.3 * rng.normal(size=(n, 2))
        bad = rng.random(n) < outliers
        uv2[bad] = rng.uniform(0, FC.W, (int(bad.sum()), 2))
        return uv1.astype(np.float32).astype(np.float64), uv2.astype(np.float32).astype(np.float64), bad
    c = SC.two_view_case(n=max(n, 8), n_models=1, seed=seed, outliers=outliers, planar=kind == "homography", facing=True)
    return c["uv1"][:n].copy(), c["uv2"][:n].copy(), c["bad"][:n].copy()


def problem(kind, n, count, seed, outliers=0.25):
    """(uv1, uv2, samples): lmeds_batch_cases.problem for the two kinds it has at its own outlier share, the same recipe otherwise."""
    if kind != "fundamental" and outliers == 0.25:
        return LC.problem(kind, n, count, seed)
    uv1, uv2, _ = points(kind, n, seed, outliers)
    return uv1, uv2, LC.draw(n, M[kind], count, seed + 1000) if n >= M[kind] else np.zeros((0, M[kind]), np.int32)


def _case(kind, probs, threshold=None, confidence=None):
    return {"kind": kind, "uv1": [p[0] for p in probs], "uv2": [p[1] for p in probs], "samples": [np.asarray(p[2], np.int32) for p in probs],
            "K": K_of(kind), "threshold": threshold_of(kind) if threshold is None else threshold,
            "confidence": CONFIDENCE[kind] if confidence is None else confidence}


def single(kind):
    return _case(kind, [problem(kind, 64, 12, 11)])


def mixed(kind):
    """n = m, 6 (below m for the fundamental kind: a "none" record), 7 (odd), 64 (one trip of a wave), 257 (a fifth trip with one lane)."""
    return _case(kind, [problem(kind, n, 6, 20 + k) for k, n in enumerate([M[kind], 6, 7, 64, 257])])


def empties(kind):
    """no samples / fewer than m points (with samples that are then ignored) between two ordinary problems."""
    m = M[kind]
    few = problem(kind, 3, 0, 52)
    few = (few[0], few[1], np.array([[0, 1, 2, 1, 0, 2, 1][:m], [2, 2, 1, 0, 1, 0, 0][:m]], dtype=np.int32))
    return _case(kind, [problem(kind, 40, 5, 50), problem(kind, 30, 0, 51), few, problem(kind, 41, 5, 53)])


def degenerate(kind):
    """Problem 0: a sample whose points coincide between two good ones; problem 1: only such samples; problem 2: ordinary."""
    m = M[kind]
    p0 = problem(kind, 50, 2, 60)
    p0 = (p0[0], p0[1], np.array([p0[2][0], [7] * m, p0[2][1]], dtype=np.int32))
    p1 = problem(kind, 50, 0, 61)
    p1 = (p1[0], p1[1], np.array([[3] * m, [9] * m], dtype=np.int32))
    return _case(kind, [p0, p1, problem(kind, 50, 4, 62)])


def ties(kind):
    """Every sample row appears twice: equal counts, the earlier candidate must win."""
    p = problem(kind, 80, 6, 70)
    q = problem(kind, 33, 4, 71)
    return _case(kind, [(p[0], p[1], np.concatenate([p[2], p[2]])), (q[0], q[1], np.repeat(q[2], 2, axis=0))])


def staged(kind, n, seed, n_bad, n_good, outliers=0.25, repeat_good=False):
    """A problem whose first n_bad samples each hold an outlier and whose next n_good hold none (repeat_good: the same one again)."""
    uv1, uv2, bad = points(kind, n, seed, outliers)
    rng = np.random.default_rng(seed + 2000)
    m, good_idx, bad_idx = M[kind], np.nonzero(~bad)[0], np.nonzero(bad)[0]
    rows = []
    for _ in range(n_bad):
        row = np.concatenate([rng.choice(bad_idx, 2, replace=False), rng.choice(good_idx, m - 2, replace=False)])
        rows.append(rng.permutation(row))
    first = rng.choice(good_idx, m, replace=False)
    rows += [first if repeat_good else rng.choice(good_idx, m, replace=False) for _ in range(n_good)]
    return uv1, uv2, np.array(rows, dtype=np.int32).reshape(-1, m)


MULTI_ROOT = {"n": 48, "n_bad": 30, "n_good": 6, "pixels": 6.0, "seeds": (310, 17)}   # seed 310: the only one of 0 .. 399 that shows it


def is_multi_root_record(trace):
    """True iff some sample's root 0.. made a record that dropped the budget below s + 1 and a LATER root of that sample made another."""
    for i, (s, r, _, _, after) in enumerate(trace):
        if after < s + 1 and any(s2 == s and r2 > r for s2, r2, *_ in trace[i + 1:]):
            return True
    return False


def multi_root():
    """Essential only. In problem 0 a later root of the record's own sample wins after root 0 has already dropped the budget below
    s + 1: thirty contaminated samples first, then clean ones, at a 6 px threshold under which several roots of a clean sample
    collect most of the inliers. tests/test_ransac_reference.py asserts that the reference shows it."""
    c = MULTI_ROOT
    return _case("essential", [staged("essential", c["n"], seed, c["n_bad"], c["n_good"]) for seed in c["seeds"]],
                 threshold=threshold_of("essential", c["pixels"]))


def early_stop(kind):
    """10 % outliers, 200 samples: n_used is far below S."""
    return _case(kind, [problem(kind, 100, 200, 90, outliers=0.1), problem(kind, 64, 200, 91, outliers=0.1)])


def boundary(kind):
    """Problem 0: the decisive record (the winner) sits at rank BOUNDARY_STAGE1 - 1, the last rank of pass 1; problem 1: at rank
    BOUNDARY_STAGE1, the first of pass 2. The clean sample is repeated behind itself: its twins tie and lose."""
    return _case(kind, [staged(kind, 60, 95, BOUNDARY_STAGE1 - 1, 40, outliers=0.1, repeat_good=True),
                        staged(kind, 60, 96, BOUNDARY_STAGE1, 40, outliers=0.1, repeat_good=True)])


def no_record(kind):
    """threshold 0: no count above m - 1."""
    return dict(single(kind), threshold=0.0)


@functools.lru_cache(maxsize=None)
def _heavy(kind):
    probs = []
    for share in (0.6, 0.7):
        uv1, uv2, bad = points(kind, 200, 5, share)
        rng = np.random.default_rng(3)
        samples = np.array([rng.choice(200, size=M[kind], replace=False) for _ in range(300)], dtype=np.int32)
        probs.append((uv1, uv2, samples, bad))
    return probs


def heavy(kind):
    """200 matches, 60 % and 70 % of them outliers, 300 random minimal samples: where LMedS cannot tell a wrong edge from a wide one."""
    return dict(_case(kind, _heavy(kind)), bad=[p[3] for p in _heavy(kind)])


def reverse(case):
    return dict(case, uv1=case["uv1"][::-1], uv2=case["uv2"][::-1], samples=case["samples"][::-1])


def normalised(case):
    """The same problems with K-normalised points, for K = NULL; the pixel thresholds of the homography and the fundamental kind
    follow the points (the essential kind's threshold is in normalised units already)."""
    f, c = case["K"][:2], case["K"][2:]
    thr = case["threshold"] if case["kind"] == "essential" else float(np.float32(case["threshold"] / ((f[0] + f[1]) / 2) ** 2))
    return dict(case, uv1=[(u - c) / f for u in case["uv1"]], uv2=[(u - c) / f for u in case["uv2"]], K=None, threshold=thr)


CASES = {"single": single, "mixed": mixed, "empties": empties, "degenerate": degenerate, "ties": ties, "early_stop": early_stop,
         "boundary": boundary, "no_record": no_record, "heavy": heavy}


def build(name, variant):
    """variant: a kind, or a kind + "_noK" (pre-normalised points, K = NULL)."""
    kind = variant.split("_")[0]
    case = multi_root() if name == "multi_root" else CASES[name](kind)
    return normalised(case) if variant.endswith("noK") else case


def every_row_the_library_builds():
    """Every (n, m, confidence, cap) of the cases: the budget rows eacham_ransac_batch builds for them, cap = the largest sample count of
    the call (at least 1), as the entry point takes it."""
    out = set()
    for kind in KINDS:
        cases = [f(kind) for f in CASES.values()] + ([multi_root()] if kind == "essential" else [])
        for c in cases:
            cap = max(1, max(len(s) for s in c["samples"]))
            out |= {(len(u), M[kind], c["confidence"], cap) for u in c["uv1"] if len(u) >= M[kind]}
    return sorted(out)
