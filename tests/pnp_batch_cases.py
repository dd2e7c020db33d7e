"""Seeded problem lists for eacham_pnp_hypotheses_batch / eacham_pnp_refit_batch and the round loop over them (shared by
tests/test_pnp_batch_reference.py, CPU, and tests/test_pnp_batch_gpu.py): the smallest shapes at which the segmented kernels and
the replayed RANSAC rule can still go wrong.

A case is a dict: X / uv = one n_p x 3 / n_p x 2 array per problem, samples = one s_p x 5 index array per problem (indices into
the problem's own points; for the RANSAC cases the stream the loop would draw, in order), K = fx fy cx cy, and for the RANSAC
cases max_iters."""
import numpy as np

import score_cases as SC

M = 5
CHUNK = 256          # pnp_detail::kChunk (include/eacham/PnPHip.hpp)
REFIT_BLOCK = 256    # eacham_amd/csrc/pnp_batch.hip: threads of a refit workgroup = points per trip of its point loop
THR = 16.0           # 4 px, squared


def draw(n, count, seed):
    """count samples of 5 distinct indices out of n (n >= 5)."""
    rng = np.random.default_rng(seed)
    return np.array([rng.choice(n, size=M, replace=False) for _ in range(count)], dtype=np.int32).reshape(count, M)


def problem(n, count, seed, outliers=0.3):
    """(X, uv, samples, true pose) of one frame: n correspondences, count random five-point samples. (Point 0 lies AT the camera
    centre of the true pose, as in score_cases.pnp_case: the scorer's z = 0 branch.)"""
    c = SC.pnp_case(n=max(n, 8), n_models=1, seed=seed, outliers=outliers)
    return c["X"][:n].copy(), c["uv"][:n].copy(), draw(n, count, seed + 1000) if n >= M else np.zeros((0, M), np.int32), c["models"][0]


K = np.asarray(SC.pnp_case(n=8, n_models=1, seed=1)["K"], dtype=np.float64)


def project(X, T):
    pc = X @ T[:9].reshape(3, 3).T + T[9:]
    with np.errstate(divide="ignore", invalid="ignore"):   # (point 0 of `problem` is the camera centre)
        return np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], 1)


def _case(probs, **kw):
    return dict({"X": [p[0] for p in probs], "uv": [p[1] for p in probs], "samples": [p[2] for p in probs], "K": K}, **kw)


def planar_problem(n, count, seed, noise=0.3):
    """A COPLANAR scene: EPnP's three-control-point form."""
    X, uv, _, T = SC.planar_pnp_case(n=n + 1, seed=seed, noise=noise)
    return X, uv.astype(np.float32).astype(np.float64), draw(n, count, seed + 1000), T


def collinear_problem(n, count, seed):
    """Every object point on one line: every sample is degenerate."""
    X0, uv, _, T = problem(n, 0, seed)
    t = np.linspace(-1.0, 1.0, n)[:, None]
    X = X0[1] + t * np.array([0.3, -0.2, 0.1])
    return X, project(X, T), draw(n, count, seed + 1000), T


# ---- one round: eacham_pnp_hypotheses_batch ------------------------------------------------------------------------------

def single():
    return _case([problem(64, 12, 11)])


def mixed():
    """4 points (below m: samples that are then not looked at), m, 6, 64, 65, 257 (a second trip of a 256-thread point loop), 600."""
    few = problem(4, 0, 20)
    few = (few[0], few[1], np.array([[0, 1, 2, 3, 0], [3, 2, 1, 0, 1]], dtype=np.int32), few[3])
    return _case([few] + [problem(n, 6, 21 + k) for k, n in enumerate([5, 6, 64, 65, REFIT_BLOCK + 1, 600])])


def empties():
    """A problem with no samples between two ordinary ones."""
    return _case([problem(40, 5, 50), problem(30, 0, 51), problem(41, 5, 53)])


def structure():
    """A coplanar scene and an all-collinear one (every sample degenerate) between ordinary problems; in problem 0 a sample of
    coincident points between two good ones."""
    p0 = problem(50, 2, 60)
    p0 = (p0[0], p0[1], np.array([p0[2][0], [7] * M, p0[2][1]], dtype=np.int32), p0[3])
    return _case([p0, planar_problem(80, 8, 3), collinear_problem(30, 4, 62), problem(50, 4, 63)])


def sample_counts():
    """Sample counts that are no multiple of the waves per workgroup (4) or of the back half's 64 lanes."""
    return _case([problem(60, c, 40 + k) for k, c in enumerate([3, 66, 129])])


def trip_edges():
    """A problem on each side of the count loop's 64-point trip (63, 64, 65 points) and of the refit's 256-point one (255, 256, 257),
    without outliers: every point but point 0 (the camera centre) lies within 4 px of the true pose, the last one included."""
    return _case([problem(n, 4, 110 + k, outliers=0.0) for k, n in enumerate([63, 64, 65, REFIT_BLOCK - 1, REFIT_BLOCK, REFIT_BLOCK + 1])])


HYP_CASES = {"single": single, "mixed": mixed, "empties": empties, "structure": structure, "sample_counts": sample_counts,
             "trip_edges": trip_edges}


# ---- the round loop -------------------------------------------------------------------------------------------------------

def rounds():
    """Problem 0 (~30 % outliers, > 64 inliers) finishes inside the first chunk; problem 1 (~60 % outliers, <= 64 inliers) needs
    at least three rounds; problem 2 has fewer than 5 points; problem 3 is collinear (never a model: the whole budget is used);
    problem 4 is coplanar. tests/test_pnp_batch_reference.py asserts all of this on the sequential reference."""
    few = problem(4, 0, 70)
    return _case([problem(300, 4 * CHUNK, 71, outliers=0.3), problem(120, 4 * CHUNK, 72, outliers=0.6), few,
                  collinear_problem(30, 4 * CHUNK, 73), planar_problem(80, 4 * CHUNK, 5)], max_iters=4 * CHUNK)


def ties():
    """Every sample row appears twice: equal counts must keep the earlier one (the rule is a strict >)."""
    a, b = problem(100, CHUNK, 80), problem(65, CHUNK, 81, outliers=0.4)
    rep = lambda p: (p[0], p[1], np.repeat(p[2], 2, axis=0), p[3])   # noqa: E731
    return _case([rep(a), rep(b)], max_iters=2 * CHUNK)


RANSAC_CASES = {"rounds": rounds, "ties": ties}


# ---- eacham_pnp_refit_batch -----------------------------------------------------------------------------------------------

def refit_case():
    """models / has_model per problem: 0 the true pose over 300 points (> 64 inliers), 1 the true pose over 40 (<= 64 inliers),
    2 no model, 3 a hand-made problem whose inliers are exactly 10 COLLINEAR points (every other pixel 50 px off its projection),
    4 a pose that fits nothing (fewer than 5 inliers), 5 the true pose over 286 points (a second trip of the compaction, inliers
    on both sides of it), 6 a coplanar scene."""
    probs = [problem(300, 0, 90), problem(40, 0, 91), problem(50, 0, 92)]
    X0, _, _, T = problem(30, 0, 93, outliers=0.0)
    X = X0.copy()
    line = np.array([3, 4, 8, 9, 13, 17, 20, 21, 26, 29])
    X[line] = X0[1] + np.linspace(-1.0, 1.0, 10)[:, None] * np.array([0.3, -0.2, 0.1])
    uv = project(X, T)
    off = np.setdiff1d(np.arange(30), line)
    uv[off] += 50.0
    probs.append((X, uv, None, T))
    bad = problem(60, 0, 94)
    probs.append((bad[0], bad[1], None, np.concatenate([np.eye(3).reshape(-1), [0.0, 0.0, 100.0]])))
    probs += [problem(REFIT_BLOCK + 30, 0, 95), planar_problem(80, 0, 7)]
    c = _case(probs)
    c["models"] = np.array([p[3] for p in probs])
    c["has_model"] = np.array([1, 1, 0, 1, 1, 1, 1], dtype=np.uint8)
    c["collinear"] = (3, line)
    return c


def refit_edges():
    """The problems of trip_edges under their true poses: n - 1 inliers, the last point of a trip and the first of the next among them."""
    c = trip_edges()
    probs = [problem(len(x), 0, 110 + k, outliers=0.0) for k, x in enumerate(c["X"])]
    c.update(models=np.array([p[3] for p in probs]), has_model=np.ones(len(probs), dtype=np.uint8))
    return c


def reverse(case):
    r = dict(case, X=case["X"][::-1], uv=case["uv"][::-1], samples=case["samples"][::-1])
    if "models" in case:
        r.update(models=case["models"][::-1].copy(), has_model=case["has_model"][::-1].copy())
    return r
