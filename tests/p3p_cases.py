"""Seeded inputs of the P3P tests (tests/test_p3p_reference.py, tests/test_p3p_gpu.py, tests/golden/make_p3p_golden.py): the scene
generator the solver's bounds were worked out on, the degenerate samples, the problem lists of the list call and the RANSAC runs.
numpy only: nothing here needs the device or mpmath."""
import os

import numpy as np

M = 4
CHUNK = 256
THR = 16.0   # 4 px, squared
K = np.array([960.0, 960.0, 400.0, 400.0])   # fx fy cx cy
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "p3p_golden.npz")


def rotation(rng):
    """Rotation matrix of a normalised Gaussian quaternion."""
    w, x, y, z = (lambda q: q / np.linalg.norm(q))(rng.standard_normal(4))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def project(X, T):
    pc = X @ T[:9].reshape(3, 3).T + T[9:]
    return np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], 1)


def scene(rng, n=4, planar=False, noise=0.0):
    """(X [n, 3], uv [n, 2], T [12] = R | t): camera points with x, y uniform in [-1, 1] and z uniform in [2, 8] (planar: on a random
    plane through that box), the pose R from a Gaussian quaternion and t ~ N(0, 1)^3, exact pixels (+ noise px of Gaussian noise)."""
    R, t = rotation(rng), rng.standard_normal(3)
    pc = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(2, 8, n)], 1)
    if planar:
        a, b, z0 = rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(3, 7)
        pc[:, 2] = z0 + a * pc[:, 0] + b * pc[:, 1]
    X = (pc - t) @ R                      # R' (pc - t)
    T = np.concatenate([R.reshape(-1), t])
    uv = np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], 1)
    if noise:
        uv = uv + noise * rng.standard_normal(uv.shape)
    return X, uv, T


def scenes(count, seed, planar=False, noise=0.0):
    """count four-point scenes in one point list: (X [4 count, 3], uv [4 count, 2], samples [count, 4], T [count, 12])."""
    rng = np.random.default_rng(seed)
    rec = [scene(rng, 4, planar, noise) for _ in range(count)]
    X, uv, T = np.concatenate([r[0] for r in rec]), np.concatenate([r[1] for r in rec]), np.array([r[2] for r in rec])
    return X, uv, np.arange(4 * count, dtype=np.int32).reshape(count, 4), T


def pose_error(models, T):
    """max-abs over R and t, per row."""
    return np.abs(np.asarray(models).reshape(-1, 12) - np.asarray(T).reshape(-1, 12)).max(1)


def degenerate():
    """{name: (X [4, 3], uv [4, 2])}: samples that must give n_models = 0."""
    rng = np.random.default_rng(7)
    X, uv, T = scene(rng)
    out = {}
    Xc = X.copy()
    Xc[2] = X[0] + 0.37 * (X[1] - X[0])
    out["collinear triple"] = (Xc, project(Xc, T))
    Xe = X.copy()
    Xe[1] = X[0]
    out["two equal object points"] = (Xe, project(Xe, T))
    for bad in (np.nan, np.inf):
        u = uv.copy()
        u[1, 0] = bad
        out[f"pixel {bad}"] = (X, u)
    Xb = X.copy()
    Xb[2] = X[0]                      # B = |X0 - X2|^2 = 0
    out["B = 0"] = (Xb, project(Xb, T))
    return out


# ---- problem lists of eacham_pnp_hypotheses_batch_p3p ---------------------------------------------------------------------

def draw(n, count, seed):
    """count samples of 4 distinct indices out of n (n >= 4)."""
    rng = np.random.default_rng(seed)
    return np.array([rng.choice(n, size=M, replace=False) for _ in range(count)], dtype=np.int32).reshape(count, M)


def problem(n, count, seed, outliers=0.3, planar=False, noise=0.3):
    """(X, uv, samples, true pose): n correspondences of one frame, a share of them with pixels anywhere in the image, count samples."""
    rng = np.random.default_rng(seed)
    X, uv, T = scene(rng, max(n, 1), planar, noise)
    bad = rng.random(len(uv)) < outliers
    uv[bad] = rng.uniform(0, 800, (int(bad.sum()), 2))
    return X[:n], uv[:n], draw(n, count, seed + 1000) if n >= M else np.zeros((0, M), np.int32), T


def collinear_problem(n, count, seed):
    """Every object point on one line: every sample is degenerate."""
    rng = np.random.default_rng(seed)
    X0, _, T = scene(rng, 2)
    X = X0[0] + np.linspace(-1.0, 1.0, n)[:, None] * (X0[1] - X0[0])
    return X, project(X, T), draw(n, count, seed + 1000), T


def _case(probs, **kw):
    return dict({"X": [p[0] for p in probs], "uv": [p[1] for p in probs], "samples": [p[2] for p in probs], "K": K}, **kw)


def hyp_case():
    """Problems of 3 (below a sample: rows that are not looked at), 4, 5, 64, 65, 257 and 600 points; a problem without samples; a
    collinear scene; a planar scene; problem 4 once more at the end (the duplicate)."""
    few = problem(3, 0, 20)
    few = (few[0], few[1], np.array([[0, 1, 2, 0], [2, 1, 0, 7]], dtype=np.int32), few[3])   # (7: outside, and never looked at)
    four = problem(4, 0, 21, outliers=0.0, noise=0.0)
    four = (four[0], four[1], np.array([[0, 1, 2, 3], [3, 1, 0, 2], [0, 0, 1, 2], [0, 1, 2, 2]], dtype=np.int32), four[3])
    probs = [few, four] + [problem(n, 7, 22 + k) for k, n in enumerate([5, 64, 65, 257, 600])]
    probs += [problem(40, 0, 30), collinear_problem(30, 5, 31), problem(80, 9, 32, planar=True), probs[4]]
    return _case(probs)


def trip_edges():
    """A problem on each side of the count loop's 64-point trip and of a 256-point one (63, 64, 65, 255, 256 and 257 points), without
    outliers: some sample of each counts every point, the last included."""
    return _case([problem(n, 4, 60 + k, outliers=0.0) for k, n in enumerate([63, 64, 65, 255, 256, 257])])


def cpp_case():
    """EXACT pixels (the outliers apart), for the C++ adapters, which draw their own samples: 300 points with ~30 % outliers (ends
    inside the first chunk), 60 with ~70 %, exactly 4 points, 3 points (turned away), a planar scene. T = the true poses."""
    probs = [problem(300, 0, 50, outliers=0.3, noise=0.0), problem(60, 0, 51, outliers=0.7, noise=0.0), problem(4, 0, 52, outliers=0.0, noise=0.0),
             problem(3, 0, 53, outliers=0.0, noise=0.0), problem(90, 0, 54, outliers=0.4, planar=True, noise=0.0)]
    return _case(probs, max_iters=4 * CHUNK, T=[p[3] for p in probs])


def ransac_case():
    """Problem 0 (~30 % outliers) ends inside the first chunk; problem 1 (~80 % outliers of 60 points) needs at least three rounds;
    problem 2 has exactly 4 points (a winner and no refit); problem 3 has 3 points (never a sample); problem 4 is planar."""
    four = problem(4, 0, 42, outliers=0.0, noise=0.0)
    four = (four[0], four[1], np.tile(np.array([[0, 1, 2, 3], [1, 2, 3, 0]], dtype=np.int32), (2 * CHUNK, 1)), four[3])
    return _case([problem(300, 4 * CHUNK, 40, outliers=0.3), problem(60, 4 * CHUNK, 41, outliers=0.8), four, problem(3, 0, 43),
                  problem(90, 4 * CHUNK, 44, outliers=0.4, planar=True)], max_iters=4 * CHUNK)
