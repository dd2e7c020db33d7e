"""The scenes of the fundamental-matrix tests (tests/test_fundamental_reference.py on the CPU, tests/test_fundamental_gpu.py on the
device): fixed seeds, 800 x 800 images, fx = fy = 960, principal point at the centre, scene points in a box 5 units ahead of the
first camera, a second camera rotated by about 0.2 rad and moved by about one unit. Exact correspondences unless said otherwise."""
import functools

import numpy as np

W = H = 800
K = np.array([[960.0, 0.0, 400.0], [0.0, 960.0, 400.0], [0.0, 0.0, 1.0]])
K4 = np.array([960.0, 960.0, 400.0, 400.0])
MASK64 = (1 << 64) - 1


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def camera(rng, angle=0.2):
    """(R, t) of the second camera: x2 = R x1 + t."""
    w = rng.normal(size=3)
    w *= angle / np.linalg.norm(w)
    t = rng.normal(size=3)
    t *= rng.uniform(0.6, 1.2) / np.linalg.norm(t)
    return rodrigues(w), t


def box(rng, n):
    return np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-1.2, 1.2, n), rng.uniform(4.0, 6.0, n)], axis=1)


def project(X, R=None, t=None):
    Xc = X if R is None else X @ R.T + t
    x = Xc @ K.T
    return x[:, :2] / x[:, 2:3]


def true_F(R, t):
    Ki = np.linalg.inv(K)
    F = Ki.T @ skew(t) @ R @ Ki
    return F / np.linalg.norm(F)


def scene(seed, n):
    """n exact correspondences: dict(uv1 [n, 2], uv2 [n, 2], R, t, F)."""
    rng = np.random.default_rng(seed)
    R, t = camera(rng)
    X = box(rng, n)
    return {"uv1": project(X), "uv2": project(X, R, t), "R": R, "t": t, "F": true_F(R, t)}


SCENES = tuple(range(200))      # test 1 and 2: seven points to solve from + 50 held out, per seed
HELD_OUT = 50


@functools.lru_cache(maxsize=None)
def minimal_scenes():
    """The 200 scenes as ONE point list of 200 x 57 correspondences and one sample per scene (its first seven points); the
    held-out points of scene k are rows 57 k + 7 .. 57 k + 56."""
    per = 7 + HELD_OUT
    sc = [scene(1000 + s, per) for s in SCENES]
    uv1 = np.concatenate([c["uv1"] for c in sc])
    uv2 = np.concatenate([c["uv2"] for c in sc])
    samples = np.array([[per * k + i for i in range(7)] for k in range(len(sc))], dtype=np.int32)
    for a in (uv1, uv2, samples):
        a.setflags(write=False)
    return uv1, uv2, samples, per


def epipolar_sym(F, a, b):
    """float64 numpy: per correspondence the sum of the two squared point-to-epipolar-line distances (px^2)."""
    x1 = np.concatenate([a, np.ones((len(a), 1))], axis=1)
    x2 = np.concatenate([b, np.ones((len(b), 1))], axis=1)
    l2, l1 = x1 @ F.T, x2 @ F
    d = np.sum(x2 * l2, axis=1)
    return d * d / (l1[:, 0] ** 2 + l1[:, 1] ** 2) + d * d / (l2[:, 0] ** 2 + l2[:, 1] ** 2)


def epipolar_max(F, a, b):
    """float64 numpy statement of FMEstimatorCallback::computeError: the larger of the two squared distances."""
    x1 = np.concatenate([a, np.ones((len(a), 1))], axis=1)
    x2 = np.concatenate([b, np.ones((len(b), 1))], axis=1)
    l2, l1 = x1 @ F.T, x2 @ F
    d = np.sum(x2 * l2, axis=1)
    return np.maximum(d * d / (l1[:, 0] ** 2 + l1[:, 1] ** 2), d * d / (l2[:, 0] ** 2 + l2[:, 1] ** 2))


# ---- the library's counter-based sample stream (include/eacham/CvSampling.hpp: mix, counter_sample), restated in python integers ------

def mix(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def counter_samples(n, m, count, seed):
    out = np.zeros((count, m), np.int32)
    for s in range(count):
        ctr, sub = 0, []
        while len(sub) < m:
            v = mix((seed * 0x100000001B3 + (s << 20) + ctr) & MASK64) % n
            ctr += 1
            if v not in sub:
                sub.append(v)
        out[s] = sub
    return out


# ---- the LMedS problem: 200 matches, 60 of them replaced by uniform random pixels, 301 counter-stream samples --------------------------
# P(no sample of 301 is outlier-free) = (1 - C(140, 7) / C(200, 7))^301 = (1 - 0.0785)^301 < 2e-11.
LMEDS_SEED = 7
LMEDS_N, LMEDS_OUT, LMEDS_SAMPLES = 200, 60, 301


@functools.lru_cache(maxsize=None)
def lmeds_problem(seed=LMEDS_SEED, n=LMEDS_N, n_out=LMEDS_OUT, n_samples=LMEDS_SAMPLES):
    rng = np.random.default_rng(seed)
    c = scene(5000 + seed, n)
    uv1, uv2 = c["uv1"].copy(), c["uv2"].copy()
    wrong = np.sort(rng.choice(n, n_out, replace=False))
    uv2[wrong] = rng.uniform(0, W, (n_out, 2))
    outlier = np.zeros(n, bool)
    outlier[wrong] = True
    samples = counter_samples(n, 7, n_samples, 12345 + seed)
    for a in (uv1, uv2, outlier, samples):
        a.setflags(write=False)
    return {"uv1": uv1, "uv2": uv2, "outlier": outlier, "samples": samples, "F": c["F"]}


# ---- special samples ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def coplanar_scene(n=12):
    """Every scene point on one plane: the seven-point system has a three-dimensional null space."""
    rng = np.random.default_rng(41)
    R, t = camera(rng)
    X = box(rng, n)
    X[:, 2] = 5.0 + 0.1 * X[:, 0] - 0.2 * X[:, 1]
    return project(X), project(X, R, t)


@functools.lru_cache(maxsize=None)
def translation_scene(n=12):
    """A pure translation: F is skew-symmetric."""
    rng = np.random.default_rng(42)
    X = box(rng, n)
    return project(X), project(X, np.eye(3), np.array([0.7, -0.2, 0.1]))
