"""Seeded inputs of the PnP refinement tests (tests/test_pnp_refine_reference.py, tests/test_pnp_refine_gpu.py,
tests/test_pnp_refine_cpp_gpu.py, tests/golden/make_pnp_refine_golden.py). The scenes are those of tests/p3p_cases.py (camera points
in a box 2..8 deep, K of 960 px); a start pose is the truth turned by `off` radians about a random axis and moved by `off` in a
random direction. numpy only: nothing here needs the device or mpmath."""
import os

import numpy as np

import p3p_cases as PC

K = PC.K
THR = PC.THR
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_refine_golden.npz")
MAX_TRIES = 20
USED_COUNTS = (3, 4, 5, 63, 64, 65, 128, 129, 300)   # on either side of the 64-row trip of the kernel
# (points, seed, off, planar) of starts so far that the loop rejects 9 or more tries on the way (the third ends at the cap of 20)
FAR_STARTS = ((70, 309, 0.9, False), (20, 321, 1.2, True), (6, 326, 1.2, True))


def unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def turned(T, off, rng):
    """T = R | t turned by `off` rad about a random axis (Rodrigues, on the left) and moved by `off`."""
    a = unit(rng)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    dR = np.eye(3) + np.sin(off) * Kx + (1 - np.cos(off)) * Kx @ Kx
    R, t = T[:9].reshape(3, 3), T[9:]
    return np.concatenate([(dR @ R).reshape(-1), dR @ t + off * unit(rng)])


def problem(n, seed, off, planar=False, noise=0.0):
    """(X [n, 3], uv [n, 2], start pose [12], true pose [12])."""
    rng = np.random.default_rng(seed)
    X, uv, T = PC.scene(rng, n, planar, noise)
    return X, uv, turned(T, off, rng), T


def seeded(count=210, seed0=7000):
    """The classes the loop was prototyped on: 3..300 points, a planar scene in every seventh case, 0 or 1 px of noise, starts off by
    0.01 / 0.05 / 0.2. Three- and four-point problems (where a far start can lead to another of P3P's poses) start 0.01 off, and
    a planar scene has six points or more (four or five noisy coplanar points leave a valley so flat that Newton from the truth
    leaves it).
    A list of dicts X, uv, T0, T, n, planar, noise, off."""
    sizes = (3, 4, 5, 6, 8, 12, 20, 33, 64, 65, 100, 150, 300)
    out = []
    for k in range(count):
        n = sizes[k % len(sizes)]
        planar = k % 7 == 6 and n >= 6
        noise = float((k // 2) % 2)
        off = (0.01, 0.05, 0.2)[k % 3] if n >= 5 else 0.01
        X, uv, T0, T = problem(n, seed0 + k, off, planar, noise)
        out.append(dict(X=X, uv=uv, T0=T0, T=T, n=n, planar=planar, noise=noise, off=off))
    return out


def lists(cases):
    return [c["X"] for c in cases], [c["uv"] for c in cases], np.array([c["T0"] for c in cases]), np.ones(len(cases), np.uint8)


def mask_with(n, used, pattern, rng):
    """A use mask over n rows with exactly `used` bytes set: 'first' rows, 'last' rows, 'alternating' (every other row from row 1,
    n >= 2 used) or 'random'."""
    m = np.zeros(n, np.uint8)
    if pattern == "first":
        m[:used] = 1
    elif pattern == "last":
        m[n - used:] = 1
    elif pattern == "alternating":
        m[1:2 * used:2] = 1
    else:
        m[rng.choice(n, used, replace=False)] = 1
    assert int(m.sum()) == used
    return m


def gpu_list():
    """The list of the byte-identity test: (X, uv, poses, has_pose, use_masks, notes). Per used-row count of USED_COUNTS a problem with
    every row used (mask all ones), one with alternating rows of twice the points, and one with random rows; in between: an empty
    problem, a problem without a pose, one with an all-zero mask, one with only its last row used, one with two used rows, a point
    behind the camera, a NaN pixel in a used row, a NaN pixel in an UNUSED row (refined as if it were not there), a planar scene, the
    three FAR_STARTS (rejected tries), a four-point exact frame. 67 problems."""
    rng = np.random.default_rng(99)
    X, uv, T0, has, use, notes = [], [], [], [], [], []

    def add(p, mask, note, pose=True):
        X.append(p[0]), uv.append(p[1]), T0.append(p[2]), has.append(1 if pose else 0), use.append(mask), notes.append(note)

    for k, m in enumerate(USED_COUNTS):
        add(problem(m, 100 + k, 0.05, noise=1.0), np.ones(m, np.uint8), f"all {m}")
        add(problem(2 * m + 1, 120 + k, 0.2, noise=1.0), mask_with(2 * m + 1, m, "alternating", rng), f"alternating {m}")
        add(problem(m + 37, 140 + k, 0.1, noise=0.5), mask_with(m + 37, m, "random", rng), f"random {m}")
        if k == 2:
            add(problem(0, 1, 0.0), np.zeros(0, np.uint8), "empty")
            add(problem(40, 160, 0.05), np.ones(40, np.uint8), "no pose", pose=False)
        if k == 4:
            add(problem(70, 161, 0.05), np.zeros(70, np.uint8), "mask none")
            add(problem(70, 162, 0.05), mask_with(70, 1, "last", rng), "only the last row")
            add(problem(9, 163, 0.05), mask_with(9, 2, "first", rng), "two rows")
        if k == 6:
            p = problem(50, 164, 0.05)
            p[0][17] = -(p[3][:9].reshape(3, 3).T @ p[3][9:]) - 3.0 * p[3][6:9]        # 3 behind the TRUE camera's centre
            add(p, np.ones(50, np.uint8), "behind")
            p = problem(50, 165, 0.05)
            p[1][11, 1] = np.nan
            add(p, np.ones(50, np.uint8), "nan used")
            p = problem(50, 166, 0.05, noise=1.0)
            p[1][11, 1] = np.nan
            m = np.ones(50, np.uint8)
            m[11] = 0
            add(p, m, "nan unused")
    add(problem(90, 170, 0.1, planar=True, noise=1.0), np.ones(90, np.uint8), "planar")
    for n, seed, off, planar in FAR_STARTS:
        add(problem(n, seed, off, planar=planar, noise=1.0), np.ones(n, np.uint8), "far start")
    add(problem(4, 172, 0.01), np.ones(4, np.uint8), "four exact")
    while len(X) < 67:
        k = len(X)
        n = int(rng.integers(5, 140))
        add(problem(n, 200 + k, 0.1, noise=1.0), mask_with(n, max(3, n // 2), "random", rng), f"filler {n}")
    return X, uv, np.array(T0), np.array(has, np.uint8), use, notes


def cpp_case():
    """For the C++ adapters, which run the RANSAC themselves: p3p_cases.cpp_case with 0.5 px of noise on every pixel (so the polish
    has something to lower), and an exact four-correspondence frame."""
    probs = [PC.problem(300, 0, 50, outliers=0.3, noise=0.5), PC.problem(60, 0, 51, outliers=0.6, noise=0.5),
             PC.problem(4, 0, 52, outliers=0.0, noise=0.0), PC.problem(3, 0, 53, outliers=0.0, noise=0.0),
             PC.problem(90, 0, 54, outliers=0.4, planar=True, noise=0.5), PC.problem(4, 0, 55, outliers=0.0, noise=0.3)]
    return dict(X=[p[0] for p in probs], uv=[p[1] for p in probs], K=K, T=[p[3] for p in probs], max_iters=4 * PC.CHUNK)
