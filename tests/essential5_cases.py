"""Seeded five-point samples the five-point solver is held on (tests/golden/make_essential5_golden.py solves them at 60 digits,
tests/test_essential5_reference.py and tests/test_essential5_gpu.py read the file). numpy only.

Every scene: N points in front of camera 1 (x, y in [-2, 2] at their depth), camera 2 = a rotation of up to ~0.2 rad and a
translation, K = (500, 500, 320, 240), S five-point samples of distinct indices. The scenes, in the order of SCENES:

  generic            depth 4..9, sideways translation of length 1, exact pixels
  generic_noise      the same with 0.5 px of Gaussian noise on both views
  outliers           0.5 px and 25 % of the correspondences replaced by a random pixel of view 2
  forward            translation along the optical axis (0.02, -0.01, 1), exact pixels
  forward_noise      the same with 0.5 px
  planar             depth 6 +- 0.01 (a near-planar scene: the degenerate configuration of the five-point problem is close), exact
  planar_noise       the same with 0.5 px
  short_noise        a baseline of 0.005 against depth 4..9, 0.5 px

The last three are the families on which the root sweep of the solver lost solutions while it stopped against the root bound
(docs/HISTORY.md): their degree-10 polynomials have roots from 1e0 to 1e4.

There is NO noise-free short baseline here. With exact pixels and a baseline of 0.005 the elimination itself loses every digit
in double (the ten constraints are almost those of a pure rotation): the restatement deviated by 0.7 from the 40-digit solution
set and returned on one sample more models than exist. That is the conditioning of the input, not of the solver, and no
double-precision solver can be held on it."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "essential5_golden.npz")
K = np.array([500.0, 500.0, 320.0, 240.0])
N, S = 100, 64

#         name             seed  depth          translation            noise  outliers
SCENES = (("generic",        11, (4.0, 9.0),    (1.0, "side"),          0.0,   0.0),
          ("generic_noise",  12, (4.0, 9.0),    (1.0, "side"),          0.5,   0.0),
          ("outliers",       13, (4.0, 9.0),    (1.0, "side"),          0.5,   0.25),
          ("forward",        14, (4.0, 9.0),    (1.0, "forward"),       0.0,   0.0),
          ("forward_noise",  15, (4.0, 9.0),    (1.0, "forward"),       0.5,   0.0),
          ("planar",         16, (5.99, 6.01),  (1.0, "side"),          0.0,   0.0),
          ("planar_noise",   17, (5.99, 6.01),  (1.0, "side"),          0.5,   0.0),
          ("short_noise",    18, (4.0, 9.0),    (0.005, "side"),        0.5,   0.0))
NAMES = tuple(s[0] for s in SCENES)
EXACT = tuple(k for k, s in enumerate(SCENES) if s[4] == 0.0 and s[5] == 0.0)          # the true E is a solution of every sample
HARD = tuple(k for k, s in enumerate(SCENES) if s[0] in ("planar", "planar_noise", "short_noise"))


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def rodrigues(w):
    th = np.linalg.norm(w)
    k = skew(w / th)
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)


def sign_fixed(E):
    """Unit Frobenius norm, the entry of largest magnitude positive: the form the solution sets are stored in."""
    E = np.asarray(E, dtype=np.float64).reshape(-1, 9)
    E = E / np.linalg.norm(E, axis=1, keepdims=True)
    lead = E[np.arange(len(E)), np.abs(E).argmax(1)]
    return E * np.where(lead < 0, -1.0, 1.0)[:, None]


def scene(k):
    """(uv1 [N, 2], uv2 [N, 2], samples [S, 5] int32, E_true [9]) of SCENES[k]."""
    _, seed, depth, (length, kind), noise, outliers = SCENES[k]
    rng = np.random.default_rng(seed)
    z = rng.uniform(depth[0], depth[1], N)
    X = np.stack([rng.uniform(-2, 2, N), rng.uniform(-2, 2, N), z], 1)
    R = rodrigues(rng.uniform(0.05, 0.2) * (lambda a: a / np.linalg.norm(a))(rng.normal(size=3)))
    if kind == "side":
        a = rng.uniform(0, 2 * np.pi)
        d = np.array([np.cos(a), np.sin(a), rng.uniform(-0.2, 0.2)])
    else:
        d = np.array([0.02, -0.01, 1.0])
    t = length * d / np.linalg.norm(d)
    Y = X @ R.T + t
    assert Y[:, 2].min() > 1.0
    uv1 = K[:2] * X[:, :2] / X[:, 2:] + K[2:]
    uv2 = K[:2] * Y[:, :2] / Y[:, 2:] + K[2:]
    if noise:
        uv1 = uv1 + noise * rng.normal(size=(N, 2))
        uv2 = uv2 + noise * rng.normal(size=(N, 2))
    if outliers:
        bad = rng.random(N) < outliers
        uv2[bad] = rng.uniform((0, 0), (640, 480), size=(int(bad.sum()), 2))
    samples = np.array([rng.choice(N, 5, replace=False) for _ in range(S)], dtype=np.int32)
    return uv1, uv2, samples, sign_fixed(skew(t) @ R)[0]


def all_scenes():
    """The fixture's inputs: uv1, uv2 [8 N, 2]; samples [8 S, 5] indexing them; scene [8 S]; E_true [8, 9]."""
    parts = [scene(k) for k in range(len(SCENES))]
    uv1, uv2 = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    samples = np.concatenate([p[2] + N * k for k, p in enumerate(parts)]).astype(np.int32)
    scene_id = np.repeat(np.arange(len(SCENES), dtype=np.int32), S)
    return uv1, uv2, samples, scene_id, np.array([p[3] for p in parts])


def load():
    """The fixture, and the slices of its problems: one per scene, the scene's own points and its samples re-based on them."""
    g = dict(np.load(GOLDEN))
    g["problems"] = [(g["uv1"][N * k:N * (k + 1)], g["uv2"][N * k:N * (k + 1)], g["samples"][g["scene"] == k] - N * k) for k in range(len(SCENES))]
    return g


def assert_solution_sets(g, models, counts, label=""):
    """models [512, 10, 9], counts [512] of a solver on the fixture's samples: on every decided sample exactly mp_count models, an
    even number, each within the file's bound of a DISTINCT 60-digit solution up to sign, every 60-digit solution met; on the exact
    scenes the model nearest to the true E is as near as the 60-digit set's nearest, within the bound. Returns the worst distance."""
    dec = g["decided"].astype(bool)
    bound = float(g["bound"])
    assert len(dec) == len(SCENES) * S == len(counts) and (~dec).sum() <= 0.05 * len(dec)
    assert bound == 8 * float(g["deviation"]) and 0 < bound <= 1e-8          # (the cap of the P3P fixture: a unit-norm E at double precision)
    assert (g["mp_count"] % 2 == 0).all() and (counts[dec] % 2 == 0).all(), label
    wrong = np.nonzero(dec & (counts != g["mp_count"]))[0]
    assert not len(wrong), f"{label}: samples {wrong.tolist()} have {counts[wrong].tolist()} models, the 60-digit sets {g['mp_count'][wrong].tolist()}"
    worst = 0.0
    for s in np.nonzero(dec)[0]:
        want = g["mp_models"][g["mp_ptr"][s]:g["mp_ptr"][s + 1]]
        assert not models[s, counts[s]:].any(), (label, s)
        d, pairs = match_sets(models[s, :counts[s]], want)
        assert pairs == len(want), (label, s)
        worst = max(worst, d)
        assert d <= bound, f"{label}: sample {s} ({NAMES[g['scene'][s]]}) is {d:.3e} from its 60-digit set, bound {bound:.3e}"
        k = int(g["scene"][s])
        if k in EXACT:
            near = lambda E: float(np.minimum(np.abs(E - g["E_true"][k]).max(1), np.abs(E + g["E_true"][k]).max(1)).min())   # noqa: E731
            assert near(want) <= 1e-7, s                                     # (pixels rounded to double, through the sample's conditioning)
            assert near(models[s, :counts[s]].reshape(-1, 9)) <= near(want) + bound, (label, s)
    return worst


def match_sets(got, want):
    """Greedy one-to-one matching up to sign of got [a, 9] to want [b, 9] (closest pair first): (worst matched distance,
    number of matched pairs). Both sets complete and within a bound <=> a == b == matched and worst <= bound."""
    got, want = np.asarray(got).reshape(-1, 9), np.asarray(want).reshape(-1, 9)
    if not len(got) or not len(want):
        return 0.0, 0
    d = np.minimum(np.abs(got[:, None] - want[None]).max(2), np.abs(got[:, None] + want[None]).max(2))
    worst, pairs = 0.0, 0
    while np.isfinite(d).any():
        i, j = np.unravel_index(np.argmin(d), d.shape)
        worst, pairs = max(worst, float(d[i, j])), pairs + 1
        d[i, :], d[:, j] = np.inf, np.inf
    return worst, pairs
