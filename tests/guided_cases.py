"""The inputs of the guided-matching tests (tests/test_match_guided_reference.py on the CPU, tests/test_match_guided_gpu.py on the
device). A case is one set of resident frames — descriptors (integers in [0, 255], one dimension per case) and pixel coordinates —
a pair list with one model per pair, and the calls made on it (max_error, ratio, max_d2, cross_check).

Cameras are those of tests/graph_verify_cases.py (_project: a small rotation about y and a sideways step, integer pixels), so
the true models are known in closed form: E = [t]x R, F = K^-T E K^-1, and for points of the plane n.X = d the homography
H = K (R + t n' / d) K^-1.
"""
import functools

import numpy as np

import graph_verify_cases as GC

K4 = GC.K4
KM = np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]])
EYE_H = np.eye(3).reshape(9)     # the homography kind with H = I: err = |a - b|^2 in pixels, an admissible set built by hand


def camera(f):
    a = 0.05 * f
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]), np.array([-0.3 * f, 0.02 * f, 0.0])


def relative(f1, f2):
    (R1, t1), (R2, t2) = camera(f1), camera(f2)
    R = R2 @ R1.T
    return R, t2 - R @ t1


def true_E(f1, f2):
    R, t = relative(f1, f2)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return tx @ R


def true_F(f1, f2):
    Ki = np.linalg.inv(KM)
    return (Ki.T @ true_E(f1, f2) @ Ki).reshape(9)


def plane_H(f1, f2, n, d):
    """Points with n . X_cam1 = d (camera f1 must be the world frame: f1 = 0)."""
    assert f1 == 0
    R, t = relative(f1, f2)
    H = KM @ (R + np.outer(t, n) / d) @ np.linalg.inv(KM)
    return (H / H[2, 2]).reshape(9)


def normalised(xy):
    return (np.asarray(xy, np.float64) - K4[2:]) / K4[:2]


def random_desc(rng, n, dim):
    return rng.integers(0, 256, (n, dim)).astype(np.float32)


def noisy(rng, base, sigma=8.0):
    return np.clip(np.rint(base + rng.normal(0, sigma, base.shape)), 0, 255).astype(np.float32)


def scene_points(rng, n):
    return np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 8, n)], axis=1)


def random_pixels(rng, n):
    return np.stack([rng.integers(0, 640, n), rng.integers(0, 480, n)], axis=1).astype(np.float64)


def force_parity(desc, parity):
    """Every row's centred squared norm gets the given parity (flip one value by 1 where it has the other)."""
    d = desc.copy()
    for r in range(len(d)):
        c = d[r].astype(np.int64) - 128
        if int((c * c).sum()) % 2 != parity:
            d[r, 0] += 1 if d[r, 0] < 255 else -1
    c = d.astype(np.int64) - 128
    assert np.all((c * c).sum(1) % 2 == parity)
    return d


def call(max_error, ratio=0.8, max_d2=0, cross_check=True):
    return {"max_error": np.float32(max_error), "ratio": float(ratio), "max_d2": int(max_d2), "cross_check": bool(cross_check)}


def twins_frames(rng, dim, n_base=55, n1=150, n2=130, seen2=100, cams=(0, 3), X=None):
    """Two frames of a scene in which every point has a twin with the same base descriptor; the rest of each frame is distractors
    (random descriptors, random pixels). Returns (descs, xys, truth): truth[q of frame 0] = its row in frame 1 or -1."""
    n_scene = 2 * n_base
    X = scene_points(rng, n_scene) if X is None else X
    base = random_desc(rng, n_base, dim)
    base = np.concatenate([base, base])                       # point i and point i + n_base are twins
    descs, xys, rows = [], [], []
    for f, n, seen in ((cams[0], n1, n_scene), (cams[1], n2, seen2)):
        d = np.concatenate([noisy(rng, base[:seen]), random_desc(rng, n - seen, dim)])
        xy = np.concatenate([GC._project(X[:seen], f), random_pixels(rng, n - seen)])
        perm = rng.permutation(n)                              # row perm[i] holds item i
        dd, xx = np.zeros_like(d), np.zeros_like(xy)
        dd[perm], xx[perm] = d, xy
        descs.append(dd), xys.append(xx), rows.append(perm)
    truth = np.full(n1, -1)
    truth[rows[0][:seen2]] = rows[1][:seen2]
    return descs, xys, truth


@functools.lru_cache(maxsize=None)
def twins(dim=128):
    """The issue's experiment: blind mutual matching finds nothing, the gate at 4 px^2 brings the matches back. Calls: the three
    thresholds, both directions of the cross-check switch; a max_d2 call is added by with_max_d2()."""
    rng = np.random.default_rng(100 + dim)
    descs, xys, truth = twins_frames(rng, dim)
    return {"name": f"twins{dim}", "dim": dim, "kind": "fundamental", "K": None, "descs": descs, "xys": xys, "truth": truth,
            "pairs": np.array([[0, 1]], np.int32), "models": true_F(0, 3)[None],
            "calls": [call(4), call(4, cross_check=False), call(0), call(np.inf), call(np.inf, cross_check=False), call(4, ratio=1.0)]}


@functools.lru_cache(maxsize=None)
def twins_essential(with_K=True):
    """The same scene under E = K' F K: with K on pixels, and with K = NULL on points normalised beforehand."""
    c = dict(twins(128))
    E = true_E(0, 3).reshape(9)
    thr = 4.0 / (K4[0] * K4[0])
    c.update(name="twinsE_K" if with_K else "twinsE_norm", kind="essential", K=K4 if with_K else None, models=E[None],
             xys=c["xys"] if with_K else [normalised(a) for a in c["xys"]], calls=[call(thr), call(thr, cross_check=False), call(np.inf)])
    return c


@functools.lru_cache(maxsize=None)
def planar():
    """The homography kind: 60 points of the plane 0.1 x + z = 6 seen by cameras 0 and 3 with their twins' descriptors, plus distractors."""
    rng = np.random.default_rng(7)
    n_base = 30
    x, y = rng.uniform(-2, 2, 2 * n_base), rng.uniform(-1.5, 1.5, 2 * n_base)
    X = np.stack([x, y, 6.0 - 0.1 * x], axis=1)
    descs, xys, truth = twins_frames(rng, 128, n_base=n_base, n1=90, n2=75, seen2=50, X=X)
    return {"name": "planar", "dim": 128, "kind": "homography", "K": None, "descs": descs, "xys": xys, "truth": truth,
            "pairs": np.array([[0, 1]], np.int32), "models": plane_H(0, 3, np.array([0.1, 0.0, 1.0]), 6.0)[None],
            "calls": [call(4), call(4, cross_check=False), call(0), call(np.inf)]}


ROW_COUNTS = (0, 1, 2, 31, 32, 33, 150)


@functools.lru_cache(maxsize=None)
def row_counts(dim=128):
    """Frames of 0, 1, 2, 31, 32, 33 and 150 rows, every ordered pair of them: frame f holds the first rows of one scene as camera
    f sees it (no permutation: the partner of row i is row i), so the small frames have admissible candidates too."""
    rng = np.random.default_rng(200 + dim)
    X = scene_points(rng, 150)
    base = random_desc(rng, 150, dim)
    descs = [noisy(rng, base[:n]) for n in ROW_COUNTS]
    xys = [GC._project(X[:n], f) for f, n in enumerate(ROW_COUNTS)]
    pairs = np.array([[a, b] for a in range(len(ROW_COUNTS)) for b in range(len(ROW_COUNTS)) if a != b], np.int32)
    return {"name": f"rows{dim}", "dim": dim, "kind": "fundamental", "K": None, "descs": descs, "xys": xys, "pairs": pairs,
            "models": np.stack([true_F(a, b) for a, b in pairs.tolist()]), "calls": [call(4), call(400, cross_check=False), call(np.inf)]}


@functools.lru_cache(maxsize=None)
def dims(dim):
    """One twins pair per stored dimension class: 32 (2 k-steps), 128 (4), 130 (stored as 256) and 256 (8)."""
    c = dict(twins(dim))
    c.update(name=f"dim{dim}", calls=[call(4), call(np.inf, cross_check=False)])
    return c


@functools.lru_cache(maxsize=None)
def parity():
    """Frame 0: every row of the even class; frame 1: every row odd; frame 2: mixed. All orientations."""
    rng = np.random.default_rng(31)
    descs, xys, _ = twins_frames(rng, 32, n_base=20, n1=70, n2=50, seen2=40)
    d2, x2, _ = twins_frames(rng, 32, n_base=20, n1=45, n2=40, seen2=40)
    descs = [force_parity(descs[0], 0), force_parity(descs[1], 1), d2[0]]
    xys = [xys[0], xys[1], x2[0]]
    pairs = np.array([[0, 1], [1, 0], [0, 2], [2, 1], [1, 2], [2, 0]], np.int32)
    F = true_F(0, 3)
    return {"name": "parity", "dim": 32, "kind": "fundamental", "K": None, "descs": descs, "xys": xys, "pairs": pairs,
            "models": np.stack([F, F.reshape(3, 3).T.reshape(9), F, F, F, F]), "calls": [call(4), call(900), call(np.inf, cross_check=False)]}


@functools.lru_cache(maxsize=None)
def duplicates():
    """Duplicated train rows under H = I (err = squared pixel distance, max_error 4):
       query 0: train rows 0 and 1 are the same descriptor, both admissible -> row 0 ranks first, the ratio test fails (1 < ratio never holds)
       query 1: train rows 2 and 3 are the same descriptor, only row 3 (the higher index) admissible -> matched with 3
       query 2: train rows 4 and 5 likewise, only row 4 admissible -> matched with 4
       query 3: its only admissible train row 6 is an exact copy of it: d2 = 0, alone -> matched
       query 4: two admissible exact copies (rows 7, 8): 0 / 0 -> rejected"""
    rng = np.random.default_rng(5)
    A = random_desc(rng, 5, 32)
    B = np.concatenate([noisy(rng, A[0:1]).repeat(2, 0), noisy(rng, A[1:2]).repeat(2, 0), noisy(rng, A[2:3]).repeat(2, 0), A[3:4], A[4:5].repeat(2, 0),
                        random_desc(rng, 3, 32)])
    xa = np.array([[10, 10], [50, 50], [90, 90], [130, 130], [170, 170]], np.float64)
    xb = np.array([[10, 10], [11, 10], [200, 200], [50, 51], [90, 90], [300, 0], [130, 131], [170, 170], [171, 171], [400, 400], [410, 400], [420, 400]], np.float64)
    return {"name": "duplicates", "dim": 32, "kind": "homography", "K": None, "descs": [A, B], "xys": [xa, xb],
            "pairs": np.array([[0, 1], [1, 0]], np.int32), "models": np.stack([EYE_H, EYE_H]),
            "calls": [call(4, cross_check=False), call(4), call(4, ratio=1.0, cross_check=False)],
            "expect_m12": {1: 3, 2: 4, 3: 6}}     # pair 0 without the cross-check: exactly these q -> t


@functools.lru_cache(maxsize=None)
def large_train():
    """4 200 train rows against 64 query rows at D = 32: beyond the 4 096 rows one existing sweep tags in a key."""
    rng = np.random.default_rng(77)
    X = scene_points(rng, 64)
    base = random_desc(rng, 64, 32)
    n2 = 4200
    where = rng.choice(n2, 64, replace=False)                  # the partners' rows in the train frame, some beyond 4 096
    where[:4] = [4199, 4100, 4096, 4095]
    dB, xB = random_desc(rng, n2, 32), random_pixels(rng, n2)
    dB[where], xB[where] = noisy(rng, base), GC._project(X, 3)
    return {"name": "large_train", "dim": 32, "kind": "fundamental", "K": None, "descs": [noisy(rng, base), dB], "xys": [GC._project(X, 0), xB],
            "pairs": np.array([[0, 1]], np.int32), "models": true_F(0, 3)[None], "calls": [call(4), call(4, cross_check=False)]}


@functools.lru_cache(maxsize=None)
def multi_pair():
    """40 pairs in one call over 6 frames (frame 4 is empty, frame 5 has one row): repeated pairs with different models, both
    orientations, an (f, f) pair, pairs with the empty frame, a NaN model, an all-zero model."""
    rng = np.random.default_rng(13)
    X = scene_points(rng, 120)
    base = random_desc(rng, 60, 128)
    base = np.concatenate([base, base])
    sizes = [120, 100, 97, 64, 0, 1]
    descs, xys = [], []
    for f, n in enumerate(sizes):
        perm = rng.permutation(n)
        d, xy = np.zeros((n, 128), np.float32), np.zeros((n, 2))
        d[perm], xy[perm] = noisy(rng, base[:n]), GC._project(X[:n], f)
        descs.append(d), xys.append(xy)
    pairs, models = [], []
    for a in range(4):
        for b in range(4):
            if a != b:
                pairs.append((a, b)), models.append(true_F(a, b))                      # both orientations of every pair
    for a, b in [(0, 1), (2, 3), (1, 0), (1, 3), (3, 2)]:
        pairs.append((a, b)), models.append(true_F(a, b) * 3.5)                      # repeated, the model rescaled
        pairs.append((a, b)), models.append(true_F(b, a))                            # repeated, the other pair's model
        pairs.append((a, b)), models.append(true_F(a, b) + 1e-7 * rng.normal(size=9))  # repeated, perturbed
    pairs.append((2, 2)), models.append(true_F(0, 3))                                # an (f, f) pair
    for a, b in [(4, 0), (0, 4), (4, 4), (5, 0), (0, 5), (5, 5), (4, 5)]:
        pairs.append((a, b)), models.append(true_F(a, b) if a != b else true_F(0, 3))   # an empty frame, a frame of one row
    nan = true_F(0, 1).copy()
    nan[4] = np.nan
    pairs.append((0, 1)), models.append(nan)                                         # a NaN model
    pairs.append((0, 1)), models.append(np.full(9, np.nan))
    pairs.append((0, 1)), models.append(np.zeros(9))                                 # the "none" record
    pairs.append((3, 1)), models.append(np.zeros(9))
    pairs.append((0, 1)), models.append(true_F(0, 1))                                # a live pair behind the dead ones
    return {"name": "multi_pair", "dim": 128, "kind": "fundamental", "K": None, "descs": descs, "xys": xys,
            "pairs": np.array(pairs, np.int32), "models": np.stack(models), "calls": [call(4), call(4, cross_check=False), call(np.inf)]}


def all_cases():
    return [twins(128), twins_essential(True), twins_essential(False), planar(), row_counts(128), dims(32), dims(130), dims(256), parity(),
            duplicates(), large_train(), multi_pair()]


def case_by_name(name):
    return {c["name"]: c for c in all_cases()}[name]


CASE_NAMES = ["twins128", "twinsE_K", "twinsE_norm", "planar", "rows128", "dim32", "dim130", "dim256", "parity", "duplicates", "large_train",
              "multi_pair"]


# ---- the reference's answers, computed once and shared ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference(name, i):
    """(counts, offsets, q, t, d2, stats) of call i of the case, from tests/guided_reference.py."""
    import guided_reference as GR
    c = case_by_name(name)
    k = calls(name)[i]
    return GR.guided(c["kind"], c["descs"], c["xys"], c["pairs"], c["models"], c["K"], k["max_error"], k["ratio"], k["max_d2"], k["cross_check"])


@functools.lru_cache(maxsize=None)
def calls(name):
    """The case's calls, plus — for the cases with a first call that finds matches — that call again under a max_d2 that cuts
    some of its matches and keeps others: the median of the first call's distances (from the reference alone)."""
    import guided_reference as GR
    c = case_by_name(name)
    out = list(c["calls"])
    if name in ("twins128", "planar", "multi_pair", "twinsE_K"):
        k = out[0]
        d2 = GR.guided(c["kind"], c["descs"], c["xys"], c["pairs"], c["models"], c["K"], k["max_error"], k["ratio"], 0, k["cross_check"])[4]
        out.append(call(k["max_error"], k["ratio"], int(np.median(d2)), k["cross_check"]))
        out.append(call(k["max_error"], k["ratio"], int(np.median(d2)), False))
    return out
