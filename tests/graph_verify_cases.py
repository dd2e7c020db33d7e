"""The match graphs the graph-verification tests run on (tests/test_graph_verify_reference.py on the CPU, tests/test_graph_verify_gpu.py
on the device), and the host side of the comparison: the numpy gather and the project's own lmeds_samples / draw_samples, run through
tests/cpp/graph_verify_driver.cpp compiled for the host alone.

small(): 5 frames, frame 1 without keypoints; pixel coordinates are INTEGERS (checkSubset's collinearity test has no knife edge);
caller offsets leave 3 unused entries behind every pair's matches.

  pair  frames  matches  what it is for
  0     0 -> 2     6     m + 1 / m + 2 points
  1     2 -> 0     5     the other orientation; n = m for the essential kind
  2     0 -> 3     0     counts = 0
  3     3 -> 4    64     the largest
  4     3 -> 4     4     a duplicated pair; n = m for the homography, fewer than m for the essential kind
  5     4 -> 0     3     fewer than m for both kinds
  6     0 -> 3    12     every image-1 point on one line: the homography's checkSubset refuses every subset, getSubset gives up
  7     2 -> 4     8     4 of the 8 image-1 points on one line: some subsets are refused, the pair's stream is irregular
  8     0 -> 4    30     a neighbour behind the two
"""
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K4 = np.array([500.0, 500.0, 320.0, 240.0])
M = {"homography": 4, "essential": 5}
COLLINEAR, REFUSING, N_EQ_M = 6, 7, {"homography": 4, "essential": 1}
ITERATIONS = (0, 3, 72, 89)


def _project(X, f):
    """Frame f's camera: a small rotation about y and a sideways step; pixels rounded to integers."""
    a = 0.05 * f
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Xc = X @ R.T + np.array([-0.3 * f, 0.02 * f, 0.0])
    return np.rint(np.stack([K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2], K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3]], axis=1))


def _graph(n_kp, pair_list, gap):
    """pair_list: (f1, f2, q, t). Returns the wire format with `gap` unused entries behind every pair's matches."""
    pairs = np.array([[f1, f2] for f1, f2, _, _ in pair_list], dtype=np.int32).reshape(-1, 2)
    counts = np.array([len(q) for _, _, q, _ in pair_list], dtype=np.int32)
    offsets = np.zeros(len(pair_list), dtype=np.int64)
    offsets[1:] = np.cumsum(counts[:-1] + gap)
    n_src = int(offsets[-1] + counts[-1])
    q = np.full(n_src, 0xFFFFFFF0, dtype=np.uint32)   # (the gaps hold no keypoint of any frame: nothing may read them)
    t = np.full(n_src, 0xFFFFFFF0, dtype=np.uint32)
    for p, (_, _, qq, tt) in enumerate(pair_list):
        q[offsets[p]:offsets[p] + counts[p]] = qq
        t[offsets[p]:offsets[p] + counts[p]] = tt
    return {"n_frames": len(n_kp), "n_kp": list(n_kp), "pairs": pairs, "counts": counts, "offsets": offsets, "q": q, "t": t, "n_src": n_src}


@functools.lru_cache(maxsize=None)
def small():
    rng = np.random.default_rng(11)
    X = np.stack([rng.uniform(-2, 2, 70), rng.uniform(-1.5, 1.5, 70), rng.uniform(4, 8, 70)], axis=1)
    seen = {0: 40, 1: 0, 2: 30, 3: 64, 4: 70}                    # frame f sees the first seen[f] scene points ...
    perm = {f: rng.permutation(n) for f, n in seen.items()}      # ... as keypoint perm[f][point]
    xy = {}
    for f, n in seen.items():
        xy[f] = np.zeros((n, 2))
        xy[f][perm[f]] = _project(X[:n], f)
    line0 = np.array([[10 + 3 * i, 20 + 5 * i] for i in range(12)], dtype=np.float64)   # frame 0: keypoints 40 .. 51
    line2 = np.array([[600 - 7 * i, 15 + 2 * i] for i in range(4)], dtype=np.float64)   # frame 2: keypoints 30 .. 33
    xy[0], xy[2] = np.concatenate([xy[0], line0]), np.concatenate([xy[2], line2])

    def scene(f1, f2, points):
        return f1, f2, perm[f1][points].astype(np.uint32), perm[f2][points].astype(np.uint32)

    pair_list = [
        scene(0, 2, rng.choice(30, 6, replace=False)),
        scene(2, 0, rng.choice(30, 5, replace=False)),
        (0, 3, np.zeros(0, np.uint32), np.zeros(0, np.uint32)),
        scene(3, 4, rng.permutation(64)),
        scene(3, 4, rng.choice(64, 4, replace=False)),
        scene(4, 0, rng.choice(40, 3, replace=False)),
        (0, 3, np.arange(40, 52, dtype=np.uint32), perm[3][rng.choice(64, 12, replace=False)].astype(np.uint32)),
        (2, 4, np.concatenate([np.arange(30, 34), perm[2][[3, 9, 17, 21]]]).astype(np.uint32)[[0, 4, 1, 5, 2, 6, 3, 7]],
         perm[4][[50, 3, 51, 9, 52, 17, 53, 21]].astype(np.uint32)),
        scene(0, 4, rng.choice(40, 30, replace=False)),
    ]
    g = _graph([len(xy[f]) for f in range(5)], pair_list, gap=3)
    g["xy"] = np.concatenate([xy[f] for f in range(5)])
    g["seeds"] = np.array([12345, 7, 0, 2 ** 63 + 5, 99, 1, 2, 3, 2 ** 40], dtype=np.uint64)
    assert np.array_equal(g["xy"], np.rint(g["xy"]))
    return g


@functools.lru_cache(maxsize=None)
def large():
    """One pair of 16 400 matches between two frames of 16 400 keypoints: above SC_MAX_LDS = 16 384, the scorer keeps its keys in
    error rows — a choice eacham_graph_verify makes from the counts the graph keeps."""
    n = 16400
    rng = np.random.default_rng(3)
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)], axis=1)
    perm = rng.permutation(n)
    xy0 = np.zeros((n, 2))
    xy0[perm] = _project(X, 0)
    g = _graph([n, n], [(0, 1, perm.astype(np.uint32), np.arange(n, dtype=np.uint32))], gap=0)
    g["xy"] = np.concatenate([xy0, _project(X, 2)])
    g["seeds"] = np.array([5], dtype=np.uint64)
    return g


@functools.lru_cache(maxsize=None)
def eight():
    """8 seeded pairs of 300 matches over 4 frames of 400 keypoints: a scene in integer pixels, a fifth of every pair's matches wrong.
    What a verification is for: models are found, the masks cut the wrong matches, the tracks differ with and without them."""
    rng = np.random.default_rng(23)
    n = 400
    X = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)], axis=1)
    perm = [rng.permutation(n) for _ in range(4)]
    xy = []
    for f in range(4):
        a = np.zeros((n, 2))
        a[perm[f]] = _project(X, f)
        xy.append(a)
    pair_list = []
    for f1, f2 in [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (2, 0), (3, 1)]:
        pts = rng.choice(n, 300, replace=False)
        other = pts.copy()
        wrong = rng.choice(300, 60, replace=False)
        other[wrong] = rng.permutation(np.setdiff1d(np.arange(n), pts))[:60]      # a point the pair does not otherwise match
        pair_list.append((f1, f2, perm[f1][pts].astype(np.uint32), perm[f2][other].astype(np.uint32)))
    g = _graph([n] * 4, pair_list, gap=5)
    g["xy"] = np.concatenate(xy)
    g["seeds"] = np.arange(100, 108, dtype=np.uint64)
    return g


def kp_offsets(g):
    kpo = np.zeros(g["n_frames"] + 1, dtype=np.int64)
    kpo[1:] = np.cumsum(g["n_kp"])
    return kpo


def gather(g):
    """The host's walk over the matches: per caller pair (uv1, uv2), n x 2 float64 each."""
    kpo, out = kp_offsets(g), []
    for p, (f1, f2) in enumerate(g["pairs"]):
        s = slice(int(g["offsets"][p]), int(g["offsets"][p] + g["counts"][p]))
        out.append((g["xy"][kpo[f1] + g["q"][s].astype(np.int64)].reshape(-1, 2), g["xy"][kpo[f2] + g["t"][s].astype(np.int64)].reshape(-1, 2)))
    return out


# ---- the project's own sample streams, compiled for the host -------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def samples_exe(include_dir=None):
    """tests/cpp/graph_verify_driver.cpp with -DGRAPH_VERIFY_HOST_ONLY: lmeds_samples of include/eacham/TwoViewHip.hpp on stdin's pairs.
    include_dir: another copy of the headers (the recorded streams were made with the parent commit's)."""
    out = os.path.join(tempfile.mkdtemp(prefix="gv_samples_"), "graph_verify_samples")
    subprocess.run(["g++", "-O1", "-std=c++17", "-DGRAPH_VERIFY_HOST_ONLY", "-I", include_dir or os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "graph_verify_driver.cpp"), "-o", out], check=True, capture_output=True)
    return out


def host_samples(points, m, check, sampling, iterations, seeds, exe=None):
    """lmeds_samples(n, m, iterations, check, uv1, uv2, seed, sampling) per pair of `points` ((uv1, uv2) as gather() returns them).
    A pair with fewer than m points draws nothing (as lmeds() returns at once). Returns one [s, m] int32 array per pair."""
    lines = [f"{m} {int(check)} {0 if sampling == 'opencv' else 1} {iterations} {len(points)}"]
    for (a, b), seed in zip(points, seeds):
        lines.append(f"{len(a)} {int(seed)}")
        lines += [f"{x1!r} {y1!r} {x2!r} {y2!r}" for (x1, y1), (x2, y2) in zip(a.tolist(), b.tolist())]
    r = subprocess.run([exe or samples_exe()], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    tok = np.array(r.stdout.split(), dtype=np.int64)
    out, at = [], 0
    for _ in points:
        s = int(tok[at])
        out.append(tok[at + 1:at + 1 + s * m].astype(np.int32).reshape(s, m))
        at += 1 + s * m
    assert at == len(tok)
    return out


def fixed_stride(samples, iterations, m):
    """The `samples` / `n_samples` outputs of eacham_graph_verify from per-pair sample lists."""
    out = np.full((len(samples), iterations, m), -1, dtype=np.int32)
    for p, s in enumerate(samples):
        out[p, :len(s)] = s
    return out, np.array([len(s) for s in samples], dtype=np.int32)


# ---- an independent statement of the OpenCV stream without a checkSubset (tests/test_cv_sampling.py states the generator the same way)

class PyRNG:
    def __init__(self, state=0xFFFFFFFFFFFFFFFF):
        self.state = state

    def uniform(self, n):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return (self.state & 0xFFFFFFFF) % n


def py_subsets(n, m, count):
    """`count` getSubset calls on one stream; returns the subsets and how many draws the duplicate rejection threw away."""
    rng, out, rejected = PyRNG(), [], 0
    for _ in range(count):
        sub = []
        while len(sub) < m:
            v = rng.uniform(n)
            if v in sub:
                rejected += 1
            else:
                sub.append(v)
        out.append(sub)
    return np.array(out, dtype=np.int32).reshape(count, m), rejected
