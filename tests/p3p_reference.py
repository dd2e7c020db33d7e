"""numpy front-end of the CPU restatement of the P3P solver (tests/cpp/p3p_reference.c). Test infrastructure only.

The C file is compiled with the host compiler into a temporary directory (keyed by its content, so a stale build is never loaded),
with -ffp-contract=off and no fast-math: every product and sum is rounded on its own, as the kernels round them. The return shapes
follow eacham_amd.pnp.solve_p3p and eacham_amd.score.score_hypotheses; `hypotheses` and `refit` are the two hooks of
eacham_amd.pnp.pnp_ransac_batch driven by the restatement (the refit is EPnP: the CPU oracle's)."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "cpp", "p3p_reference.c")
_FLAGS = ["-O2", "-fPIC", "-std=c11", "-Wall", "-Wextra", "-fno-fast-math", "-ffp-contract=off"]
_LIB = None
M = 4


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        with open(_SRC, "rb") as f:
            key = hashlib.sha1(f.read() + " ".join(_FLAGS).encode()).hexdigest()[:12]
        d = os.path.join(tempfile.gettempdir(), f"eacham_p3pref_{os.getuid()}")
        os.makedirs(d, exist_ok=True)
        so = os.path.join(d, f"libp3pref-{key}.so")
        if not os.path.exists(so):
            tmp = so + f".{os.getpid()}.tmp"
            r = subprocess.run([os.environ.get("CC", "gcc"), *_FLAGS, "-shared", "-o", tmp, _SRC, "-lm"], capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("P3P reference build failed:\n" + r.stdout + r.stderr)
            os.replace(tmp, so)
        _LIB = C.CDLL(so)
        for name in ("p3pref_solve", "p3pref_score"):
            getattr(_LIB, name).restype = None
    return _LIB


def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _K4(K):
    K = np.asarray(K, dtype=np.float64)
    return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]) if K.shape == (3, 3) else np.ascontiguousarray(K).reshape(4)


def _points(X, uv):
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
    uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    if len(X) != len(uv):
        raise ValueError("point lists disagree")
    return X, uv


def solve_p3p(X, uv, K, samples, want_quartic: bool = False):
    """(models [s, 12], n_models [s], candidates [s, 4, 12], n_candidates [s]) [, quartic [s, 5] = A0..A4, roots [s, 4], n_roots [s]]."""
    X, uv = _points(X, uv)
    idx = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, M)
    if idx.size and (idx.min() < 0 or idx.max() >= len(X)):
        raise ValueError("sample index outside the points")
    s = idx.shape[0]
    models, nm = np.zeros((s, 12)), np.zeros(s, np.int32)
    cand, nc = np.zeros((s, 4, 12)), np.zeros(s, np.int32)
    quartic = np.zeros((s, 5)) if want_quartic else None
    roots = np.zeros((s, 4)) if want_quartic else None
    nr = np.zeros(s, np.int32) if want_quartic else None
    lib().p3pref_solve(_vp(X), _vp(uv), _vp(_K4(K)), s, _vp(idx), _vp(models), _vp(nm), _vp(cand), _vp(nc), _vp(quartic), _vp(roots), _vp(nr))
    return (models, nm, cand, nc, quartic, roots, nr) if want_quartic else (models, nm, cand, nc)


def score(X, uv, models, K, threshold: float = 0.0):
    """(errors [nm, n] float32, inlier counts [nm] int32) of eacham_score_hypotheses(kind PNP)."""
    X, uv = _points(X, uv)
    models = np.ascontiguousarray(models, dtype=np.float64).reshape(-1, 12)
    err, cnt = np.zeros((len(models), len(X)), np.float32), np.zeros(len(models), np.int32)
    lib().p3pref_score(len(X), _vp(X), _vp(uv), _vp(_K4(K)), len(models), _vp(models), C.c_float(threshold), _vp(err), _vp(cnt))
    return err, cnt


def compose_hypotheses(solve, count, X, uv, K, samples, thr):
    """Per problem (models [s, 12], n_models [s], counts [s]): solve(X, uv, K, rows) -> (models, n_models, ...) on the problem's rows,
    count(X, uv, models, K, thr) -> inlier counts; a problem with fewer than 4 points is not looked at."""
    out = []
    for x, u, rows in zip(X, uv, samples):
        rows = np.asarray(rows, np.int32).reshape(-1, M)
        s = len(rows)
        if s == 0 or len(u) < M:
            out.append((np.zeros((s, 12)), np.zeros(s, np.int32), np.zeros(s, np.int32)))
            continue
        r = solve(x, u, K, rows)
        models, ok = r[0], r[1]
        cnt = count(x, u, models, K, thr)
        out.append((models, ok, np.where(ok != 0, cnt, 0).astype(np.int32)))
    return out


def hypotheses(X, uv, K, rows, thr, want_models=True):
    """The `hypotheses=` hook of pnp_ransac_batch(solver="p3p") on the restatement."""
    from eacham_amd import pnp
    recs = compose_hypotheses(solve_p3p, lambda x, u, m, k, t: score(x, u, m, k, t)[1], X, uv, K, rows, thr)
    return pnp.PnpHypotheses([r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs], None, None)


def refit(X, uv, K, models, has_model, thr):
    """The `refit=` hook: the mask of the restatement's scorer, then the CPU oracle's EPnP on the inliers (5 or more)."""
    from eacham_amd import pnp
    import oracle_api as O
    masks, ni, out, ok = [], [], [], []
    for p, (x, u) in enumerate(zip(X, uv)):
        mask, r, rok = np.zeros(len(u), np.uint8), np.zeros(12), 0
        if has_model[p]:
            err, _ = score(x, u, models[p], K, thr)
            mask = (err[0] <= np.float32(thr)).astype(np.uint8)
            rows = np.nonzero(mask)[0].astype(np.int32)
            if len(rows) >= 5:
                m, k = O.solve_pnp(x, u, K, rows[None])
                r, rok = (m[0], 1) if k[0] else (r, 0)
        masks.append(mask), ni.append(int(mask.sum())), out.append(r), ok.append(rok)
    return pnp.PnpRefit(masks, np.array(ni, np.int32), np.array(out).reshape(-1, 12), np.array(ok, np.int32), None)
