"""numpy front-end of the CPU reference of the fundamental-matrix kind (tests/cpp/fundamental_reference.c). Test infrastructure only.

The C file is compiled with the host compiler into a temporary directory (keyed by its content, so a stale build is never loaded),
with -ffp-contract=off and no fast-math: every product and sum is rounded on its own, as the kernels round them. The return shapes
follow eacham_amd.score.solve_minimal / score_hypotheses and one problem of eacham_amd.lmeds.lmeds_batch."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "cpp", "fundamental_reference.c")
_FLAGS = ["-O2", "-fPIC", "-std=c11", "-Wall", "-Wextra", "-fno-fast-math", "-ffp-contract=off"]
_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        with open(_SRC, "rb") as f:
            key = hashlib.sha1(f.read() + " ".join(_FLAGS).encode()).hexdigest()[:12]
        d = os.path.join(tempfile.gettempdir(), f"eacham_fundref_{os.getuid()}")
        os.makedirs(d, exist_ok=True)
        so = os.path.join(d, f"libfundref-{key}.so")
        if not os.path.exists(so):
            tmp = so + f".{os.getpid()}.tmp"
            r = subprocess.run([os.environ.get("CC", "gcc"), *_FLAGS, "-shared", "-o", tmp, _SRC, "-lm"], capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("fundamental reference build failed:\n" + r.stdout + r.stderr)
            os.replace(tmp, so)
        _LIB = C.CDLL(so)
        for name in ("fref_solve_minimal", "fref_score", "fref_lmeds"):
            getattr(_LIB, name).restype = None
    return _LIB


def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _points(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 2)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1, 2)
    if a.shape != b.shape:
        raise ValueError("point lists disagree")
    return a, b


def solve_minimal(a, b, samples, want_cubic: bool = False):
    """(models [s, 3, 9], n_models [s]) [, cubic [s, 4] = run7Point's c[0] z^3 + .. + c[3], roots [s, 3] ascending]."""
    a, b = _points(a, b)
    idx = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 7)
    if idx.size and (idx.min() < 0 or idx.max() >= len(a)):
        raise ValueError("sample index outside the points")
    s = idx.shape[0]
    models = np.zeros((s, 3, 9), np.float64)
    counts = np.zeros(s, np.int32)
    cubic = np.zeros((s, 4), np.float64) if want_cubic else None
    roots = np.zeros((s, 3), np.float64) if want_cubic else None
    lib().fref_solve_minimal(_vp(a), _vp(b), s, _vp(idx), _vp(models), _vp(counts), _vp(cubic), _vp(roots))
    return (models, counts, cubic, roots) if want_cubic else (models, counts)


def score_hypotheses(a, b, models, threshold: float = 0.0):
    """(errors [nm, n] float32, inlier counts [nm] int32, medians [nm] float32)."""
    a, b = _points(a, b)
    models = np.ascontiguousarray(models, dtype=np.float64).reshape(-1, 9)
    n, nm = len(a), len(models)
    err = np.zeros((nm, n), np.float32)
    cnt = np.zeros(nm, np.int32)
    med = np.zeros(nm, np.float32)
    lib().fref_score(n, _vp(a), _vp(b), nm, _vp(models), C.c_float(threshold), _vp(err), _vp(cnt), _vp(med))
    return err, cnt, med


def lmeds(a, b, samples):
    """One problem of eacham_lmeds_batch, kind fundamental: dict(model, median, threshold, inliers, mask, winner, candidates)."""
    a, b = _points(a, b)
    idx = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 7)
    n = len(a)
    if n >= 7 and idx.size and (idx.min() < 0 or idx.max() >= n):
        raise ValueError("sample index outside the points")
    model = np.zeros(9, np.float64)
    med, thr = np.zeros(1, np.float32), np.zeros(1, np.float32)
    inl, nc = np.zeros(1, np.int32), np.zeros(1, np.int32)
    win = np.zeros(3, np.int32)
    mask = np.zeros(max(n, 1), np.uint8)
    lib().fref_lmeds(n, _vp(a), _vp(b), idx.shape[0], _vp(idx), _vp(model), _vp(med), _vp(thr), _vp(inl), _vp(mask), _vp(win), _vp(nc))
    return {"model": model, "median": med[0], "threshold": thr[0], "inliers": int(inl[0]), "mask": mask[:n].copy(),
            "winner": tuple(int(x) for x in win), "candidates": int(nc[0])}
