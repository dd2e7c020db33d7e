"""numpy front-end of the CPU reference of the dot-product matcher (tests/cpp/dot_reference.c). Test infrastructure only.

The C file is compiled with the host compiler into a temporary directory (keyed by its content, so a stale build is never
loaded); the return shapes follow HipContext.match_pairs_directed_dot / match_all_pairs_dot."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "cpp", "dot_reference.c")
_FLAGS = ["-O2", "-march=native", "-fopenmp", "-fPIC", "-std=c11", "-Wall", "-Wextra", "-fno-fast-math", "-ffp-contract=off"]
_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        cpu = b""
        try:  # -march=native: the build belongs to this CPU
            with open("/proc/cpuinfo", "rb") as f:
                cpu = next((line for line in f if line.startswith(b"flags")), b"")
        except OSError:
            pass
        with open(_SRC, "rb") as f:
            key = hashlib.sha1(f.read() + " ".join(_FLAGS).encode() + cpu).hexdigest()[:12]
        d = os.path.join(tempfile.gettempdir(), f"eacham_dotref_{os.getuid()}")
        os.makedirs(d, exist_ok=True)
        so = os.path.join(d, f"libdotref-{key}.so")
        if not os.path.exists(so):
            tmp = so + f".{os.getpid()}.tmp"
            r = subprocess.run([os.environ.get("CC", "gcc"), *_FLAGS, "-shared", "-o", tmp, _SRC, "-lm"], capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("dot reference build failed:\n" + r.stdout + r.stderr)
            os.replace(tmp, so)
        _LIB = C.CDLL(so)
        _LIB.dotref_match_directed.restype = C.c_int
        _LIB.dotref_match_mutual.restype = C.c_int
        _LIB.dotref_argmax.restype = None
    return _LIB


def _f32(a, dim=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2:
        a = a.reshape(0, dim or 0)
    return a


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _dim(A, B):
    return A.shape[1] if A.shape[1] else B.shape[1]


def argmax(A, B):
    """(best, score): per row of A the index of its most similar row of B (-1: none) and that similarity."""
    A, B = _f32(A), _f32(B)
    n1 = A.shape[0]
    best = np.full(max(n1, 1), -1, np.int32)
    score = np.full(max(n1, 1), -np.inf, np.float32)
    lib().dotref_argmax(_vp(A), n1, _vp(B), B.shape[0], _dim(A, B), _vp(best), _vp(score))
    return best[:n1], score[:n1]


def match_directed(A, B, min_score):
    """(q, t, score) of the directed match A -> B, sorted by q."""
    A, B = _f32(A), _f32(B)
    n1 = A.shape[0]
    q = np.empty(max(n1, 1), np.uint32)
    t = np.empty(max(n1, 1), np.uint32)
    s = np.empty(max(n1, 1), np.float32)
    cnt = lib().dotref_match_directed(_vp(A), n1, _vp(B), B.shape[0], _dim(A, B), C.c_float(min_score), _vp(q), _vp(t), _vp(s))
    return q[:cnt].copy(), t[:cnt].copy(), s[:cnt].copy()


def match_mutual(A, B, min_score, min_dir, min_mutual):
    """(q, t, score, stats): the pair's emitted matches (empty unless it is an edge) and {|m12|, |m21|, |mutual|, edge}."""
    A, B = _f32(A), _f32(B)
    n1 = A.shape[0]
    q = np.empty(max(n1, 1), np.uint32)
    t = np.empty(max(n1, 1), np.uint32)
    s = np.empty(max(n1, 1), np.float32)
    stats = np.zeros(4, np.int32)
    cnt = lib().dotref_match_mutual(_vp(A), n1, _vp(B), B.shape[0], _dim(A, B), C.c_float(min_score), int(min_dir), int(min_mutual),
                                    _vp(q), _vp(t), _vp(s), _vp(stats))
    return q[:cnt].copy(), t[:cnt].copy(), s[:cnt].copy(), stats


def _csr(per_pair):
    counts = np.array([len(r[0]) for r in per_pair], np.int32)
    offsets = np.zeros(len(per_pair) + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    cat = lambda k, dt: np.concatenate([r[k] for r in per_pair]).astype(dt) if per_pair else np.zeros(0, dt)  # noqa: E731
    return counts, offsets, cat(0, np.uint32), cat(1, np.uint32), cat(2, np.float32)


def match_pairs_directed(descs, ordered_pairs, min_score):
    """(counts, offsets, q, t, scores): CSR over the ordered pairs."""
    pairs = np.asarray(ordered_pairs, np.int32).reshape(-1, 2)
    return _csr([match_directed(descs[a], descs[b], min_score) for a, b in pairs])


def match_all_pairs(descs, pairs, min_score, min_dir, min_mutual):
    """(counts, offsets, q, t, scores, stats): CSR over the pairs in the form of eacham_match_all_pairs_dot."""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    res = [match_mutual(descs[a], descs[b], min_score, min_dir, min_mutual) for a, b in pairs]
    stats = np.array([r[3] for r in res], np.int32).reshape(-1, 4)
    return (*_csr(res), stats)
