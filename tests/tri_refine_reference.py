"""numpy front-end of the CPU restatement of eacham_triangulate_refine_tracks (tests/cpp/tri_refine_reference.c). Test infrastructure only.

The C file is compiled with the host compiler into a temporary directory (keyed by its content, so a stale build is never loaded),
with -ffp-contract=off and no fast-math: every product and sum is rounded on its own, as the kernel rounds them. refine_tracks returns
the TrackRefine eacham_amd.triangulate.refine_tracks returns (plus, when asked for, the per-try trace); write_cases / build_program
serve the stand-alone program the sanitizer test runs."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import struct
import subprocess
import tempfile

import numpy as np

from eacham_amd import triangulate as tri

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "cpp", "tri_refine_reference.c")
FLAGS = ["-O2", "-fPIC", "-std=c11", "-Wall", "-Wextra", "-fno-fast-math", "-ffp-contract=off"]
_LIB = None
CONVERGED, CAP, NOT_REFINED = 0, 1, 2


def _dir():
    d = os.path.join(tempfile.gettempdir(), f"eacham_trirefineref_{os.getuid()}")
    os.makedirs(d, exist_ok=True)
    return d


def _key(flags):
    with open(SRC, "rb") as f:
        return hashlib.sha1(f.read() + " ".join(flags).encode()).hexdigest()[:12]


def _compile(flags, out):
    if not os.path.exists(out):
        tmp = out + f".{os.getpid()}.tmp"
        r = subprocess.run([os.environ.get("CC", "gcc"), *flags, "-o", tmp, SRC, "-lm"], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("track refine reference build failed:\n" + r.stdout + r.stderr)
        os.replace(tmp, out)
    return out


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(_compile([*FLAGS, "-shared"], os.path.join(_dir(), f"libtrirefineref-{_key(FLAGS)}.so")))
        for name in ("trirefine_tracks", "trirefine_jacobian"):
            getattr(_LIB, name).restype = None
    return _LIB


def build_program(extra=()):
    """The restatement as a program of its own (its main reads a case file), built with `extra` flags on top of the library's."""
    flags = [f for f in FLAGS if f != "-fPIC"] + ["-DTRI_REFINE_MAIN", *extra]
    return _compile(flags, os.path.join(_dir(), f"tri_refine_reference-{_key(flags)}"))


_vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731


def _wire(transforms, track_ptr, obs_frame, obs_uv, K, points, has_point, use_mask):
    T = np.ascontiguousarray(transforms, dtype=np.float64).reshape(-1, 16)
    tp = np.ascontiguousarray(track_ptr, dtype=np.int64).reshape(-1)
    of = np.ascontiguousarray(obs_frame, dtype=np.uint32).reshape(-1)
    uv = np.ascontiguousarray(obs_uv, dtype=np.float64).reshape(-1, 2)
    n = len(tp) - 1
    P3 = np.ascontiguousarray(points, dtype=np.float64).reshape(n, 3)
    has = np.ascontiguousarray(has_point, dtype=np.uint8).reshape(n)
    use = None if use_mask is None else np.ascontiguousarray(use_mask, dtype=np.uint8).reshape(-1)
    if len(of) != len(uv) or int(tp[-1]) != len(of) or (use is not None and len(use) != len(of)):
        raise ValueError("track_ptr / observation arrays disagree")
    if len(of) and int(of.max()) >= len(T):
        raise ValueError("an observation names a frame that is not there")
    return T, tp, of, uv, tri._K4(K), P3, has, use


def refine_tracks(transforms, track_ptr, obs_frame, obs_uv, K, points, has_point, use_mask=None, max_tries: int = 20,
                  max_repr_error: float = 4.0, want_trace: bool = False):
    """TrackRefine of the restatement [, trace [n, max_tries, 3] = candidate cost, accepted (-1: no candidate), lambda of the try]."""
    T, tp, of, uv, K4, P3, has, use = _wire(transforms, track_ptr, obs_frame, obs_uv, K, points, has_point, use_mask)
    n = len(has)
    refined, cost = np.zeros((n, 3)), np.zeros((n, 2))
    tries, status, ni = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    mask = np.zeros(len(of), np.uint8)
    trace = np.zeros((n, max_tries, 3)) if want_trace else None
    lib().trirefine_tracks(_vp(T), n, _vp(tp), _vp(of), _vp(uv), _vp(K4), _vp(P3), _vp(has), _vp(use), int(max_tries), C.c_float(max_repr_error),
                           _vp(refined), _vp(cost), _vp(tries), _vp(status), _vp(mask), _vp(ni), _vp(trace))
    out = tri.TrackRefine(refined, cost, tries, status, mask, ni)
    return (out, trace) if want_trace else out


def jacobian(T, uv, X, K):
    """(J [2, 3], r [2]) of one observation (T 4 x 4, pixel uv) at the point X, as the restatement's loop forms them."""
    J, r = np.zeros((2, 3)), np.zeros(2)
    lib().trirefine_jacobian(_vp(np.ascontiguousarray(T, dtype=np.float64).reshape(16)), _vp(np.ascontiguousarray(uv, dtype=np.float64)),
                             _vp(np.ascontiguousarray(X, dtype=np.float64)), _vp(tri._K4(K)), _vp(J), _vp(r))
    return J, r


def write_cases(path, transforms, track_ptr, obs_frame, obs_uv, K, points, has_point, use_mask=None, max_tries: int = 20,
                max_repr_error: float = 4.0):
    """The case file the stand-alone program reads."""
    T, tp, of, uv, K4, P3, has, use = _wire(transforms, track_ptr, obs_frame, obs_uv, K, points, has_point, use_mask)
    with open(path, "wb") as f:
        f.write(struct.pack("iiiif", len(has), len(T), max_tries, int(use is not None), max_repr_error))
        for a in (K4, tp, T, of, uv, P3, has) + ((use,) if use is not None else ()):
            f.write(np.ascontiguousarray(a).tobytes())
