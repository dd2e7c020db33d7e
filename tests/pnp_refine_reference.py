"""numpy front-end of the CPU restatement of eacham_pnp_refine_batch (tests/cpp/pnp_refine_reference.c). Test infrastructure only.

The C file is compiled with the host compiler into a temporary directory (keyed by its content, so a stale build is never loaded),
with -ffp-contract=off and no fast-math: every product and sum is rounded on its own, as the kernel rounds them. refine_batch returns
the tuple eacham_amd.pnp.pnp_refine_batch returns (plus, when asked for, the per-try trace); write_cases / build_program serve the
stand-alone program the sanitizer test runs."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import struct
import subprocess
import tempfile

import numpy as np

from eacham_amd import pnp

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "cpp", "pnp_refine_reference.c")
FLAGS = ["-O2", "-fPIC", "-std=c11", "-Wall", "-Wextra", "-fno-fast-math", "-ffp-contract=off"]
_LIB = None
CONVERGED, CAP, NOT_REFINED = 0, 1, 2


def _dir():
    d = os.path.join(tempfile.gettempdir(), f"eacham_pnprefineref_{os.getuid()}")
    os.makedirs(d, exist_ok=True)
    return d


def _key(flags):
    with open(SRC, "rb") as f:
        return hashlib.sha1(f.read() + " ".join(flags).encode()).hexdigest()[:12]


def _compile(flags, out):
    if not os.path.exists(out):
        tmp = out + f".{os.getpid()}.tmp"
        r = subprocess.run([os.environ.get("CC", "gcc"), *flags, "-o", tmp, SRC], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("PnP refine reference build failed:\n" + r.stdout + r.stderr)
        os.replace(tmp, out)
    return out


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(_compile([*FLAGS, "-shared"], os.path.join(_dir(), f"libpnprefineref-{_key(FLAGS)}.so")))
        for name in ("pnprefine_batch", "pnprefine_jacobian"):
            getattr(_LIB, name).restype = None
    return _LIB


def build_program(extra=()):
    """The restatement as a program of its own (its main reads a case file), built with `extra` flags on top of the library's."""
    flags = [f for f in FLAGS if f != "-fPIC"] + ["-DPNP_REFINE_MAIN", *extra]
    return _compile(flags, os.path.join(_dir(), f"pnp_refine_reference-{_key(flags)}"))


_vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731


def _wire(X, uv, K, poses, has_pose, use_masks):
    point_ptr, A, B = pnp.pack_points(X, uv)
    P = len(point_ptr) - 1
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(P, 12)
    has = np.ascontiguousarray(has_pose, dtype=np.uint8).reshape(P)
    use = None if use_masks is None else pnp._cat([np.asarray(m, np.uint8).reshape(-1) for m in use_masks], (0,), np.uint8)
    if use is not None and len(use) != len(B):
        raise ValueError("one use byte per point")
    return point_ptr, A, B, pnp._K4(K), poses, has, use


def refine_batch(X, uv, K, poses, has_pose, use_masks=None, max_tries: int = 20, threshold: float = 16.0, want_trace: bool = False):
    """PnpRefine of the restatement [, trace [P, max_tries, 3] = candidate cost, accepted (-1: no candidate), lambda of the try]."""
    point_ptr, A, B, K4, poses, has, use = _wire(X, uv, K, poses, has_pose, use_masks)
    P = len(has)
    refined, cost = np.zeros((P, 12)), np.zeros((P, 2))
    tries, status, ni = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
    mask = np.zeros(len(B), np.uint8)
    trace = np.zeros((P, max_tries, 3)) if want_trace else None
    lib().pnprefine_batch(P, _vp(point_ptr), _vp(A), _vp(B), _vp(K4), _vp(poses), _vp(has), _vp(use), int(max_tries), C.c_float(threshold),
                          _vp(refined), _vp(cost), _vp(tries), _vp(status), _vp(mask), _vp(ni), _vp(trace))
    out = pnp.PnpRefine(refined, cost, tries, status, pnp._seg(mask, point_ptr), ni, point_ptr)
    return (out, trace) if want_trace else out


def jacobian(X, uv, M, K):
    """(J [2, 6], r [2]) of one correspondence under the pose M, as the restatement's loop forms them."""
    J, r = np.zeros((2, 6)), np.zeros(2)
    lib().pnprefine_jacobian(_vp(np.ascontiguousarray(X, dtype=np.float64)), _vp(np.ascontiguousarray(uv, dtype=np.float64)),
                             _vp(np.ascontiguousarray(M, dtype=np.float64)), _vp(pnp._K4(K)), _vp(J), _vp(r))
    return J, r


def write_cases(path, X, uv, K, poses, has_pose, use_masks=None, max_tries: int = 20, threshold: float = 16.0):
    """The case file the stand-alone program reads."""
    point_ptr, A, B, K4, poses, has, use = _wire(X, uv, K, poses, has_pose, use_masks)
    with open(path, "wb") as f:
        f.write(struct.pack("iiif", len(has), max_tries, int(use is not None), threshold))
        for a in (K4, point_ptr, A, B, poses, has) + ((use,) if use is not None else ()):
            f.write(np.ascontiguousarray(a).tobytes())
