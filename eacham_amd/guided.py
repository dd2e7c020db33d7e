"""Host-side mirror of guided matching (include/eacham_hip.h: eacham_match_guided / eacham_graph_match_guided).

  match_guided(ctx, kind, pairs, models, keypoints, max_error, ...)   the list form on the context's resident int8 frames
  ResidentGraph.match_guided(kind, models, max_error, ...)            the resident form: pairs and keypoints are the graph's

Both return GuidedMatches: the CSR match graph over the caller's pairs, sorted by q — what ResidentGraph(...) and
build_tracks(...) take — with the squared descriptor distances and the per-pair {|m12|, |m21|, |result|}.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import capi
from .matcher import RATIO

KINDS = {"essential": capi.SCORE_ESSENTIAL, "homography": capi.SCORE_HOMOGRAPHY, "fundamental": capi.SCORE_FUNDAMENTAL}


class GuidedMatches(NamedTuple):
    counts: np.ndarray    # [npairs] int32
    offsets: np.ndarray   # [npairs + 1] int64
    q: np.ndarray         # [total] uint32, rows of pairs[p][0]
    t: np.ndarray         # [total] uint32, rows of pairs[p][1]
    d2: np.ndarray        # [total] uint32 squared L2 of the descriptors
    stats: np.ndarray     # [npairs, 3] int32: |m12|, |m21| (0 without the cross-check), |result|


def pack_keypoints(keypoints):
    """A list of per-frame [n_f, 2] arrays -> (kp_offsets [n_frames + 1] int64, xy [total, 2] float64); a (kp_offsets, xy) tuple of
    arrays in that layout is passed through."""
    if isinstance(keypoints, tuple) and len(keypoints) == 2 and np.ndim(keypoints[0]) == 1 and np.ndim(keypoints[1]) == 2:
        return np.ascontiguousarray(keypoints[0], dtype=np.int64), np.ascontiguousarray(keypoints[1], dtype=np.float64).reshape(-1, 2)
    per = [np.asarray(a, dtype=np.float64).reshape(-1, 2) for a in keypoints]
    kpo = np.zeros(len(per) + 1, dtype=np.int64)
    kpo[1:] = np.cumsum([len(a) for a in per])
    xy = np.concatenate(per) if per else np.zeros((0, 2))
    return kpo, np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)


def _ptr(a):
    return None if a is None or a.size == 0 else a.ctypes.data


def guided_raw(ctx, kind: int, models, K, max_error: float, ratio: float, max_d2: int, cross_check: int, npairs: int, cap: int,
               pairs=None, kpo=None, xy=None, graph=None, preset: int = 0):
    """The call itself on integer codes, nothing checked here (the library's own checks answer): the list form, or with `graph`
    (a graph handle) the resident form. Returns (rc, total, GuidedMatches over the whole buffers); every output is filled with
    the byte `preset` beforehand (tests of the error paths)."""
    L = ctx._L
    P = max(int(npairs), 0)

    def filled(shape, dtype):   # every BYTE is `preset`
        return np.full(np.prod(shape, dtype=np.int64) * np.dtype(dtype).itemsize, preset, dtype=np.uint8).view(dtype).reshape(shape)

    counts, offsets = filled(P, np.int32), filled(P + 1, np.int64)
    q, t, d2 = (filled(max(int(cap), 0), np.uint32) for _ in range(3))
    stats = filled((P, 3), np.int32)
    total = C.c_int64(preset)
    m = None if models is None else np.ascontiguousarray(models, dtype=np.float64).reshape(-1, 9)
    K4 = None if K is None else np.ascontiguousarray(K, dtype=np.float64).reshape(4)
    out = (counts.ctypes.data if P else None, offsets.ctypes.data, _ptr(q), _ptr(t), _ptr(d2), int(cap), C.byref(total), _ptr(stats))
    if graph is not None:
        rc = L.eacham_graph_match_guided(graph, int(kind), _ptr(m), _ptr(K4), float(max_error), float(ratio), int(max_d2), int(cross_check), *out)
    else:
        pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        rc = L.eacham_match_guided(ctx.handle, int(kind), _ptr(pr), int(npairs), _ptr(m), _ptr(K4), None if kpo is None else kpo.ctypes.data, _ptr(xy),
                                   float(max_error), float(ratio), int(max_d2), int(cross_check), *out)
    return rc, int(total.value), GuidedMatches(counts, offsets, q, t, d2, stats)


def _trim(ctx, rc, total, g: GuidedMatches) -> GuidedMatches:
    ctx._check(rc)
    return GuidedMatches(g.counts, g.offsets, g.q[:total].copy(), g.t[:total].copy(), g.d2[:total].copy(), g.stats)


def match_guided(ctx, kind: str, pairs, models, keypoints, max_error: float, ratio: float = RATIO, max_d2: int = 0,
                 cross_check: bool = True, K=None, cap: int | None = None) -> GuidedMatches:
    """eacham_match_guided. kind: "essential" (K = fx fy cx cy, or None for normalised points), "homography" or "fundamental";
    models [npairs, 9]; keypoints: per-frame [n_f, 2] arrays indexed by frame id, or (kp_offsets, xy); max_error in the error's
    own unit (squared pixels for H and F; inf = no gate). cap defaults to the sum of the query frames' rows, which always suffices."""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    kpo, xy = pack_keypoints(keypoints)
    if cap is None:
        cap = int(sum(int(kpo[f + 1] - kpo[f]) for f in pairs[:, 0])) if len(pairs) else 0
    return _trim(ctx, *guided_raw(ctx, KINDS[kind], models, K, max_error, ratio, max_d2, int(bool(cross_check)), len(pairs), cap,
                                  pairs=pairs, kpo=kpo, xy=xy))


def graph_match_guided(ctx, graph_handle, npairs: int, cap: int, kind: str, models, max_error: float, ratio: float = RATIO, max_d2: int = 0,
                       cross_check: bool = True, K=None) -> GuidedMatches:
    """eacham_graph_match_guided on a graph handle (ResidentGraph.match_guided)."""
    return _trim(ctx, *guided_raw(ctx, KINDS[kind], models, K, max_error, ratio, max_d2, int(bool(cross_check)), npairs, cap, graph=graph_handle))
