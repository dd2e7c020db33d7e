"""Host-side mirror of eacham_two_view_batch (include/eacham_hip.h): the second half of RecoverPoseTwoView
(modules/sfm/reconstruction/ReconstructionManager.cpp:89-180) — candidate relative poses -> the winning one and its kept
3-D points — for a whole list of pairs in one call. Per pair the rule is cv::recoverPose's cheirality vote followed by the
structure of its winner ("poses", the E branch) or the choice among the solutions of cv::decomposeHomographyMat
("solutions", the H branch). Decomposing E / H into the candidates stays with the caller. Test / bench driver."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import capi
from .triangulate import _K4

RULES = {"poses": capi.TWOVIEW_POSES, "solutions": capi.TWOVIEW_SOLUTIONS}


class TwoViewBatch(NamedTuple):
    winner: np.ndarray       # [P] int32: the winning candidate, local to the problem (-1: none)
    good: np.ndarray         # [P] int32: cheirality votes of the winner ("poses"; 0 otherwise)
    kept: np.ndarray         # [P] int32: bytes set in keep
    cand_counts: list        # P arrays of int32, one count per candidate of the problem
    points: list             # P arrays [n_p, 3] float64: the winner's points (zeros: none)
    keep: list               # P arrays of uint8
    pose_mask: list          # P arrays of uint8
    point_ptr: np.ndarray    # [P + 1] int64
    transform_ptr: np.ndarray  # [P + 1] int64


def pack(uv1, uv2, transforms, in_mask=None):
    """The wire form of a list of problems: (point_ptr, uv1, uv2, transform_ptr, transforms, in_mask or None).
    uv1[p] / uv2[p]: n_p x 2 pixels, transforms[p]: nt_p x 16 (or x 4 x 4), in_mask[p]: n_p bytes."""
    if not (len(uv1) == len(uv2) == len(transforms)) or (in_mask is not None and len(in_mask) != len(uv1)):
        raise ValueError("one entry per problem in uv1, uv2, transforms and in_mask")
    A = [np.asarray(x, dtype=np.float64).reshape(-1, 2) for x in uv1]
    B = [np.asarray(x, dtype=np.float64).reshape(-1, 2) for x in uv2]
    T = [np.asarray(x, dtype=np.float64).reshape(-1, 16) for x in transforms]
    if any(len(x) != len(y) for x, y in zip(A, B)):
        raise ValueError("point lists disagree")
    point_ptr = np.zeros(len(A) + 1, dtype=np.int64)
    transform_ptr = np.zeros(len(A) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in A], out=point_ptr[1:])
    np.cumsum([len(x) for x in T], out=transform_ptr[1:])
    cat = lambda xs, shape, dt: np.ascontiguousarray(np.concatenate(xs)) if xs else np.zeros(shape, dt)   # noqa: E731
    M = None
    if in_mask is not None:
        M = [np.asarray(x, dtype=np.uint8).reshape(-1) for x in in_mask]
        if any(len(m) != len(a) for m, a in zip(M, A)):
            raise ValueError("in_mask and point lists disagree")
        M = cat(M, (0,), np.uint8)
    return point_ptr, cat(A, (0, 2), np.float64), cat(B, (0, 2), np.float64), transform_ptr, cat(T, (0, 16), np.float64), M


def two_view_batch_raw(ctx, point_ptr, uv1, uv2, K, rule, transform_ptr, transforms, in_mask, max_repr_error, min_tri_angle,
                       distance_thresh=50.0, min_solution_matches=20, n_problems=None, out=None):
    """eacham_two_view_batch on arrays already in its wire form (nothing is checked here: the library's own checks answer).
    out = (winner, good, kept, cand_counts, points, keep, pose_mask) to write into the caller's arrays."""
    ptr = lambda x: None if x is None else C.c_void_p(x.ctypes.data)   # noqa: E731
    i64 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.int64)   # noqa: E731
    f64 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)   # noqa: E731
    point_ptr, transform_ptr, uv1, uv2, transforms = i64(point_ptr), i64(transform_ptr), f64(uv1), f64(uv2), f64(transforms)
    rule = None if rule is None else np.ascontiguousarray(rule, dtype=np.int32)
    in_mask = None if in_mask is None else np.ascontiguousarray(in_mask, dtype=np.uint8)
    K4 = None if K is None else _K4(K)
    P = (len(point_ptr) - 1 if point_ptr is not None else 0) if n_problems is None else int(n_problems)
    last = lambda t: max(int(t[-1]), 0) if t is not None and len(t) and P > 0 else 0   # noqa: E731
    npts, ncand = last(point_ptr), last(transform_ptr)
    if out is None:
        if npts > 1 << 28 or ncand > 1 << 28:   # (tables the library is about to refuse: nothing that size is allocated for them)
            npts = ncand = 0
        out = (np.zeros(max(P, 0), np.int32), np.zeros(max(P, 0), np.int32), np.zeros(max(P, 0), np.int32), np.zeros(ncand, np.int32),
               np.zeros((npts, 3), np.float64), np.zeros(npts, np.uint8), np.zeros(npts, np.uint8))
    ctx._check(capi.lib().eacham_two_view_batch(
        ctx.handle, P, ptr(point_ptr), ptr(uv1), ptr(uv2), ptr(K4), ptr(rule), ptr(transform_ptr), ptr(transforms), ptr(in_mask),
        float(max_repr_error), float(min_tri_angle), float(distance_thresh), int(min_solution_matches), *[ptr(o) for o in out]))
    winner, good, kept, cc, pts, keep, pm = out
    seg = lambda x, t: [x[int(t[p]):int(t[p + 1])] for p in range(max(P, 0))]   # noqa: E731
    return TwoViewBatch(winner, good, kept, seg(cc, transform_ptr), seg(pts, point_ptr), seg(keep, point_ptr), seg(pm, point_ptr),
                        point_ptr, transform_ptr)


def two_view_batch(ctx, uv1, uv2, K, rules, transforms, max_repr_error: float, min_tri_angle: float, in_mask=None,
                   distance_thresh: float = 50.0, min_solution_matches: int = 20) -> TwoViewBatch:
    """uv1[p], uv2[p]: the n_p x 2 matches of pair p; rules[p]: "poses" | "solutions" (or the C constant); transforms[p]: its
    candidate camera-1 -> camera-2 transforms; K: 3 x 3 or fx fy cx cy, shared; in_mask: None or one byte array per pair."""
    point_ptr, a, b, transform_ptr, T, M = pack(uv1, uv2, transforms, in_mask)
    rule = np.array([RULES.get(r, r) for r in rules], dtype=np.int32)
    if len(rule) != len(point_ptr) - 1:
        raise ValueError("one rule per problem")
    return two_view_batch_raw(ctx, point_ptr, a, b, K, rule, transform_ptr, T, M, max_repr_error, min_tri_angle, distance_thresh,
                              min_solution_matches)
