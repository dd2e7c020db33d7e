"""Host-side mirror of eacham_lmeds_batch (include/eacham_hip.h): cv::findEssentialMat(LMEDS) / cv::findHomography(LMEDS) — the
robust stage of RecoverPoseTwoView (modules/sfm/reconstruction/ReconstructionManager.cpp:57-61, :75) — for a whole list of
pairs in one call: every minimal sample solved, every candidate's median taken, the first smallest kept, the points classified
against sigma^2, with no host turn in between. Test / bench driver."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import capi
from .score import SOLVERS

KINDS = {"homography": "homography4", "essential": "essential5", "fundamental": "fundamental7",
         "homography4": "homography4", "essential5": "essential5", "fundamental7": "fundamental7"}


class LmedsBatch(NamedTuple):
    models: np.ndarray        # [P, 9] float64: the winning model as solved (zeros: none)
    medians: np.ndarray       # [P] float32 (NaN: none)
    thresholds: np.ndarray    # [P] float32: (float)(sigma * sigma)
    inliers: np.ndarray       # [P] int32
    masks: list               # P arrays of uint8, one byte per point of the problem
    winner: np.ndarray        # [P, 3] int32: candidate, sample, root (-1 -1 -1: none)
    n_candidates: np.ndarray  # [P] int32
    point_ptr: np.ndarray     # [P + 1] int64
    sample_ptr: np.ndarray    # [P + 1] int64


def pack(kind: str, uv1, uv2, samples):
    """The wire form of a list of problems: (point_ptr, a, b, sample_ptr, sample_idx). uv1[p] / uv2[p]: n_p x 2 points,
    samples[p]: s_p x m indices into them."""
    _, m, _ = SOLVERS[KINDS[kind]]
    if not (len(uv1) == len(uv2) == len(samples)):
        raise ValueError("one entry per problem in uv1, uv2 and samples")
    A = [np.asarray(x, dtype=np.float64).reshape(-1, 2) for x in uv1]
    B = [np.asarray(x, dtype=np.float64).reshape(-1, 2) for x in uv2]
    I = [np.asarray(x, dtype=np.int32).reshape(-1, m) for x in samples]
    if any(len(x) != len(y) for x, y in zip(A, B)):
        raise ValueError("point lists disagree")
    point_ptr = np.zeros(len(A) + 1, dtype=np.int64)
    sample_ptr = np.zeros(len(A) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in A], out=point_ptr[1:])
    np.cumsum([len(x) for x in I], out=sample_ptr[1:])
    cat = lambda xs, shape, dt: np.ascontiguousarray(np.concatenate(xs)) if xs else np.zeros(shape, dt)   # noqa: E731
    return point_ptr, cat(A, (0, 2), np.float64), cat(B, (0, 2), np.float64), sample_ptr, cat(I, (0, m), np.int32)


def lmeds_batch_raw(ctx, kind: str, point_ptr, a, b, sample_ptr, sample_idx, K=None):
    """eacham_lmeds_batch on arrays already in its wire form (nothing is checked here: the library's own checks answer)."""
    k, _, _ = SOLVERS[KINDS[kind]]
    return _call(ctx, k, point_ptr, a, b, sample_ptr, sample_idx, K)


def _call(ctx, k, point_ptr, a, b, sample_ptr, sample_idx, K):
    point_ptr = np.ascontiguousarray(point_ptr, dtype=np.int64)
    sample_ptr = np.ascontiguousarray(sample_ptr, dtype=np.int64)
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    sample_idx = np.ascontiguousarray(sample_idx, dtype=np.int32)
    K4 = None if K is None else np.ascontiguousarray(K, dtype=np.float64).reshape(4)
    P = len(point_ptr) - 1
    npts = max(int(point_ptr[-1]), 0) if P >= 0 and len(point_ptr) else 0
    models = np.zeros((max(P, 0), 9), dtype=np.float64)
    med = np.zeros(max(P, 0), dtype=np.float32)
    thr = np.zeros(max(P, 0), dtype=np.float32)
    inl = np.zeros(max(P, 0), dtype=np.int32)
    masks = np.zeros(npts, dtype=np.uint8)
    win = np.zeros((max(P, 0), 3), dtype=np.int32)
    nc = np.zeros(max(P, 0), dtype=np.int32)
    vp = C.c_void_p
    ctx._check(capi.lib().eacham_lmeds_batch(
        ctx.handle, k, P, vp(point_ptr.ctypes.data), vp(a.ctypes.data), vp(b.ctypes.data), vp(K4.ctypes.data) if K4 is not None else None,
        vp(sample_ptr.ctypes.data), vp(sample_idx.ctypes.data), vp(models.ctypes.data), vp(med.ctypes.data), vp(thr.ctypes.data),
        vp(inl.ctypes.data), vp(masks.ctypes.data), vp(win.ctypes.data), vp(nc.ctypes.data)))
    split = [masks[int(point_ptr[p]):int(point_ptr[p + 1])] for p in range(P)]
    return LmedsBatch(models, med, thr, inl, split, win, nc, point_ptr, sample_ptr)


def lmeds_batch(ctx, kind: str, uv1, uv2, samples, K=None) -> LmedsBatch:
    """kind "essential" (5-point samples, K = fx fy cx cy or None for normalised points), "homography" (4-point samples) or
    "fundamental" (7-point samples on pixels, K ignored).
    uv1[p], uv2[p]: the n_p x 2 matches of pair p; samples[p]: its s_p x m minimal samples (indices into its own matches)."""
    k, _, _ = SOLVERS[KINDS[kind]]
    point_ptr, a, b, sample_ptr, idx = pack(kind, uv1, uv2, samples)
    return _call(ctx, k, point_ptr, a, b, sample_ptr, idx, K)
