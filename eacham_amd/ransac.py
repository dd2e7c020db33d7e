"""Host-side mirror of eacham_ransac_batch (include/eacham_hip.h): cv::findEssentialMat / cv::findHomography /
cv::findFundamentalMat with cv::RANSAC for a whole list of pairs in one call — every candidate's inlier count against a squared
threshold, the most inliers win (the earlier candidate on ties), every record shrinks the sample budget by the confidence, and the
samples behind a problem's budget are not solved. Test / bench driver; the wire form is eacham_amd.lmeds.pack's."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import capi
from .lmeds import KINDS, pack
from .score import SOLVERS


class RansacBatch(NamedTuple):
    models: np.ndarray        # [P, 9] float64: the winning model as solved (zeros: none)
    inliers: np.ndarray       # [P] int32: the winner's count
    masks: list               # P arrays of uint8, one byte per point of the problem
    winner: np.ndarray        # [P, 3] int32: candidate (among the consumed samples' candidates), sample, root (-1 -1 -1: none)
    n_candidates: np.ndarray  # [P] int32: candidates of the consumed samples
    n_used: np.ndarray        # [P] int32: samples consumed
    point_ptr: np.ndarray     # [P + 1] int64
    sample_ptr: np.ndarray    # [P + 1] int64


def ransac_batch_raw(ctx, kind, point_ptr, a, b, sample_ptr, sample_idx, threshold, confidence, stage1=0, K=None) -> RansacBatch:
    """eacham_ransac_batch on arrays already in its wire form (nothing is checked here: the library's own checks answer). kind: a
    name of eacham_amd.lmeds.KINDS or the integer code itself."""
    k = kind if isinstance(kind, int) else SOLVERS[KINDS[kind]][0]
    point_ptr = np.ascontiguousarray(point_ptr, dtype=np.int64)
    sample_ptr = np.ascontiguousarray(sample_ptr, dtype=np.int64)
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    sample_idx = np.ascontiguousarray(sample_idx, dtype=np.int32)
    K4 = None if K is None else np.ascontiguousarray(K, dtype=np.float64).reshape(4)
    P = max(len(point_ptr) - 1, 0)
    npts = max(int(point_ptr[-1]), 0) if len(point_ptr) else 0
    models = np.zeros((P, 9), dtype=np.float64)
    inl, nc, nu = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
    masks = np.zeros(npts, dtype=np.uint8)
    win = np.zeros((P, 3), dtype=np.int32)
    vp = C.c_void_p
    ctx._check(capi.lib().eacham_ransac_batch(
        ctx.handle, k, len(point_ptr) - 1, vp(point_ptr.ctypes.data), vp(a.ctypes.data), vp(b.ctypes.data),
        vp(K4.ctypes.data) if K4 is not None else None, vp(sample_ptr.ctypes.data), vp(sample_idx.ctypes.data), float(threshold), float(confidence),
        int(stage1), vp(models.ctypes.data), vp(inl.ctypes.data), vp(masks.ctypes.data), vp(win.ctypes.data), vp(nc.ctypes.data), vp(nu.ctypes.data)))
    split = [masks[int(point_ptr[p]):int(point_ptr[p + 1])] for p in range(P)]
    return RansacBatch(models, inl, split, win, nc, nu, point_ptr, sample_ptr)


def ransac_batch(ctx, kind: str, uv1, uv2, samples, threshold: float, confidence: float, stage1: int = 0, K=None) -> RansacBatch:
    """kind "essential" (5-point samples, K = fx fy cx cy or None for normalised points), "homography" (4-point samples) or
    "fundamental" (7-point samples on pixels, K ignored). threshold: squared, in the error's units (essential with K: squared
    K-normalised units). uv1[p], uv2[p]: the n_p x 2 matches of pair p; samples[p]: its s_p x m minimal samples, in the order the
    loop would draw them. stage1: 0 = the library's default; >= the largest s_p = one pass."""
    point_ptr, a, b, sample_ptr, idx = pack(kind, uv1, uv2, samples)
    return ransac_batch_raw(ctx, kind, point_ptr, a, b, sample_ptr, idx, threshold, confidence, stage1, K)


def debug_last(ctx):
    """eacham_ransac_debug_last: (samples solved over both passes, host ms spent building the budget rows) of the context's last call."""
    n, ms = C.c_int64(0), C.c_double(0.0)
    ctx._check(capi.lib().eacham_ransac_debug_last(ctx.handle, C.byref(n), C.byref(ms)))
    return int(n.value), float(ms.value)
