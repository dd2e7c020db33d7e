"""Host-side mirror of eacham_pnp_hypotheses_batch / eacham_pnp_refit_batch (include/eacham_hip.h): cv::solvePnPRansac with EPnP —
RecoverPosePnP's estimator (modules/sfm/reconstruction/ReconstructionManager.cpp:227-228) — for a whole list of (map points,
pixels) problems: one call per RANSAC round of CHUNK samples for every problem still running, one call for all the refits, and
the sequential rule replayed per problem on the host in between (pnp_ransac_batch, what SolvePnPRansacBatch of
include/eacham/PnPHip.hpp does). Drawing the samples stays with the caller. Test / bench driver.
The P3P form (eacham_solve_p3p / eacham_pnp_hypotheses_batch_p3p; SolvePnPRansacP3P[Batch] of include/eacham/PnPP3PHip.hpp) draws
four-point samples: solve_p3p, pnp_hypotheses_batch_p3p[_raw] and pnp_ransac_batch(solver="p3p"); the refit stays EPnP.
The polish (eacham_pnp_refine_batch; RefinePnP[Batch] and SolvePnPRansac[P3P]Refined[Batch] of the two headers) is
pnp_refine_batch[_raw]: Levenberg-Marquardt on the reprojection error of one pose per problem over the rows a mask names, a PnpRefine."""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import numpy as np

from . import capi

CHUNK = 256   # pnp_detail::kChunk: samples per problem and round


class PnpHypotheses(NamedTuple):
    models: list | None       # P arrays [s_p, 12] float64 = R | t (zeros: degenerate sample); None: not asked for
    n_models: list            # P arrays [s_p] int32
    inlier_counts: list       # P arrays [s_p] int32
    point_ptr: np.ndarray     # [P + 1] int64
    sample_ptr: np.ndarray    # [P + 1] int64


class PnpRefit(NamedTuple):
    masks: list               # P arrays of uint8, one byte per point of the problem
    n_inliers: np.ndarray     # [P] int32
    refit: np.ndarray         # [P, 12] float64 (zeros where refit_ok is 0)
    refit_ok: np.ndarray      # [P] int32
    point_ptr: np.ndarray


class PnpRefine(NamedTuple):
    refined: np.ndarray       # [P, 12] float64 = R | t (the input pose where status is NOT_REFINED; zeros without a pose)
    cost: np.ndarray          # [P, 2] float64: sum of squared pixels over the used rows before, after
    tries: np.ndarray         # [P] int32
    status: np.ndarray        # [P] int32: REFINE_CONVERGED, REFINE_CAP, REFINE_NOT_REFINED
    masks: list | None        # P arrays of uint8: err <= threshold under the refined pose; None: not asked for
    n_inliers: np.ndarray | None
    point_ptr: np.ndarray


REFINE_CONVERGED, REFINE_CAP, REFINE_NOT_REFINED = 0, 1, 2   # EACHAM_PNP_REFINE_*


def _K4(K):
    K = np.asarray(K, dtype=np.float64)
    return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]) if K.shape == (3, 3) else np.ascontiguousarray(K).reshape(4)


def _cat(xs, shape, dt):
    return np.ascontiguousarray(np.concatenate(xs)) if len(xs) else np.zeros(shape, dt)


def _ptr(lengths):
    t = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=t[1:])
    return t


def pack_points(X, uv):
    """(point_ptr, object rows, image rows) of a list of problems. X[p]: n_p x 3, uv[p]: n_p x 2."""
    A = [np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in X]
    B = [np.asarray(x, dtype=np.float64).reshape(-1, 2) for x in uv]
    if len(A) != len(B) or any(len(a) != len(b) for a, b in zip(A, B)):
        raise ValueError("point lists disagree")
    return _ptr([len(a) for a in A]), _cat(A, (0, 3), np.float64), _cat(B, (0, 2), np.float64)


def _seg(x, t):
    return [x[int(t[p]):int(t[p + 1])] for p in range(len(t) - 1)]


_vp = lambda x: None if x is None else C.c_void_p(x.ctypes.data)   # noqa: E731  (a raw call's array, or its NULL)
_as = lambda x, dt: None if x is None else np.ascontiguousarray(x, dtype=dt)   # noqa: E731


def _hypotheses_raw(entry, ctx, point_ptr, X, uv, K, sample_ptr, sample_size, sample_idx, threshold, want_models, n_problems):
    """Either hypotheses entry on arrays already in its wire form; sample_size None: the entry has no such argument (P3P)."""
    point_ptr, sample_ptr = _as(point_ptr, np.int64), _as(sample_ptr, np.int64)
    X, uv, sample_idx = _as(X, np.float64), _as(uv, np.float64), _as(sample_idx, np.int32)
    K4 = None if K is None else _K4(K)
    P = (len(point_ptr) - 1 if point_ptr is not None else 0) if n_problems is None else int(n_problems)
    S = max(int(sample_ptr[-1]), 0) if sample_ptr is not None and len(sample_ptr) and P > 0 else 0
    if S > 1 << 28:   # (a table the library is about to refuse: nothing that size is allocated for it)
        S = 0
    models = np.zeros((S, 12), np.float64) if want_models else None
    nm, cnt = np.zeros(S, np.int32), np.zeros(S, np.int32)
    m = () if sample_size is None else (int(sample_size),)
    ctx._check(getattr(capi.lib(), entry)(ctx.handle, P, _vp(point_ptr), _vp(X), _vp(uv), _vp(K4), _vp(sample_ptr), *m, _vp(sample_idx),
                                          float(threshold), _vp(models), _vp(nm), _vp(cnt)))
    return PnpHypotheses(_seg(models, sample_ptr) if want_models else None, _seg(nm, sample_ptr), _seg(cnt, sample_ptr), point_ptr, sample_ptr)


def pnp_hypotheses_batch_raw(ctx, point_ptr, X, uv, K, sample_ptr, sample_size, sample_idx, threshold, want_models=True, n_problems=None):
    """eacham_pnp_hypotheses_batch on arrays already in its wire form (nothing is checked here: the library's own checks answer)."""
    return _hypotheses_raw("eacham_pnp_hypotheses_batch", ctx, point_ptr, X, uv, K, sample_ptr, sample_size, sample_idx, threshold, want_models, n_problems)


def pnp_hypotheses_batch(ctx, X, uv, K, samples, threshold: float = 16.0, want_models: bool = True) -> PnpHypotheses:
    """One RANSAC round: X[p] / uv[p] the n_p object points / pixels of problem p, samples[p] its s_p x m rows of indices into
    them (5 <= m <= 64, the same m for every problem; s_p may be 0), threshold in squared pixels."""
    point_ptr, A, B = pack_points(X, uv)
    I = [np.asarray(s, dtype=np.int32) for s in samples]
    ms = {i.shape[1] for i in I if i.ndim == 2 and len(i)}
    if len(I) != len(point_ptr) - 1 or len(ms) > 1:
        raise ValueError("one [s_p, m] index array per problem, one m for all")
    m = ms.pop() if ms else 5
    I = [i.reshape(-1, m) for i in I]
    return pnp_hypotheses_batch_raw(ctx, point_ptr, A, B, K, _ptr([len(i) for i in I]), m, _cat(I, (0, m), np.int32), threshold, want_models)


def pnp_hypotheses_batch_p3p_raw(ctx, point_ptr, X, uv, K, sample_ptr, sample_idx, threshold, want_models=True, n_problems=None):
    """eacham_pnp_hypotheses_batch_p3p on arrays already in its wire form (nothing is checked here: the library's own checks answer)."""
    return _hypotheses_raw("eacham_pnp_hypotheses_batch_p3p", ctx, point_ptr, X, uv, K, sample_ptr, None, sample_idx, threshold, want_models, n_problems)


def pnp_hypotheses_batch_p3p(ctx, X, uv, K, samples, threshold: float = 16.0, want_models: bool = True) -> PnpHypotheses:
    """One RANSAC round on four-point samples: pnp_hypotheses_batch with samples[p] = s_p x 4 rows (three points solve, the fourth picks
    among the up-to-four poses) and ONE launch for the whole list."""
    point_ptr, A, B = pack_points(X, uv)
    I = [np.asarray(s, dtype=np.int32).reshape(-1, 4) for s in samples]
    if len(I) != len(point_ptr) - 1:
        raise ValueError("one [s_p, 4] index array per problem")
    return pnp_hypotheses_batch_p3p_raw(ctx, point_ptr, A, B, K, _ptr([len(i) for i in I]), _cat(I, (0, 4), np.int32), threshold, want_models)


def solve_p3p(ctx, X, uv, K, samples, want_candidates: bool = True):
    """eacham_solve_p3p: every row of `samples` (4 indices into X / uv) -> (models [s, 12] = R | t, n_models [s]) and, when wanted,
    (candidates [s, 4, 12] in root order, the slots behind the count zero, n_candidates [s])."""
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
    uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    if len(X) != len(uv):
        raise ValueError("point lists disagree")
    idx = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 4)
    K4 = _K4(K)
    s = idx.shape[0]
    models, nm = np.zeros((s, 12), np.float64), np.zeros(s, np.int32)
    cand = np.zeros((s, 4, 12), np.float64) if want_candidates else None
    nc = np.zeros(s, np.int32) if want_candidates else None
    ctx._check(capi.lib().eacham_solve_p3p(ctx.handle, len(X), _vp(X), _vp(uv), _vp(K4), s, _vp(idx), _vp(models), _vp(nm), _vp(cand), _vp(nc)))
    return (models, nm, cand, nc) if want_candidates else (models, nm)


def pnp_refit_batch_raw(ctx, point_ptr, X, uv, K, models, has_model, threshold, n_problems=None):
    """eacham_pnp_refit_batch on arrays already in its wire form."""
    point_ptr, X, uv, models = _as(point_ptr, np.int64), _as(X, np.float64), _as(uv, np.float64), _as(models, np.float64)
    has_model = _as(has_model, np.uint8)
    K4 = None if K is None else _K4(K)
    P = (len(point_ptr) - 1 if point_ptr is not None else 0) if n_problems is None else int(n_problems)
    npts = max(int(point_ptr[-1]), 0) if point_ptr is not None and len(point_ptr) and P > 0 else 0
    if npts > 1 << 28:
        npts = 0
    mask, ni = np.zeros(npts, np.uint8), np.zeros(max(P, 0), np.int32)
    refit, ok = np.zeros((max(P, 0), 12), np.float64), np.zeros(max(P, 0), np.int32)
    ctx._check(capi.lib().eacham_pnp_refit_batch(ctx.handle, P, _vp(point_ptr), _vp(X), _vp(uv), _vp(K4), _vp(models), _vp(has_model),
                                                 float(threshold), _vp(mask), _vp(ni), _vp(refit), _vp(ok)))
    return PnpRefit(_seg(mask, point_ptr), ni, refit, ok, point_ptr)


def pnp_refit_batch(ctx, X, uv, K, models, has_model, threshold: float = 16.0) -> PnpRefit:
    """The tail of solvePnPRansac per problem: the mask of models[p] (12 doubles; has_model[p] = 0: none), and EPnP on its inliers."""
    point_ptr, A, B = pack_points(X, uv)
    models = np.ascontiguousarray(models, dtype=np.float64).reshape(-1, 12)
    has_model = np.ascontiguousarray(has_model, dtype=np.uint8).reshape(-1)
    if not (len(models) == len(has_model) == len(point_ptr) - 1):
        raise ValueError("one model and one has_model byte per problem")
    return pnp_refit_batch_raw(ctx, point_ptr, A, B, K, models, has_model, threshold)


def pnp_refine_batch_raw(ctx, point_ptr, X, uv, K, poses, has_pose, use_mask=None, max_tries=20, threshold=16.0, want_recount=True,
                         n_problems=None):
    """eacham_pnp_refine_batch on arrays already in its wire form (nothing is checked here: the library's own checks answer)."""
    point_ptr, X, uv, poses = _as(point_ptr, np.int64), _as(X, np.float64), _as(uv, np.float64), _as(poses, np.float64)
    has_pose, use_mask = _as(has_pose, np.uint8), _as(use_mask, np.uint8)
    K4 = None if K is None else _K4(K)
    P = (len(point_ptr) - 1 if point_ptr is not None else 0) if n_problems is None else int(n_problems)
    npts = max(int(point_ptr[-1]), 0) if point_ptr is not None and len(point_ptr) and P > 0 else 0
    if npts > 1 << 28:
        npts = 0
    Pz = max(P, 0)
    refined, cost = np.zeros((Pz, 12), np.float64), np.zeros((Pz, 2), np.float64)
    tries, status = np.zeros(Pz, np.int32), np.zeros(Pz, np.int32)
    mask = np.zeros(npts, np.uint8) if want_recount else None
    ni = np.zeros(Pz, np.int32) if want_recount else None
    ctx._check(capi.lib().eacham_pnp_refine_batch(ctx.handle, P, _vp(point_ptr), _vp(X), _vp(uv), _vp(K4), _vp(poses), _vp(has_pose), _vp(use_mask),
                                                  int(max_tries), float(threshold), _vp(refined), _vp(cost), _vp(tries), _vp(status), _vp(mask), _vp(ni)))
    return PnpRefine(refined, cost, tries, status, _seg(mask, point_ptr) if want_recount else None, ni, point_ptr)


def pnp_refine_batch(ctx, X, uv, K, poses, has_pose, use_masks=None, max_tries: int = 20, threshold: float = 16.0,
                     want_recount: bool = True) -> PnpRefine:
    """cv::solvePnPRefineLM per problem: Levenberg-Marquardt on the reprojection error of poses[p] (12 doubles; has_pose[p] = 0: none)
    over the rows of problem p with a non-zero byte in use_masks[p] (None: every row), at most max_tries tries; then the recount of
    err <= threshold (squared pixels) over all of the problem's points under the refined pose."""
    point_ptr, A, B = pack_points(X, uv)
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
    has_pose = np.ascontiguousarray(has_pose, dtype=np.uint8).reshape(-1)
    if not (len(poses) == len(has_pose) == len(point_ptr) - 1):
        raise ValueError("one pose and one has_pose byte per problem")
    use = None
    if use_masks is not None:
        use = _cat([np.asarray(m, dtype=np.uint8).reshape(-1) for m in use_masks], (0,), np.uint8)
        if len(use_masks) != len(poses) or len(use) != len(B):
            raise ValueError("one use byte per point")
    return pnp_refine_batch_raw(ctx, point_ptr, A, B, K, poses, has_pose, use, max_tries, threshold, want_recount)


def ransac_update_num_iters(p: float, ep: float, m: int, max_iters: int) -> int:
    """RANSACUpdateNumIters as twoview_detail::ransac_update_num_iters states it (host log and pow, lround)."""
    tiny = np.finfo(np.float64).tiny
    p, ep = min(max(p, 0.0), 1.0), min(max(ep, 0.0), 1.0)
    num, denom = max(1.0 - p, tiny), 1.0 - (1.0 - ep) ** m
    if denom < tiny:
        return 0
    num, denom = math.log(num), math.log(denom)
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters
    x = num / denom
    f = math.floor(abs(x))
    return int(math.copysign(f + (1 if abs(x) - f >= 0.5 else 0), x))


def pnp_ransac_batch(ctx, X, uv, K, samples, max_iters: int, reprojection_error: float = 4.0, confidence: float = 0.999,
                     hypotheses=None, refit=None, solver: str = "epnp"):
    """cv::solvePnPRansac per problem over rounds of CHUNK samples. samples[p]: the stream problem p would draw, in order, s x 5
    (rows past its end are not drawn: give at least as many as the loop consumes). solver "p3p": SOLVEPNP_P3P, s x 4 rows, the
    round is eacham_pnp_hypotheses_batch_p3p and a winner needs 4 inliers; the refit stays EPnP and is kept only where it has 5. Returns (results, turns): per problem a dict
    ok, iterations, winner (sample index, -1: none) and when ok: model, inliers, pose; turns = device calls made (rounds + 1).
    hypotheses / refit: the two calls (default: this context's batched entry points), same signatures as pnp_hypotheses_batch /
    pnp_refit_batch without the context."""
    if solver not in ("epnp", "p3p"):
        raise ValueError(f"unknown solver {solver!r}")
    hypotheses = hypotheses or (lambda *a: (pnp_hypotheses_batch_p3p if solver == "p3p" else pnp_hypotheses_batch)(ctx, *a))
    refit = refit or (lambda *a: pnp_refit_batch(ctx, *a))
    m = 4 if solver == "p3p" else 5
    X = [np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in X]
    uv = [np.asarray(x, dtype=np.float64).reshape(-1, 2) for x in uv]
    S = [np.asarray(s, dtype=np.int32).reshape(-1, m) for s in samples]
    P = len(X)
    thr = float(np.float32(reprojection_error) * np.float32(reprojection_error))
    out = [{"ok": False, "iterations": 0, "winner": -1} for _ in range(P)]
    budget = [max_iters if len(uv[p]) >= m and max_iters > 0 and len(S[p]) else 0 for p in range(P)]
    best = [-1] * P
    model = np.zeros((P, 12))
    turns, first = 0, 0
    while any(first < min(budget[p], len(S[p])) for p in range(P)):
        rows = [S[p][first:min(first + CHUNK, max_iters)] if first < budget[p] else np.zeros((0, m), np.int32) for p in range(P)]
        h = hypotheses(X, uv, K, rows, thr, True)
        turns += 1
        for p in range(P):
            n = len(uv[p])
            for k in range(len(rows[p])):
                if first + k >= budget[p]:
                    break
                out[p]["iterations"] = first + k + 1
                if h.n_models[p][k] and h.inlier_counts[p][k] > max(best[p], m - 1):
                    best[p] = int(h.inlier_counts[p][k])
                    out[p]["winner"] = first + k
                    model[p] = h.models[p][k]
                    budget[p] = ransac_update_num_iters(confidence, (n - best[p]) / n, m, budget[p])
        first += CHUNK
    has = np.array([b >= m for b in best], dtype=np.uint8)
    if has.any():
        r = refit(X, uv, K, model, has, thr)
        turns += 1
        for p in np.nonzero(has)[0]:
            out[p].update(ok=True, model=model[p].copy(), inliers=np.nonzero(r.masks[p])[0].astype(np.int32),
                          pose=r.refit[p].copy() if r.refit_ok[p] else model[p].copy())
    return out, turns
