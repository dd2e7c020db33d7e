"""Host-side mirror of the view-graph query on the CSR match graph.

  best_pair_for_valid(...)  <->  Graph::GetBestPairForValid (modules/sfm/data/Graph.h:59-106)

The match graph is the wire format `HipContext.match_all_pairs` returns: (pairs, counts, offsets, q, t);
pair p with counts[p] > 0 is the factor f1 -> f2 (matches q -> t) and the factor f2 -> f1 (t -> q),
i.e. the two Graph::Connect calls of apps/sfm/main.cpp:144-145.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from .matcher import HipContext

NONE = 0xFFFFFFFF  # std::numeric_limits<unsigned>::max() of the reference's empty result


def pack_has3d(per_frame) -> tuple[np.ndarray, np.ndarray]:
    """per_frame[f] = bool array over the keypoints of frame f (HasPoint3d && !IsPoint3dTwoView)."""
    sizes = np.array([len(a) for a in per_frame], dtype=np.int64)
    kp_offsets = np.zeros(len(per_frame) + 1, dtype=np.int64)
    kp_offsets[1:] = np.cumsum(sizes)
    flat = np.concatenate([np.asarray(a, dtype=np.uint8) for a in per_frame]) if len(per_frame) else np.zeros(0, np.uint8)
    return kp_offsets, np.ascontiguousarray(flat, dtype=np.uint8)


def best_pair_for_valid(ctx: HipContext, n_frames: int, pairs, counts, offsets, q, t, valid, has3d_per_frame,
                        excluded=None, want_edge_counts: bool = False):
    """Returns (id, id2, points3dCount) [, edge_counts npairs x 2]."""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    q = np.ascontiguousarray(q, dtype=np.uint32)
    t = np.ascontiguousarray(t, dtype=np.uint32)
    valid = np.ascontiguousarray(valid, dtype=np.uint8)
    excl = None if excluded is None else np.ascontiguousarray(excluded, dtype=np.uint8)
    kp_offsets, flat = pack_has3d(has3d_per_frame)
    if valid.size != n_frames or kp_offsets.size != n_frames + 1 or (excl is not None and excl.size != n_frames):
        raise ValueError("per-frame arrays must have n_frames entries")
    ec = np.zeros((pairs.shape[0], 2), dtype=np.uint32)
    best = np.zeros(3, dtype=np.uint32)
    ctx._check(ctx._L.eacham_graph_best_pair(
        ctx.handle, n_frames, pairs.ctypes.data, pairs.shape[0], counts.ctypes.data, offsets.ctypes.data, q.ctypes.data,
        t.ctypes.data, valid.ctypes.data, excl.ctypes.data if excl is not None else None, kp_offsets.ctypes.data,
        flat.ctypes.data, ec.ctypes.data, best.ctypes.data))
    out = (int(best[0]), int(best[1]), int(best[2]))
    return (out, ec) if want_edge_counts else out


SAMPLINGS = {"opencv": 0, "counter": 1}


class GraphVerify(NamedTuple):
    """eacham_graph_verify: the LmedsBatch fields per caller pair, the mask in the caller's match index space, the samples drawn."""
    models: np.ndarray        # [npairs, 9] float64: the winning model as solved (zeros: none)
    medians: np.ndarray       # [npairs] float32 (NaN: none)
    thresholds: np.ndarray    # [npairs] float32
    inliers: np.ndarray       # [npairs] int32
    masks: np.ndarray         # [n_src] uint8, indexed like the q / t the graph was made from: the `keep` of ResidentGraph.tracks
    winner: np.ndarray        # [npairs, 3] int32: candidate, sample, root (-1 -1 -1: none)
    n_candidates: np.ndarray  # [npairs] int32
    n_samples: np.ndarray     # [npairs] int32: the samples each pair used
    samples: np.ndarray | None  # [npairs, iterations, m] int32, -1 behind a pair's n_samples (want_samples)


class GraphVerifyRansac(NamedTuple):
    """eacham_graph_verify_ransac: the RansacBatch fields per caller pair, the mask in the caller's match index space, the samples drawn."""
    models: np.ndarray        # [npairs, 9] float64: the winning model as solved (zeros: none)
    inliers: np.ndarray       # [npairs] int32
    masks: np.ndarray         # [n_src] uint8, indexed like the q / t the graph was made from
    winner: np.ndarray        # [npairs, 3] int32: candidate, sample, root (-1 -1 -1: none)
    n_candidates: np.ndarray  # [npairs] int32: candidates of the consumed samples
    n_used: np.ndarray        # [npairs] int32: samples consumed
    n_samples: np.ndarray     # [npairs] int32: the samples each pair drew
    samples: np.ndarray | None  # [npairs, iterations, m] int32, -1 behind a pair's n_samples (want_samples)


def lmeds_iterations(kind: str, max_iters: int | None = None, confidence: float | None = None) -> int:
    """The samples LMeDSPointSetRegistrator::run asks for, as twoview_detail::lmeds computes them: RANSACUpdateNumIters at an
    assumed outlier ratio of 0.45, at least 3, at most max_iters. Defaults: the reference's calls (essential 1000 / 0.99 -> 89,
    homography 100 / 0.999 -> 72) and cv::findFundamentalMat's own (fundamental 1000 / 0.99 -> 300)."""
    import math
    essential = kind.startswith("essential") or kind.startswith("fundamental")   # (cv::findFundamentalMat's defaults are 1000 / 0.99 too)
    m = 7 if kind.startswith("fundamental") else (5 if essential else 4)
    max_iters = (1000 if essential else 100) if max_iters is None else int(max_iters)
    p = min(max((0.99 if essential else 0.999) if confidence is None else float(confidence), 0.0), 1.0)
    tiny = np.finfo(np.float64).tiny
    num, denom = max(1.0 - p, tiny), 1.0 - (1.0 - 0.45) ** m
    if denom < tiny:
        n = 0
    else:
        ln, ld = math.log(num), math.log(denom)
        n = max_iters if ld >= 0 or -ln >= max_iters * (-ld) else int(math.floor(ln / ld + 0.5))
    return max(min(max_iters, max(n, 3)), 0)


class ResidentGraph:
    """eacham_graph_create / _set_frame / _query: the match graph uploaded once, the per-frame state set frame by frame,
    the query two small kernels — what the incremental loop of apps/sfm/main.cpp:188-214 uses after every frame it adds."""

    def __init__(self, ctx: HipContext, n_frames: int, pairs, counts, offsets, q, t, keypoints_per_frame):
        import ctypes as C
        self._C, self.ctx, self.n_frames = C, ctx, n_frames
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        q = np.ascontiguousarray(q, dtype=np.uint32)
        t = np.ascontiguousarray(t, dtype=np.uint32)
        kpo = np.zeros(n_frames + 1, dtype=np.int64)
        kpo[1:] = np.cumsum(np.asarray(keypoints_per_frame, dtype=np.int64))
        h = C.c_void_p()
        ctx._check(ctx._L.eacham_graph_create(ctx.handle, n_frames, pairs.ctypes.data, pairs.shape[0], counts.ctypes.data, offsets.ctypes.data,
                                              q.ctypes.data, t.ctypes.data, kpo.ctypes.data, C.byref(h)))
        self._h = h
        self._n_nodes, self._n_matches = int(kpo[-1]), int(counts[counts > 0].sum())
        self._npairs = int(pairs.shape[0])
        ends = offsets[:counts.size] + counts    # (offsets may carry the CSR's closing entry)
        self._n_src = int(ends[counts > 0].max()) if (counts > 0).any() else 0   # the length of a `keep` mask
        self._query_rows = int(sum(int(kpo[f + 1] - kpo[f]) for f in pairs[:, 0]))   # what a guided re-match of every pair can return at most

    def match_guided(self, kind: str, models, max_error: float, ratio: float | None = None, max_d2: int = 0, cross_check: bool = True,
                     K=None, cap: int | None = None):
        """eacham_graph_match_guided: every pair of the graph matched again with only the candidates admitted whose error under
        the pair's model (models [npairs, 9], as verify() / verify_ransac() returned them) is <= max_error; pairs and keypoints
        are the graph's (set_keypoints). Returns eacham_amd.guided.GuidedMatches, the wire format a new ResidentGraph takes."""
        from .guided import graph_match_guided
        from .matcher import RATIO
        return graph_match_guided(self.ctx, self._h, self._npairs, self._query_rows if cap is None else int(cap), kind, models, max_error,
                                  RATIO if ratio is None else ratio, max_d2, cross_check, K)

    def set_keypoints(self, xy):
        """eacham_graph_set_keypoints: the pixel coordinates of every keypoint, frame-major ([total keypoints, 2], or a list of
        per-frame [n_f, 2] arrays). Uploaded once; a later call replaces them and drops a retained mask."""
        if isinstance(xy, (list, tuple)):
            xy = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1, 2) for a in xy]) if len(xy) else np.zeros((0, 2))
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        if xy.shape[0] != self._n_nodes:
            raise ValueError(f"xy has {xy.shape[0]} rows, the graph {self._n_nodes} keypoints")
        self.ctx._check(self.ctx._L.eacham_graph_set_keypoints(self._h, xy.ctypes.data if xy.size else None))

    def verify(self, kind: str, K=None, sampling: str = "opencv", iterations: int | None = None, seeds=None, retain: bool = False,
               want_samples: bool = False) -> GraphVerify:
        """eacham_graph_verify: LMedS ("essential" with K = fx fy cx cy or None for normalised points, "homography", or
        "fundamental": pixels, K ignored) for every pair of the graph, gathered, sampled and solved on the device. iterations defaults to lmeds_iterations(kind); seeds: one
        per pair for sampling="counter" (None: 12345). retain=True keeps the mask on the device for tracks_verified()."""
        from . import capi
        homography, fundamental = kind.startswith("homography"), kind.startswith("fundamental")
        if not homography and not fundamental and not kind.startswith("essential"):
            raise ValueError(f"unknown kind {kind!r}")
        k, m = (capi.SOLVE_HOMOGRAPHY4, 4) if homography else ((capi.SOLVE_FUNDAMENTAL7, 7) if fundamental else (capi.SOLVE_ESSENTIAL5, 5))
        its = lmeds_iterations(kind) if iterations is None else int(iterations)
        return self._verify_raw(k, m, K, SAMPLINGS[sampling], its, seeds, retain, want_samples)

    def _verify_raw(self, k: int, m: int, K, sampling: int, its: int, seeds, retain: bool, want_samples: bool, preset=None) -> GraphVerify:
        """The call itself on integer codes (nothing is checked here: the library's own checks answer). preset: a value every
        output array is filled with beforehand (tests of the error paths)."""
        P = self._npairs
        K4 = None if K is None else np.ascontiguousarray(K, dtype=np.float64).reshape(4)
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        if sd is not None and sd.size != P:
            raise ValueError("one seed per pair")
        fill = 0 if preset is None else preset
        models = np.full((P, 9), fill, dtype=np.float64)
        med, thr = np.full(P, fill, dtype=np.float32), np.full(P, fill, dtype=np.float32)
        inl, nc, ns = np.full(P, fill, dtype=np.int32), np.full(P, fill, dtype=np.int32), np.full(P, fill, dtype=np.int32)
        win = np.full((P, 3), fill, dtype=np.int32)
        masks = np.full(self._n_src, fill, dtype=np.uint8)
        samples = np.full((P, max(its, 0), m), fill, dtype=np.int32) if want_samples else None
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data   # noqa: E731
        self.ctx._check(self.ctx._L.eacham_graph_verify(
            self._h, k, ptr(K4), sampling, its, ptr(sd), int(bool(retain)), ptr(models), ptr(med), ptr(thr), ptr(inl), ptr(masks), ptr(win),
            ptr(nc), ptr(ns), ptr(samples)))
        return GraphVerify(models, med, thr, inl, masks, win, nc, ns, samples)

    def verify_ransac(self, kind: str, threshold: float, confidence: float, iterations: int, K=None, sampling: str = "opencv", seeds=None,
                      retain: bool = False, want_samples: bool = False, stage1: int = 0) -> GraphVerifyRansac:
        """eacham_graph_verify_ransac: threshold RANSAC (eacham_amd/ransac.py) for every pair of the graph, gathered, sampled and solved
        on the device. threshold: squared, in the error's units; iterations: the samples drawn per pair (maxIters); stage1: 0 = the
        library's default. retain=True keeps the mask on the device for tracks_verified()."""
        from . import capi
        homography, fundamental = kind.startswith("homography"), kind.startswith("fundamental")
        if not homography and not fundamental and not kind.startswith("essential"):
            raise ValueError(f"unknown kind {kind!r}")
        k, m = (capi.SOLVE_HOMOGRAPHY4, 4) if homography else ((capi.SOLVE_FUNDAMENTAL7, 7) if fundamental else (capi.SOLVE_ESSENTIAL5, 5))
        P, its = self._npairs, int(iterations)
        K4 = None if K is None else np.ascontiguousarray(K, dtype=np.float64).reshape(4)
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        if sd is not None and sd.size != P:
            raise ValueError("one seed per pair")
        models = np.zeros((P, 9), dtype=np.float64)
        inl, nc, nu, ns = (np.zeros(P, dtype=np.int32) for _ in range(4))
        win = np.zeros((P, 3), dtype=np.int32)
        masks = np.zeros(self._n_src, dtype=np.uint8)
        samples = np.zeros((P, max(its, 0), m), dtype=np.int32) if want_samples else None
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data   # noqa: E731
        self.ctx._check(self.ctx._L.eacham_graph_verify_ransac(
            self._h, k, ptr(K4), SAMPLINGS[sampling], its, ptr(sd), int(bool(retain)), float(threshold), float(confidence), int(stage1),
            ptr(models), ptr(inl), ptr(masks), ptr(win), ptr(nc), ptr(nu), ptr(ns), ptr(samples)))
        return GraphVerifyRansac(models, inl, masks, win, nc, nu, ns, samples)

    def tracks_verified(self, min_len: int = 2, conflict_policy: int = 0, cap_obs=None, cap_tracks=None):
        """eacham_graph_tracks_verified: tracks() with the mask the last verify(retain=True) left on the device; nothing is uploaded."""
        from .tracks import graph_tracks_verified
        return graph_tracks_verified(self.ctx, self._h, self._n_nodes, self._n_matches, min_len, conflict_policy, cap_obs, cap_tracks)

    def tracks(self, keep=None, min_len: int = 2, conflict_policy: int = 0, cap_obs=None, cap_tracks=None):
        """eacham_graph_tracks: the multi-view tracks of the resident graph (eacham_amd/tracks.py); only `keep` — a byte per match,
        indexed like the q and t the graph was made from — is uploaded."""
        from .tracks import graph_tracks
        return graph_tracks(self.ctx, self._h, self._n_nodes, self._n_matches, keep, min_len, conflict_policy, cap_obs, cap_tracks)

    def set_frame(self, frame: int, valid: bool, has3d=None):
        f = None if has3d is None else np.ascontiguousarray(has3d, dtype=np.uint8)
        self.ctx._check(self.ctx._L.eacham_graph_set_frame(self._h, int(frame), int(bool(valid)), None if f is None else f.ctypes.data,
                                                           0 if f is None else f.size))

    def set_frames(self, frames, valid, has3d_per_frame):
        """eacham_graph_set_frames: several frames in one copy + one kernel (has3d_per_frame[i]: the full flag array of frames[i])."""
        fr = np.ascontiguousarray(frames, dtype=np.int32)
        va = np.ascontiguousarray(valid, dtype=np.uint8)
        off = np.zeros(len(fr) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(a) for a in has3d_per_frame])
        fl = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.uint8) for a in has3d_per_frame]) if len(fr) else np.zeros(0, np.uint8))
        self.ctx._check(self.ctx._L.eacham_graph_set_frames(self._h, int(len(fr)), fr.ctypes.data, va.ctypes.data, fl.ctypes.data if fl.size else None, off.ctypes.data))

    def query(self, excluded_frames=()):
        ex = np.ascontiguousarray(list(excluded_frames), dtype=np.int32)
        best = np.zeros(3, dtype=np.uint32)
        self.ctx._check(self.ctx._L.eacham_graph_query(self._h, ex.ctypes.data if ex.size else None, int(ex.size), best.ctypes.data))
        return int(best[0]), int(best[1]), int(best[2])

    def close(self):
        if self._h:
            self.ctx._L.eacham_graph_destroy(self._h)
            self._h = None
