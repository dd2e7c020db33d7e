"""Host-side mirror of the reference matcher interface, on top of the C-ABI.

  FeatureMatcherHip.Match(d1, d2)    <->  FeatureMatcherFlann::Match / IFeatureMatcher<T>::Match
                                          (modules/base/features/FeatureMatcherFlann.h:14-19,
                                           modules/base/features/IFeatureMatcher.h:8-20)
  HipContext.match_all_pairs(pairs)  <->  the pair loop + mutual check of apps/sfm/main.cpp:84-147

Python is only the test/bench driver here (the reference is C++; its adapter is
include/eacham/FeatureMatcherHip.hpp). Same names, argument meaning and error behaviour.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

# literals of the reference
RATIO = 0.8        # FeatureMatcherFlann.cpp:23 (the ctor's inliersRatio is stored but never used)
MIN_DIRECTED = 30  # apps/sfm/main.cpp:111  `matches12.size() < 30` -> drop
MIN_MUTUAL = 30    # apps/sfm/main.cpp:142  `bestMatches12.size() > 30` -> connect
MIN_SCORE = 0.5    # modules/onnx/lightglue/FeatureMatcherLightglue.cpp:118  `mscores0 > 0.5` -> keep


class HipContext:
    """One HIP device + stream + resident descriptor store (eacham_ctx)."""

    def __init__(self, device_id: int = 0):
        self._L = capi.lib()
        h = C.c_void_p()
        rc = self._L.eacham_ctx_create(device_id, C.byref(h))
        if rc != capi.OK:
            raise capi.EachamError(rc, "eacham_ctx_create failed (no HIP device? the hot path has no CPU fallback)")
        self._h = h

    @classmethod
    def borrowed(cls, handle):
        """A view of a context that somebody else owns (a device of an eacham_comm): never destroyed from here."""
        self = cls.__new__(cls)
        self._L = capi.lib()
        self._h = handle
        self._borrowed = True
        return self

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                self._L.eacham_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int):
        if rc != capi.OK:
            raise capi.EachamError(rc, self._L.eacham_last_error(self._h).decode())

    @property
    def handle(self):
        return self._h

    @property
    def stream(self) -> int:
        return int(self._L.eacham_ctx_stream(self._h) or 0)

    def stream2_info(self) -> dict:
        """What the second-stream search of eacham_ctx_create decided (eacham_ctx_stream2_info)."""
        a, ms = C.c_int(-1), C.c_float(-1.0)
        self._check(self._L.eacham_ctx_stream2_info(self._h, C.byref(a), C.byref(ms)))
        return {"attempt": a.value, "lead_ms": round(ms.value, 4), "own_queue": bool(ms.value > 0.010)}

    def sync(self):
        self._check(self._L.eacham_ctx_sync(self._h))

    # ---- descriptor store ------------------------------------------------------------------
    def upload_descriptors(self, frame_id: int, desc: np.ndarray):
        d = np.ascontiguousarray(desc, dtype=np.float32)
        if d.ndim != 2:
            raise ValueError("descriptors must be an N x D matrix")
        self._check(self._L.eacham_upload_descriptors(self._h, frame_id, d.ctypes.data, d.shape[0], d.shape[1]))

    def upload_descriptors_f32(self, frame_id: int, desc: np.ndarray):
        """Float descriptors (SuperPoint / LightGlue style): fp32 MFMA path, any values."""
        d = np.ascontiguousarray(desc, dtype=np.float32)
        if d.ndim != 2:
            raise ValueError("descriptors must be an N x D matrix")
        self._check(self._L.eacham_upload_descriptors_f32(self._h, frame_id, d.ctypes.data, d.shape[0], d.shape[1]))

    def upload_descriptors_dev(self, frame_id: int, dev_ptr: int, n: int, dim: int):
        self._check(self._L.eacham_upload_descriptors_dev(self._h, frame_id, C.c_void_p(dev_ptr), n, dim))

    def frame_rows(self, frame_id: int) -> int:
        n = self._L.eacham_frame_rows(self._h, frame_id)
        if n < 0:
            self._check(n)
        return n

    def clear_descriptors(self):
        self._check(self._L.eacham_clear_descriptors(self._h))

    # ---- matching --------------------------------------------------------------------------
    def match_pair(self, f1: int, f2: int, ratio: float = RATIO):
        cap = max(self.frame_rows(f1), 1)
        q = np.empty(cap, dtype=np.uint32)
        t = np.empty(cap, dtype=np.uint32)
        cnt = C.c_int(0)
        self._check(self._L.eacham_match_pair(self._h, f1, f2, ratio, q.ctypes.data, t.ctypes.data, cap, C.byref(cnt)))
        return q[:cnt.value].copy(), t[:cnt.value].copy()

    def match_all_pairs(self, pairs: np.ndarray, ratio: float = RATIO, min_dir: int = MIN_DIRECTED,
                        min_mutual: int = MIN_MUTUAL, cap: int | None = None, stats: bool = True):
        """Returns (counts, offsets, q, t, stats): CSR over pairs, see include/eacham_hip.h. stats=False passes NULL for the
        per-pair statistics (what the pair loop of apps/sfm/main.cpp needs: the library then evaluates the column direction
        for candidate columns only) and returns None in their place."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        npairs = pairs.shape[0]
        if cap is None:
            cap = int(sum(self.frame_rows(int(p[0])) for p in pairs)) if npairs else 0
        counts = np.zeros(npairs, dtype=np.int32)
        offsets = np.zeros(npairs + 1, dtype=np.int64)
        q = np.empty(max(cap, 1), dtype=np.uint32)
        t = np.empty(max(cap, 1), dtype=np.uint32)
        st = np.zeros((npairs, 4), dtype=np.int32) if stats else None
        total = C.c_int64(0)
        self._check(self._L.eacham_match_all_pairs(
            self._h, pairs.ctypes.data, npairs, ratio, min_dir, min_mutual, counts.ctypes.data,
            offsets.ctypes.data, q.ctypes.data, t.ctypes.data, cap, C.byref(total), st.ctypes.data if stats else None))
        return counts, offsets, q[:total.value].copy(), t[:total.value].copy(), st

    def match_batches(self, npairs: int, stats: bool = False):
        """(starts, slots): first pair of every launch the library would cut a job of `npairs` pairs into, and the number of
        workspace slots the launches rotate through (eacham_match_debug_batches)."""
        starts = np.zeros(4096, dtype=np.int32)
        nb, ns = C.c_int(0), C.c_int(0)
        self._check(self._L.eacham_match_debug_batches(self._h, npairs, int(stats), starts.ctypes.data, len(starts), C.byref(nb), C.byref(ns)))
        return starts[:min(nb.value, len(starts))].copy(), ns.value

    def match_plan(self, npairs: int, stats: bool = False):
        """(batch, round_pairs, tail_pairs): the most pairs of a launch, the unit launches are sized in and the most pairs of a job's
        short last launch, for a job of `npairs` pairs of the resident frames (eacham_match_debug_plan)."""
        b, r, t = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self._L.eacham_match_debug_plan(self._h, npairs, int(stats), C.byref(b), C.byref(r), C.byref(t)))
        return b.value, r.value, t.value

    def match_colprune(self):
        """(settled, verified): candidate columns of the last match_all_pairs call that the arg-min pass settled from the row sweep's
        minima / that went through the column pass (eacham_match_debug_colprune)."""
        s, v = C.c_int64(0), C.c_int64(0)
        self._check(self._L.eacham_match_debug_colprune(self._h, C.byref(s), C.byref(v)))
        return s.value, v.value

    def match_screen(self):
        """(rows, open): real query rows the screen sweeps of the last matching call met / rows their bound left open for the exact
        pass (eacham_match_debug_screen); (0, 0) when the call ran another form of the row sweep."""
        r, o = C.c_int64(0), C.c_int64(0)
        self._check(self._L.eacham_match_debug_screen(self._h, C.byref(r), C.byref(o)))
        return r.value, o.value

    def match_screen_items(self) -> int:
        """Work items the exact pass of the last matching call took those open rows in, over all its launches
        (eacham_match_debug_screen_items): up to 256 open rows of consecutive pairs that share their train frame per item."""
        n = C.c_int64(0)
        self._check(self._L.eacham_match_debug_screen_items(self._h, C.byref(n)))
        return n.value

    def match_screen_pair(self, f1: int, f2: int):
        """(n1, L1, U2) per row of f1, as the screen sweep writes them for the ordered pair (f1, f2) before the exact pass
        (eacham_match_debug_screen_pair): the smallest squared code difference, a lower bound of the row's smallest squared
        distance, an upper bound of its second smallest (-1: a padding value)."""
        n = max(self.frame_rows(f1), 1)
        n1 = np.zeros(n, dtype=np.uint32)
        l1 = np.zeros(n, dtype=np.int32)
        u2 = np.zeros(n, dtype=np.int32)
        self._check(self._L.eacham_match_debug_screen_pair(self._h, f1, f2, n1.ctypes.data, l1.ctypes.data, u2.ctypes.data, n))
        k = self.frame_rows(f1)
        return n1[:k], l1[:k], u2[:k]

    def match_pairs_directed(self, frames, ordered_pairs, ratio: float = RATIO, f32: bool = False) -> list:
        """Uploads `frames` (list of N x D matrices) as frames 0.. and runs every ordered pair (i, j) as one directed
        Match(frames[i], frames[j]) in ONE launch sequence; returns a list of {queryIdx: trainIdx} dicts."""
        self.clear_descriptors()
        for f, d in enumerate(frames):
            (self.upload_descriptors_f32 if f32 else self.upload_descriptors)(f, d)
        pairs = np.ascontiguousarray(ordered_pairs, dtype=np.int32).reshape(-1, 2)
        npairs = pairs.shape[0]
        cap = int(sum(frames[int(p[0])].shape[0] for p in pairs))
        counts = np.zeros(npairs, dtype=np.int32)
        offsets = np.zeros(npairs + 1, dtype=np.int64)
        q = np.empty(max(cap, 1), dtype=np.uint32)
        t = np.empty(max(cap, 1), dtype=np.uint32)
        total = C.c_int64(0)
        self._check(self._L.eacham_match_pairs_directed(self._h, pairs.ctypes.data, npairs, ratio, counts.ctypes.data,
                                                        offsets.ctypes.data, q.ctypes.data, t.ctypes.data, cap, C.byref(total)))
        return [dict(zip(q[offsets[p]:offsets[p + 1]].tolist(), t[offsets[p]:offsets[p + 1]].tolist())) for p in range(npairs)]

    def match_guided(self, kind: str, pairs, models, keypoints, max_error: float, **kw):
        """eacham_match_guided on the resident int8 frames (eacham_amd/guided.py: match_guided has the arguments)."""
        from .guided import match_guided
        return match_guided(self, kind, pairs, models, keypoints, max_error, **kw)

    # ---- dot-product similarity (float frames), scores returned ----------------------------
    def match_pair_dot(self, f1: int, f2: int, min_score: float = MIN_SCORE):
        """(q, t, scores) of the directed match f1 -> f2: argmax of a.b per row, kept iff the similarity > min_score."""
        cap = max(self.frame_rows(f1), 1)
        q = np.empty(cap, dtype=np.uint32)
        t = np.empty(cap, dtype=np.uint32)
        s = np.empty(cap, dtype=np.float32)
        cnt = C.c_int(0)
        self._check(self._L.eacham_match_pair_dot(self._h, f1, f2, min_score, q.ctypes.data, t.ctypes.data, s.ctypes.data, cap, C.byref(cnt)))
        return q[:cnt.value].copy(), t[:cnt.value].copy(), s[:cnt.value].copy()

    def _dot_buffers(self, pairs, cap):
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        npairs = pairs.shape[0]
        if cap is None:
            cap = int(sum(self.frame_rows(int(p[0])) for p in pairs)) if npairs else 0
        return (pairs, npairs, cap, np.zeros(npairs, dtype=np.int32), np.zeros(npairs + 1, dtype=np.int64),
                np.empty(max(cap, 1), dtype=np.uint32), np.empty(max(cap, 1), dtype=np.uint32), np.empty(max(cap, 1), dtype=np.float32))

    def match_pairs_directed_dot(self, ordered_pairs, min_score: float = MIN_SCORE, cap: int | None = None):
        """Every ordered pair (i, j) of the RESIDENT float frames as one directed dot-product match, in one launch sequence.
        Returns (counts, offsets, q, t, scores): CSR over the pairs."""
        pairs, npairs, cap, counts, offsets, q, t, s = self._dot_buffers(ordered_pairs, cap)
        total = C.c_int64(0)
        self._check(self._L.eacham_match_pairs_directed_dot(self._h, pairs.ctypes.data, npairs, min_score, counts.ctypes.data,
                                                            offsets.ctypes.data, q.ctypes.data, t.ctypes.data, s.ctypes.data, cap, C.byref(total)))
        n = total.value
        return counts, offsets, q[:n].copy(), t[:n].copy(), s[:n].copy()

    def match_all_pairs_dot(self, pairs, min_score: float = MIN_SCORE, min_dir: int = MIN_DIRECTED, min_mutual: int = MIN_MUTUAL,
                            cap: int | None = None, stats: bool = True, screened: bool = False):
        """The mutual form (eacham_match_all_pairs_dot). Returns (counts, offsets, q, t, scores, stats). screened=True runs
        eacham_match_all_pairs_dot_screened: an fp16 sweep + exact fp32 work where it decides nothing — the same bytes."""
        pairs, npairs, cap, counts, offsets, q, t, s = self._dot_buffers(pairs, cap)
        st = np.zeros((npairs, 4), dtype=np.int32) if stats else None
        total = C.c_int64(0)
        call = self._L.eacham_match_all_pairs_dot_screened if screened else self._L.eacham_match_all_pairs_dot
        self._check(call(
            self._h, pairs.ctypes.data, npairs, min_score, min_dir, min_mutual, counts.ctypes.data, offsets.ctypes.data,
            q.ctypes.data, t.ctypes.data, s.ctypes.data, cap, C.byref(total), st.ctypes.data if stats else None))
        n = total.value
        return counts, offsets, q[:n].copy(), t[:n].copy(), s[:n].copy(), st

    def match_dot_screen(self):
        """{rows: (dead, settled, open), cols: (dead, settled, open), fallback_pairs} of the last screened call
        (eacham_match_debug_dot_screen)."""
        out = (C.c_int64 * 7)()
        self._check(self._L.eacham_match_debug_dot_screen(self._h, out))
        v = [int(x) for x in out]
        return {"rows": tuple(v[0:3]), "cols": tuple(v[3:6]), "fallback_pairs": v[6]}

    def match_dot_coarse(self, f1: int, f2: int):
        """(s_coarse, row_E, col_E): the fp16 sweep's raw n1 x n2 similarities of the pair and the error bounds it classifies rows
        and columns with (eacham_match_debug_dot_coarse; test hook, frames of <= 4096 rows)."""
        n1, n2 = self.frame_rows(f1), self.frame_rows(f2)
        s = np.zeros((n1, n2), dtype=np.float32)
        re, ce = np.zeros(max(n1, 1), dtype=np.float32), np.zeros(max(n2, 1), dtype=np.float32)
        self._check(self._L.eacham_match_debug_dot_coarse(self._h, f1, f2, s.ctypes.data if s.size else None, re.ctypes.data, ce.ctypes.data))
        return s, re[:n1], ce[:n2]

    # ---- binary descriptors under Hamming distance, distances returned ----------------------
    def upload_descriptors_bits(self, frame_id: int, rows: np.ndarray):
        """Packed binary descriptors (ORB / BRIEF / AKAZE): an N x B uint8 matrix, B = 1..32 bytes per row."""
        d = np.ascontiguousarray(rows, dtype=np.uint8)
        if d.ndim != 2:
            raise ValueError("binary descriptors must be an N x B uint8 matrix")
        self._check(self._L.eacham_upload_descriptors_bits(self._h, frame_id, d.ctypes.data, d.shape[0], d.shape[1]))

    def upload_descriptors_bits_dev(self, frame_id: int, dev_ptr: int, n: int, bytes_per_row: int):
        self._check(self._L.eacham_upload_descriptors_bits_dev(self._h, frame_id, C.c_void_p(dev_ptr), n, bytes_per_row))

    def upload_descriptors_bits_wide(self, frame_id: int, rows: np.ndarray):
        """Packed binary descriptors of up to 64 bytes per row (BRISK, FREAK, AKAZE's 61-byte MLDB): an N x B uint8 matrix, a frame
        of the wide kind; the match_*_hamming calls take it as they take the narrow kind."""
        d = np.ascontiguousarray(rows, dtype=np.uint8)
        if d.ndim != 2:
            raise ValueError("binary descriptors must be an N x B uint8 matrix")
        self._check(self._L.eacham_upload_descriptors_bits_wide(self._h, frame_id, d.ctypes.data, d.shape[0], d.shape[1]))

    def upload_descriptors_bits_wide_dev(self, frame_id: int, dev_ptr: int, n: int, bytes_per_row: int):
        self._check(self._L.eacham_upload_descriptors_bits_wide_dev(self._h, frame_id, C.c_void_p(dev_ptr), n, bytes_per_row))

    def match_debug_hamming_wide_pair(self, f1: int, f2: int):
        """(best, h0, h1) per row of f1: the wide sweep's own top-2 over the rows of f2 (eacham_match_debug_hamming_wide_pair)."""
        n = self.frame_rows(f1)
        best, h0, h1 = (np.zeros(max(n, 1), dtype=np.int32) for _ in range(3))
        self._check(self._L.eacham_match_debug_hamming_wide_pair(self._h, f1, f2, best.ctypes.data, h0.ctypes.data, h1.ctypes.data, n))
        return best[:n], h0[:n], h1[:n]

    def match_debug_hamming_wide(self) -> dict:
        """{batches, pairs_per_batch, sweep_launches, query_rows} of the last matching call on wide frames."""
        out = (C.c_int64 * 4)()
        self._check(self._L.eacham_match_debug_hamming_wide(self._h, out))
        return dict(zip(("batches", "pairs_per_batch", "sweep_launches", "query_rows"), (int(v) for v in out)))

    def match_pair_hamming(self, f1: int, f2: int, ratio: float = RATIO):
        """(q, t, dist) of the directed match f1 -> f2 of two binary frames: BFMatcher(NORM_HAMMING) + the ratio test."""
        cap = max(self.frame_rows(f1), 1)
        q = np.empty(cap, dtype=np.uint32)
        t = np.empty(cap, dtype=np.uint32)
        d = np.empty(cap, dtype=np.int32)
        cnt = C.c_int(0)
        self._check(self._L.eacham_match_pair_hamming(self._h, f1, f2, ratio, q.ctypes.data, t.ctypes.data, d.ctypes.data, cap, C.byref(cnt)))
        return q[:cnt.value].copy(), t[:cnt.value].copy(), d[:cnt.value].copy()

    def _ham_buffers(self, pairs, cap):
        pairs, npairs, cap, counts, offsets, q, t, _ = self._dot_buffers(pairs, cap)
        return pairs, npairs, cap, counts, offsets, q, t, np.empty(max(cap, 1), dtype=np.int32)

    def match_pairs_directed_hamming(self, ordered_pairs, ratio: float = RATIO, cap: int | None = None):
        """Every ordered pair (i, j) of the RESIDENT binary frames as one directed Hamming match, in one launch sequence.
        Returns (counts, offsets, q, t, dist): CSR over the pairs."""
        pairs, npairs, cap, counts, offsets, q, t, d = self._ham_buffers(ordered_pairs, cap)
        total = C.c_int64(0)
        self._check(self._L.eacham_match_pairs_directed_hamming(self._h, pairs.ctypes.data, npairs, ratio, counts.ctypes.data,
                                                                offsets.ctypes.data, q.ctypes.data, t.ctypes.data, d.ctypes.data, cap, C.byref(total)))
        n = total.value
        return counts, offsets, q[:n].copy(), t[:n].copy(), d[:n].copy()

    def match_all_pairs_hamming(self, pairs, ratio: float = RATIO, min_dir: int = MIN_DIRECTED, min_mutual: int = MIN_MUTUAL,
                                cap: int | None = None, stats: bool = True):
        """The mutual form (eacham_match_all_pairs_hamming). Returns (counts, offsets, q, t, dist, stats)."""
        pairs, npairs, cap, counts, offsets, q, t, d = self._ham_buffers(pairs, cap)
        st = np.zeros((npairs, 4), dtype=np.int32) if stats else None
        total = C.c_int64(0)
        self._check(self._L.eacham_match_all_pairs_hamming(
            self._h, pairs.ctypes.data, npairs, ratio, min_dir, min_mutual, counts.ctypes.data, offsets.ctypes.data,
            q.ctypes.data, t.ctypes.data, d.ctypes.data, cap, C.byref(total), st.ctypes.data if stats else None))
        n = total.value
        return counts, offsets, q[:n].copy(), t[:n].copy(), d[:n].copy(), st

    def match_all_pairs_hamming_dev(self, pairs_dev: int, npairs: int, counts_dev: int, offsets_dev: int,
                                    edges_dev: int, edge_cap: int, total_dev: int, stats_dev: int = 0, dist_dev: int = 0,
                                    ratio: float = RATIO, min_dir: int = MIN_DIRECTED, min_mutual: int = MIN_MUTUAL):
        vp = C.c_void_p
        self._check(self._L.eacham_match_all_pairs_hamming_dev(
            self._h, vp(pairs_dev), npairs, ratio, min_dir, min_mutual, vp(counts_dev), vp(offsets_dev),
            vp(edges_dev), edge_cap, vp(total_dev), vp(stats_dev) if stats_dev else None, vp(dist_dev) if dist_dev else None))

    def match_all_pairs_dev(self, pairs_dev: int, npairs: int, counts_dev: int, offsets_dev: int,
                            edges_dev: int, edge_cap: int, total_dev: int, stats_dev: int = 0,
                            ratio: float = RATIO, min_dir: int = MIN_DIRECTED, min_mutual: int = MIN_MUTUAL):
        vp = C.c_void_p
        self._check(self._L.eacham_match_all_pairs_dev(
            self._h, vp(pairs_dev), npairs, ratio, min_dir, min_mutual, vp(counts_dev), vp(offsets_dev),
            vp(edges_dev), edge_cap, vp(total_dev), vp(stats_dev) if stats_dev else None))

    # ---- profiling -------------------------------------------------------------------------
    def lmeds_batch(self, kind: str, uv1, uv2, samples, K=None):
        """eacham_lmeds_batch: LMedS two-view estimation of a list of pairs in one call (eacham_amd/lmeds.py); kind "essential",
        "homography" or "fundamental" (7-point samples on pixels, K ignored)."""
        from . import lmeds
        return lmeds.lmeds_batch(self, kind, uv1, uv2, samples, K)

    def ransac_batch(self, kind: str, uv1, uv2, samples, threshold: float, confidence: float, stage1: int = 0, K=None):
        """eacham_ransac_batch: threshold RANSAC two-view estimation of a list of pairs in one call (eacham_amd/ransac.py)."""
        from . import ransac
        return ransac.ransac_batch(self, kind, uv1, uv2, samples, threshold, confidence, stage1, K)

    def two_view_batch(self, uv1, uv2, K, rules, transforms, max_repr_error: float, min_tri_angle: float, in_mask=None,
                       distance_thresh: float = 50.0, min_solution_matches: int = 20):
        """eacham_two_view_batch: candidate poses -> the winner and its kept points, for a list of pairs in one call (eacham_amd/twoview.py)."""
        from . import twoview
        return twoview.two_view_batch(self, uv1, uv2, K, rules, transforms, max_repr_error, min_tri_angle, in_mask, distance_thresh,
                                      min_solution_matches)

    def pnp_hypotheses_batch(self, X, uv, K, samples, threshold: float = 16.0, want_models: bool = True):
        """eacham_pnp_hypotheses_batch: one PnP RANSAC round (EPnP per sample, its inlier count) for a list of problems (eacham_amd/pnp.py)."""
        from . import pnp
        return pnp.pnp_hypotheses_batch(self, X, uv, K, samples, threshold, want_models)

    def pnp_refit_batch(self, X, uv, K, models, has_model, threshold: float = 16.0):
        """eacham_pnp_refit_batch: the inlier mask of one model per problem and EPnP on its inliers, for a list of problems (eacham_amd/pnp.py)."""
        from . import pnp
        return pnp.pnp_refit_batch(self, X, uv, K, models, has_model, threshold)

    def pnp_refine_batch(self, X, uv, K, poses, has_pose, use_masks=None, max_tries: int = 20, threshold: float = 16.0,
                         want_recount: bool = True):
        """eacham_pnp_refine_batch: Levenberg-Marquardt on the reprojection error of one pose per problem over the rows its mask names,
        and the recount under the refined pose, for a list of problems in one launch (eacham_amd/pnp.py)."""
        from . import pnp
        return pnp.pnp_refine_batch(self, X, uv, K, poses, has_pose, use_masks, max_tries, threshold, want_recount)

    def refine_tracks(self, transforms, track_ptr, obs_frame, obs_uv, K, points, has_point, use_mask=None, max_tries: int = 20,
                      max_repr_error: float = 4.0, want_recount: bool = True):
        """eacham_triangulate_refine_tracks: Levenberg-Marquardt on the reprojection error of one 3-D point per track over the
        observations its mask names, the cameras fixed, and the recount at the refined point, for a list of tracks in one launch
        (eacham_amd/triangulate.py)."""
        from . import triangulate
        return triangulate.refine_tracks(self, transforms, track_ptr, obs_frame, obs_uv, K, points, has_point, use_mask, max_tries,
                                         max_repr_error, want_recount)

    def solve_p3p(self, X, uv, K, samples, want_candidates: bool = True):
        """eacham_solve_p3p: P3P on every row of `samples` (4 point indices per row: three solve, the fourth picks) (eacham_amd/pnp.py)."""
        from . import pnp
        return pnp.solve_p3p(self, X, uv, K, samples, want_candidates)

    def pnp_hypotheses_batch_p3p(self, X, uv, K, samples, threshold: float = 16.0, want_models: bool = True):
        """eacham_pnp_hypotheses_batch_p3p: one PnP RANSAC round on four-point samples (P3P per sample, its inlier count) for a list of
        problems, one launch (eacham_amd/pnp.py)."""
        from . import pnp
        return pnp.pnp_hypotheses_batch_p3p(self, X, uv, K, samples, threshold, want_models)

    def profile_enable(self, on: bool = True):
        self._check(self._L.eacham_profile_enable(self._h, int(on)))

    def profile_reset(self):
        self._check(self._L.eacham_profile_reset(self._h))

    def profile_get(self, kernel_id: int):
        n, ms = C.c_int64(0), C.c_double(0.0)
        self._check(self._L.eacham_profile_get(self._h, kernel_id, C.byref(n), C.byref(ms)))
        return n.value, ms.value


class FeatureMatcherHip:
    """Drop-in shape of eacham::FeatureMatcherFlann (FeatureMatcherFlann.h:11-25).

    `Match(descriptor1, descriptor2)` takes two N x D fp32 matrices (cv::Mat CV_32F layout) and
    returns {queryIdx: trainIdx}. As in the reference, the constructor's `inliersRatio` is kept
    but the ratio test uses the literal 0.8 unless `ratio` is given explicitly.
    """

    def __init__(self, inliersRatio: float = 0.8, ratio: float = RATIO, context: HipContext | None = None):
        self.inliersRatio = inliersRatio
        self.ratio = ratio
        self.ctx = context or HipContext()
        self._f32 = False  # the first non-integer frame switches the instance to the fp32 path for good

    def Match(self, descriptor1: np.ndarray, descriptor2: np.ndarray) -> dict:
        """Two frame slots (0 and 1) of the context's store are rewritten per call; the store is cleared only
        when the descriptor kind changes. (The C++ adapter include/eacham/FeatureMatcherHip.hpp additionally
        caches uploads by buffer address and combines concurrent callers; numpy temporaries reuse addresses too
        freely for that to be safe here, and this class only drives tests.)"""
        if not self._f32:
            try:  # SIFT-style integers: exact int8 path
                self.ctx.upload_descriptors(0, descriptor1)
                self.ctx.upload_descriptors(1, descriptor2)
            except capi.EachamError as e:
                if e.code not in (capi.ERR_NOT_INTEGER, capi.ERR_UNSUPPORTED):
                    raise
                self._f32 = True  # other floats: fp32 MFMA path; all resident frames must be of one kind
                self.ctx.clear_descriptors()
        if self._f32:
            self.ctx.upload_descriptors_f32(0, descriptor1)
            self.ctx.upload_descriptors_f32(1, descriptor2)
        q, t = self.ctx.match_pair(0, 1, self.ratio)
        return dict(zip(q.tolist(), t.tolist()))

    def MatchPairs(self, frames, ordered_pairs) -> list:
        """eacham_match_pairs_directed: every (i, j) of `ordered_pairs` is one Match(frames[i], frames[j])."""
        return self.ctx.match_pairs_directed(frames, ordered_pairs, self.ratio, f32=self._f32)


class FeatureMatcherDotHip:
    """Mirror of eacham::hip::FeatureMatcherDotHip (include/eacham/FeatureMatcherHip.hpp): float descriptors matched by
    dot-product similarity. `Match(d1, d2)` returns {queryIdx: trainIdx}: with `mutual` the one-to-one matches of the pair
    (what LightGlue's matches0 are), without it the directed match; `LastScores()` gives {queryIdx: similarity} of that call."""

    def __init__(self, minScore: float = MIN_SCORE, mutual: bool = True, context: HipContext | None = None):
        self.minScore = minScore
        self.mutual = mutual
        self.ctx = context or HipContext()
        self._scores = {}

    def Match(self, descriptor1: np.ndarray, descriptor2: np.ndarray) -> dict:
        self.ctx.clear_descriptors()
        self.ctx.upload_descriptors_f32(0, descriptor1)
        self.ctx.upload_descriptors_f32(1, descriptor2)
        if self.mutual:
            _, _, q, t, s, _ = self.ctx.match_all_pairs_dot([[0, 1]], self.minScore, 0, -1, stats=False)
        else:
            q, t, s = self.ctx.match_pair_dot(0, 1, self.minScore)
        self._scores = dict(zip(q.tolist(), s.tolist()))
        return dict(zip(q.tolist(), t.tolist()))

    def LastScores(self) -> dict:
        return self._scores


class FeatureMatcherHammingHip:
    """Mirror of eacham::hip::FeatureMatcherHammingHip (include/eacham/FeatureMatcherHip.hpp): packed binary descriptors
    (N x B uint8, cv::Mat CV_8U layout, B up to 64) matched under Hamming distance. `Match(d1, d2)` returns {queryIdx: trainIdx}: the
    directed ratio-test match, or with `mutual` the pair's one-to-one matches; `LastDistances()` gives
    {queryIdx: Hamming distance} of that call."""

    def __init__(self, ratio: float = RATIO, mutual: bool = False, context: HipContext | None = None):
        self.ratio = ratio
        self.mutual = mutual
        self.ctx = context or HipContext()
        self._dist = {}

    def Match(self, descriptor1: np.ndarray, descriptor2: np.ndarray) -> dict:
        self.ctx.clear_descriptors()
        # rows of 33..64 bytes are frames of the wide kind; up to 32 bytes the narrow kind, as before
        wide = max(np.shape(descriptor1)[-1], np.shape(descriptor2)[-1]) > 32
        upload = self.ctx.upload_descriptors_bits_wide if wide else self.ctx.upload_descriptors_bits
        upload(0, descriptor1)
        upload(1, descriptor2)
        if self.mutual:
            _, _, q, t, d, _ = self.ctx.match_all_pairs_hamming([[0, 1]], self.ratio, 0, -1, stats=False)
        else:
            q, t, d = self.ctx.match_pair_hamming(0, 1, self.ratio)
        self._dist = dict(zip(q.tolist(), d.tolist()))
        return dict(zip(q.tolist(), t.tolist()))

    def LastDistances(self) -> dict:
        return self._dist
