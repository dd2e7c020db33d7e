"""Host-side mirror of the track-building stage (eacham_tracks_build / eacham_graph_tracks, csrc/tracks.hip).

  build_tracks(ctx, n_frames, pairs, counts, offsets, q, t, keypoints_per_frame, ...)  ->  Tracks
  ResidentGraph.tracks(...)                                                            ->  Tracks   (eacham_amd/graph.py)

The match graph is the wire format `HipContext.match_all_pairs` returns; `keep` is an optional byte per match (the inlier masks
of the LMedS batch, concatenated in pair order). A track is a connected component of kept matches over (frame, keypoint) nodes
with at least min_len nodes; tracks come out ordered by their smallest node id, observations frame-major then by keypoint.
`Tracks.obs_frame` and `Tracks.track_ptr32()` go straight into `triangulate.triangulate_tracks`.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from .matcher import HipContext

CONFLICT_FLAG, CONFLICT_DROP = 0, 1


@dataclass
class Tracks:
    track_ptr: np.ndarray    # int64 [n_tracks + 1]
    obs_frame: np.ndarray    # uint32 [n_obs]
    obs_kp: np.ndarray       # uint32 [n_obs]  keypoint index inside its frame
    flags: np.ndarray        # uint8 [n_tracks]  bit 0: two keypoints of one frame
    node_track: np.ndarray   # int32 [total keypoints]  -1 = in no track

    @property
    def n_tracks(self) -> int:
        return int(self.flags.size)

    def track_ptr32(self) -> np.ndarray:
        return self.track_ptr.astype(np.int32)

    def gather_pixels(self, keypoints_per_frame) -> np.ndarray:
        """obs_uv [n_obs, 2] float64 from per-frame keypoint arrays [n_f, 2]."""
        uv = np.zeros((self.obs_frame.size, 2), dtype=np.float64)
        for f in np.unique(self.obs_frame):
            m = self.obs_frame == f
            uv[m] = np.asarray(keypoints_per_frame[int(f)], dtype=np.float64)[self.obs_kp[m]]
        return uv


def kp_offsets_of(keypoints_per_frame) -> np.ndarray:
    kpo = np.zeros(len(keypoints_per_frame) + 1, dtype=np.int64)
    kpo[1:] = np.cumsum(np.asarray(keypoints_per_frame, dtype=np.int64))
    return kpo


def output_bounds(n_nodes: int, n_matches: int) -> tuple[int, int]:
    """(cap_obs, cap_tracks) that always suffice: n_obs <= min(nodes, 2 x matches), n_tracks <= n_obs / 2."""
    cap_obs = int(min(n_nodes, 2 * n_matches))
    return cap_obs, cap_obs // 2


class _Out:
    def __init__(self, n_nodes: int, cap_obs: int, cap_tracks: int):
        self.cap_obs, self.cap_tracks = int(cap_obs), int(cap_tracks)
        self.n_tracks, self.n_obs = C.c_int32(0), C.c_int64(0)
        self.track_ptr = np.zeros(self.cap_tracks + 1, dtype=np.int64)
        self.obs_frame = np.zeros(max(self.cap_obs, 1), dtype=np.uint32)
        self.obs_kp = np.zeros(max(self.cap_obs, 1), dtype=np.uint32)
        self.flags = np.zeros(max(self.cap_tracks, 1), dtype=np.uint8)
        self.node_track = np.zeros(max(int(n_nodes), 1), dtype=np.int32)
        self.n_nodes = int(n_nodes)

    def args(self):
        return (self.cap_obs, self.cap_tracks, C.byref(self.n_tracks), C.byref(self.n_obs), self.track_ptr.ctypes.data,
                self.obs_frame.ctypes.data, self.obs_kp.ctypes.data, self.flags.ctypes.data, self.node_track.ctypes.data)

    def result(self) -> Tracks:
        nt, no = int(self.n_tracks.value), int(self.n_obs.value)
        return Tracks(self.track_ptr[:nt + 1].copy(), self.obs_frame[:no].copy(), self.obs_kp[:no].copy(), self.flags[:nt].copy(),
                      self.node_track[:self.n_nodes].copy())


def build_tracks(ctx: HipContext, n_frames: int, pairs, counts, offsets, q, t, keypoints_per_frame, keep=None, min_len: int = 2,
                 conflict_policy: int = CONFLICT_FLAG, cap_obs: int | None = None, cap_tracks: int | None = None) -> Tracks:
    """eacham_tracks_build. cap_obs / cap_tracks default to the bounds that always suffice; a smaller one that does not raises
    EachamError with code ERR_CAPACITY."""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    q = np.ascontiguousarray(q, dtype=np.uint32)
    t = np.ascontiguousarray(t, dtype=np.uint32)
    kpo = kp_offsets_of(keypoints_per_frame)
    if kpo.size != n_frames + 1:
        raise ValueError("keypoints_per_frame must have n_frames entries")
    k = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    if k is not None and k.size != q.size:
        raise ValueError("keep must have one byte per match")
    bound_obs, bound_tracks = output_bounds(int(kpo[-1]), int(counts.sum()))
    out = _Out(int(kpo[-1]), bound_obs if cap_obs is None else cap_obs, bound_tracks if cap_tracks is None else cap_tracks)
    ctx._check(ctx._L.eacham_tracks_build(ctx.handle, n_frames, pairs.ctypes.data, pairs.shape[0], counts.ctypes.data, offsets.ctypes.data,
                                          q.ctypes.data, t.ctypes.data, kpo.ctypes.data, None if k is None else k.ctypes.data,
                                          int(min_len), int(conflict_policy), *out.args()))
    return out.result()


def graph_tracks(ctx: HipContext, graph_handle, n_nodes: int, n_matches: int, keep=None, min_len: int = 2,
                 conflict_policy: int = CONFLICT_FLAG, cap_obs: int | None = None, cap_tracks: int | None = None) -> Tracks:
    """eacham_graph_tracks on a resident graph (ResidentGraph.tracks calls this)."""
    k = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    bound_obs, bound_tracks = output_bounds(n_nodes, n_matches)
    out = _Out(n_nodes, bound_obs if cap_obs is None else cap_obs, bound_tracks if cap_tracks is None else cap_tracks)
    ctx._check(ctx._L.eacham_graph_tracks(graph_handle, None if k is None else k.ctypes.data, int(min_len), int(conflict_policy), *out.args()))
    return out.result()


def graph_tracks_verified(ctx: HipContext, graph_handle, n_nodes: int, n_matches: int, min_len: int = 2, conflict_policy: int = CONFLICT_FLAG,
                          cap_obs: int | None = None, cap_tracks: int | None = None) -> Tracks:
    """eacham_graph_tracks_verified: the tracks of a resident graph under the mask its last verify(retain=True) left on the device
    (ResidentGraph.tracks_verified calls this)."""
    bound_obs, bound_tracks = output_bounds(n_nodes, n_matches)
    out = _Out(n_nodes, bound_obs if cap_obs is None else cap_obs, bound_tracks if cap_tracks is None else cap_tracks)
    ctx._check(ctx._L.eacham_graph_tracks_verified(graph_handle, int(min_len), int(conflict_policy), *out.args()))
    return out.result()


def last_call_info(ctx: HipContext) -> dict:
    """eacham_tracks_debug_last: rounds of the last track-building call on this context, their cap, its read-backs of status words,
    and the device time by HIP events (-1 unless profiling is enabled on the context)."""
    r, cap, rb, ms = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_float(-1.0)
    ctx._check(ctx._L.eacham_tracks_debug_last(ctx.handle, C.byref(r), C.byref(cap), C.byref(rb), C.byref(ms)))
    return {"rounds": int(r.value), "round_cap": int(cap.value), "readbacks": int(rb.value), "kernel_ms": float(ms.value)}


__all__ = ["Tracks", "build_tracks", "graph_tracks", "graph_tracks_verified", "last_call_info", "output_bounds", "kp_offsets_of", "CONFLICT_FLAG", "CONFLICT_DROP"]
