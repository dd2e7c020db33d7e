"""CPU reference of the Hamming matcher, numpy only. Test infrastructure only.

What cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) and the ratio test of FeatureMatcherFlann.cpp:23 compute on packed binary
rows: the distance is the number of differing bits (an int stored as float), the two nearest train rows of every query row
with ties to the lower index, and q -> t0 kept iff (double)((float)h0 / (float)h1) < ratio. The mutual form is the pair loop of
apps/sfm/main.cpp:111-146. Return shapes follow tests/dot_reference.py, with int32 distances in the place of the scores."""
from __future__ import annotations

import numpy as np

POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.uint8)   # popcount by table


def _u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a if a.ndim == 2 else a.reshape(0, 0)


def popcount(rows):
    """Set bits per row of an N x B uint8 matrix."""
    return POPCOUNT[_u8(rows)].sum(axis=1, dtype=np.int32)


def distances(A, B):
    """n1 x n2 int32 Hamming distances of the rows of A against the rows of B."""
    A, B = _u8(A), _u8(B)
    out = np.zeros((A.shape[0], B.shape[0]), np.int32)
    if out.size == 0:
        return out
    step = max(1, (1 << 24) // max(B.size, 1))
    for i in range(0, A.shape[0], step):
        out[i:i + step] = POPCOUNT[A[i:i + step, None, :] ^ B[None, :, :]].sum(axis=2, dtype=np.int32)
    return out


def embed(rows):
    """The rows as the matcher stores them: one value 255 b per bit b (np.unpackbits' order), float32."""
    rows = _u8(rows)
    return np.unpackbits(rows, axis=1).astype(np.float32) * np.float32(255.0)


def ratio_pass(h0, h1, ratio):
    """(double)((float)h0 / (float)h1) < ratio, elementwise; 0/0 is NaN and fails."""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.asarray(h0).astype(np.float32) / np.asarray(h1).astype(np.float32)
    return q.astype(np.float64) < float(ratio)


def top2(D):
    """(best, h0, h1) per row of a distance matrix with at least two columns: the lowest index of the minimum, the minimum, and
    the smallest distance over the other columns."""
    best = np.argmin(D, axis=1)                       # first occurrence = the lower index on a tie
    rows = np.arange(D.shape[0])
    h0 = D[rows, best]
    rest = D.copy()
    rest[rows, best] = np.iinfo(np.int32).max
    return best.astype(np.int64), h0, rest.min(axis=1)


def directed_from(D, ratio):
    """(q, t, dist) of the directed match from its distance matrix, sorted by q; empty when there are fewer than two train rows."""
    if D.shape[0] == 0 or D.shape[1] < 2:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.int32)
    best, h0, h1 = top2(D)
    ok = ratio_pass(h0, h1, ratio)
    return np.nonzero(ok)[0].astype(np.uint32), best[ok].astype(np.uint32), h0[ok].astype(np.int32)


def match_directed(A, B, ratio):
    return directed_from(distances(A, B), ratio)


def mutual_from(D, ratio, min_dir, min_mutual):
    """(q, t, dist, stats): the pair's emitted matches (empty unless it is an edge) and {|m12|, |m21|, |mutual|, edge}."""
    q12, t12, d12 = directed_from(D, ratio)
    q21, t21, _ = directed_from(np.ascontiguousarray(D.T), ratio)
    back = np.full(D.shape[1], -1, np.int64)
    back[q21] = t21
    keep = back[t12] == q12 if len(q12) else np.zeros(0, bool)
    n_mut = int(keep.sum())
    edge = len(q12) >= min_dir and len(q21) >= min_dir and n_mut > min_mutual
    stats = np.array([len(q12), len(q21), n_mut, int(edge)], np.int32)
    if not edge:
        keep = np.zeros(len(q12), bool)
    return q12[keep], t12[keep], d12[keep], stats


def match_mutual(A, B, ratio, min_dir, min_mutual):
    return mutual_from(distances(A, B), ratio, min_dir, min_mutual)


def _csr(per_pair):
    counts = np.array([len(r[0]) for r in per_pair], np.int32)
    offsets = np.zeros(len(per_pair) + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    cat = lambda k, dt: np.concatenate([r[k] for r in per_pair]).astype(dt) if per_pair else np.zeros(0, dt)  # noqa: E731
    return counts, offsets, cat(0, np.uint32), cat(1, np.uint32), cat(2, np.int32)


class Scene:
    """The frames of a scene with their distance matrices computed once and shared by every form."""

    def __init__(self, descs):
        self.descs = [_u8(d) for d in descs]
        self._D = {}

    def D(self, a, b):
        a, b = int(a), int(b)
        if (a, b) not in self._D:
            self._D[(a, b)] = self._D[(b, a)].T if (b, a) in self._D else distances(self.descs[a], self.descs[b])
        return self._D[(a, b)]

    def match_pairs_directed(self, ordered_pairs, ratio):
        """(counts, offsets, q, t, dist): CSR over the ordered pairs."""
        pairs = np.asarray(ordered_pairs, np.int32).reshape(-1, 2)
        return _csr([directed_from(self.D(a, b), ratio) for a, b in pairs])

    def match_all_pairs(self, pairs, ratio, min_dir, min_mutual):
        """(counts, offsets, q, t, dist, stats): CSR over the pairs in the form of eacham_match_all_pairs_hamming."""
        pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        res = [mutual_from(self.D(a, b), ratio, min_dir, min_mutual) for a, b in pairs]
        stats = np.array([r[3] for r in res], np.int32).reshape(-1, 4)
        return (*_csr(res), stats)


def match_pairs_directed(descs, ordered_pairs, ratio):
    return Scene(descs).match_pairs_directed(ordered_pairs, ratio)


def match_all_pairs(descs, pairs, ratio, min_dir, min_mutual):
    return Scene(descs).match_all_pairs(pairs, ratio, min_dir, min_mutual)
