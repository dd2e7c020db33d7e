"""Scenes of the screened dot-product matcher (eacham_match_all_pairs_dot_screened) and a CPU model of its fp16 sweep, shared by
the CPU test (what each scene proves: which branch it reaches, that the input-rounding part of the bound holds) and the GPU test.

The model restates eacham_amd/csrc/matcher_dot16.hip with numpy's float16: the image flushes |x| < 2^-14 to zero and rounds to
nearest even; N' >= |x|_2 + 2^-3 sqrt(flushed elements); E_row = kappa N'_q max_t N'_t, kappa = 2^-10 + (D + 16) 2^-22 with D the
padded dimension. The model's coarse score is the float64 dot product of the images (the device accumulates in fp32: the two
differ by the MFMA term of the bound, so counts of open rows may differ by a row near a boundary; branches do not)."""
from __future__ import annotations

import numpy as np

import dot_cases as DC
import dot_reference as R

NEG_INF = float("-inf")
EPS0 = 2.0 ** -100


def padded_dim(dim):
    return 64 if dim <= 64 else (128 if dim <= 128 else 256)


def kappa(dim):
    return 2.0 ** -10 + (padded_dim(dim) + 16) * 2.0 ** -22


def screenable(X):
    return bool(np.all(np.abs(X) <= 65504.0))          # False for NaN, Inf and values beyond the fp16 range


def image16(X):
    """(image as float64, N' per row as float64 upper bounds, flushed elements per row)."""
    X = np.asarray(X, np.float32)
    tiny = (np.abs(X) < 2.0 ** -14) & (X != 0)
    with np.errstate(over="ignore"):
        img = np.where(tiny, np.float32(0), X).astype(np.float16).astype(np.float64)
    flushed = tiny.sum(axis=1)
    n = np.sqrt((X.astype(np.float64) ** 2).sum(axis=1)) * (1 + 2.0 ** -40) + 0.125 * np.sqrt(flushed)
    return img, n, flushed


def coarse(A, B):
    """(s~ model n1 x n2 float64, row_E, col_E)."""
    ia, na, _ = image16(A)
    ib, nb, _ = image16(B)
    k = kappa(A.shape[1] if A.shape[1] else B.shape[1])
    row_E = k * na * (nb.max() if len(nb) else 0.0) + EPS0
    col_E = k * nb * (na.max() if len(na) else 0.0) + EPS0
    return ia @ ib.T, row_E, col_E


def classify(S, E, min_score):
    """Per row of S: 0 dead, 1 settled, 2 open — the rule of dot_screen_classify_kernel. Also the coarse arg-max."""
    n1, n2 = S.shape
    state = np.zeros(n1, np.int32)
    best = np.full(n1, -1, np.int64)
    if n2 == 0:
        return state, best
    best = S.argmax(axis=1)                                   # first maximum: the lower index
    s1 = S[np.arange(n1), best]
    if n2 > 1:
        T = S.copy()
        T[np.arange(n1), best] = NEG_INF
        s2 = T.max(axis=1)
    else:
        s2 = np.full(n1, NEG_INF)
    dead = s1 + E <= min_score
    settled = ~dead & (s2 > NEG_INF) & (s1 - s2 > 2 * E)
    state[:] = np.where(dead, 0, np.where(settled, 1, 2))
    return state, best


def exact_scores(A, B):
    """s(q, t) of the reference for every (q, t): n2 calls of its arg-max against a one-row train frame."""
    out = np.empty((A.shape[0], B.shape[0]), np.float32)
    for t in range(B.shape[0]):
        out[:, t] = R.argmax(A, B[t:t + 1])[1]
    return out


def _bump(x, up):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf), dtype=np.float32)


def near_duplicates():
    """(A, B, rows): B = a d64 frame + three appended copies of rows of it. For the query rows `rows` = (higher, lower, tie):
    the copy of the first one's best row differs by ONE fp32 ulp in one element and scores higher (fp32 picks the copy, the higher
    index), the second's copy scores lower by one ulp of one element (fp32 keeps the lower index), the third's copy is identical
    (the lower index wins the tie). The rows are mutual matches above MIN_SCORE; the elements are searched so that the reference's chain really changes."""
    fr = DC.scene("d64")
    A, B0 = fr[0], fr[1]
    best, _ = R.argmax(A, B0)
    mutual = [int(q) for q in R.match_mutual(A, B0, DC.MIN_SCORE, 0, -1)[0]]      # rows whose match reaches the output
    picked, extra = [], []
    for want_higher in (True, False):
        for q in mutual:
            if q in picked:
                continue
            t = int(best[q])
            base = R.argmax(A[q:q + 1], B0[t:t + 1])[1][0]
            found = None
            for k in np.argsort(-np.abs(A[q] * B0[t])):
                c = B0[t].copy()
                c[k] = _bump(c[k], (A[q, k] > 0) == want_higher)
                s = R.argmax(A[q:q + 1], c[None])[1][0]
                if (s > base) if want_higher else (s < base):
                    found = c
                    break
            if found is not None:
                picked.append(q)
                extra.append(found)
                break
    q_tie = next(q for q in mutual if q not in picked)
    picked.append(q_tie)
    extra.append(B0[int(best[q_tie])].copy())
    B = np.ascontiguousarray(np.concatenate([B0, np.stack(extra)]), np.float32)
    return A, B, tuple(picked)


def fallback_frames():
    """Four d64 frames: 1 holds a value beyond the fp16 range and a -Inf, 2 a NaN; 0 and 3 are clean (their pair is screened)."""
    fr = [f.copy() for f in DC.scene("d64")]
    fr[1][3, 5] = 1.0e5
    fr[1][40, 0] = -np.inf
    fr[2][7, 2] = np.nan
    return fr


def tiny_value_frames():
    """d64 frames with values below 2^-14 (fp16's smallest normal): single elements, and one whole row scaled by 2^-18."""
    fr = [f.copy() for f in DC.scene("d64")[:3]]
    for f, X in enumerate(fr):
        X[5 + f, 3] = 1.0e-5
        X[9, 10 + f] = -3.0e-6
        X[11, 0] = 1.0e-8
        X[20 + f, 7] = 2.0 ** -14          # the smallest normal itself: kept
    fr[0][30] *= 2.0 ** -18
    fr[1][31] *= 2.0 ** -18
    return fr


def tiny_shapes():
    """Train frames of 0, 1 and 2 rows next to query frames of 33 and 70 rows (one row past a tile; a padded tile behind)."""
    A = DC.scene("d64")[0]
    return [A[:33].copy(), A[:70].copy(), A[5:6].copy(), A[5:7].copy(), np.zeros((0, A.shape[1]), np.float32)]


def all_ordered(n):
    return DC.ordered_pairs(n)


# name -> (frames, pairs); every scene is run by the GPU test at min_score 0.5 and -inf, thresholds 0/-1 and 30/30
def scenes():
    out = {}
    for name in sorted(DC.SCENES):
        fr = DC.scene(name)
        out["a_" + name] = (fr, all_ordered(len(fr)))
    A, B, _ = near_duplicates()
    out["b_near_duplicates"] = ([A, B], np.array([[0, 1], [1, 0]], np.int32))
    fr = fallback_frames()
    out["c_fallback"] = (fr, all_ordered(len(fr)))
    fr = tiny_value_frames()
    out["d_tiny_values"] = (fr, all_ordered(len(fr)))
    a, b = DC.negative_pair()
    out["e_negative"] = ([a, b], np.array([[0, 1], [1, 0]], np.int32))
    fr = tiny_shapes()
    out["f_tiny_shapes"] = (fr, all_ordered(len(fr)))
    return out
