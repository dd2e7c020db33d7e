"""A plain, sequential statement of guided matching (include/eacham_hip.h: eacham_match_guided) — test infrastructure.

The gate is the CPU scorers' error on the n1 x n2 expanded correspondences (oracle_api.score_hypotheses for the essential and
homography kinds, fundamental_reference.score_hypotheses for the fundamental kind: what tests/ransac_reference.py counts
inliers with), distances are int64, the ratio predicate is np_reference.directed's. One decision per line.
"""
import numpy as np

import fundamental_reference as FR
import np_reference as NR
import oracle_api as O


def errors(kind, xy1, xy2, model, K):
    """err[q, t] (float32) of the correspondence xy1[q] <-> xy2[t] under `model`, as eacham_score_hypotheses returns it."""
    xy1, xy2 = np.asarray(xy1, np.float64).reshape(-1, 2), np.asarray(xy2, np.float64).reshape(-1, 2)
    n1, n2 = len(xy1), len(xy2)
    if n1 == 0 or n2 == 0:
        return np.zeros((n1, n2), np.float32)
    a, b = np.repeat(xy1, n2, axis=0), np.tile(xy2, (n1, 1))
    model = np.asarray(model, np.float64).reshape(1, 9)
    if kind == "fundamental":
        err = FR.score_hypotheses(a, b, model, 0.0)[0]
    else:
        err = O.score_hypotheses(kind, a, b, model, K, 0.0)[0]
    return err[0].reshape(n1, n2)


def admissible(kind, xy1, xy2, model, K, max_error):
    """The pair's one bipartite mask [n1, n2]."""
    err = errors(kind, xy1, xy2, model, K)
    if not np.any(np.asarray(model, np.float64) != 0):          # the estimators' "none" record: nothing is admissible, by rule
        return np.zeros(err.shape, bool)
    with np.errstate(invalid="ignore"):
        return err <= np.float32(max_error)                     # a NaN error is not admissible


def passes(d0, d1, ratio):
    """eacham_match_pair's predicate on two squared distances (np_reference.directed's lines)."""
    s0, s1 = np.sqrt(np.float32(d0)), np.sqrt(np.float32(d1))
    with np.errstate(divide="ignore", invalid="ignore"):
        quot = np.float32(s0 / s1)
    return bool(np.float64(quot) < ratio)                       # 0 / 0 = NaN: rejected


def directed(D, mask, ratio, max_d2):
    """{q: (t, d2)} over the rows of D [n1, n2] (int64) under mask [n1, n2]."""
    out = {}
    for q in range(D.shape[0]):
        cand = np.nonzero(mask[q])[0]
        if len(cand) == 0:
            continue                                            # none admissible: no match
        order = cand[np.argsort(D[q, cand], kind="stable")]     # ties -> the lower train index
        t0 = int(order[0])
        d0 = int(D[q, t0])
        if max_d2 > 0 and d0 > max_d2:
            continue
        if len(cand) >= 2 and not passes(d0, int(D[q, order[1]]), ratio):
            continue                                            # (exactly one: the runner-up counts as +inf, matched)
        out[q] = (t0, d0)
    return out


def guided_pair(kind, A, B, xy1, xy2, model, K, max_error, ratio=0.8, max_d2=0, cross_check=True):
    """One pair: (q, t, d2, stats = [|m12|, |m21|, |result|]); |m21| = 0 without the cross-check (not computed)."""
    n1, n2 = len(A), len(B)
    D = NR.sq_dists(A, B) if n1 and n2 else np.zeros((n1, n2), np.int64)
    mask = admissible(kind, xy1, xy2, model, K, max_error)
    m12 = directed(D, mask, ratio, max_d2)
    keep, m21 = m12, {}
    if cross_check:
        m21 = directed(D.T, mask.T, ratio, max_d2)
        keep = {q: v for q, v in m12.items() if m21.get(v[0], (-1, 0))[0] == q}
    qs = sorted(keep)
    q = np.array(qs, dtype=np.uint32)
    t = np.array([keep[k][0] for k in qs], dtype=np.uint32)
    d2 = np.array([keep[k][1] for k in qs], dtype=np.uint32)
    return q, t, d2, np.array([len(m12), len(m21), len(keep)], dtype=np.int32)


def guided(kind, descs, xys, pairs, models, K, max_error, ratio=0.8, max_d2=0, cross_check=True):
    """The whole call: (counts, offsets, q, t, d2, stats [npairs, 3]) in the CSR form of the C-ABI."""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    models = np.asarray(models, np.float64).reshape(-1, 9)
    res = [guided_pair(kind, descs[f1], descs[f2], xys[f1], xys[f2], models[p], K, max_error, ratio, max_d2, cross_check)
           for p, (f1, f2) in enumerate(pairs.tolist())]
    counts = np.array([len(r[0]) for r in res], dtype=np.int32)
    offsets = np.zeros(len(res) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    cat = lambda i: np.concatenate([r[i] for r in res]).astype(np.uint32) if res else np.zeros(0, np.uint32)   # noqa: E731
    return counts, offsets, cat(0), cat(1), cat(2), np.array([r[3] for r in res], dtype=np.int32).reshape(-1, 3)
