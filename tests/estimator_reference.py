"""A plain, sequential statement of the four estimator loops of include/eacham/TwoViewHip.hpp and PnPHip.hpp (test
infrastructure; tests/test_estimators.py holds the headers to it).

Written from the OpenCV behaviour the headers cite — RANSACUpdateNumIters, LMeDSPointSetRegistrator::run and
RANSACPointSetRegistrator::run (ptsetreg.cpp), the refinement at the end of cv::findHomography (fundam.cpp), cv::recoverPose
(five-point.cpp) — one sample at a time, one candidate at a time, no batches. The arithmetic underneath (minimal solvers,
per-point errors, medians, triangulation) is the CPU oracle's (oracle_api), which the GPU tests hold the device library to bit
for bit; the samples are handed in, so every discrete decision below is fully determined.
"""
import math

import numpy as np

import oracle_api as O

DBL_MIN = np.finfo(np.float64).tiny
LD = np.longdouble


def lround(x):
    """C lround: to nearest, halves away from zero."""
    f = math.floor(abs(x))
    return int(math.copysign(f + (1 if abs(x) - f >= 0.5 else 0), x))


def update_num_iters(p, ep, m, max_iters):
    """RANSACUpdateNumIters: the number of samples after which one of m inliers has been drawn with probability p when a share
    ep of the data are outliers, at most max_iters (the header rounds with lround, as stated in tests/test_estimators.py)."""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - (1.0 - ep) ** m
    if denom < DBL_MIN:
        return 0
    num, denom = math.log(num), math.log(denom)
    return max_iters if denom >= 0 or -num >= max_iters * (-denom) else lround(num / denom)


def lmeds_iterations(confidence, m, max_iters):
    """LMeDSPointSetRegistrator::run fixes its count up front: an outlier share of 0.45 is assumed, at least 3, at most maxIters."""
    return min(max_iters, max(update_num_iters(confidence, 0.45, m, max_iters), 3))


def lmeds(kind, uv1, uv2, K4, samples):
    """Least median of squares over the given minimal samples. kind: "essential" (5 points, up to 10 models per sample) or
    "homography" (4 points, one). Returns a dict: ok, and when ok: sample, root (where the winner came from), candidate (its
    place when every model of every sample is counted in order), candidates, model, median (float32), sigma, threshold
    (float32), mask, inliers."""
    solver, m = {"essential": ("essential5", 5), "homography": ("homography4", 4)}[kind]
    uv1, uv2 = np.asarray(uv1, float).reshape(-1, 2), np.asarray(uv2, float).reshape(-1, 2)
    n = len(uv1)
    samples = np.asarray(samples, np.int32).reshape(-1, m)
    out = {"ok": False, "iterations": len(samples) if n >= m else 0, "candidates": 0}
    if n < m:
        return out
    best, seen = None, 0
    for s, sample in enumerate(samples):
        models, counts = O.solve_minimal(solver, uv1, uv2, sample[None], K4)
        for r in range(int(counts[0])):
            _, _, med = O.score_hypotheses(kind, uv1, uv2, models[0, r], K4, 0.0)
            if not np.isnan(med[0]) and (best is None or med[0] < best["median"]):      # strictly smaller: the first one stays
                best = {"sample": s, "root": r, "candidate": seen, "model": models[0, r].copy(), "median": med[0]}
            seen += 1
    out["candidates"] = seen
    if best is None:
        return out
    # sigma = 2.5 * 1.4826 * (1 + 5 / (n - m)) * sqrt(median), floored at 0.001, squared: the bound on the (squared) errors
    sigma = 2.5 * 1.4826 * (1.0 + 5.0 / max(n - m, 1)) * math.sqrt(float(best["median"]))
    sigma = max(sigma, 0.001)
    thr = np.float32(sigma * sigma)
    err, cnt, _ = O.score_hypotheses(kind, uv1, uv2, best["model"], K4, float(thr))
    out.update(best, ok=True, sigma=sigma, threshold=thr, mask=(err[0] <= thr).astype(np.uint8), inliers=int(cnt[0]))
    return out


# ---- the homography refit: WHAT it is to find, in extended precision ----------------------------------------------------

def transfer(H, uv):
    """uv (n x 2) mapped by H (9 or 3 x 3), in the precision of H."""
    H = np.asarray(H).reshape(3, 3)
    p = np.c_[uv.astype(H.dtype), np.ones(len(uv), H.dtype)] @ H.T
    return p[:, :2] / p[:, 2:]


def transfer_cost(H, uv1, uv2):
    """Sum of squared forward transfer errors |H uv1 - uv2|^2, in long double."""
    d = transfer(np.asarray(H, LD), np.asarray(uv1, LD)) - np.asarray(uv2, LD)
    return (d * d).sum()


def _solve_ld(A, b):
    """Gaussian elimination with partial pivoting in long double (numpy.linalg has none)."""
    A, b = A.astype(LD).copy(), b.astype(LD).copy()
    n = len(b)
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if A[p, c] == 0:
            return None
        A[[c, p]], b[[c, p]] = A[[p, c]], b[[p, c]]
        for r in range(c + 1, n):
            f = A[r, c] / A[c, c]
            A[r, c:] -= f * A[c, c:]
            b[r] -= f * b[c]
    x = np.zeros(n, LD)
    for c in range(n - 1, -1, -1):
        x[c] = (b[c] - A[c, c + 1:] @ x[c + 1:]) / A[c, c]
    return x


def _normalisation(p):
    """Hartley: centroid to the origin, mean distance sqrt(2) — one ISOTROPIC scale, so squared distances keep their ratios."""
    c = p.mean(0)
    s = math.sqrt(2.0) / np.linalg.norm(p - c, axis=1).mean()
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def dlt_homography(uv1, uv2):
    """Normalised DLT by SVD: (H with H[8] = 1, or None when the points do not determine one; relative gap of the null space)."""
    T1, T2 = _normalisation(uv1), _normalisation(uv2)
    a, b = transfer(T1, uv1), transfer(T2, uv2)
    rows = []
    for (X, Y), (x, y) in zip(a, b):
        rows.append([X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x])
        rows.append([0, 0, 0, X, Y, 1, -y * X, -y * Y, -y])
    _, S, Vt = np.linalg.svd(np.array(rows), full_matrices=True)
    S = np.r_[S, np.zeros(9 - len(S))]
    if S[7] <= 1e-9 * S[0]:                      # a null space of more than one dimension: collinear / coincident points
        return None
    H = np.linalg.inv(T2) @ Vt[8].reshape(3, 3) @ T1
    return None if abs(H[2, 2]) < 1e-300 else H / H[2, 2]


def refit_homography(uv1, uv2, mask=None, max_steps=200):
    """The minimiser of the forward transfer error sum |H uv1 - uv2|^2 over the points the mask keeps, as H with H[8] = 1:
    Levenberg-Marquardt in long double from the normalised DLT, run until no step lowers the cost any more and the gradient is
    at rounding level. The work is done in normalised coordinates (an isotropic scaling of the target image multiplies the cost
    by a constant, and any reparametrisation of H keeps the minimiser, so it is the pixel-space minimiser that comes back).
    Returns (H float64 [9], H_dlt [9], info) or None for fewer than 4 points or a degenerate set."""
    uv1, uv2 = np.asarray(uv1, float).reshape(-1, 2), np.asarray(uv2, float).reshape(-1, 2)
    keep = np.ones(len(uv1), bool) if mask is None or len(mask) == 0 else np.asarray(mask, bool)
    a, b = uv1[keep], uv2[keep]
    if len(a) < 4:
        return None
    Hd = dlt_homography(a, b)
    if Hd is None:
        return None
    T1, T2 = _normalisation(a).astype(LD), _normalisation(b).astype(LD)
    A, B = transfer(T1, a.astype(LD)), transfer(T2, b.astype(LD))
    G = T2 @ Hd.astype(LD) @ _inv3(T1)
    h = (G / G[2, 2]).reshape(9)[:8].copy()

    def residuals(h):
        w = h[6] * A[:, 0] + h[7] * A[:, 1] + 1
        x, y = (h[0] * A[:, 0] + h[1] * A[:, 1] + h[2]) / w, (h[3] * A[:, 0] + h[4] * A[:, 1] + h[5]) / w
        return w, x, y, np.r_[x - B[:, 0], y - B[:, 1]]

    lam, steps = LD(1e-3), 0
    w, x, y, r = residuals(h)
    cost = r @ r
    for steps in range(1, max_steps + 1):
        X, Y, one, zero = A[:, 0] / w, A[:, 1] / w, 1 / w, np.zeros(len(A), LD)
        J = np.r_[np.c_[X, Y, one, zero, zero, zero, -X * x, -Y * x], np.c_[zero, zero, zero, X, Y, one, -X * y, -Y * y]]
        JtJ, g = J.T @ J, J.T @ r
        moved = False
        while lam < 1e12:
            d = _solve_ld(JtJ + lam * np.diag(np.diag(JtJ)), -g)
            if d is not None:
                w2, x2, y2, r2 = residuals(h + d)
                if r2 @ r2 < cost:
                    h, w, x, y, r, cost, lam, moved = h + d, w2, x2, y2, r2, r2 @ r2, lam / 10, True
                    break
            lam *= 10
        if not moved:
            break
        lam = max(lam, LD(1e-30))
    Hn = np.r_[h, LD(1)].reshape(3, 3)
    H = _inv3(T2) @ Hn @ T1
    H = (H / H[2, 2]).reshape(9)
    scale = np.sqrt((J * J).sum(0)) * max(np.sqrt(cost), LD(1e-300))
    info = {"steps": steps, "gradient": float(np.abs(g / np.where(scale > 0, scale, 1)).max()), "cost": float(transfer_cost(H, a, b))}
    return H.astype(np.float64), Hd.reshape(9), info


def _inv3(T):
    """Inverse of a scale-and-shift matrix [[s, 0, a], [0, s, b], [0, 0, 1]] in its own precision."""
    s = T[0, 0]
    return np.array([[1 / s, 0, -T[0, 2] / s], [0, 1 / s, -T[1, 2] / s], [0, 0, 1]], T.dtype)


# ---- cv::recoverPose ----------------------------------------------------------------------------------------------------

def decompose_essential(E):
    """cv::decomposeEssentialMat: E = U diag(1, 1, 0) V^T with det U, det V > 0; R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2].
    (An SVD leaves the signs of the third columns free: another valid one gives R1 and R2 swapped and/or -t. The SET
    {R1, R2} x {t, -t} is what is defined.)"""
    U, _, Vt = np.linalg.svd(np.asarray(E, float).reshape(3, 3))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1.0]])
    return U @ W @ Vt, U @ W.T @ Vt, U[:, 2].copy()


def recover_pose(E, uv1, uv2, K, distance_threshold=50.0, mask=None, labelled_as=None):
    """cv::recoverPose(E, pts1, pts2, K, R, t, distanceThresh, mask): the candidates [R1|t], [R2|t], [R1|-t], [R2|-t] in that
    order, every correspondence triangulated under each (the library's two-view triangulation, O.two_view_points), good = kept by
    `mask` and depth in (0, distanceThresh) in both cameras, most good points wins, the first on ties. K: 3 x 3.
    labelled_as = (R1, R2, t) of another decomposition of the same E: the candidates are numbered as THAT one numbers them (see
    decompose_essential: which rotation is "R1" and which sign "t" is the SVD's choice, not a property of E).
    Returns dict: R, t, good, mask, winner, votes."""
    K = np.asarray(K, float).reshape(3, 3)
    K4 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    uv1, uv2 = np.asarray(uv1, float).reshape(-1, 2), np.asarray(uv2, float).reshape(-1, 2)
    R1, R2, t = decompose_essential(E)
    if labelled_as is not None:
        L1, L2, lt = (np.asarray(x, float) for x in labelled_as)
        if np.abs(R1 - L1.reshape(3, 3)).max() > np.abs(R2 - L1.reshape(3, 3)).max():
            R1, R2 = R2, R1
        if np.abs(t - lt).max() > np.abs(t + lt).max():
            t = -t
    cands = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
    keep = np.ones(len(uv1), bool) if mask is None else np.asarray(mask, bool)
    best, votes = None, []
    for k, (R, tt) in enumerate(cands):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, tt
        pts, _, _ = O.two_view_points(uv1, uv2, K4, T.reshape(1, 16), float(np.finfo(np.float32).max), 0.0, False)
        X = pts[0]
        z1 = X[:, 2]
        z2 = ((T[2, 0] * X[:, 0] + T[2, 1] * X[:, 1]) + T[2, 2] * X[:, 2]) + T[2, 3]
        with np.errstate(invalid="ignore"):
            good = keep & (z1 > 0) & (z1 < distance_threshold) & (z2 > 0) & (z2 < distance_threshold)
        votes.append(int(good.sum()))
        if best is None or votes[k] > best["good"]:
            best = {"R": R, "t": tt, "good": votes[k], "mask": good.astype(np.uint8), "winner": k}
    best["votes"] = votes
    return best


# ---- cv::solvePnPRansac -------------------------------------------------------------------------------------------------

def pnp_ransac(X, uv, K4, samples, max_iters, reprojection_error=4.0, confidence=0.999):
    """RANSACPointSetRegistrator::run with EPnP on five points, then EPnP on the winner's inliers. samples: the stream the loop
    would draw, in order (at least as many rows as it ends up consuming). Returns dict: ok, iterations (samples consumed),
    winner (index of the winning sample, -1: none), and when ok: model (R | t, 12), inliers (indices), pose (the refit)."""
    X, uv = np.asarray(X, float).reshape(-1, 3), np.asarray(uv, float).reshape(-1, 2)
    n, m = len(uv), 5
    out = {"ok": False, "iterations": 0, "winner": -1}
    if n < m or max_iters <= 0:
        return out
    samples = np.asarray(samples, np.int32).reshape(-1, m)
    thr = float(np.float32(reprojection_error) * np.float32(reprojection_error))      # squared pixels, as a float
    budget, best_count, best_model, i = max_iters, -1, None, 0
    while i < budget:
        model, ok = O.solve_pnp(X, uv, K4, samples[i][None])
        i += 1
        if not ok[0]:
            continue
        _, cnt, _ = O.score_hypotheses("pnp", X, uv, model[0], K4, thr)
        if cnt[0] > max(best_count, m - 1):
            best_count, best_model, out["winner"] = int(cnt[0]), model[0].copy(), i - 1
            budget = update_num_iters(confidence, (n - best_count) / n, m, budget)
    out["iterations"] = i
    if best_model is None:
        return out
    err, _, _ = O.score_hypotheses("pnp", X, uv, best_model, K4, thr)
    inliers = np.nonzero(err[0] <= np.float32(thr))[0].astype(np.int32)
    refit, rok = O.solve_pnp(X, uv, K4, inliers[None])
    out.update(ok=True, model=best_model, inliers=inliers, pose=refit[0] if rok[0] else best_model)
    return out
