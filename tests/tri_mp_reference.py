"""The triangulation operation at 60 digits (mpmath), written from the reference's statements, not from the kernel:
  TriangulationAngle / TriangulatePoint / IsPositiveDepth / TriangulatePointRansac   Triangulator.cpp:21-186
  CalcReprojectionError                                                               ProjectionHelper.cpp:32-38
  the per-match loops and the choice among candidates of RecoverPoseTwoView           ReconstructionManager.cpp:98-180
  (cv::recoverPose's cheirality vote as tests/estimator_reference.py restates it).

Besides the values it returns what a double-precision implementation can be held to:
  kappa    = sigma_1 / (sigma_3 - sigma_4) / (|x_3| / ||x||): how far the dehomogenised null vector moves, relative to itself,
             per unit of relative perturbation of the DLT matrix;
  defined  = False where sigma_3 = sigma_4 at 60 digits (zero baseline: every point of a line is a null vector);
  a Decision per threshold comparison: the outcome at 60 digits, its margin to the threshold, and the bound on the error of the
  compared quantity in an implementation whose points obey the rule  max|X - X_ref| <= C * 2^-52 * kappa * max|X_ref|.
  The bound is that point error carried through the quantity's first derivatives (a_* below) plus the roundings of the
  evaluation itself (b_*, a few units of 2^-53 times the magnitudes that are added or subtracted), plus one float ulp
  where the reference compares a float. A decision is decided when margin > bound; when both are exactly zero (a point
  that must be returned exactly, e.g. the origin under a candidate without translation) the outcome is determined too.
"""
import mpmath as mp
import numpy as np

mp.mp.dps = 60
U = 2.0 ** -53
EPS = mp.mpf(2.220446049250313e-16)          # std::numeric_limits<double>::epsilon()
SHORT = mp.mpf(float(np.float32(0.0000001)))  # `std::abs(norm) < 0.0000001f`
ANGLE, ERR, DEPTH, Z = range(4)               # kinds of decision
I4 = np.eye(4)

_solve_cache, _inv_cache = {}, {}


def mpf_vec(a):
    return [mp.mpf(float(x)) for x in np.asarray(a, np.float64).reshape(-1)]


class Decision:
    def __init__(self, kind, outcome, margin, bound):
        self.kind, self.outcome, self.margin, self.bound = kind, bool(outcome), float(margin), float(bound)
        self.decided = self.margin > self.bound or (self.margin == 0.0 and self.bound == 0.0)


def conj(decs):
    """A conjunction: (outcome, determined). One decided False settles it whatever the others are."""
    outcome = all(d.outcome for d in decs)
    return outcome, all(d.decided for d in decs) or any(d.decided and not d.outcome for d in decs)


class Solve:
    """TriangulatePoint of one pair: the point as mpf (None: undefined), kappa, defined."""
    def __init__(self, X, kappa, defined):
        self.X, self.kappa, self.defined = X, kappa, defined


def solve_pair(T1, T2, p1, p2, K):
    key = b"".join(np.ascontiguousarray(a, np.float64).tobytes() for a in (T1, T2, p1, p2, K))
    if key in _solve_cache:
        return _solve_cache[key]
    Kq, a, b, (u1, v1), (u2, v2) = mpf_vec(K), mpf_vec(T1), mpf_vec(T2), mpf_vec(p1), mpf_vec(p2)
    x1, y1, x2, y2 = (u1 - Kq[2]) / Kq[0], (v1 - Kq[3]) / Kq[1], (u2 - Kq[2]) / Kq[0], (v2 - Kq[3]) / Kq[1]
    A = mp.matrix(4, 4)
    for j in range(4):
        A[1, j] = x1 * a[8 + j] - a[j]          # Triangulator.cpp:55-58
        A[0, j] = y1 * a[8 + j] - a[4 + j]
        A[3, j] = x2 * b[8 + j] - b[j]
        A[2, j] = y2 * b[8 + j] - b[4 + j]
    _, S, V = mp.svd_r(A)
    s = sorted((S[i] for i in range(4)), reverse=True)
    order = sorted(range(4), key=lambda i: S[i])
    x = [V[order[0], j] for j in range(4)]                                     # svd.matrixV().col(3)
    norm = mp.sqrt(sum(t * t for t in x))
    x = [t if abs(t) > norm * mp.mpf(10) ** -50 else mp.mpf(0) for t in x]
    gap = s[2] - s[3]
    if gap <= s[0] * mp.mpf(10) ** -45 or x[3] == 0:
        sol = Solve(None, float("inf"), False)
    else:
        kappa = float(np.float32(float(s[0] / gap / (abs(x[3]) / norm))))      # (held as a float: the fixture's size)
        sol = Solve([x[0] / x[3], x[1] / x[3], x[2] / x[3]], kappa, True)     # hnormalized()
    _solve_cache[key] = sol
    return sol


def centre(T):
    """transform.inverse().block<3, 1>(0, 3)"""
    key = np.ascontiguousarray(T, np.float64).tobytes()
    if key not in _inv_cache:
        M = mp.matrix(4, 4)
        t = mpf_vec(T)
        for i in range(4):
            for j in range(4):
                M[i, j] = t[4 * i + j]
        inv = mp.inverse(M)
        _inv_cache[key] = [inv[0, 3], inv[1, 3], inv[2, 3]]
    return _inv_cache[key]


def norm3(v):
    return mp.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def point_bound(sol, C):
    """(relative, absolute) bound on the error of the pair's point under the rule."""
    rel = C * 2.0 ** -52 * sol.kappa
    return rel, rel * float(max(abs(t) for t in sol.X))


def angle(T1, T2, X, delta, decs, kind=ANGLE):
    """TriangulationAngle, its short-ray decisions appended to decs: (angle, bound on its error)."""
    c1, c2 = centre(T1), centre(T2)
    scale = float(norm3(X)) + max(float(norm3(c1)), float(norm3(c2)))
    ray_bound = np.sqrt(3.0) * delta + 16 * U * scale          # the ray X - c: the point's error and the subtraction's operands
    norms = []
    for c in (c1, c2):
        r = [X[i] - c[i] for i in range(3)]
        n = norm3(r)
        d = Decision(kind, not n < SHORT, abs(n - SHORT), ray_bound)       # outcome: the ray is long enough
        decs.append(d)
        if not d.outcome:
            return mp.mpf(0), 0.0 if d.decided else float("inf")          # `return false`
        norms.append((r, n))
    (r1, n1), (r2, n2) = norms
    cosine = (r1[0] * r2[0] + r1[1] * r2[1] + r1[2] * r2[2]) / (n1 * n2)
    raw = mp.acos(max(min(cosine, mp.mpf(1)), mp.mpf(-1)))
    ang = min(raw, mp.pi - raw)
    # each ray turns by at most its error over its length; acos of a cosine rounded to double moves by u / sin
    bound = ray_bound * float(1 / n1 + 1 / n2) + 8 * U / max(float(mp.sin(raw)), 2.0 ** -26) + 4 * U * float(ang)
    return ang, bound


def projection(T, uv, K, X, delta):
    """CalcReprojectionError(uv, transformPoint3d(X, T), K) and the camera z: (err, err_bound, pz, pz_bound)."""
    t, Kq, (u0, v0) = mpf_vec(T), mpf_vec(K), mpf_vec(uv)
    p, pa, pb = [], [], []
    for i in range(3):
        row = t[4 * i:4 * i + 4]
        p.append(row[0] * X[0] + row[1] * X[1] + row[2] * X[2] + row[3])
        pa.append(float(abs(row[0]) + abs(row[1]) + abs(row[2])) * delta)
        pb.append(8 * U * float(abs(row[0] * X[0]) + abs(row[1] * X[1]) + abs(row[2] * X[2]) + abs(row[3])))
    pzb = pa[2] + pb[2]
    if p[2] == 0:
        return mp.inf, 0.0, p[2], pzb
    u, v = Kq[0] * p[0] / p[2] + Kq[2], Kq[1] * p[1] / p[2] + Kq[3]
    err = mp.sqrt((u0 - u) ** 2 + (v0 - v) ** 2)
    z = float(abs(p[2]))
    if z < 1e-150 or not np.isfinite(float(err)):             # (the double behind it overflows: the float is inf either way)
        return err, 0.0, p[2], pzb
    bound = sum(float(Kq[i]) * ((pa[i] + pb[i]) / z + float(abs(p[i])) * pzb / z ** 2) for i in range(2))
    bound += 8 * U * float(abs(u) + abs(v) + abs(u0) + abs(v0) + abs(Kq[2]) + abs(Kq[3]) + err)
    return err, bound, p[2], pzb


def float_ulp(x):
    x = abs(float(x))
    return float("inf") if not np.isfinite(np.float32(x)) else float(np.spacing(np.float32(x)))


def inlier(T, uv, K, X, delta, max_err, decs):
    """`err < maxReprError && IsPositiveDepth(transform, point3d)` with err a float."""
    err, eb, pz, pzb = projection(T, uv, K, X, delta)
    mine = [Decision(ERR, err < max_err, abs(err - max_err), eb + float_ulp(max_err) if mp.isfinite(err) else 0.0),
            Decision(DEPTH, pz >= EPS, abs(pz - EPS), pzb)]
    decs += mine
    return mine[0].outcome and mine[1].outcome


def as_float(X):
    return [float("nan")] * 3 if X is None else [float(t) for t in X]


def track(Ts, uvs, K, max_err, min_angle, C):
    """TriangulatePointRansac and TriangulateFrame's `every observation an inlier` for one track. An undefined pair is never
    accepted. Returns a dict of plain values."""
    m = len(Ts)
    max_err, min_angle = mp.mpf(float(np.float32(max_err))), mp.mpf(float(np.float32(min_angle)))
    decs, out = [], {"point": [0.0] * 3, "mask": [0] * m, "status": 0, "bits": 3, "kappa": 0.0, "defined": True, "tol": 0.0,
                     "angle": float("nan"), "angle_tol": float("nan")}

    def pair(r1, r2):
        """(the solve, angle gate passed, inlier list or None)"""
        sol = solve_pair(Ts[r1], Ts[r2], uvs[r1], uvs[r2], K)
        if not sol.defined:
            return sol, False, None
        _, delta = point_bound(sol, C)
        ang, ab = angle(Ts[r1], Ts[r2], sol.X, delta, decs)
        gate = Decision(ANGLE, ang >= min_angle, abs(ang - min_angle), ab)
        decs.append(gate)
        if m == 2:
            out["angle"], out["angle_tol"] = float(ang), ab
        if not gate.outcome:
            return sol, False, None
        return sol, True, [inlier(Ts[i], uvs[i], K, sol.X, delta, max_err, decs) for i in range(m)]

    def z_positive(sol):
        d = Decision(Z, sol.X[2] > 0, abs(sol.X[2]), point_bound(sol, C)[1])
        decs.append(d)
        return d.outcome

    sol, best, mask = None, 0, None
    if m == 2:
        sol, ok, inl = pair(0, 1)
        if ok:
            mask, best = inl, sum(inl)
            out["status"] = (1 if z_positive(sol) else 0) | (2 if best == 2 else 0)
    elif m > 2:
        for r1 in range(m - 1):
            for r2 in range(r1 + 1, m):
                sol, ok, inl = pair(r1, r2)
                if ok and sum(inl) > best:
                    best, mask = sum(inl), inl
        if best > 2 and not sol.defined:
            out["bits"] = 2                                   # `point3d.z() > 0` of a point that is anything
        ransac = best > 2 and sol.defined and z_positive(sol)
        out["status"] = (1 if ransac else 0) | (2 if mask is not None and best == m else 0)
    if mask is not None:
        out["mask"] = [int(x) for x in mask]
    if sol is not None:
        out["point"], out["kappa"], out["defined"] = as_float(sol.X), sol.kappa, sol.defined
        out["tol"] = point_bound(sol, C)[0] if sol.defined else float("inf")
    summarise(out, decs)
    return out


def summarise(out, decs):
    ratio = [float("inf")] * 4
    for d in decs:
        r = d.margin / d.bound if d.bound > 0 else float("inf")   # (a bound of zero: determined exactly)
        ratio[d.kind] = min(ratio[d.kind], r)
    out["margin"] = ratio                                    # per kind: the smallest margin / bound among the item's decisions
    out["n_decisions"], out["n_undecided"] = len(decs), sum(not d.decided for d in decs)
    out["decided"] = out["n_undecided"] == 0


def reprojection(T, uv, K, X):
    """(float error as the reference returns it, bound on the double behind it)"""
    err, bound, _, _ = projection(T, uv, K, mpf_vec(X), 0.0)
    with np.errstate(over="ignore"):
        return float(np.float32(float(err))) if mp.isfinite(err) else float("inf"), bound


def two_view_item(T, p1, p2, K, max_err, min_angle, dist, C):
    """One match under one candidate: the point, keep under the strict (:114-129) and the other (:163-176) angle test, the
    cheirality vote, each with whether it is determined."""
    max_err, min_angle, dist = mp.mpf(float(np.float32(max_err))), mp.mpf(float(np.float32(min_angle))), mp.mpf(float(dist))
    sol = solve_pair(I4, T, p1, p2, K)
    out = {"point": as_float(sol.X), "kappa": sol.kappa, "defined": sol.defined, "tol": float("inf"), "keep_strict": 0, "keep": 0,
           "vote": 0, "det_keep": True, "det_vote": True}
    decs = []
    if sol.defined:
        rel, delta = point_bound(sol, C)
        out["tol"] = rel
        X = sol.X
        front = Decision(Z, X[2] > 0, abs(X[2]), delta)
        decs.append(front)
        keep = [front]
        if front.outcome:
            err, eb, _, _ = projection(I4, p1, K, X, delta)
            keep.append(Decision(ERR, err < max_err, abs(err - max_err), eb + float_ulp(max_err)))
            ang, ab = angle(I4, T, X, delta, keep)
            keep.append(Decision(ANGLE, ang > min_angle, abs(ang - min_angle), ab))   # `>` and `!(<)` part only on equality
            decs += keep[1:]
        out["keep_strict"] = out["keep"] = int(conj(keep)[0])
        out["det_keep"] = conj(keep)[1]
        t = mpf_vec(T)
        z2 = t[8] * X[0] + t[9] * X[1] + t[10] * X[2] + t[11]
        z2b = float(abs(t[8]) + abs(t[9]) + abs(t[10])) * delta + 8 * U * float(abs(t[8] * X[0]) + abs(t[9] * X[1]) + abs(t[10] * X[2]) + abs(t[11]))
        vote = [front, Decision(Z, X[2] < dist, abs(dist - X[2]), delta), Decision(DEPTH, z2 > 0, abs(z2), z2b),
                Decision(DEPTH, z2 < dist, abs(dist - z2), z2b)]
        decs += vote[1:]
        out["vote"], out["det_vote"] = int(conj(vote)[0]), conj(vote)[1]
    summarise(out, decs)
    out["decided"] = out["det_keep"] and out["det_vote"]
    out["n_undecided"] = int(not out["det_keep"]) + int(not out["det_vote"])
    out["n_decisions"] = 2
    return out


def choose(rule, counts, min_solution_matches):
    """The winner among a problem's candidates: cv::recoverPose keeps the first candidate with the most votes ("poses"); the
    solutions loop keeps the first with strictly more matches than any before it, and the result only above the minimum."""
    if rule == "poses":
        best = 0 if len(counts) else -1
        for k in range(1, len(counts)):
            if counts[k] > counts[best]:
                best = k
        return best
    best, best_count = -1, 0
    for k, c in enumerate(counts):
        if c > best_count:
            best, best_count = k, c
    return best if best_count > min_solution_matches else -1


# ---- whole groups of tests/tri_hard_cases.py -> arrays, as tests/golden/tri_hard_golden.npz holds them -------------------

RULES = ("poses", "solutions")


def evaluate_tracks(g, C):
    ptr, T = g["ptr"], g["T"].reshape(-1, 4, 4)
    recs = [track([T[f] for f in g["frame"][a:b]], list(g["uv"][a:b]), g["K"], g["max_err"], g["min_angle"], C)
            for a, b in zip(ptr[:-1], ptr[1:])]
    col = lambda k, dt: np.array([r[k] for r in recs], dtype=dt)   # noqa: E731
    return {"points": col("point", np.float64).reshape(-1, 3), "status": col("status", np.int32), "bits": col("bits", np.int32),
            "masks": np.array([x for r in recs for x in r["mask"]], np.uint8), "kappa": col("kappa", np.float32),
            "defined": col("defined", np.bool_), "decided": col("decided", np.bool_), "margin": col("margin", np.float32).reshape(-1, 4),
            "angle": col("angle", np.float64), "angle_tol": col("angle_tol", np.float32),
            "n_decisions": col("n_decisions", np.int32), "n_undecided": col("n_undecided", np.int32)}


def evaluate_reprojection(g):
    T = g["T"].reshape(-1, 4, 4)
    recs = [reprojection(T[f], p, g["K"], X) for f, X, p in zip(g["frame"], g["X"], g["uv"])]
    return {"err": np.array([r[0] for r in recs], np.float32), "err_tol": np.array([r[1] for r in recs], np.float64)}


def evaluate_twoview(g, C):
    """Items in the order of eacham_two_view_batch's workspace: problem, candidate, match."""
    recs, item_ptr = [], [0]
    per_rule = {r: {"winner": [], "good": [], "kept": [], "decided": []} for r in RULES}
    for uv1, uv2, Ts in g["problems"]:
        mine = [[two_view_item(T.reshape(4, 4), a, b, g["K"], g["max_err"], g["min_angle"], g["dist"], C) for a, b in zip(uv1, uv2)] for T in Ts]
        for rule in RULES:
            key, det = ("vote", "det_vote") if rule == "poses" else ("keep_strict", "det_keep")
            counts = [sum(r[key] for r in row) for row in mine]
            w = choose(rule, counts, g["min_solution_matches"])
            per_rule[rule]["winner"].append(w)
            per_rule[rule]["good"].append(counts[w] if rule == "poses" and w >= 0 else 0)
            per_rule[rule]["kept"].append(sum(r["keep"] for r in mine[w]) if w >= 0 else 0)
            ok = all(r[det] for row in mine for r in row) and (rule != "poses" or w < 0 or all(r["det_keep"] for r in mine[w]))
            per_rule[rule]["decided"].append(ok)
        recs += [r for row in mine for r in row]
        item_ptr.append(len(recs))
    col = lambda k, dt: np.array([r[k] for r in recs], dtype=dt)   # noqa: E731
    out = {"item_ptr": np.array(item_ptr, np.int64), "points": col("point", np.float64).reshape(-1, 3), "kappa": col("kappa", np.float32),
           "defined": col("defined", np.bool_), "keep": col("keep", np.uint8), "vote": col("vote", np.uint8),
           "det_keep": col("det_keep", np.bool_), "det_vote": col("det_vote", np.bool_),
           "margin": np.array([min(r["margin"]) for r in recs], np.float32), "n_decisions": col("n_decisions", np.int32),
           "n_undecided": col("n_undecided", np.int32)}
    for rule in RULES:
        for k, v in per_rule[rule].items():
            out[f"{rule}_{k}"] = np.array(v, np.bool_ if k == "decided" else np.int32)
    return out


def evaluate(g, C):
    return {"tracks": lambda: evaluate_tracks(g, C), "reproj": lambda: evaluate_reprojection(g), "twoview": lambda: evaluate_twoview(g, C)}[g["kind"]]()
