"""Seeded problem lists for eacham_two_view_batch and its yardstick (shared by tests/test_two_view_batch_reference.py, CPU, and
tests/test_two_view_batch_gpu.py): the smallest shapes at which the segmented kernels can still go wrong.

A case is a dict: uv1 / uv2 = one n_p x 2 array per problem, rules = "poses" | "solutions" per problem, transforms = one
nt_p x 16 array of candidate camera-1 -> camera-2 transforms per problem, in_mask = None or one n_p byte array per problem,
K = fx fy cx cy, and the call's scalars max_err / min_angle / dist / min_solution_matches.

compose(two_view_points_fn, case) is the yardstick: per problem ONE call of the single-pair entry point
(eacham_two_view_points' signature: uv1, uv2, K4, transforms, max_err, min_angle, angle_strict -> points [nt, n, 3], keep
[nt, n], counts [nt]) with all of the problem's candidates, then the host rules of include/eacham_hip.h in numpy."""
import numpy as np

import estimator_reference as ER
import score_cases as SC

TRI_BLOCK = 256          # eacham_amd/csrc/triangulate.hip: threads of a workgroup
MAX_ERR, MIN_ANGLE, DIST, MIN_SOLUTION = 4.0, float(np.deg2rad(1.0)), 50.0, 20
K = np.array(SC.two_view_case(n=8, n_models=1, seed=1)["K"], dtype=np.float64)


def candidates(c, nt, roll):
    """nt of the four poses of the true E, as [R1|t], [R1|-t], [R2|t], [R2|-t] rolled by `roll`: any two neighbours hold a
    t-flipped one (negative depths), and the true pose is not always candidate 0."""
    R1, R2, t = ER.decompose_essential(c["E"][0])
    T = []
    for R, s in ((R1, 1.0), (R1, -1.0), (R2, 1.0), (R2, -1.0)):
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = R, s * t
        T.append(M.reshape(16))
    return np.roll(np.array(T), -roll, axis=0)[:nt].copy()


def problem(n, nt, seed, planar=False):
    """(uv1, uv2, transforms) of one pair: n matches (a quarter of them gross outliers), nt candidates."""
    c = SC.two_view_case(n=max(n, 8), n_models=1, seed=seed, outliers=0.25, planar=planar, facing=True)
    return c["uv1"][:n].copy(), c["uv2"][:n].copy(), candidates(c, nt, seed % 4)


def _case(probs, rules, in_mask=None, **scalars):
    case = {"uv1": [p[0] for p in probs], "uv2": [p[1] for p in probs], "transforms": [p[2] for p in probs], "rules": list(rules),
            "in_mask": in_mask, "K": K, "max_err": MAX_ERR, "min_angle": MIN_ANGLE, "dist": DIST, "min_solution_matches": MIN_SOLUTION}
    case.update(scalars)
    return case


def random_mask(case, seed=5):
    rng = np.random.default_rng(seed)
    return dict(case, in_mask=[(rng.random(len(u)) < 0.6).astype(np.uint8) for u in case["uv1"]])


def single():
    """One POSES problem, 70 matches, 4 candidates: more than a wave, less than a workgroup."""
    return _case([problem(70, 4, 11)], ["poses"])


MIXED_SIZES = [1, 63, 64, 65, 255, 256, 257, 300]


def mixed():
    """Segment boundaries inside waves and workgroups: rules alternate, 1-4 candidates each."""
    probs = [problem(n, 1 + (k + 1) % 4, 20 + k) for k, n in enumerate(MIXED_SIZES)]
    return _case(probs, ["poses" if k % 2 == 0 else "solutions" for k in range(len(probs))])


def empties():
    """Problems without points and problems without candidates, first, last and between ordinary ones, under both rules."""
    nopts = lambda nt, seed: problem(0, nt, seed)                                    # noqa: E731
    nocand = lambda n, seed: problem(n, 0, seed)                                     # noqa: E731
    probs = [nopts(3, 30), problem(40, 4, 31), nocand(33, 32), nocand(0, 33), problem(70, 2, 34), nopts(2, 35), problem(41, 3, 36), nocand(20, 37)]
    return _case(probs, ["poses", "poses", "poses", "solutions", "solutions", "solutions", "poses", "solutions"])


def twins():
    """Every candidate appears twice (k and k + 4), under each rule: the earlier one must win."""
    probs = []
    for seed in (40, 41):
        u1, u2, T = problem(90, 4, seed)
        probs.append((u1, u2, np.concatenate([T, T])))
    return _case(probs, ["poses", "solutions"])


def masked_out():
    """POSES with in_mask all zero: winner 0, good 0, keep still computed."""
    case = _case([problem(100, 4, 50), problem(64, 2, 51)], ["poses", "poses"])
    return dict(case, in_mask=[np.zeros(len(u), np.uint8) for u in case["uv1"]])


def solutions_only(min_solution_matches=MIN_SOLUTION):
    return _case([problem(120, 4, 60), problem(257, 3, 61)], ["solutions", "solutions"], min_solution_matches=min_solution_matches)


def degenerate():
    """A candidate equal to the identity (zero baseline: the points are not finite) among ordinary ones, under both rules, and
    alone."""
    eye = np.eye(4).reshape(1, 16)
    probs = []
    for seed, where in ((70, 0), (71, 2), (72, 1)):
        u1, u2, T = problem(80, 3, seed)
        probs.append((u1, u2, np.insert(T, where, eye, axis=0)))
    u1, u2, _ = problem(65, 1, 73)
    probs.append((u1, u2, eye.copy()))
    return _case(probs, ["poses", "solutions", "poses", "solutions"])


def multi_block():
    """64 problems x 300 matches x 4 candidates: many workgroups in both kernels."""
    return _case([problem(300, 4, 100 + k, planar=k % 3 == 0) for k in range(64)], ["poses" if k % 2 == 0 else "solutions" for k in range(64)])


def reverse(case):
    return dict(case, uv1=case["uv1"][::-1], uv2=case["uv2"][::-1], transforms=case["transforms"][::-1], rules=case["rules"][::-1],
                in_mask=None if case["in_mask"] is None else case["in_mask"][::-1])


CASES = {"single": single, "mixed": mixed, "empties": empties, "twins": twins, "masked_out": masked_out, "solutions_only": solutions_only,
         "degenerate": degenerate, "multi_block": multi_block}


# ---- the yardstick --------------------------------------------------------------------------------------------------------

def none_record(n, counts):
    return {"winner": -1, "good": 0, "kept": 0, "cand_counts": np.asarray(counts, np.int32), "points": np.zeros((n, 3)),
            "keep": np.zeros(n, np.uint8), "pose_mask": np.zeros(n, np.uint8)}


def compose_one(two_view_points_fn, rule, uv1, uv2, K4, T, in_mask, max_err, min_angle, dist, min_solution_matches):
    n, nt = len(uv1), len(T)
    if nt == 0:
        return none_record(n, [])
    pts, keep, _ = two_view_points_fn(uv1, uv2, K4, T, max_err, min_angle, rule == "solutions")
    if rule == "solutions":
        counts = [int(keep[k].sum()) for k in range(nt)]
        best, best_count = -1, 0
        for k in range(nt):
            if counts[k] > best_count:                         # strictly larger: the first one stays
                best, best_count = k, counts[k]
        if best < 0 or not best_count > min_solution_matches:
            return none_record(n, counts)
        return {"winner": best, "good": 0, "kept": best_count, "cand_counts": np.asarray(counts, np.int32), "points": pts[best].copy(),
                "keep": keep[best].copy(), "pose_mask": np.zeros(n, np.uint8)}
    allowed = np.ones(n, bool) if in_mask is None else np.asarray(in_mask, bool)
    counts, masks = [], []
    for k in range(nt):
        M, X = T[k], pts[k]
        with np.errstate(invalid="ignore", over="ignore"):
            z1 = X[:, 2]
            z2 = ((M[8] * X[:, 0] + M[9] * X[:, 1]) + M[10] * X[:, 2]) + M[11]   # every operation rounded on its own
            ch = allowed & (z1 > 0) & (z1 < dist) & (z2 > 0) & (z2 < dist)
        masks.append(ch.astype(np.uint8))
        counts.append(int(ch.sum()))
    best = 0
    for k in range(1, nt):
        if counts[k] > counts[best]:
            best = k
    return {"winner": best, "good": counts[best], "kept": int(keep[best].sum()), "cand_counts": np.asarray(counts, np.int32),
            "points": pts[best].copy(), "keep": keep[best].copy(), "pose_mask": masks[best]}


def compose(two_view_points_fn, case):
    P = len(case["uv1"])
    return [compose_one(two_view_points_fn, case["rules"][p], case["uv1"][p], case["uv2"][p], case["K"], case["transforms"][p],
                        None if case["in_mask"] is None else case["in_mask"][p], case["max_err"], case["min_angle"], case["dist"],
                        case["min_solution_matches"]) for p in range(P)]
