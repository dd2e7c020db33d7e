"""The rules that tests/golden/tri_hard_golden.npz is read by, shared by tests/test_tri_hard_reference.py (the CPU oracle and the
LAPACK statement) and tests/test_tri_hard_gpu.py (the kernels). Numpy only.

Points:   max|X - X_ref| <= C * 2^-52 * kappa * max|X_ref| wherever the reference is defined, C = 8 x the largest ratio that
          oracle/tri_oracle.c reaches on the fixture (`oracle_ratio`, measured by the generator): the same algorithm under another
          contraction of multiply-adds gets three bits of room. A reference point that is exactly zero must come back exactly.
Verdicts: status bits, masks, keep flags, counts, winners, good / kept equal the reference's wherever every decision behind them
          is decided (the margin at 60 digits exceeds the point bound carried to the compared quantity); an item that hangs on
          an undecided decision is compared with `other` (the oracle's answer) instead, where one is given.
Undefined items (zero baseline) are never accepted: the reference records status 0 / mask 0 / keep 0 / no vote for them and
          they are compared like every other verdict; their points are not compared.
"""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tri_hard_golden.npz")
RULES = ("poses", "solutions")


def pack(groups):
    """{group: {field: array}} -> the fixture's members: one float64 vector per group (every field is exact in a double) and one
    JSON layout, so the archive pays for a few members, not for hundreds."""
    layout, members = {}, {}
    for name, g in groups.items():
        fields, parts = [], []
        for k, v in g.items():
            if k == "kind":
                continue
            v = np.asarray(v)
            fields.append([k, v.dtype.str, list(v.shape)])
            parts.append(v.astype(np.float64).reshape(-1))
        layout[name] = {"kind": str(g["kind"]), "fields": fields}
        members[name] = np.concatenate(parts)
    members["layout"] = np.array(json.dumps(layout))
    return members


def load(path=GOLD):
    """{group: {field: array}} and the measured oracle_ratio."""
    groups = {}
    with np.load(path) as z:
        layout = json.loads(str(z["layout"]))
        ratio = float(z["oracle_ratio"])
        for name, desc in layout.items():
            flat, at, g = z[name], 0, {"kind": desc["kind"]}
            for k, dt, shape in desc["fields"]:
                n = int(np.prod(shape))
                with np.errstate(invalid="ignore"):
                    g[k] = flat[at:at + n].astype(np.dtype(dt)).reshape(shape)
                at += n
            groups[name] = g
    return groups, ratio


PER_TRACK = ("points", "status", "bits", "kappa", "defined", "decided", "margin", "angle", "angle_tol", "n_decisions", "n_undecided")


def take(g, order):
    """The "tracks" group made of g's tracks `order` (repeats allowed): inputs and reference alike."""
    ptr, order = g["ptr"], np.asarray(order, np.int64)
    obs = np.concatenate([np.arange(ptr[t], ptr[t + 1]) for t in order]) if len(order) else np.zeros(0, np.int64)
    out = dict(g)
    out["ptr"] = np.concatenate([[0], np.cumsum((ptr[1:] - ptr[:-1])[order])]).astype(np.int32)
    for k in ("frame", "uv", "masks"):
        out[k] = g[k][obs]
    for k in PER_TRACK:
        out[k] = g[k][order]
    return out


def tiled(g, n):
    """n tracks drawn in turn from g's: track t is g's track 7 t mod len."""
    return take(g, (7 * np.arange(n)) % (len(g["ptr"]) - 1))


def concat(gs):
    """Several "tracks" groups with equal K and thresholds as one call: (group, first track of each part)."""
    assert all(np.array_equal(g["K"], gs[0]["K"]) and g["max_err"] == gs[0]["max_err"] and g["min_angle"] == gs[0]["min_angle"] for g in gs)
    out = dict(gs[0])
    frames = np.cumsum([0] + [len(g["T"]) for g in gs])
    obs = np.cumsum([0] + [len(g["frame"]) for g in gs])
    out["T"] = np.concatenate([g["T"] for g in gs])
    out["frame"] = np.concatenate([g["frame"] + np.uint32(f) for g, f in zip(gs, frames)]).astype(np.uint32)
    out["ptr"] = np.concatenate([[0]] + [g["ptr"][1:] + o for g, o in zip(gs, obs)]).astype(np.int32)
    for k in ("uv", "masks") + PER_TRACK:
        out[k] = np.concatenate([g[k] for g in gs])
    return out, np.cumsum([0] + [len(g["ptr"]) - 1 for g in gs])


def flatten(case, ref):
    """One group's inputs and reference arrays as the fixture holds them."""
    out = {k: v for k, v in case.items() if k != "problems"}
    if case["kind"] == "twoview":
        P = case["problems"]
        out["point_ptr"] = np.cumsum([0] + [len(p[0]) for p in P]).astype(np.int64)
        out["transform_ptr"] = np.cumsum([0] + [len(p[2]) for p in P]).astype(np.int64)
        out["uv1"] = np.concatenate([p[0] for p in P]).reshape(-1, 2)
        out["uv2"] = np.concatenate([p[1] for p in P]).reshape(-1, 2)
        out["Ts"] = np.concatenate([p[2] for p in P]).reshape(-1, 16)
    out.update(ref)
    return {k: np.asarray(v) for k, v in out.items()}


INPUTS = {"tracks": ("T", "ptr", "frame", "uv", "K", "max_err", "min_angle"), "reproj": ("T", "frame", "X", "uv", "K"),
          "twoview": ("point_ptr", "transform_ptr", "uv1", "uv2", "Ts", "K", "max_err", "min_angle", "dist", "min_solution_matches")}


def as_case(g):
    """A fixture group's inputs in the form of tests/tri_hard_cases.py (what the reference is evaluated on)."""
    case = {k: g[k] for k in INPUTS[g["kind"]] + ("kind", "ladder")}
    if g["kind"] == "twoview":
        case["problems"] = problems(g)
    return case


def problems(g):
    pp, tp = g["point_ptr"], g["transform_ptr"]
    return [(g["uv1"][pp[p]:pp[p + 1]], g["uv2"][pp[p]:pp[p + 1]], g["Ts"][tp[p]:tp[p + 1]]) for p in range(len(pp) - 1)]


def point_ratio(X, ref, kappa, defined):
    """Per item: max|X - X_ref| / max|X_ref| / (2^-52 kappa); nan where undefined; an exactly zero reference point gives 0
    when met exactly and inf otherwise."""
    X, ref = np.asarray(X, np.float64).reshape(-1, 3), np.asarray(ref, np.float64).reshape(-1, 3)
    out = np.full(len(ref), np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        err = np.abs(X - ref).max(1)
        scale = np.abs(ref).max(1) * 2.0 ** -52 * kappa
        r = np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))
    r[np.isnan(r)] = np.inf                                    # a defined point came back as NaN
    out[defined] = r[defined]
    return out


def worst(r):
    r = r[~np.isnan(r)]
    return float(r.max()) if r.size else 0.0


def check_tracks(name, g, got, C, other=None):
    pts, status, masks = got
    ratio = point_ratio(pts, g["points"], g["kappa"], g["defined"])
    bad = np.flatnonzero(ratio > C)
    assert bad.size == 0, f"{name}: points of tracks {bad[:8]} at {ratio[bad[:8]]} x 2^-52 kappa, allowed {C:.3g}"
    ptr = g["ptr"]
    for t in range(len(ptr) - 1):
        a, b, bits = ptr[t], ptr[t + 1], g["bits"][t]
        if g["decided"][t]:
            want_status, want_mask = g["status"][t], g["masks"][a:b]
        elif other is not None:
            want_status, want_mask = other[1][t], other[2][a:b]
        else:
            continue
        assert (status[t] & bits) == (want_status & bits), f"{name}: track {t}: status {status[t]}, expected {want_status} (bits {bits})"
        assert np.array_equal(masks[a:b], want_mask), f"{name}: track {t}: mask {masks[a:b]}, expected {want_mask}"
    return worst(ratio)


def check_reprojection(name, g, err):
    ref, tol = g["err"], g["err_tol"]
    fin = np.isfinite(ref)
    assert np.array_equal(err[~fin], ref[~fin]), f"{name}: {err[~fin]} where the reference overflows a float"
    slack = np.spacing(np.abs(ref[fin])).astype(np.float64) + tol[fin]
    off = np.abs(err[fin].astype(np.float64) - ref[fin]) / slack
    assert (off <= 1.0).all(), f"{name}: errors {err[fin][off > 1]} against {ref[fin][off > 1]}"
    return float(off.max())


def items(g, p):
    """(slice of problem p's items, nt, n)"""
    nt = int(g["transform_ptr"][p + 1] - g["transform_ptr"][p])
    n = int(g["point_ptr"][p + 1] - g["point_ptr"][p])
    return slice(int(g["item_ptr"][p]), int(g["item_ptr"][p + 1])), nt, n


def check_two_view_points(name, g, p, got, C, other=None):
    """One problem through eacham_two_view_points (either value of strict: they part only on an angle equal to the threshold)."""
    pts, keep, counts = got
    sl, nt, n = items(g, p)
    ratio = point_ratio(pts, g["points"][sl], g["kappa"][sl], g["defined"][sl])
    bad = np.flatnonzero(ratio > C)
    assert bad.size == 0, f"{name}[{p}]: points of items {bad[:8]} at {ratio[bad[:8]]} x 2^-52 kappa, allowed {C:.3g}"
    want, det = g["keep"][sl].copy(), g["det_keep"][sl]
    if other is not None:
        want[~det] = np.asarray(other[1]).reshape(-1)[~det]
        det = np.ones_like(det)
    assert np.array_equal(np.asarray(keep).reshape(-1)[det], want[det]), f"{name}[{p}]: keep differs at {np.flatnonzero((np.asarray(keep).reshape(-1) != want) & det)[:8]}"
    assert np.array_equal(counts, np.asarray(keep).reshape(nt, n).sum(1)), f"{name}[{p}]: counts"
    return worst(ratio)


def check_batch(name, g, rule, got, C, other=None):
    """eacham_two_view_batch over the group's problems, all under `rule`. got: eacham_amd.twoview.TwoViewBatch (or its fields
    by name); other: tests/two_view_batch_cases.compose records of the oracle."""
    top = 0.0
    for p in range(len(g["point_ptr"]) - 1):
        sl, nt, n = items(g, p)
        at = f"{name}[{p}] under {rule}"
        if not g[f"{rule}_decided"][p]:
            if other is not None:
                o = other[p]
                assert (int(got.winner[p]), int(got.good[p]), int(got.kept[p])) == (o["winner"], o["good"], o["kept"]), at
                assert np.array_equal(got.keep[p], o["keep"]) and np.array_equal(got.pose_mask[p], o["pose_mask"]), at
            continue
        keep, vote = g["keep"][sl].reshape(nt, n), g["vote"][sl].reshape(nt, n)
        counts = (vote if rule == "poses" else keep).sum(1)
        w = int(g[f"{rule}_winner"][p])
        assert np.array_equal(got.cand_counts[p], counts), f"{at}: counts {got.cand_counts[p]}, expected {counts}"
        assert (int(got.winner[p]), int(got.good[p]), int(got.kept[p])) == (w, int(g[f"{rule}_good"][p]), int(g[f"{rule}_kept"][p])), at
        if w < 0:
            assert not got.keep[p].any() and not got.pose_mask[p].any() and got.points[p].tobytes() == bytes(got.points[p].nbytes), at
            continue
        assert np.array_equal(got.keep[p], keep[w]), at
        assert np.array_equal(got.pose_mask[p], vote[w] if rule == "poses" else np.zeros(n, np.uint8)), at
        mine = slice(sl.start + w * n, sl.start + (w + 1) * n)
        ratio = point_ratio(got.points[p], g["points"][mine], g["kappa"][mine], g["defined"][mine])
        assert not (ratio > C).any(), f"{at}: points at {worst(ratio)} x 2^-52 kappa, allowed {C:.3g}"
        top = max(top, worst(ratio))
    return top


def undecided_share(g):
    """The share of the group's items (tracks; (candidate, match) items) that hang on at least one undecided decision."""
    return float((g["n_undecided"] > 0).mean()) if "n_undecided" in g else 0.0
