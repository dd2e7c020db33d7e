"""Generates tests/golden/tri_hard_golden.npz: the hard-geometry cases of tests/tri_hard_cases.py, what tests/tri_mp_reference.py
(mpmath, 60 digits) says they give, and how far oracle/tri_oracle.c is from that (`oracle_ratio`, which sets the constant of the
point rule: tests/tri_hard_rules.py). Nothing in it comes from the reference project's files. Checks its own conditions: at most
64 KB, at most 10 % of any group's items undecided and none in a group that is not built on a ladder.
Run from the repo root:  python tests/golden/make_tri_hard_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_api as O  # noqa: E402
import tri_hard_cases as HC  # noqa: E402
import tri_hard_rules as HR  # noqa: E402
import tri_mp_reference as MR  # noqa: E402

MAX_BYTES = 64 * 1024
MAX_UNDECIDED = 0.10


def oracle_points(case):
    """The oracle's points for a group, in the order of the reference's arrays (None: the group has none)."""
    if case["kind"] == "tracks":
        return O.tri_tracks(case["T"], case["ptr"], case["frame"], case["uv"], case["K"], float(case["max_err"]), float(case["min_angle"]))[0]
    if case["kind"] == "twoview":
        pts = [O.two_view_points(u1, u2, case["K"], Ts, float(case["max_err"]), float(case["min_angle"]), True)[0].reshape(-1, 3)
               for u1, u2, Ts in case["problems"]]
        return np.concatenate(pts)
    return None


def measure_oracle_ratio(cases, refs):
    top = {}
    for name, case in cases.items():
        pts = oracle_points(case)
        if pts is not None:
            top[name] = HR.worst(HR.point_ratio(pts, refs[name]["points"], refs[name]["kappa"], refs[name]["defined"]))
    return top


def build(oracle_ratio=None, cases=None):
    """(the fixture's groups, oracle_ratio, per-group oracle ratios). oracle_ratio given: the decided flags for that constant;
    None: measured here. cases given: the reference on those inputs (tests/test_tri_hard_reference.py passes the fixture's own
    and asks its arrays back); None: tests/tri_hard_cases.py."""
    cases = HC.groups() if cases is None else cases
    measured = None
    if oracle_ratio is None:
        measured = measure_oracle_ratio(cases, {n: MR.evaluate(c, 1.0) for n, c in cases.items()})   # (points and kappa do not depend on C)
        oracle_ratio = max(measured.values())
    C = 8.0 * oracle_ratio
    groups = {name: HR.flatten({k: v for k, v in case.items() if k not in ("point_ptr", "transform_ptr", "uv1", "uv2", "Ts")}, MR.evaluate(case, C))
              for name, case in cases.items()}
    return groups, float(oracle_ratio), measured


def main():
    groups, oracle_ratio, measured = build()
    print(f"oracle_ratio {oracle_ratio:.4g}  (C = {8 * oracle_ratio:.4g})")
    for name, g in groups.items():
        share = HR.undecided_share(g)
        print(f"{name:22s} items {len(g.get('n_undecided', [])):5d}  undecided {share:6.1%}  ladder {bool(g['ladder'])}  oracle ratio {measured.get(name, float('nan')):.3g}")
        assert share <= MAX_UNDECIDED, f"{name}: {share:.1%} of the items are undecided"
        assert bool(g["ladder"]) or share == 0.0, f"{name}: undecided items in a group that is not a ladder"
    path = os.path.join(ROOT, "tests", "golden", "tri_hard_golden.npz")
    np.savez_compressed(path, oracle_ratio=np.float64(oracle_ratio), **HR.pack(groups))
    size = os.path.getsize(path)
    print("bytes", size)
    assert size <= MAX_BYTES, size


if __name__ == "__main__":
    main()
