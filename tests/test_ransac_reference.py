"""CPU: what eacham_ransac_batch rests on, held without a GPU.

1. The budget rows (eacham_amd/csrc/ransac_rule.hpp: ransac_budget_row, built by the stand-alone tests/cpp/ransac_rule_driver.cpp) for
   every (n, m, confidence) of tests/ransac_cases.py, at the cap the library builds them with (the largest sample count of the
   case's call) and at 100 and 1000: B[g] is estimator_reference.update_num_iters at (n - g) / n, the identity
   update_num_iters(c, (n - g) / n, m, cur) == min(cur, B[g]) for every cur up to the cap, and B non-increasing in g.
2. The rule on the rows — the walk the device runs, the order-free form (stated in the driver) and the two-pass use of the walk for
   several stage1 — against the sequential loop that calls ransac_update_num_iters itself, on 20 000 random count sequences with
   multi-root samples; once more in an AddressSanitizer + UBSan build of the same stand-alone program.
3. The cases hold what they are for (through the reference, before the GPU test relies on it), and on `heavy` the threshold rule
   keeps at most a fifth of the outliers LMedS keeps.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import estimator_reference as ER
import ransac_cases as RC
import ransac_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "ransac_rule_driver.cpp")
CAPS = (100, 1000)


def build_driver(tmp, flags=()):
    exe = os.path.join(tmp, "ransac_rule_driver" + ("_san" if flags else ""))
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("ransac_rule")))


def row(driver, confidence, n, m, cap):
    r = subprocess.run([driver, "row", repr(confidence), str(n), str(m), str(cap)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [int(x) for x in r.stdout.split()]


def test_the_budget_rows_are_the_update_function(driver):
    """Every row with the cap the library builds it with (the largest sample count of the case's call), and with caps 100 and 1000."""
    rows = RC.every_row_the_library_builds()
    own_caps = {cap for _, _, _, cap in rows}
    assert {6, 12, 200, 300} <= own_caps                                                                 # mixed, single, early_stop, heavy
    todo = sorted(set(rows) | {(n, m, c, cap) for n, m, c, _ in rows for cap in CAPS})
    checked = 0
    for n, m, confidence, cap in todo:
        B = row(driver, confidence, n, m, cap)
        assert len(B) == n + 1
        assert all(B[g] >= B[g + 1] for g in range(n)), (n, m, confidence, cap)                         # non-increasing in g
        curs = sorted(c for c in set(range(0, 40)) | {cap // 2, cap - 1, cap} if 0 <= c <= cap)
        for g in range(n + 1):
            ep = (n - g) / n
            assert B[g] == ER.update_num_iters(confidence, ep, m, cap), (n, m, confidence, cap, g)
            for cur in curs:
                assert ER.update_num_iters(confidence, ep, m, cur) == min(cur, B[g]), (n, m, confidence, cap, g, cur)
                checked += 1
    assert checked > 100000


def test_the_rule_on_the_rows_is_the_sequential_loop(driver):
    r = subprocess.run([driver, "fuzz", "20241", "20000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    s = json.loads(r.stdout)
    assert s["trials"] == 20000 and s["mismatches"] == 0
    assert s["multi_root"] > 5000 and s["early_stop"] > 2000 and s["late_root_past_budget"] > 20, s   # the sequences reach what they are for


def test_the_rule_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = build_driver(str(tmp_path), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))
    r = subprocess.run([exe, "fuzz", "7", "4000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert json.loads(r.stdout)["mismatches"] == 0
    assert subprocess.run([exe, "row", "0.999", "257", "5", "1000"], capture_output=True, text=True).returncode == 0


def test_the_cases_hold_what_they_are_for():
    for kind in RC.KINDS:
        emp = RR.ransac_case(RC.empties(kind))
        assert [e["winner"][0] >= 0 for e in emp] == [True, False, False, True]
        assert emp[1]["n_used"] == 0 and emp[2]["n_used"] == 0 and len(RC.empties(kind)["samples"][2]) == 2     # no samples / samples not looked at
        deg = RR.ransac_case(RC.degenerate(kind))
        assert deg[0]["winner"][0] >= 0 and deg[1]["winner"] == (-1, -1, -1) and deg[1]["candidates"] == 0 and deg[1]["n_used"] == 2
        tie = RC.ties(kind)
        for p, t in enumerate(RR.ransac_case(tie)):
            rows = tie["samples"][p]
            first = min(s for s in range(len(rows)) if np.array_equal(rows[s], rows[t["winner"][1]]))
            assert t["winner"][1] == first and sum(np.array_equal(r, rows[first]) for r in rows) == 2           # its twin tied and lost, or was not reached
        early = RC.early_stop(kind)
        assert all(e["winner"][0] >= 0 and 4 * e["n_used"] < len(s) for e, s in zip(RR.ransac_case(early), early["samples"]))
        bnd = RR.ransac_case(RC.boundary(kind))
        assert [b["winner"][1] for b in bnd] == [RC.BOUNDARY_STAGE1 - 1, RC.BOUNDARY_STAGE1]
        none = RR.ransac_case(RC.no_record(kind))[0]
        assert none["winner"] == (-1, -1, -1) and none["candidates"] > 0 and none["n_used"] == 12 and not none["mask"].any()
        mix = RR.ransac_case(RC.mixed(kind))
        assert [x["winner"][0] >= 0 for x in mix] == [True, kind != "fundamental", True, True, True]
    trace = []
    multi = RR.ransac_case(RC.multi_root(), trace)
    assert RC.is_multi_root_record(trace[0]) and multi[0]["winner"][2] > 0     # a later root of the record's own sample won past the budget
    assert multi[0]["n_used"] == multi[0]["winner"][1] + 1


@pytest.mark.parametrize("kind", ["homography", "essential"])
def test_on_heavy_outliers_the_threshold_rule_keeps_a_fifth_of_what_lmeds_keeps(kind, capsys):
    case = RC.heavy(kind)
    for p, r in enumerate(RR.ransac_case(case)):
        bad = case["bad"][p]
        lmeds = ER.lmeds(kind, case["uv1"][p], case["uv2"][p], case["K"], case["samples"][p])
        bad_ransac, bad_lmeds = int((r["mask"].astype(bool) & bad).sum()), int((lmeds["mask"].astype(bool) & bad).sum())
        with capsys.disabled():
            print(f"\n  {kind} outliers {bad.mean():.2f}: true inliers {int((~bad).sum())}, RANSAC good / bad {int((r['mask'].astype(bool) & ~bad).sum())} / {bad_ransac}"
                  f" ({r['n_used']} samples), LMedS good / bad {int((lmeds['mask'].astype(bool) & ~bad).sum())} / {bad_lmeds}")
        assert 5 * bad_ransac < bad_lmeds
