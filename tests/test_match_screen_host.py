"""CPU: the FP6 grid and the bound arithmetic of the 256-D screen sweep (eacham_amd/csrc/match_screen.hpp), compiled on its own with
g++ and EXECUTED by tests/cpp/match_screen_driver.cpp: every value 0..255 gets the nearest grid value, the 64 codes round-trip and
are symmetric in sign, the dense 6-bit packing round-trips, and L1 <= d2 <= U2 holds on seeded random row pairs (half-normal and
uniform values, 16 / 129 / 160 / 255 / 256 dimensions) and on the extremes (all 0, all 255, values midway between grid points at
every step size), with the row's own quantisation error and with the frame maximum; the clamp and the L1 = 0 case."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("screen") / "match_screen_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "match_screen_driver.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    return json.loads(r.stdout)


def test_grid_codes_and_bounds_hold(report):
    assert report["bad"] == 0, report
    assert report["pairs"] >= 4000
    assert report["max_err"] == 8          # the coarsest grid step is 16: no value is further than 8 from its grid value


def test_the_edge_cases_were_met(report):
    assert report["l_zero"] > 0 and report["clamped"] > 0   # pairs with L1 = 0 and pairs whose U2 hit the clamp were among them
    assert report["worst_l"] >= 0 and report["worst_u"] >= 0
