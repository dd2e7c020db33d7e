"""CPU: the grid of match_argmin_kernel as the driver sizes it (eacham_amd/csrc/match_plan.hpp: argmin_grid), compiled with g++ and
executed by tests/cpp/argmin_grid_driver.cpp on plain numbers.

The kernel is one wave per workgroup, persistent over a list whose length only the device knows; it holds 100 VGPRs, so sixteen of its
waves fill a CU. Stated here independently of the header: a launch with the chip to itself gets min(nb x wgs_per_pair, 16 x CUs)
workgroups — on the 256 CUs of an MI355X the 4 096 of every build before — and a launch whose tail runs beside the next screen sweep
half of that; never less than one workgroup, never more than nb x wgs_per_pair, the upper bound of the list's length."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("argmin_grid") / "argmin_grid_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "argmin_grid_driver.cpp")],
                   check=True, capture_output=True)

    def run(cases):
        r = subprocess.run([exe], input="".join("%d %d %d %d\n" % c for c in cases), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-400:]
        out = [int(x) for x in r.stdout.split()]
        assert len(out) == len(cases)
        return out
    return run


def test_the_headline_launches(grid):
    # S200: 9 344 + 9 344 + 1 212 pairs of 63 tiles (8 workgroups per pair) on 256 CUs: the first two tails run beside a sweep
    assert grid([(9344, 8, 256, 1), (9344, 8, 256, 1), (1212, 8, 256, 0)]) == [2048, 2048, 4096]
    assert grid([(9344, 8, 256, 0)]) == [4096]                   # the same launch with the chip to itself: the grid it always had


def test_against_the_rule_stated_alone(grid):
    cases = [(nb, wgs, cus, beside) for nb in (0, 1, 2, 11, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1212, 9344, 300000)
             for wgs in (1, 3, 8, 63) for cus in (1, 8, 64, 104, 256, 304) for beside in (0, 1)]
    got = grid(cases)
    for (nb, wgs, cus, beside), g in zip(cases, got):
        want = max(1, min(max(nb * wgs, 1), cus * (8 if beside else 16)))
        assert g == want, (nb, wgs, cus, beside, g, want)
        assert 1 <= g <= max(nb * wgs, 1)
    # half the round beside a sweep wherever the list can be that long, the same grid where it cannot
    by = dict(zip(cases, got))
    for (nb, wgs, cus, beside), g in by.items():
        if beside:
            alone = by[nb, wgs, cus, 0]
            assert g == alone if nb * wgs <= 8 * cus else g == 8 * cus and alone == min(nb * wgs, 16 * cus)


def test_large_jobs_do_not_overflow(grid):
    assert grid([(2 ** 31 - 1, 63, 256, 0), (2 ** 31 - 1, 63, 256, 1), (40000000, 64, 304, 0)]) == [4096, 2048, 4864]
