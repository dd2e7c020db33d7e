"""CPU: the workspace sizes devprim.hpp announces (scan_ws_elems, radix_nseg, radix_ws_ints), printed by the host-only mode
of tests/cpp/devprim_driver.hip (no HIP call), against what the passes use — derived in tests/devprim_cases.py from the
segment size, the scan tile and the pass rule as DESIGN.md §4.1a states them, not by calling the code under test."""
import os
import subprocess

import numpy as np
import pytest

import devprim_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "eacham_amd", "lib", "exp", "devprim_driver")
N_MAX = (1 << 30) // 1024 * DC.RS_SEG    # 2^30 histogram entries (the limit tracks.hip documents) = 2^20 segments


@pytest.fixture(scope="module")
def info():
    if not os.path.isfile(DRIVER):
        pytest.skip("eacham_amd/lib/exp/devprim_driver is not built (build() makes it)")
    rng = np.random.default_rng(2024)
    ns = set(DC.SCAN_SIZES) | set(DC.SORT_SIZES) | {DC.SORT_LARGE, (1 << 30) // 1024, N_MAX - 1, N_MAX}
    ns |= {int(v) for v in rng.integers(0, (1 << 30) // 1024 + 1, 300)} | {int(v) for v in rng.integers(0, N_MAX + 1, 300)}
    ns |= {k * DC.RS_SEG + d for k in (1, 4, 16, 4096, 4097) for d in (-1, 0, 1)}
    ns = sorted(ns)
    r = subprocess.run([DRIVER, "--host-info"] + [str(n) for n in ns], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = [tuple(int(t) for t in line.split()) for line in r.stdout.splitlines()]
    assert [row[0] for row in rows] == ns
    return rows


def test_radix_workspace_covers_the_widest_pass(info):
    for n, _, nseg, ws in info:
        assert nseg == -(-n // DC.RS_SEG), n
        assert ws >= DC.radix_ws_needed(n), n


def test_radix_workspace_is_non_decreasing(info):
    ws = [row[3] for row in info]
    assert all(a <= b for a, b in zip(ws, ws[1:]))


def test_scan_workspace_holds_one_sum_per_tile(info):
    for n, scan_ws, _, _ in info:
        assert scan_ws >= -(-n // 2048), n
