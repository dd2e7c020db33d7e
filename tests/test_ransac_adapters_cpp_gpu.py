"""GPU: the C++ adapters of threshold RANSAC (include/eacham/TwoViewHip.hpp: Find*Ransac / Find*RansacBatch, GraphVerifyHip.hpp:
Verify*Ransac) through tests/cpp/ransac_adapter_driver.cpp, compiled with the host compiler against libeacham_hip.so: the batch forms
against the single-pair forms field for field, the resident-graph forms against the batch forms on host-gathered points (pairs
of exactly m matches included), the retained mask as the track builder's `keep` — under both sample streams and for stage1 = default, 3 and a single pass."""
import os
import subprocess

import pytest

import graph_verify_cases as GC
import test_graph_verify_gpu as GV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ransac_cpp") / "ransac_adapter_driver")
    lib = os.path.join(ROOT, "eacham_amd", "lib")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + CPP,
           os.path.join(CPP, "ransac_adapter_driver.cpp"), "-L" + lib, "-leacham_hip", "-Wl,-rpath," + lib, "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("name", ["eight", "small"])
def test_batch_single_and_resident_forms_agree_field_for_field(driver, tmp_path, name):
    g = getattr(GC, name)()
    case = str(tmp_path / "case.bin")
    GV.write_case(case, g)
    r = subprocess.run([driver, case], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and not [ln for ln in lines if ln.startswith("DIFFERENT")], r.stdout[-3000:] + r.stderr[-2000:]
    P = len(g["counts"])
    skipped = sum(int((g["counts"] == m).sum()) for m in (5, 7))      # without the points a pair of exactly m matches is the device rule's
    assert len([ln for ln in lines if ln.startswith("same")]) == 6 * (3 * P + 3 * P + 2 * P - skipped + 1)
    info = [ln for ln in lines if ln.startswith("info") and "pairs_with_a_model" in ln]
    assert len(info) == 6
    for ln in info:
        tok = ln.split()
        found = {k: int(tok[tok.index(k) + 1]) for k in ("essential", "fundamental", "homography")}
        assert all(v > 0 for v in found.values()), ln
        if name == "eight":
            assert found["essential"] == P and found["fundamental"] == P, ln
    if name == "eight":
        assert all(int(ln.split()[-1]) > 0 for ln in lines if ln.startswith("info tracks"))
