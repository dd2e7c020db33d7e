"""GPU: the C++ adapters of the PnP polish (include/eacham/PnPHip.hpp: SolvePnPRansacRefined[Batch], RefinePnPBatch;
include/eacham/PnPP3PHip.hpp: SolvePnPRansacP3PRefined[Batch]) through tests/cpp/pnp_refine_driver.cpp: the list forms against the
per-problem calls, every field byte for byte; the polish against the CPU restatement run from the plain RANSAC result on its inliers;
and a frame of exactly four correspondences, which the P3P form returns polished where EPnP's refit has nothing to say. The problems
(tests/pnp_refine_cases.py: cpp_case): 300 points with outliers, 60 with more, 4 exact points, 3 points (turned away), a planar
scene, 4 noisy points."""
import os
import subprocess

import numpy as np
import pytest

import pnp_refine_cases as RC
import pnp_refine_reference as R
from test_p3p_cpp_gpu import read_groups, write_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
PLAIN = ["ok", "R", "rvec", "t", "inliers", "iterations"]
REFINED = PLAIN + ["cost_before", "cost_after", "tries", "status"]


def build_driver(exe, link):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + CPP,
           os.path.join(CPP, "pnp_refine_driver.cpp"), *link, "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.gpu
def test_the_batch_adapters_equal_the_single_ones_and_four_points_come_back_polished(tmp_path):
    lib = os.path.join(ROOT, "eacham_amd", "lib")
    exe = build_driver(str(tmp_path / "pnp_refine_driver"), ["-L" + lib, "-leacham_hip", "-Wl,-rpath," + lib])
    case = RC.cpp_case()
    P = len(case["X"])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_input(fin, case, case["max_iters"])
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    plain, s_p3p, b_p3p, s_epnp, b_epnp, rb = read_groups(fout, [PLAIN] + [REFINED] * 5, P)
    i32 = lambda b: int(np.frombuffer(b, np.int32)[0])   # noqa: E731
    f64 = lambda b: np.frombuffer(b, np.float64)   # noqa: E731
    for what, got, want in (("P3P", b_p3p, s_p3p), ("EPnP", b_epnp, s_epnp), ("RefinePnPBatch", rb, s_p3p)):
        for p, (g, w) in enumerate(zip(got, want)):
            for name in REFINED:
                assert g[name] == w[name], f"{what}, problem {p} ({len(case['uv'][p])} points): {name} differs"
    assert [i32(x["ok"]) for x in s_p3p] == [1, 1, 1, 0, 1, 1] and [i32(x["ok"]) for x in s_epnp] == [1, 1, 0, 0, 1, 0]
    # the polish leaves ok, inliers and iterations as the RANSAC call gave them, and is the restatement's from that pose on those rows
    poses = np.array([np.concatenate([f64(b["R"]), f64(b["t"])]) for b in plain])
    has = np.array([i32(b["ok"]) for b in plain], np.uint8)
    use = []
    for p, b in enumerate(plain):
        m = np.zeros(len(case["uv"][p]), np.uint8)
        m[np.frombuffer(b["inliers"], np.int32)] = 1
        use.append(m)
    want = R.refine_batch(case["X"], case["uv"], RC.K, poses, has, use, RC.MAX_TRIES, RC.THR)
    for p, (s, b) in enumerate(zip(s_p3p, plain)):
        for name in ("ok", "inliers", "iterations"):
            assert s[name] == b[name], (p, name)
        assert i32(s["status"]) == want.status[p] and i32(s["tries"]) == want.tries[p], p
        assert np.array_equal(f64(s["cost_before"]).view(np.uint64), want.cost[p, :1].view(np.uint64)), p
        assert np.array_equal(f64(s["cost_after"]).view(np.uint64), want.cost[p, 1:].view(np.uint64)), p
        if has[p]:
            assert np.array_equal(np.concatenate([f64(s["R"]), f64(s["t"])]).view(np.uint64), want.refined[p].view(np.uint64)), p
    # the four-correspondence frames: registered by P3P, polished by the LM loop (EPnP's refit needs five rows)
    for p in (2, 5):
        s = s_p3p[p]
        assert len(case["uv"][p]) == 4 and len(s["inliers"]) // 4 == 4 and i32(s["status"]) == R.CONVERGED and i32(s["tries"]) >= 1, p
        assert i32(s_epnp[p]["status"]) == R.NOT_REFINED and i32(s_epnp[p]["tries"]) == 0, p
    s, b = s_p3p[5], plain[5]
    before, after = float(f64(s["cost_before"])[0]), float(f64(s["cost_after"])[0])
    print(f"four noisy correspondences: cost {before:.4f} -> {after:.4f} px^2 in {i32(s['tries'])} tries")
    assert after < before and s["R"] != b["R"] and s["t"] != b["t"]
    for p in (0, 1, 4):
        for s in (s_p3p[p], s_epnp[p]):
            before, after = float(f64(s["cost_before"])[0]), float(f64(s["cost_after"])[0])
            pose = np.concatenate([f64(s["R"]), f64(s["t"])])
            print(f"problem {p}: {len(s['inliers']) // 4} inliers, cost {before:.2f} -> {after:.2f} px^2 in {i32(s['tries'])} tries, "
                  f"pose error {float(np.abs(pose - case['T'][p]).max()):.2e}")
            assert i32(s["status"]) == R.CONVERGED and after <= before, p
