"""GPU: the C++ adapters of the P3P form of PnP RANSAC (include/eacham/PnPP3PHip.hpp) — SolvePnPRansacP3PBatch, rounds + 1 device
calls for the whole list, against SolvePnPRansacP3P problem by problem, under both samplings (tests/cpp/p3p_driver.cpp): every field
identical, byte for byte — ok, R, rvec, t, inliers, iterations and the trace — and, the pixels being exact, the recovered pose
within 1e-6 of the truth. The problems (tests/p3p_cases.py: cpp_case): one that ends inside the first chunk, one with 70 % outliers,
one of exactly 4 points (a winner and no refit), one of 3 points (turned away), a planar one."""
import os
import struct
import subprocess

import numpy as np
import pytest

import p3p_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
RESULT = ["ok", "R", "rvec", "t", "inliers", "iterations", "samples", "winner"]


def build_driver(exe, link):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + CPP,
           os.path.join(CPP, "p3p_driver.cpp"), *link, "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def write_input(path, case, iterations):
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(case["X"])))
        f.write(np.ascontiguousarray(case["K"], dtype=np.float64).tobytes())
        f.write(struct.pack("i", iterations))
        for X, uv in zip(case["X"], case["uv"]):
            f.write(struct.pack("i", len(uv)))
            f.write(np.ascontiguousarray(X, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(uv, dtype=np.float64).tobytes())


def read_groups(path, layout, P):
    groups = []
    with open(path, "rb") as f:
        for fields in layout:
            recs = []
            for _ in range(P):
                rec = {}
                for name in fields:
                    n, size = struct.unpack("qq", f.read(16))
                    rec[name] = f.read(n * size)
                recs.append(rec)
            groups.append(recs)
        assert f.read() == b""
    return groups


@pytest.mark.gpu
def test_the_batch_adapter_equals_the_single_problem_one_and_finds_the_pose(tmp_path):
    lib = os.path.join(ROOT, "eacham_amd", "lib")
    exe = build_driver(str(tmp_path / "p3p_driver"), ["-L" + lib, "-leacham_hip", "-Wl,-rpath," + lib])
    case = PC.cpp_case()
    P = len(case["X"])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_input(fin, case, case["max_iters"])
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    s_cv, b_cv, s_ctr, b_ctr = read_groups(fout, [RESULT] * 4, P)
    i32 = lambda b: int(np.frombuffer(b, np.int32)[0])   # noqa: E731
    for what, got, want in (("OpenCV sampling", b_cv, s_cv), ("Counter sampling", b_ctr, s_ctr)):
        for p, (g, w) in enumerate(zip(got, want)):
            for name in RESULT:
                assert g[name] == w[name], f"{what}, problem {p} ({len(case['uv'][p])} points): {name} differs"
    for single in (s_cv, s_ctr):
        assert [i32(x["ok"]) for x in single] == [1, 1, 1, 0, 1]
        assert 0 < i32(single[0]["iterations"]) <= PC.CHUNK and i32(single[3]["iterations"]) == 0 and i32(single[3]["winner"]) == -1
        assert len(single[2]["inliers"]) // 4 == 4 and len(single[0]["inliers"]) // 4 > 64
        for p in (0, 1, 2, 4):
            pose = np.concatenate([np.frombuffer(single[p]["R"], np.float64), np.frombuffer(single[p]["t"], np.float64)])
            err = float(PC.pose_error(pose, case["T"][p])[0])
            print(f"problem {p}: {len(single[p]['inliers']) // 4} inliers after {i32(single[p]['iterations'])} samples, pose error {err:.3e}")
            assert err <= 1e-6, p
            truth = np.nonzero(np.abs(PC.project(case["X"][p], case["T"][p]) - case["uv"][p]).max(1) < 1e-6)[0]
            assert set(truth) <= set(np.frombuffer(single[p]["inliers"], np.int32))
