"""GPU: the batch adapters of PnP registration — SolvePnPRansacBatch (include/eacham/PnPHip.hpp: rounds + 1 device calls for the
whole list) and ReconstructionManagerHip::RecoverPosePnPBatch (include/eacham/ReconstructionHip.hpp) — against SolvePnPRansac
problem by problem, under both samplings, and against RecoverPosePnP on the pairs one after another, on the stand-ins of
tests/cpp/ref_standins.hpp (tests/cpp/pnp_batch_driver.cpp). The problems are tests/pnp_batch_cases.py: rounds — one that ends
inside the first chunk, one that needs several, one below 5 points (and below minPnpInliers), a collinear one, a coplanar one:
five candidate frames for one map. Every field identical, byte for byte: ok, R, rvec, t, inliers, iterations and the trace; the
returned flags, every node transform, the validity flags and the factor transforms."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pnp_batch_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
RESULT = ["ok", "R", "rvec", "t", "inliers", "iterations", "samples", "winner"]
NODE = ["flag", "transform", "valid", "factor"]
MIN_PNP_INLIERS = 30


def build_driver(exe, link):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + CPP,
           os.path.join(CPP, "pnp_batch_driver.cpp"), *link, "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def write_input(path, case, iterations):
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(case["X"])))
        f.write(np.ascontiguousarray(case["K"], dtype=np.float64).tobytes())
        f.write(struct.pack("ii", iterations, MIN_PNP_INLIERS))
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
def test_batch_adapters_equal_the_single_problem_ones(tmp_path):
    lib = os.path.join(ROOT, "eacham_amd", "lib")
    exe = build_driver(str(tmp_path / "pnp_batch_driver"), ["-L" + lib, "-leacham_hip", "-Wl,-rpath," + lib])
    case = PC.rounds()
    P = len(case["X"])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_input(fin, case, case["max_iters"])
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    s_cv, b_cv, s_ctr, b_ctr, seq, bat = read_groups(fout, [RESULT] * 4 + [NODE] * 2, P)
    i32 = lambda b: int(np.frombuffer(b, np.int32)[0])   # noqa: E731
    for what, got, want, fields in (("SolvePnPRansacBatch / OpenCV", b_cv, s_cv, RESULT), ("SolvePnPRansacBatch / Counter", b_ctr, s_ctr, RESULT),
                                    ("RecoverPosePnPBatch", bat, seq, NODE)):
        for p, (g, w) in enumerate(zip(got, want)):
            for name in fields:
                assert g[name] == w[name], f"{what}, problem {p} ({len(case['uv'][p])} points): {name} differs"
    for single in (s_cv, s_ctr):                               # the single path does what the cases are for
        assert [i32(x["ok"]) for x in single] == [1, 1, 0, 0, 1]
        assert 0 < i32(single[0]["iterations"]) <= PC.CHUNK < i32(single[1]["iterations"]) and i32(single[2]["iterations"]) == 0
        assert i32(single[3]["iterations"]) == case["max_iters"] and i32(single[3]["winner"]) == -1
        assert len(single[0]["inliers"]) // 4 > 64 >= len(single[1]["inliers"]) // 4 >= 5
    assert [i32(x["flag"]) for x in seq] == [1, 1, 0, 0, 1] == [i32(x["valid"]) for x in seq]
    assert len(case["uv"][2]) < MIN_PNP_INLIERS <= len(case["uv"][3])        # one frame below minPnpInliers, one refused by the estimator
