"""GPU: FindEssentialMatBatch / FindHomographyBatch (include/eacham/TwoViewHip.hpp, one eacham_lmeds_batch call for the whole
list) against FindEssentialMat / FindHomography pair by pair, on 6 seeded pairs of different sizes, one of them with fewer than
5 matches: every RobustModel field (the refitted H included) and every LmedsTrace field identical, byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

import score_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
FIELDS = ["model", "mask", "ints(inliers, iterations, ok, candidates, candidate, sample, root)", "median", "samples", "sigma", "threshold", "winner"]
SIZES = [(300, False), (4, False), (57, True), (5, False), (130, True), (301, False)]   # (matches, planar scene)


@pytest.mark.gpu
def test_batch_adapters_equal_the_single_pair_ones(tmp_path):
    exe = str(tmp_path / "twoview_batch_driver")
    lib = os.path.join(ROOT, "eacham_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(CPP, "twoview_batch_driver.cpp"), "-o", exe, "-L" + lib, "-leacham_hip", "-Wl,-rpath," + lib, "-lpthread"],
                   check=True, capture_output=True)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", len(SIZES)))
        cases = [SC.two_view_case(n=max(n, 8), n_models=1, seed=90 + k, outliers=0.25, planar=planar, facing=True) for k, (n, planar) in enumerate(SIZES)]
        K = np.asarray(cases[0]["K"], dtype=np.float64)
        f.write(K.tobytes())
        for (n, _), c in zip(SIZES, cases):
            f.write(struct.pack("i", n)); f.write(np.ascontiguousarray(c["uv1"][:n]).tobytes()); f.write(np.ascontiguousarray(c["uv2"][:n]).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    item = {"model": 8, "mask": 1, "ints": 4, "median": 4, "samples": 4, "sigma": 8, "threshold": 4, "winner": 8}
    groups = []
    with open(fout, "rb") as f:
        for _ in range(4):                                   # E batch, E single, H batch, H single
            recs = []
            for _ in SIZES:
                rec = []
                for name in FIELDS:
                    count = struct.unpack("q", f.read(8))[0]
                    rec.append(f.read(count * item[name.split("(")[0]]))
                recs.append(rec)
            groups.append(recs)
        assert f.read() == b""
    P = len(SIZES)
    for what, batch, single in (("E", groups[0], groups[1]), ("H", groups[2], groups[3])):
        oks = []
        for p in range(P):
            for name, g, w in zip(FIELDS, batch[p], single[p]):
                assert g == w, f"{what} pair {p} ({SIZES[p][0]} matches): {name} differs"
            ints = np.frombuffer(single[p][2], np.int32)
            oks.append(int(ints[2]))
            if ints[2]:
                assert len(single[p][1]) == SIZES[p][0] and int(np.frombuffer(single[p][1], np.uint8).sum()) == ints[0]
        assert oks[0] == 1 and oks[5] == 1, (what, oks)
        if what == "E":                                      # the pair with 4 matches has no essential matrix and drew no samples
            assert oks[1] == 0 and np.frombuffer(single[1][2], np.int32)[1] == 0 and single[1][4] == b""
    assert np.frombuffer(groups[0][0][2], np.int32)[1] == 89 and np.frombuffer(groups[2][0][2], np.int32)[1] == 72   # LMedS' fixed budgets
