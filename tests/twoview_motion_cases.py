"""The seeded pairs of tests/test_twoview_motion_gpu.py and their wire form for tests/cpp/twoview_motion_driver.cpp (shared with the
CPU check that the pairs reach both branches of RecoverPoseTwoView, tests/test_twoview_motion_reference.py)."""
import os
import struct
import subprocess

import numpy as np

import score_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
# (matches, planar scene, gross outliers): planar and non-planar pairs, one with fewer than 5 matches, the sizes 57, 130, 300, 301.
# The LMedS masks are scale-free, so a wholly planar and a wholly general scene both give H_E_ratio ~ 1 and take the homography
# branch (include/eacham/ReconstructionHip.hpp says why). planar = a fraction in (0, 1) puts that share of the matches on the plane
# and leaves the rest in general position: the homography's median then sits on the plane, its mask keeps the plane's matches
# only, the ratio falls below 0.9 and the pair takes the essential branch.
PAIRS = [(300, False, 0.25), (4, False, 0.25), (57, True, 0.25), (130, True, 0.25), (301, False, 0.25), (120, False, 0.25), (130, 0.6, 0.1),
         (301, 0.6, 0.0)]
SINGLE = ["transform", "ids", "points", "branch"]
POSE = ["R", "t", "good", "mask"]
ITEM = {"transform": 8, "ids": 4, "points": 8, "branch": 4, "R": 8, "t": 8, "good": 4, "mask": 1}


def write_input(path):
    cases = []
    for k, (n, planar, o) in enumerate(PAIRS):
        c = SC.two_view_case(n=max(n, 8), n_models=1, seed=190 + k, outliers=o, planar=bool(planar), facing=True)
        if 0 < planar < 1:   # the same cameras and landmarks (same seed), the landmarks left where they were: the rows beyond the plane's share
            g = SC.two_view_case(n=max(n, 8), n_models=1, seed=190 + k, outliers=o, planar=False, facing=True)
            on = np.arange(len(c["uv1"])) % 5 < round(5 * planar)
            c = dict(c, uv1=np.where(on[:, None], c["uv1"], g["uv1"]), uv2=np.where(on[:, None], c["uv2"], g["uv2"]))
        cases.append(c)
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(PAIRS)))
        f.write(np.asarray(cases[0]["K"], dtype=np.float64).tobytes())
        for (n, _, _), c in zip(PAIRS, cases):
            f.write(struct.pack("i", n))
            f.write(np.ascontiguousarray(c["uv1"][:n]).tobytes())
            f.write(np.ascontiguousarray(c["uv2"][:n]).tobytes())


def build_driver(exe, link, defines=()):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + CPP, *["-D" + d for d in defines],
           os.path.join(CPP, "twoview_motion_driver.cpp"), *link, "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def read_groups(path, layout):
    """layout: the field lists of the groups in file order; one record per directed pair (two per pair) in each group."""
    groups = []
    with open(path, "rb") as f:
        for fields in layout:
            recs = []
            for _ in range(2 * len(PAIRS)):
                rec = {}
                for name in fields:
                    count = struct.unpack("q", f.read(8))[0]
                    rec[name] = f.read(count * ITEM[name])
                recs.append(rec)
            groups.append(recs)
        assert f.read() == b""
    return groups


def branches(single):
    return [int(np.frombuffer(r["branch"], np.int32)[0]) for r in single]


def assert_coverage(single, pose):
    """What the set of pairs is for, on the records of the single-pair path."""
    br = branches(single)
    kept = [len(r["ids"]) // 8 for r in single]
    sizes = [n for n, _, _ in PAIRS for _ in range(2)]
    assert {57, 130, 300, 301} <= set(sizes) and min(sizes) < 5 and len(PAIRS) >= 6
    assert br.count(1) >= 4 and br.count(0) >= 4 and br.count(-1) == 2                    # both branches, in both directions; the 4-match pair
    assert all(b == -1 for b, n in zip(br, sizes) if n < 5) and all(k == 0 for k, b in zip(kept, br) if b == -1)
    assert any(b == 1 and k > 20 for b, k in zip(br, kept)) and any(b == 1 and k == 0 for b, k in zip(br, kept))   # a solution accepted / none
    assert all(k > 20 for k, b in zip(kept, br) if b == 0)
    for r, n in zip(pose, sizes):
        assert len(r["mask"]) == n and int(np.frombuffer(r["mask"], np.uint8).sum()) == int(np.frombuffer(r["good"], np.int32)[0])
