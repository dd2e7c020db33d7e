"""GPU: the C++ adapters of the track polish (include/eacham/TriangulatorHip.hpp: TriangulateTracksRefined, RefineTrackPoints,
RefinePoint) through tests/cpp/tri_refine_driver.cpp: the composed call against eacham_triangulate_tracks and
eacham_triangulate_refine_tracks called by hand, every field byte for byte; eacham_triangulate_tracks' own outputs as the call alone
gives them; the one-track form against the list; and the polish against the CPU restatement. The tracks (tests/tri_refine_cases.py:
cpp_case): 2..9 noisy views, every fifth with an observation 40 px off (not added, so not refined), a track of one view."""
import os
import struct
import subprocess

import numpy as np
import pytest

import tri_refine_cases as RC
import tri_refine_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
PLAIN = ["points", "status", "masks"]
REFINED = PLAIN + ["refined", "cost_before", "cost_after", "tries", "refine_status", "inliers", "n_inliers"]
BY_HAND = PLAIN + ["refined", "cost", "tries", "refine_status", "inliers", "n_inliers"]
SINGLE = ["refined", "cost_before", "cost_after", "refine_status"]


def build_driver(exe, link):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + CPP,
           os.path.join(CPP, "tri_refine_driver.cpp"), *link, "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def read_groups(path, layout):
    groups = []
    with open(path, "rb") as f:
        for fields in layout:
            rec = {}
            for name in fields:
                n, size = struct.unpack("qq", f.read(16))
                rec[name] = f.read(n * size)
            groups.append(rec)
        assert f.read() == b""
    return groups


@pytest.mark.gpu
def test_the_composed_adapter_equals_the_two_calls_by_hand(tmp_path):
    lib = os.path.join(ROOT, "eacham_amd", "lib")
    exe = build_driver(str(tmp_path / "tri_refine_driver"), ["-L" + lib, "-leacham_hip", "-Wl,-rpath," + lib])
    case = RC.cpp_case()
    c = case["list"]
    n, F = len(c["track_ptr"]) - 1, len(c["transforms"])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("iiiff", n, F, RC.MAX_TRIES, case["max_repr_error"], case["min_tri_angle"]))
        for a in (RC.K, c["track_ptr"], c["transforms"], c["obs_frame"], c["obs_uv"]):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    plain, adapter, hand, single = read_groups(fout, [PLAIN, REFINED, BY_HAND, SINGLE])
    f64 = lambda b: np.frombuffer(b, np.float64)   # noqa: E731
    i32 = lambda b: np.frombuffer(b, np.int32)   # noqa: E731
    # eacham_triangulate_tracks' own outputs are what the call alone gives
    for name in PLAIN:
        assert adapter[name] == plain[name] and hand[name] == plain[name], name
    # the adapter is the two C calls composed by hand
    for name in ("refined", "tries", "refine_status", "inliers", "n_inliers"):
        assert adapter[name] == hand[name], name
    cost = f64(hand["cost"]).reshape(n, 2)
    assert adapter["cost_before"] == np.ascontiguousarray(cost[:, 0]).tobytes() and adapter["cost_after"] == np.ascontiguousarray(cost[:, 1]).tobytes()
    # and the restatement's polish from those points over those masks
    status, masks, points = i32(plain["status"]), np.frombuffer(plain["masks"], np.uint8), f64(plain["points"]).reshape(n, 3)
    added = status == 3
    assert 20 <= added.sum() < n
    want = R.refine_tracks(c["transforms"], c["track_ptr"], c["obs_frame"], c["obs_uv"], RC.K, points, added.astype(np.uint8), masks,
                           RC.MAX_TRIES, case["max_repr_error"])
    assert np.array_equal(f64(adapter["refined"]).view(np.uint64), want.refined.reshape(-1).view(np.uint64))
    assert np.array_equal(cost.view(np.uint64), want.cost.view(np.uint64))
    assert np.array_equal(i32(adapter["tries"]), want.tries) and np.array_equal(i32(adapter["refine_status"]), want.status)
    assert np.array_equal(np.frombuffer(adapter["inliers"], np.uint8), want.masks) and np.array_equal(i32(adapter["n_inliers"]), want.n_inliers)
    rs = i32(adapter["refine_status"])
    assert (rs[added] == R.CONVERGED).all() and (rs[~added] == R.NOT_REFINED).all()
    assert not f64(adapter["refined"]).reshape(n, 3)[~added].any()
    # the one-track form gives the list's bytes
    sp, ss = f64(single["refined"]).reshape(n, 3), i32(single["refine_status"])
    assert np.array_equal(sp[added].view(np.uint64), want.refined[added].view(np.uint64)) and np.array_equal(ss, want.status)
    assert np.array_equal(f64(single["cost_before"])[added].view(np.uint64), np.ascontiguousarray(want.cost[added, 0]).view(np.uint64))
    assert np.array_equal(f64(single["cost_after"])[added].view(np.uint64), np.ascontiguousarray(want.cost[added, 1]).view(np.uint64))
    before, after = want.cost[added, 0].sum(), want.cost[added, 1].sum()
    print(f"{int(added.sum())} of {n} tracks added and refined: cost {before:.1f} -> {after:.1f} px^2, most tries {int(want.tries.max())}")
    assert after < before
