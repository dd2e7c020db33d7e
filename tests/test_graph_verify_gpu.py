"""GPU: eacham_graph_set_keypoints / eacham_graph_verify / eacham_graph_tracks_verified (eacham_amd/csrc/graph_verify.hip) against the
host composition the project already has, on the same context: the numpy gather of every pair's matches, the project's own
lmeds_samples / draw_samples compiled for the host (tests/graph_verify_cases.py: host_samples), eacham_lmeds_batch. Everything has an
exact answer — doubles are copied, the sample streams are integer recurrences, the lb_* kernels are the ones eacham_lmeds_batch runs —
so EVERY output is compared as bytes; no tolerance anywhere. The output arrays are preset to 85 before every call: an entry the call
should have written and did not (a gap of the mask, a sample slot behind a pair's count) shows."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import graph_verify_cases as GC
from eacham_amd import ResidentGraph, capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SC_MAX_LDS = 16384
KIND_CODE = {"homography": capi.SOLVE_HOMOGRAPHY4, "essential": capi.SOLVE_ESSENTIAL5}
SAMPLING_CODE = {"opencv": capi.SAMPLING_OPENCV, "counter": capi.SAMPLING_COUNTER}
PRESET = 0x55
FIELDS = ["models", "medians", "thresholds", "inliers", "masks", "winner", "n_candidates", "n_samples", "samples"]


def resident(ctx, g):
    rg = ResidentGraph(ctx, g["n_frames"], g["pairs"], g["counts"], g["offsets"], g["q"], g["t"], g["n_kp"])
    rg.set_keypoints(g["xy"])
    return rg


@pytest.fixture(scope="module")
def graphs(hip_ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = resident(hip_ctx, getattr(GC, name)())
        return made[name]

    yield get
    for rg in made.values():
        rg.close()


_expected = {}


def expected(ctx, name, kind, K, sampling, iterations, seeded):
    """The host composition, computed once per combination and left unchanged: dict of the arrays eacham_graph_verify returns."""
    key = (name, kind, K is not None, sampling, iterations, seeded)
    if key not in _expected:
        g, m = getattr(GC, name)(), GC.M[kind]
        pts = GC.gather(g)
        seeds = g["seeds"] if seeded else np.full(len(pts), 12345, dtype=np.uint64)
        samples = GC.host_samples(pts, m, kind == "homography", sampling, iterations, seeds)
        lb = ctx.lmeds_batch(kind, [a for a, _ in pts], [b for _, b in pts], samples, K)
        masks = np.zeros(g["n_src"], dtype=np.uint8)
        for p, mk in enumerate(lb.masks):
            masks[int(g["offsets"][p]):int(g["offsets"][p]) + len(mk)] = mk
        fixed, n_samples = GC.fixed_stride(samples, iterations, m)
        _expected[key] = dict(models=lb.models, medians=lb.medians, thresholds=lb.thresholds, inliers=lb.inliers, masks=masks, winner=lb.winner,
                              n_candidates=lb.n_candidates, n_samples=n_samples, samples=fixed)
        for v in _expected[key].values():
            v.setflags(write=False)
    return _expected[key]


def verify(rg, g, kind, K, sampling, iterations, seeded, retain=False):
    return rg._verify_raw(KIND_CODE[kind], GC.M[kind], K, SAMPLING_CODE[sampling], iterations, g["seeds"] if seeded else None, retain, True, preset=PRESET)


def assert_same(got, want, label):
    for name in FIELDS:
        a, b = getattr(got, name), want[name]
        assert a.dtype == b.dtype and a.shape == b.shape, f"{label}: {name}"
        assert a.tobytes() == b.tobytes(), f"{label}: {name} differs at {np.flatnonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8))[:8]}"


@pytest.mark.parametrize("seeded", [True, False], ids=["seeds", "seeds_null"])
@pytest.mark.parametrize("iterations", GC.ITERATIONS)
@pytest.mark.parametrize("sampling", ["opencv", "counter"])
@pytest.mark.parametrize("kind", ["homography", "essential", "essential_noK"])
def test_every_output_equals_the_host_composition(hip_ctx, graphs, kind, sampling, iterations, seeded):
    g, rg = GC.small(), graphs("small")
    K = GC.K4 if kind == "essential" else None
    kind = kind.split("_")[0]
    want = expected(hip_ctx, "small", kind, K, sampling, iterations, seeded)
    got = verify(rg, g, kind, K, sampling, iterations, seeded)
    assert_same(got, want, f"{kind}/{sampling}/{iterations}")
    m = GC.M[kind]
    used = np.zeros(g["n_src"], dtype=bool)
    for p in range(len(g["counts"])):
        used[int(g["offsets"][p]):int(g["offsets"][p] + g["counts"][p])] = True
    assert (~used).sum() == 3 * (len(g["counts"]) - 1) and not got.masks[~used].any()           # the gaps of the caller's offsets: zero
    draws = (g["counts"] >= m) & (iterations > 0)
    if kind == "homography" and sampling == "opencv":
        draws[GC.COLLINEAR] = False                                                              # getSubset gives up at once
    assert np.array_equal(got.n_samples, np.where(draws, iterations, 0))
    for p in np.flatnonzero(~draws):                                                             # the "none" record
        assert got.winner[p].tolist() == [-1, -1, -1] and np.isnan(got.medians[p]) and not got.models[p].any() and got.inliers[p] == 0
        assert (got.samples[p] == -1).all()
    if iterations >= 72:
        assert all(got.winner[p, 0] >= 0 for p in (3, 8)), "the neighbours of the pairs without samples have their models"


@pytest.mark.parametrize("kind,sampling", [("homography", "opencv"), ("essential", "counter")])
def test_one_pair_above_the_lds_limit_of_the_scorer(hip_ctx, graphs, kind, sampling):
    g, rg = GC.large(), graphs("large")
    assert g["counts"].max() > SC_MAX_LDS
    K = GC.K4 if kind == "essential" else None
    want = expected(hip_ctx, "large", kind, K, sampling, 3, True)
    got = verify(rg, g, kind, K, sampling, 3, True)
    assert_same(got, want, f"large/{kind}/{sampling}")
    assert got.winner[0, 0] >= 0 and got.n_samples[0] == 3


@pytest.mark.parametrize("kind,sampling", [("homography", "opencv"), ("essential", "opencv"), ("essential", "counter")])
def test_eight_pairs_of_300_matches(hip_ctx, graphs, kind, sampling):
    g, rg = GC.eight(), graphs("eight")
    K = GC.K4 if kind == "essential" else None
    its = 72 if kind == "homography" else 89
    want = expected(hip_ctx, "eight", kind, K, sampling, its, True)
    got = verify(rg, g, kind, K, sampling, its, True)
    assert_same(got, want, f"eight/{kind}/{sampling}")
    assert (got.winner[:, 0] >= 0).all() and (got.inliers > 0).all() and (got.inliers < 300).any()


def tracks_equal(a, b):
    return all(getattr(a, f).tobytes() == getattr(b, f).tobytes() and getattr(a, f).shape == getattr(b, f).shape
               for f in ("track_ptr", "obs_frame", "obs_kp", "flags", "node_track"))


def test_retained_mask_is_the_keep_of_the_track_builder(hip_ctx):
    g = GC.eight()
    rg = resident(hip_ctx, g)
    try:
        E = verify(rg, g, "essential", GC.K4, "opencv", 89, True, retain=True)
        for policy in (0, 1):
            got, want = rg.tracks_verified(conflict_policy=policy), rg.tracks(keep=E.masks, conflict_policy=policy)
            assert tracks_equal(got, want) and want.n_tracks > 0
            assert not tracks_equal(got, rg.tracks(conflict_policy=policy)), "the mask cuts matches: not the tracks of the whole graph"
        H = verify(rg, g, "homography", None, "counter", 72, True, retain=True)              # a later call of another kind replaces the mask
        assert H.masks.tobytes() != E.masks.tobytes()
        for policy in (0, 1):
            assert tracks_equal(rg.tracks_verified(conflict_policy=policy), rg.tracks(keep=H.masks, conflict_policy=policy))
            assert not tracks_equal(rg.tracks_verified(conflict_policy=policy), rg.tracks(keep=E.masks, conflict_policy=policy))
        verify(rg, g, "essential", GC.K4, "opencv", 89, True, retain=False)                  # without retain the graph keeps what it has
        assert tracks_equal(rg.tracks_verified(), rg.tracks(keep=H.masks))
        rg.set_keypoints(g["xy"])                                                            # new coordinates drop the mask
        with pytest.raises(capi.EachamError) as e:
            rg.tracks_verified()
        assert e.value.code == capi.ERR_INVALID and "retained" in str(e.value)
        again = verify(rg, g, "essential", GC.K4, "opencv", 89, True, retain=True)
        assert again.masks.tobytes() == E.masks.tobytes() and tracks_equal(rg.tracks_verified(), rg.tracks(keep=E.masks))
    finally:
        rg.close()


def test_small_graph_tracks_with_gaps_and_an_empty_frame(hip_ctx, graphs):
    g, rg = GC.small(), graphs("small")
    E = verify(rg, g, "essential", GC.K4, "counter", 89, True, retain=True)
    for policy in (0, 1):
        assert tracks_equal(rg.tracks_verified(conflict_policy=policy), rg.tracks(keep=E.masks, conflict_policy=policy))


def raw_verify(rg, kind, sampling, iterations, P, n_src, m=5):
    """The C call on preset arrays; returns (return code, the arrays)."""
    its = max(iterations, 1)
    arrays = [np.full((P, 9), PRESET, np.float64), np.full(P, PRESET, np.float32), np.full(P, PRESET, np.float32), np.full(P, PRESET, np.int32),
              np.full(n_src, PRESET, np.uint8), np.full((P, 3), PRESET, np.int32), np.full(P, PRESET, np.int32), np.full(P, PRESET, np.int32),
              np.full((P, its, m), PRESET, np.int32)]
    before = [a.copy() for a in arrays]
    vp = C.c_void_p
    rc = capi.lib().eacham_graph_verify(rg._h, kind, vp(GC.K4.ctypes.data), sampling, iterations, None, 1, *[vp(a.ctypes.data) for a in arrays])
    return rc, arrays, before


def untouched(arrays, before):
    return all(a.tobytes() == b.tobytes() for a, b in zip(arrays, before))


def test_error_returns_write_nothing(hip_ctx):
    g = GC.small()
    P, n_src = len(g["counts"]), g["n_src"]
    rg = ResidentGraph(hip_ctx, g["n_frames"], g["pairs"], g["counts"], g["offsets"], g["q"], g["t"], g["n_kp"])
    try:
        rc, arrays, before = raw_verify(rg, capi.SOLVE_ESSENTIAL5, capi.SAMPLING_OPENCV, 3, P, n_src)     # before set_keypoints
        assert rc == capi.ERR_INVALID and untouched(arrays, before)
        with pytest.raises(capi.EachamError) as e:
            rg.verify("essential", GC.K4, iterations=3)
        assert e.value.code == capi.ERR_INVALID and "keypoint" in str(e.value)
        with pytest.raises(capi.EachamError) as e:                                               # a null xy while the graph has keypoints
            hip_ctx._check(capi.lib().eacham_graph_set_keypoints(rg._h, None))
        assert e.value.code == capi.ERR_INVALID
        rg.set_keypoints(g["xy"])
        for kind, sampling, its in ((7, capi.SAMPLING_OPENCV, 3), (-1, capi.SAMPLING_COUNTER, 3), (capi.SOLVE_ESSENTIAL5, 2, 3),
                                    (capi.SOLVE_ESSENTIAL5, -1, 3), (capi.SOLVE_HOMOGRAPHY4, capi.SAMPLING_COUNTER, -1)):
            rc, arrays, before = raw_verify(rg, kind, sampling, its, P, n_src)
            assert rc == capi.ERR_INVALID and untouched(arrays, before), (kind, sampling, its)
        with pytest.raises(capi.EachamError) as e:                                               # no call has retained a mask (the refused ones asked to)
            rg.tracks_verified()
        assert e.value.code == capi.ERR_INVALID
        rc, arrays, before = raw_verify(rg, capi.SOLVE_ESSENTIAL5, capi.SAMPLING_OPENCV, 3, P, n_src)     # and the graph still works
        assert rc == capi.OK and not any(a.tobytes() == b.tobytes() for a, b in zip(arrays, before))
        want = expected(hip_ctx, "small", "essential", GC.K4, "opencv", 3, False)
        assert arrays[4].tobytes() == want["masks"].tobytes() and arrays[8].tobytes() == want["samples"].tobytes()
        assert rg.tracks_verified().n_tracks >= 0
    finally:
        rg.close()


def test_outputs_are_optional(hip_ctx, graphs):
    g, rg = GC.small(), graphs("small")
    med = np.full(len(g["counts"]), PRESET, np.float32)
    vp = C.c_void_p
    hip_ctx._check(capi.lib().eacham_graph_verify(rg._h, capi.SOLVE_HOMOGRAPHY4, None, capi.SAMPLING_OPENCV, 72, None, 0, None, vp(med.ctypes.data),
                                                  None, None, None, None, None, None, None))
    assert med.tobytes() == expected(hip_ctx, "small", "homography", None, "opencv", 72, False)["medians"].tobytes()


def test_a_graph_without_pairs_or_matches(hip_ctx):
    e2 = np.zeros((0, 2), np.int32)
    rg = ResidentGraph(hip_ctx, 2, e2, np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.uint32), [3, 0])
    try:
        rg.set_keypoints(np.arange(6, dtype=np.float64).reshape(3, 2))
        r = rg.verify("essential", GC.K4, iterations=5, want_samples=True)
        assert r.medians.size == 0 and r.masks.size == 0 and r.samples.shape == (0, 5, 5)
    finally:
        rg.close()
    rg = ResidentGraph(hip_ctx, 2, np.array([[0, 1], [1, 0]], np.int32), np.zeros(2, np.int32), np.zeros(2, np.int64), np.zeros(0, np.uint32),
                       np.zeros(0, np.uint32), [3, 2])
    try:
        rg.set_keypoints(np.arange(10, dtype=np.float64).reshape(5, 2))
        for sampling in ("opencv", "counter"):
            r = rg.verify("homography", None, sampling=sampling, iterations=4, want_samples=True, retain=True)
            assert r.winner.tolist() == [[-1, -1, -1]] * 2 and np.isnan(r.medians).all() and (r.samples == -1).all() and not r.n_samples.any()
        assert rg.tracks_verified().n_tracks == 0
    finally:
        rg.close()


# ---- the C++ adapters (include/eacham/GraphVerifyHip.hpp) ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gv") / "graph_verify_driver")
    lib = os.path.join(ROOT, "eacham_amd", "lib")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + CPP,
           os.path.join(CPP, "graph_verify_driver.cpp"), "-L" + lib, "-leacham_hip", "-Wl,-rpath," + lib, "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def write_case(path, g):
    with open(path, "wb") as f:
        f.write(struct.pack("i", g["n_frames"]) + np.asarray(g["n_kp"], dtype=np.int64).tobytes())
        f.write(struct.pack("i", len(g["counts"])) + g["pairs"].astype(np.int32).tobytes() + g["counts"].astype(np.int32).tobytes())
        f.write(g["offsets"].astype(np.int64).tobytes() + struct.pack("q", g["n_src"]) + g["q"].tobytes() + g["t"].tobytes())
        f.write(np.ascontiguousarray(g["xy"], dtype=np.float64).tobytes() + GC.K4.tobytes() + g["seeds"].astype(np.uint64).tobytes())


@pytest.mark.parametrize("name", ["eight", "small"])
def test_cpp_adapters_equal_the_batch_adapters_on_host_gathered_points(driver, tmp_path, name):
    """VerifyEssential / VerifyHomography against FindEssentialMatBatch / FindHomographyBatch, every RobustModel field and every trace
    field, both sample streams, per-pair seeds and the default seed; TracksVerified against ResidentMatchGraph::Tracks(masks)."""
    g = getattr(GC, name)()
    case = str(tmp_path / "case.bin")
    write_case(case, g)
    r = subprocess.run([driver, case], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and not [ln for ln in lines if ln.startswith("DIFFERENT")], r.stdout[-3000:] + r.stderr[-2000:]
    P = len(g["counts"])
    assert len([ln for ln in lines if ln.startswith("same")]) == 5 * (1 + 2 * P) + 4
    with_model = {ln[5:ln.index(" pairs_with_a_model")]: int(ln.split("pairs_with_a_model")[1].split()[0]) for ln in lines if "pairs_with_a_model" in ln}
    assert len(with_model) == 5 and all(v > 0 for v in with_model.values())
    if name == "eight":
        assert all(v == P for v in with_model.values())
        assert all(int(ln.split()[-1]) > 0 for ln in lines if ln.startswith("info tracks"))
