"""The estimator LOOPS of include/eacham/TwoViewHip.hpp and PnPHip.hpp — FindEssentialMat / FindHomography (LMedS),
RefitHomography, RecoverPose, SolvePnPRansac, ransac_update_num_iters — held to tests/estimator_reference.py: a sequential,
one-candidate-at-a-time statement of the same OpenCV loops, fed the samples the header reports it used.

tests/cpp/twoview_driver.cpp runs every case below twice: linked with tests/cpp/oracle_abi.cpp (the CPU oracle behind the
C-ABI: no GPU needed, these are the `oracle` ids) and with libeacham_hip.so (`hip` ids, marked gpu). Same cases, same assertions.
The arithmetic under the loops is bit-identical between the two by the existing GPU tests, so every discrete decision — number of
iterations, the winner's place, the model's, median's and threshold's bits, every mask element, the inlier count, ok — is compared
EXACTLY. Against a high-precision statement instead: RecoverPose's R, t (1e-12, what test_twoview_cpp.py asks of the same SVD)
and the homography refit.

ransac_update_num_iters: the header rounds with lround where OpenCV's cvRound rounds halves to even. The reference rounds as the
header does; the two roundings differ only on a quotient that ends in exactly .5, which no point of the grid produces.

The refit's margin, MEASURED (CPU; H_ref = the long double minimiser of estimator_reference.refit_homography, never the code
under test). Over the 12 RefitHomography cases (4 / 5 / 50 / 3000 inliers, 0 / 0.5 / 2 px noise, coordinates around 4000 px) and
the 63 FindHomography runs of the pipeline cases that reach the refit. "Residual" cases are those where the minimiser leaves
an RMS residual above 1e-9 px (all with noise, float-rounded pixels included), "exact" the others (4 points, noise-free doubles):

                                                       RefitHomography cases            pipeline cases
    cost(H_lib) / cost(H_ref) - 1, residual cases      worst 5.3e-15 (5 pts, 0.5 px)    worst 6.5e-14 (exactfacing-0.45); most below 1e-16
    transfer distance H_lib vs H_ref, residual cases   worst 1.5e-9 px (5 pts, 2 px)    worst 9.4e-6 px (n16384, a NON-planar scene)
    transfer distance H_lib vs H_ref, exact cases      worst 3.8e-12 px (4 pts)         worst below 1e-11 px (n = 5, 6)
    cost(H_lib) / cost(H_ref) - 1, exact cases         -0.4 .. 76: two costs of ~1e-25, the ratio means nothing

REFIT_RATIO below is 10 x the worst measured ratio. On exact cases the transfer distance is bounded instead, by
REFIT_EXACT_PX = 1e-8 px = double rounding (2.2e-16) x the coordinates (4e3) x a condition number of the eight parameters of at
most ~1e4 for these spread-out point sets.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import estimator_reference as R
import oracle
import oracle_api as O
import score_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
REFIT_RATIO = 6.5e-13        # 10 x the worst measured cost(H_lib) / cost(H_ref) - 1 (see the module docstring); the issue's cap is 1e-6
REFIT_EXACT_PX = 1e-8       # noise-free cases (see the module docstring)
CHUNK = 256                 # pnp_detail::kChunk of PnPHip.hpp (asserted below)
OPENCV, COUNTER, GIVEN = 0, 1, 2

BACKENDS = [pytest.param("oracle", id="oracle"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]


def build_driver(backend, tmp):
    exe = os.path.join(tmp, "twoview_driver_" + backend)
    cmd = ["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(CPP, "twoview_driver.cpp")]
    if backend == "oracle":
        so = oracle.build()
        cmd += [os.path.join(CPP, "oracle_abi.cpp"), so, "-Wl,-rpath," + os.path.dirname(so)]
    else:
        lib = os.path.join(ROOT, "eacham_amd", "lib")
        cmd += ["-L" + lib, "-leacham_hip", "-Wl,-rpath," + lib]
    r = subprocess.run(cmd + ["-o", exe, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_driver(exe, mode, fin, fout, seconds=300):
    r = subprocess.run(["timeout", "-k", "10", str(seconds), exe, mode, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and "twoview driver ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def _vec(f, dtype):
    n = struct.unpack("q", f.read(8))[0]
    return np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype=dtype).copy()


def K9(K4):
    return np.array([K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1.0])


# ---- the two-view cases -------------------------------------------------------------------------------------------------

def tv(name, c, n=None, sampling=OPENCV, seed=7, e=(1000, 0.99), h=(100, 0.999), dist=50.0, pmask=0, givenE=(), givenH=(), **kw):
    uv1, uv2 = c["uv1"][:n], c["uv2"][:n]
    return dict(name=name, uv1=np.ascontiguousarray(uv1), uv2=np.ascontiguousarray(uv2), K=np.asarray(c["K"], float), sampling=sampling,
                seed=seed, e=e, h=h, dist=dist, pmask=pmask, givenE=np.asarray(givenE, np.int32).reshape(-1, 5),
                givenH=np.asarray(givenH, np.int32).reshape(-1, 4), **kw)


def random_samples(n, m, count, seed):
    rng = np.random.default_rng(seed)
    return np.array([rng.choice(n, m, replace=False) for _ in range(count)], np.int32)


def two_view_cases():
    cases = []
    scenes = {"general": dict(seed=31), "planar": dict(seed=35, planar=True), "facing": dict(seed=32, planar=True, facing=True),
              "exact": dict(seed=33, noise=0.0), "exactfacing": dict(seed=34, planar=True, facing=True, noise=0.0)}
    for sname, kw in scenes.items():
        for share in (0.0, 0.25, 0.45, 0.6):                      # 0.6 is past LMedS' breakdown point: alike, whatever happens
            c = SC.two_view_case(n=600, n_models=1, outliers=share, **kw)
            for sampling in (OPENCV, COUNTER):
                cases.append(tv(f"{sname}-{share}-{'cv' if sampling == OPENCV else 'ctr'}", c, sampling=sampling, noisy=kw.get("noise", 0.5) > 0))
    g = SC.two_view_case(n=16385, n_models=1, seed=41, outliers=0.25)
    f = SC.two_view_case(n=300, n_models=1, seed=42, outliers=0.25, planar=True, facing=True)
    for n in (3, 4, 5, 6, 8):                                     # n = m - 1, m, m + 1 for both estimators, and 8
        for sampling in (OPENCV, COUNTER):
            cases.append(tv(f"n{n}-{'cv' if sampling == OPENCV else 'ctr'}", f, n=n, sampling=sampling))
    for n in (16384, 16385):                                      # both sides of the scorer's LDS key buffer
        cases.append(tv(f"n{n}", g, n=n, sampling=COUNTER, h=(8, 0.999)))
    same = {"uv1": np.tile([[321.5, 207.25]], (50, 1)), "uv2": np.tile([[300.0, 211.0]], (50, 1)), "K": g["K"]}
    line1 = np.c_[100.0 + 12 * np.arange(50), 0.5 * (100.0 + 12 * np.arange(50)) + 20]      # (exactly on the line, in float too)
    line = {"uv1": line1, "uv2": line1 + [3.0, -2.0], "K": g["K"]}
    for sampling in (OPENCV, COUNTER):
        cases.append(tv(f"identical-{'cv' if sampling == OPENCV else 'ctr'}", same, sampling=sampling))
        cases.append(tv(f"collinear-{'cv' if sampling == OPENCV else 'ctr'}", line, sampling=sampling))
    small = SC.two_view_case(n=300, n_models=1, seed=43, outliers=0.25)
    for it in (1, 3, 50, 72, 89):                                 # 72 / 89 are the reference's own budgets, 50 lies below the computed count
        cases.append(tv(f"maxiters{it}", small, sampling=COUNTER, e=(it, 0.99), h=(it, 0.999), iters=it))
    for conf in (0.5, 0.99, 0.999, 1.0):
        cases.append(tv(f"confidence{conf}", small, sampling=OPENCV, e=(1000, conf), h=(1000, conf)))
    # an exact tie for the smallest median: the winner's sample once more, EARLIER in the list — the first must win
    for kind, m in (("essential", 5), ("homography", 4)):
        c = small if kind == "essential" else f
        base = random_samples(300, m, 12, seed=5)
        K4 = c["K"] if kind == "essential" else None
        w = R.lmeds(kind, c["uv1"], c["uv2"], K4, base)
        base[[w["sample"], 11]] = base[[11, w["sample"]]]           # the winner last: whatever ties with it comes earlier
        w = R.lmeds(kind, c["uv1"], c["uv2"], K4, base)
        assert w["ok"] and w["sample"] == 11
        tied = np.r_[base[:1], base[w["sample"]][None], base[1:]]
        key = "givenE" if kind == "essential" else "givenH"
        cases.append(tv(f"tie-{kind}", c, sampling=GIVEN, **{key: tied, ("givenH" if key == "givenE" else "givenE"): random_samples(300, 9 - m, 12, seed=6)},
                        tie=(kind, 1, 1 + w["sample"])))
    # recoverPose: no mask, an all-zero mask (every candidate has no vote: the first is kept), a threshold inside the scene
    cases.append(tv("pose-nomask", small, sampling=COUNTER, pmask=1))
    cases.append(tv("pose-allzero", small, sampling=COUNTER, pmask=2))
    cases.append(tv("pose-near", small, sampling=COUNTER, dist=4.0))
    return cases


def write_two_view(cases, path):
    with open(path, "wb") as f:
        for c in cases:
            f.write(struct.pack("i", -1))
            f.write(np.array([len(c["uv1"]), c["sampling"], c["seed"], c["e"][0], c["e"][1], c["h"][0], c["h"][1], c["dist"], c["pmask"],
                              len(c["givenE"]), len(c["givenH"]), 0], float).tobytes())
            f.write(c["givenE"].tobytes()); f.write(c["givenH"].tobytes())
            f.write(c["uv1"].tobytes()); f.write(c["uv2"].tobytes()); f.write(K9(c["K"]).tobytes())


def read_two_view(cases, path):
    res = {}
    with open(path, "rb") as f:
        for c in cases:
            r = {}
            r["meta"], r["E"], r["H"] = _vec(f, np.float64), _vec(f, np.float64), _vec(f, np.float64)
            r["emask"], r["hmask"] = _vec(f, np.uint8), _vec(f, np.uint8)
            r["esamples"], r["hsamples"] = _vec(f, np.int32).reshape(-1, 5), _vec(f, np.int32).reshape(-1, 4)
            r["trace"], r["hwinner"], r["dec"], r["pose"], r["pmask"] = (_vec(f, np.float64), _vec(f, np.float64), _vec(f, np.float64),
                                                                          _vec(f, np.float64), _vec(f, np.uint8))
            res[c["name"]] = r
        assert f.read() == b""
    return res


TWO_VIEW = two_view_cases()
TWO_VIEW_BY_NAME = {c["name"]: c for c in TWO_VIEW}
assert len(TWO_VIEW_BY_NAME) == len(TWO_VIEW)


@pytest.fixture(scope="module", params=BACKENDS)
def two_view_run(request, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("est_tv_" + request.param))
    exe = build_driver(request.param, tmp)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    write_two_view(TWO_VIEW, fin)
    run_driver(exe, "pipeline", fin, fout)
    return read_two_view(TWO_VIEW, fout)


def bits(a, dtype):
    return np.asarray(a, dtype).view({4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize])


def check_lmeds(kind, c, got_ok, got_inliers, got_median, got_iters, model, mask, samples, trace, max_iters, conf):
    """One LMedS run of the header against the reference on the header's samples: everything exactly."""
    m = 5 if kind == "essential" else 4
    n = len(c["uv1"])
    planned = R.lmeds_iterations(conf, m, max_iters)
    assert got_iters == len(samples) and len(samples) <= planned
    if n < m:
        assert got_iters == 0 and not got_ok
        return None
    if c["sampling"] == COUNTER:
        assert len(samples) == planned                              # only OpenCV's getSubset may give up early
    if c["sampling"] == GIVEN:
        assert np.array_equal(samples, (c["givenE"] if m == 5 else c["givenH"])[:planned])
    assert all(len(set(s)) == m for s in samples.tolist()) and (len(samples) == 0 or (samples.min() >= 0 and samples.max() < n))
    want = R.lmeds(kind, c["uv1"], c["uv2"], c["K"] if kind == "essential" else None, samples)
    assert bool(got_ok) == want["ok"] and trace[0] == want["candidates"]
    if not want["ok"]:
        return want
    assert (trace[1], trace[2], trace[3]) == (want["candidate"], want["sample"], want["root"])
    assert np.array_equal(bits(model, np.float64), bits(want["model"], np.float64))
    assert bits(got_median, np.float32) == bits(want["median"], np.float32)
    assert trace[4] == want["sigma"] and bits(trace[5], np.float32) == bits(want["threshold"], np.float32)
    assert np.array_equal(mask, want["mask"]) and got_inliers == want["inliers"] == int(want["mask"].sum())
    return want


@pytest.mark.parametrize("name", [c["name"] for c in TWO_VIEW])
def test_find_essential_mat_replays_step_by_step(two_view_run, name):
    c, r = TWO_VIEW_BY_NAME[name], two_view_run[name]
    meta, tr = r["meta"], r["trace"]
    want = check_lmeds("essential", c, meta[0], meta[1], meta[2], meta[6], r["E"], r["emask"], r["esamples"], tr[:6], *c["e"])
    if "iters" in c:
        assert meta[6] == min(c["iters"], 89)                      # 1000 asked at 0.99 / 5 points are 89
    if c.get("tie", ("",))[0] == "essential":
        assert (tr[2], want["sample"]) == (c["tie"][1], c["tie"][1]) and np.array_equal(r["esamples"][c["tie"][1]], r["esamples"][c["tie"][2]])


@pytest.mark.parametrize("name", [c["name"] for c in TWO_VIEW])
def test_find_homography_replays_step_by_step(two_view_run, name):
    c, r = TWO_VIEW_BY_NAME[name], two_view_run[name]
    meta, tr = r["meta"], r["trace"]
    want = check_lmeds("homography", c, meta[3], meta[4], meta[5], meta[7], r["hwinner"], r["hmask"], r["hsamples"], tr[6:], *c["h"])
    if "iters" in c:
        assert meta[7] == min(c["iters"], 72)                      # 100 asked at 0.999 / 4 points are 72
    if c.get("tie", ("",))[0] == "homography":
        assert (tr[8], want["sample"]) == (c["tie"][1], c["tie"][1]) and np.array_equal(r["hsamples"][c["tie"][1]], r["hsamples"][c["tie"][2]])
    if name == "collinear-cv":                                     # checkSubset refuses every subset: getSubset gives up at once
        assert meta[7] == 0 and not meta[3]
    if want is None or not want["ok"]:
        return
    # the refit: the model handed back is the minimiser over the winner's inliers (or the winner itself where there is none)
    ref = R.refit_homography(c["uv1"], c["uv2"], r["hmask"]) if len(c["uv1"]) > 4 else None
    if ref is None:
        assert np.array_equal(bits(r["H"], np.float64), bits(r["hwinner"], np.float64))
        return
    check_refit(r["H"], ref, c["uv1"], c["uv2"], r["hmask"].astype(bool), r["hwinner"], name)


def check_refit(H, ref, uv1, uv2, keep, winner, label):
    """The refitted H against the long double minimiser. Where the minimiser leaves residuals above rounding (RMS > 1e-9 px: every
    case with noise, pixels rounded to float included) the costs are compared; where it fits exactly, the transfer distance."""
    Href, Hdlt, info = ref
    a, b = uv1[keep], uv2[keep]
    noisy = float(R.transfer_cost(Href, a, b)) / len(a) > 1e-18
    c_lib, c_ref, c_dlt = (R.transfer_cost(M, a, b) for M in (H, Href, Hdlt))
    dist = float(np.linalg.norm((R.transfer(np.asarray(H, R.LD), a) - R.transfer(np.asarray(Href, R.LD), a)).astype(float), axis=1).max())
    ratio = float(c_lib / c_ref - 1) if c_ref > 0 else float("nan")
    print(f"refit {'noisy' if noisy else 'exact'} {label}: inliers {len(a)} cost_ref {float(c_ref):.6e} ratio-1 {ratio:.3e} distance {dist:.3e} px ref steps {info['steps']}")
    assert H[8] == 1.0
    if noisy:
        assert ratio <= REFIT_RATIO
        assert c_lib <= c_dlt
        if winner is not None:
            assert c_lib < R.transfer_cost(winner, a, b)
    else:
        assert dist <= REFIT_EXACT_PX


@pytest.mark.parametrize("name", [c["name"] for c in TWO_VIEW])
def test_recover_pose_votes_like_the_reference(two_view_run, name):
    c, r = TWO_VIEW_BY_NAME[name], two_view_run[name]
    if not r["meta"][0]:
        assert len(r["pose"]) == 0
        return
    n = len(c["uv1"])
    dec = r["dec"]
    lib_dec = (dec[:9].reshape(3, 3), dec[9:18].reshape(3, 3), dec[18:])
    mask = {0: r["emask"], 1: None, 2: np.zeros(n, np.uint8)}[c["pmask"]]
    want = R.recover_pose(r["E"], c["uv1"], c["uv2"], K9(c["K"]), c["dist"], mask, labelled_as=lib_dec)
    ref_dec = R.decompose_essential(r["E"])                           # the header's decomposition is one of the valid ones
    assert min(np.abs(lib_dec[0] - ref_dec[k]).max() + np.abs(lib_dec[1] - ref_dec[1 - k]).max() for k in (0, 1)) < 1e-12
    assert min(np.abs(lib_dec[2] - ref_dec[2]).max(), np.abs(lib_dec[2] + ref_dec[2]).max()) < 1e-12
    Rm, t, good = r["pose"][:9].reshape(3, 3), r["pose"][9:12], r["pose"][12]
    assert np.abs(Rm - want["R"]).max() < 1e-12 and np.abs(t - want["t"]).max() < 1e-12
    assert good == want["good"] and np.array_equal(r["pmask"], want["mask"])
    if c["pmask"] == 2:                                               # no votes at all: [R1 | t], the first candidate
        assert want["winner"] == 0 and good == 0 and np.array_equal(Rm, lib_dec[0]) and np.array_equal(t, lib_dec[2])
    if name == "pose-nomask":
        assert sorted(want["votes"])[-2] < want["votes"][want["winner"]]     # (an unambiguous case)


def test_the_two_view_cases_cover_what_they_are_for(two_view_run):
    """Candidates flattened across samples with 0, 2, 4, ... roots; a winner that is neither root 0 nor in the first sample;
    a case past the breakdown point; getSubset giving up; masks that differ from 'all' and 'none'."""
    r = two_view_run["general-0.25-ctr"]
    c = TWO_VIEW_BY_NAME["general-0.25-ctr"]
    _, counts = O.solve_minimal("essential5", c["uv1"], c["uv2"], r["esamples"], c["K"])
    assert len(set(counts.tolist())) >= 3                          # samples with different numbers of roots in one run
    mixed = [n for n, x in two_view_run.items() if x["meta"][0] and x["trace"][3] > 0 and x["trace"][2] > 0 and x["trace"][1] != x["trace"][2]]
    assert len(mixed) >= 5, mixed
    assert any(x["meta"][7] < 72 and TWO_VIEW_BY_NAME[n]["h"] == (100, 0.999) and len(TWO_VIEW_BY_NAME[n]["uv1"]) >= 4 for n, x in two_view_run.items())
    for n in ("general-0.25-cv", "facing-0.25-cv"):
        x = two_view_run[n]
        assert 0.5 < x["emask"].mean() < 1.0 and 0.2 < x["hmask"].mean() < 1.0


# ---- solvePnPRansac -----------------------------------------------------------------------------------------------------

def pnp(name, X, uv, K, sampling=OPENCV, seed=5, iters=10000, thr=4.0, conf=0.999, given=(), **kw):
    return dict(name=name, X=np.ascontiguousarray(X, float), uv=np.ascontiguousarray(uv, float), K=np.asarray(K, float), sampling=sampling, seed=seed,
                iters=iters, thr=thr, conf=conf, given=np.asarray(given, np.int32).reshape(-1, 5), **kw)


def pnp_cases():
    cases = []
    for share, iters in ((1.0, 10000), (0.7, 10000), (0.3, 10000), (0.05, 600)):      # 0.05: the budget never shrinks, so 600 asked, 600 used
        c = SC.pnp_case(n=500, n_models=1, seed=11, outliers=1.0 - share)
        for sampling in (OPENCV, COUNTER):
            cases.append(pnp(f"share{share}-{'cv' if sampling == OPENCV else 'ctr'}", c["X"][1:], c["uv"][1:], c["K"], sampling=sampling, iters=iters,
                             all_used=share == 0.05, fails=share == 0.05))
        if share == 0.05:
            for it in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
                cases.append(pnp(f"share{share}-iters{it}", c["X"][1:], c["uv"][1:], c["K"], sampling=COUNTER, iters=it, all_used=True, fails=True))
    c = SC.pnp_case(n=500, n_models=1, seed=11, outliers=0.3)
    X, uv, K, bad = c["X"][1:], c["uv"][1:].copy(), c["K"], c["bad"][1:]
    for conf in (0.5, 0.99, 1.0):
        cases.append(pnp(f"confidence{conf}", X, uv, K, conf=conf, iters=700))
    few = uv.copy()
    rng = np.random.default_rng(3)
    spoil = np.nonzero(~bad)[0][3:]                                  # all but three of the good points displaced: no model reaches 5 inliers
    few[spoil] += rng.normal(0, 80, size=(len(spoil), 2))
    cases.append(pnp("three-inliers", X[:120], few[:120], K, iters=300, fails=True))
    good = np.nonzero(~bad)[0]
    cases.append(pnp("n5", X[good[:5]], uv[good[:5]], K, iters=50))
    cases.append(pnp("n4", X[good[:4]], uv[good[:4]], K, iters=50, fails=True))
    Xp, uvp, Kp, _ = SC.planar_pnp_case(n=300, seed=3, noise=0.5)
    cases.append(pnp("planar", Xp, uvp.astype(np.float32).astype(float), Kp))
    # the point at which the sequential loop stops, by construction: half the points are outliers; every sample of the list is
    # spoilt by outliers except a first good one at index 3 (it sets the budget B) and a better one placed at B - 1 (the last
    # sample the loop looks at: it wins) or at B (the first it does not: it must not win, though its batch has been solved)
    c = SC.pnp_case(n=200, n_models=1, seed=17, outliers=0.5)
    X, uv, K, bad = c["X"][1:], c["uv"][1:], c["K"], c["bad"][1:]
    good, out = np.nonzero(~bad)[0], np.nonzero(bad)[0]
    rng = np.random.default_rng(8)
    pool = np.array([rng.choice(good, 5, replace=False) for _ in range(40)], np.int32)
    models, ok = O.solve_pnp(X, uv, K, pool)
    _, cnt, _ = O.score_hypotheses("pnp", X, uv, models, K, 16.0)
    order = np.argsort(np.where(ok > 0, cnt, -1), kind="stable")
    first, better = pool[order[len(order) // 2]], pool[order[-1]]
    c_first, c_better = int(cnt[order[len(order) // 2]]), int(cnt[order[-1]])
    assert c_better > c_first >= 5
    spoilt = np.array([np.r_[rng.choice(out, 3, replace=False), rng.choice(good, 2, replace=False)] for _ in range(2 * CHUNK + 2)], np.int32)
    for iters in (CHUNK - 1, CHUNK, CHUNK + 1):
        lst = spoilt[:iters].copy()
        lst[3] = first
        B = R.pnp_ransac(X, uv, K, lst, iters)["iterations"]
        assert 3 < B < CHUNK - 1, B                                   # the loop stops inside the first batch
        for where, tag in ((B - 1, "last-before"), (B, "first-after")):
            planted = lst.copy()
            planted[where] = better
            cases.append(pnp(f"stop-{tag}-iters{iters}", X, uv, K, sampling=GIVEN, iters=iters, given=planted,
                             stop=(B, where, c_first, c_better)))
    return cases


PNP = pnp_cases()
PNP_BY_NAME = {c["name"]: c for c in PNP}
assert len(PNP_BY_NAME) == len(PNP)


@pytest.fixture(scope="module", params=BACKENDS)
def pnp_run(request, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("est_pnp_" + request.param))
    exe = build_driver(request.param, tmp)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        for c in PNP:
            f.write(struct.pack("i", -1))
            f.write(np.array([len(c["X"]), c["sampling"], c["seed"], c["iters"], c["thr"], c["conf"], len(c["given"]), 0], float).tobytes())
            f.write(c["given"].tobytes()); f.write(c["X"].tobytes()); f.write(c["uv"].tobytes()); f.write(K9(c["K"]).tobytes())
    run_driver(exe, "pnp", fin, fout)
    res = {}
    with open(fout, "rb") as f:
        for c in PNP:
            res[c["name"]] = dict(pose=_vec(f, np.float64), inliers=_vec(f, np.int32), samples=_vec(f, np.int32).reshape(-1, 5), trace=_vec(f, np.float64))
        assert f.read() == b""
    return res


def test_the_batch_size_is_the_headers():
    with open(os.path.join(ROOT, "include", "eacham", "PnPHip.hpp")) as f:
        assert f"const int kChunk = {CHUNK};" in f.read()


@pytest.mark.parametrize("name", [c["name"] for c in PNP])
def test_solve_pnp_ransac_replays_step_by_step(pnp_run, name):
    c, r = PNP_BY_NAME[name], pnp_run[name]
    pose, n = r["pose"], len(c["X"])
    ok, iters, Rm, rvec, t = pose[0], int(pose[1]), pose[2:11], pose[11:14], pose[14:17]
    if n < 5:
        assert not ok and iters == 0 and len(r["samples"]) == 0
        return
    samples = r["samples"]
    assert len(samples) >= iters and len(samples) % CHUNK in (0, c["iters"] % CHUNK) and len(samples) <= c["iters"]
    assert all(len(set(s)) == 5 for s in samples.tolist()) and samples.min() >= 0 and samples.max() < n
    if c["sampling"] == GIVEN:
        assert np.array_equal(samples, c["given"][:len(samples)])
    want = R.pnp_ransac(c["X"], c["uv"], c["K"], samples, c["iters"], c["thr"], c["conf"])
    assert (bool(ok), iters, int(r["trace"][0])) == (want["ok"], want["iterations"], want["winner"])
    assert bool(ok) != bool(c.get("fails", False))
    if c.get("all_used"):
        assert iters == c["iters"]
    if "stop" in c:
        B, where, c_first, c_better = c["stop"]
        assert iters == B and want["winner"] == (where if where < B else 3)
    if not want["ok"]:
        assert len(r["inliers"]) == 0
        return
    assert np.array_equal(r["inliers"], want["inliers"])
    assert np.array_equal(bits(np.r_[Rm, t], np.float64), bits(want["pose"], np.float64))   # one EPnP call on an index list proved equal
    assert np.abs(SC.synth.so3_exp(rvec) - Rm.reshape(3, 3)).max() < 1e-9


def test_the_pnp_cases_cover_what_they_are_for(pnp_run):
    its = {n: int(x["pose"][1]) for n, x in pnp_run.items()}
    assert its["share1.0-cv"] < 10 and its["share1.0-ctr"] < 10                 # every point an inlier: the budget collapses at once
    assert 10 < its["share0.7-cv"] < 200 and CHUNK < its["share0.3-cv"] < 10000   # (0.3: more than one batch, far fewer than asked)
    assert its["confidence0.5"] < its["confidence0.99"] < its["confidence1.0"]


# ---- host-only code: ransac_update_num_iters, RefitHomography ----------------------------------------------------------

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return build_driver("oracle", str(tmp_path_factory.mktemp("est_host")))


def test_ransac_update_num_iters_on_a_grid(host_exe, tmp_path):
    grid = [(p, ep, m, it) for p in (0.0, 0.5, 0.9, 0.99, 0.999, 1.0, -0.5, 1.5)
            for ep in (0.0, 1e-12, 1e-3, 0.05, 0.3, 0.45, 0.5, 0.7, 0.95, 1 - 1e-12, 1.0, -1.0, 2.0)
            for m in (4, 5, 64, 299) for it in (1, 3, 72, 89, 100, 10000)]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", len(grid))); f.write(np.array(grid, float).tobytes())
    run_driver(host_exe, "iters", fin, fout)
    with open(fout, "rb") as f:
        got = _vec(f, np.int32)
    want = [R.update_num_iters(*g) for g in grid]
    assert got.tolist() == want
    assert len(set(want)) > 40 and 0 in want                        # (the grid reaches zero, the cap and many values between)
    assert R.update_num_iters(0.99, 0.45, 5, 1000) == 89 and R.update_num_iters(0.999, 0.45, 4, 100) == 72
    assert R.lmeds_iterations(0.99, 5, 2) == 2 and R.lmeds_iterations(0.0, 5, 1000) == 3


def refit_cases():
    rng = np.random.default_rng(12)
    Kmat = np.array([[960, 0, 400], [0, 960, 400], [0, 0, 1.0]])
    Hn = SC.synth.so3_exp(np.array([0.05, -0.1, 0.08])) + np.outer([0.3, -0.1, 0.05], [0.1, -0.2, 0.97]) / 4.0
    H = Kmat @ Hn @ np.linalg.inv(Kmat)
    shift = np.array([[1, 0, 3600.0], [0, 1, 3900.0], [0, 0, 1]])          # pixel coordinates around 4000: the normalisation matters
    H = shift @ H @ np.linalg.inv(shift)
    H /= H[2, 2]
    cases = []
    for m in (4, 5, 50, 3000):
        for noise in (0.0, 0.5, 2.0):
            n = m + m // 3 + 2
            uv1 = rng.uniform(0, 800, size=(n, 2)) + [3600.0, 3900.0]
            uv2 = R.transfer(H, uv1) + noise * rng.normal(size=(n, 2))
            mask = np.zeros(n, np.uint8)
            mask[rng.choice(n, m, replace=False)] = 1
            uv2[mask == 0] += 300.0                                        # what the mask drops must not matter
            cases.append(dict(name=f"{m}pts-{noise}px", uv1=uv1, uv2=uv2, mask=mask, noisy=noise > 0 and m > 4, ok=True))
    c = cases[7]
    cases.append(dict(name="no-mask", uv1=c["uv1"][c["mask"] > 0], uv2=c["uv2"][c["mask"] > 0], mask=np.zeros(0, np.uint8), noisy=True, ok=True))
    three = c["mask"].copy()
    three[np.nonzero(three)[0][3:]] = 0
    cases.append(dict(name="three-set", uv1=c["uv1"], uv2=c["uv2"], mask=three, noisy=False, ok=False))
    x = np.linspace(3700, 4300, 40)
    line = np.c_[x, 0.37 * x + 2500.0]
    cases.append(dict(name="on-a-line", uv1=line, uv2=line + [5.0, -3.0], mask=np.ones(40, np.uint8), noisy=False, ok=False))
    cases.append(dict(name="on-a-vertical-line", uv1=np.c_[np.full(40, 3800.0), x], uv2=np.c_[np.full(40, 3810.0), x + 2], mask=np.ones(40, np.uint8),
                      noisy=False, ok=False))
    return cases


def test_refit_homography_finds_the_minimiser(host_exe, tmp_path, capsys):
    cases = refit_cases()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        for c in cases:
            f.write(struct.pack("ii", len(c["uv1"]), len(c["mask"])))
            f.write(c["uv1"].tobytes()); f.write(c["uv2"].tobytes()); f.write(c["mask"].tobytes())
    run_driver(host_exe, "refit", fin, fout)
    with open(fout, "rb") as f:
        for c in cases:
            got = _vec(f, np.float64)
            ref = R.refit_homography(c["uv1"], c["uv2"], c["mask"])
            assert bool(got[0]) == c["ok"] == (ref is not None), c["name"]
            if ref is None:
                continue
            keep = c["mask"].astype(bool) if len(c["mask"]) else np.ones(len(c["uv1"]), bool)
            if c["noisy"]:                                              # the reference stands at a stationary point: the residual is
                assert ref[2]["gradient"] < 1e-12, (c["name"], ref[2])  # orthogonal to every column of the Jacobian (cosines; the cost is then within 1e-24 of its minimum)
            check_refit(got[1:], ref, c["uv1"], c["uv2"], keep, None, c["name"])
            if c["noisy"]:                                              # the refit MOVES: the DLT start is not the minimiser
                assert R.transfer_cost(got[1:], c["uv1"][keep], c["uv2"][keep]) < R.transfer_cost(ref[1], c["uv1"][keep], c["uv2"][keep])
