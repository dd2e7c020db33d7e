"""GPU: the fundamental-matrix kind through its four entry points — eacham_solve_minimal (kind FUNDAMENTAL7), eacham_score_hypotheses
(kind FUNDAMENTAL), eacham_lmeds_batch and eacham_graph_verify — and the C++ adapters, against the CPU reference
(tests/fundamental_reference.py, itself held to float64 numpy by tests/test_fundamental_reference.py). Every comparison is of bits.
The shapes are the smallest at which the kernels can still go wrong: more samples than one workgroup holds, odd and even point
counts for the median, problems below / at / above the sample size, a problem above SC_MAX_LDS for the error-row path."""
import os
import struct
import subprocess

import numpy as np
import pytest

import fundamental_cases as FC
import fundamental_reference as FR
import graph_verify_cases as GC
from eacham_amd import ResidentGraph, capi, lmeds, score

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SC_MAX_LDS = 16384


def bits(x, dtype):
    return np.ascontiguousarray(x, dtype=dtype).view({4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize])


def same_bits(a, b, dtype):
    return np.array_equal(bits(a, dtype), bits(b, dtype))


# ---- 1. eacham_solve_minimal ---------------------------------------------------------------------------------------------------------------

def test_solve_minimal_equals_the_reference(hip_ctx):
    c = FC.scene(77, 40)
    samples = FC.counter_samples(40, 7, 64, 5)
    samples[13] = 21                                                                  # a degenerate sample: all seven indices equal
    got_m, got_n = score.solve_minimal(hip_ctx, "fundamental7", c["uv1"], c["uv2"], samples)
    want_m, want_n = FR.solve_minimal(c["uv1"], c["uv2"], samples)
    assert got_m.shape == (64, 3, 9) and np.array_equal(got_n, want_n) and same_bits(got_m, want_m, np.float64)
    assert got_n[13] == 0 and not got_m[13].any()
    assert set(np.unique(got_n)) >= {0, 1, 3}
    for s in range(64):
        assert not got_m[s, got_n[s]:].any()                                          # the slots behind n_models are zero
    withK, _ = score.solve_minimal(hip_ctx, "fundamental7", c["uv1"], c["uv2"], samples, K=FC.K4)
    assert same_bits(withK, got_m, np.float64)                                        # K is not read


@pytest.mark.parametrize("name", ["coplanar_scene", "translation_scene"])
def test_solve_minimal_on_special_geometry(hip_ctx, name):
    uv1, uv2 = getattr(FC, name)()
    samples = FC.counter_samples(len(uv1), 7, 5, 3)
    got_m, got_n = score.solve_minimal(hip_ctx, "fundamental7", uv1, uv2, samples)
    want_m, want_n = FR.solve_minimal(uv1, uv2, samples)
    assert np.array_equal(got_n, want_n) and same_bits(got_m, want_m, np.float64)


# ---- 2. eacham_score_hypotheses ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scored_problem():
    """301 matches (a fifth wrong) and 5 models: the truth, three solved from samples, one far off."""
    c = FC.lmeds_problem(seed=3, n=301, n_out=60, n_samples=8)
    models, counts = FR.solve_minimal(c["uv1"], c["uv2"], c["samples"])
    cand = [models[s, k] for s in range(len(counts)) for k in range(counts[s])][:3]
    assert len(cand) == 3
    return c, np.array([c["F"].ravel(), *cand, np.arange(1.0, 10.0) / 17.0])


@pytest.mark.parametrize("n", [301, 300])
def test_score_hypotheses_equals_the_reference(hip_ctx, scored_problem, n):
    c, models = scored_problem
    a, b = c["uv1"][:n], c["uv2"][:n]
    thr = 2.5
    err, cnt, med = score.score_hypotheses(hip_ctx, "fundamental", a, b, models, None, thr)
    werr, wcnt, wmed = FR.score_hypotheses(a, b, models, thr)
    assert same_bits(err, werr, np.float32) and np.array_equal(cnt, wcnt) and same_bits(med, wmed, np.float32)
    assert 0 < cnt[0] < n
    errK, cntK, medK = score.score_hypotheses(hip_ctx, "fundamental", a, b, models, FC.K4, thr)
    assert errK.tobytes() == err.tobytes() and cntK.tobytes() == cnt.tobytes() and medK.tobytes() == med.tobytes()   # K is ignored


# ---- 3. eacham_lmeds_batch -----------------------------------------------------------------------------------------------------------------

def none_record(n, candidates=0):
    return {"model": np.zeros(9), "median": np.float32(np.nan), "threshold": np.float32(0), "inliers": 0, "mask": np.zeros(n, np.uint8),
            "winner": (-1, -1, -1), "candidates": candidates}


def device_compose(ctx, uv1, uv2, samples):
    """One problem by the composition of entry points (1) and (2) on the device, the LMedS rule between them in Python float64."""
    import math
    n = len(uv1)
    samples = np.asarray(samples, np.int32).reshape(-1, 7)
    if n < 7 or len(samples) == 0:
        return none_record(n)
    models, counts = score.solve_minimal(ctx, "fundamental7", uv1, uv2, samples)
    where = [(s, r) for s in range(len(samples)) for r in range(int(counts[s]))]
    if not where:
        return none_record(n)
    cand = np.array([models[s, r] for s, r in where])
    _, _, med = score.score_hypotheses(ctx, "fundamental", uv1, uv2, cand, None, 0.0)
    best = -1
    for k in range(len(where)):
        if not np.isnan(med[k]) and (best < 0 or med[k] < med[best]):
            best = k
    if best < 0:
        return none_record(n, len(where))
    sigma = max(2.5 * 1.4826 * (1.0 + 5.0 / max(n - 7, 1)) * math.sqrt(float(med[best])), 0.001)
    thr = np.float32(sigma * sigma)
    err, cnt, _ = score.score_hypotheses(ctx, "fundamental", uv1, uv2, cand[best], None, float(thr))
    return {"model": cand[best].copy(), "median": med[best], "threshold": thr, "inliers": int(cnt[0]), "mask": (err[0] <= thr).astype(np.uint8),
            "winner": (best, where[best][0], where[best][1]), "candidates": len(where)}


def assert_problem(got, p, w, at):
    assert tuple(int(x) for x in got.winner[p]) == w["winner"], at
    assert int(got.n_candidates[p]) == w["candidates"], at
    assert same_bits(got.models[p], w["model"], np.float64), at
    assert same_bits(got.medians[p], w["median"], np.float32) or (np.isnan(got.medians[p]) and np.isnan(w["median"])), at
    assert same_bits(got.thresholds[p], w["threshold"], np.float32), at
    assert int(got.inliers[p]) == w["inliers"] and np.array_equal(got.masks[p], w["mask"]), at


@pytest.fixture(scope="module")
def problem_list():
    """Problems of 0, 6, 7, 8, 40 and 300 points, one without samples, one whose samples are all degenerate."""
    big = FC.lmeds_problem(seed=4, n=300, n_out=60, n_samples=24)
    c = FC.scene(31, 40)
    sizes = [0, 6, 7, 8, 40, 300, 40, 40]
    uv1 = [c["uv1"][:n] if n <= 40 else big["uv1"] for n in sizes]
    uv2 = [c["uv2"][:n] if n <= 40 else big["uv2"] for n in sizes]
    samples = [np.zeros((2, 7), np.int32),                        # 0 points: its samples are not looked at
               np.tile(np.arange(6, dtype=np.int32).repeat([2, 1, 1, 1, 1, 1]), (2, 1)),   # 6 points: fewer than a sample has
               np.arange(7, dtype=np.int32)[None].repeat(2, 0),   # n = m: the one subset, twice (a tie: the first stays)
               FC.counter_samples(8, 7, 5, 1),
               FC.counter_samples(40, 7, 9, 2),
               big["samples"],
               np.zeros((0, 7), np.int32),                        # no samples
               np.array([[3] * 7, [11] * 7, [39] * 7], np.int32)]  # every sample degenerate
    return uv1, uv2, samples


def test_lmeds_batch_equals_the_composition_and_the_reference(hip_ctx, problem_list):
    uv1, uv2, samples = problem_list
    got = hip_ctx.lmeds_batch("fundamental", uv1, uv2, samples)
    for p in range(len(uv1)):
        assert_problem(got, p, device_compose(hip_ctx, uv1[p], uv2[p], samples[p]), f"composition, problem {p}")
        assert_problem(got, p, FR.lmeds(uv1[p], uv2[p], samples[p]), f"reference, problem {p}")
    has = [int(got.winner[p, 0]) >= 0 for p in range(len(uv1))]
    assert has == [False, False, True, True, True, True, False, False]            # the "none" records where the contract puts them
    for p in np.flatnonzero(~np.array(has)):
        assert np.isnan(got.medians[p]) and not got.models[p].any() and not got.masks[p].any() and got.inliers[p] == 0 and got.thresholds[p] == 0
        assert got.n_candidates[p] == 0
    assert got.winner[2, 1] == 0                                                    # equal medians keep the earlier candidate
    withK = hip_ctx.lmeds_batch("fundamental", uv1, uv2, samples, FC.K4)            # K is ignored, NULL or not
    assert same_bits(withK.models, got.models, np.float64) and withK.medians.tobytes() == got.medians.tobytes()
    assert all(np.array_equal(x, y) for x, y in zip(withK.masks, got.masks))


def test_lmeds_batch_above_the_lds_limit_of_the_scorer(hip_ctx):
    n = 16400
    assert n > SC_MAX_LDS
    c = FC.lmeds_problem(seed=6, n=n, n_out=n // 5, n_samples=3)
    small = FC.scene(31, 40)
    uv1, uv2 = [c["uv1"], small["uv1"]], [c["uv2"], small["uv2"]]
    samples = [c["samples"], FC.counter_samples(40, 7, 4, 9)]
    got = hip_ctx.lmeds_batch("fundamental", uv1, uv2, samples)
    for p in range(2):
        assert_problem(got, p, FR.lmeds(uv1[p], uv2[p], samples[p]), f"reference, problem {p}")
    assert got.winner[0, 0] >= 0 and got.winner[1, 0] >= 0


def test_lmeds_batch_error_paths(hip_ctx, problem_list):
    uv1, uv2, samples = problem_list
    pp, a, b, sp, idx = lmeds.pack("fundamental", uv1, uv2, samples)
    want = hip_ctx.lmeds_batch("fundamental", uv1, uv2, samples)
    out = idx.copy()
    out[int(sp[4]) + 1, 6] = 40                                                     # one past the end of problem 4's points
    with pytest.raises(capi.EachamError) as e:
        lmeds.lmeds_batch_raw(hip_ctx, "fundamental", pp, a, b, sp, out)
    assert e.value.code == capi.ERR_INVALID and "problem 4" in str(e.value)
    with pytest.raises(capi.EachamError) as e:                                      # 7 is no kind: the sample size is not the code
        lmeds._call(hip_ctx, 7, pp, a, b, sp, idx, None)
    assert e.value.code == capi.ERR_INVALID and "kind" in str(e.value)
    again = hip_ctx.lmeds_batch("fundamental", uv1, uv2, samples)                   # the context is still usable
    assert same_bits(again.models, want.models, np.float64) and np.array_equal(again.winner, want.winner)


# ---- 4. eacham_graph_verify ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fund") / "fundamental_samples")
    subprocess.run(["g++", "-std=c++17", "-O1", "-DFUNDAMENTAL_HOST_ONLY", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(CPP, "fundamental_driver.cpp"), "-o", out], check=True, capture_output=True)
    return out


def host_samples(exe, points, sampling, iterations, seeds):
    lines = [f"{0 if sampling == 'opencv' else 1} {iterations} {len(points)}"]
    for (a, b), seed in zip(points, seeds):
        lines.append(f"{len(a)} {int(seed)}")
        lines += [f"{x1!r} {y1!r} {x2!r} {y2!r}" for (x1, y1), (x2, y2) in zip(a.tolist(), b.tolist())]
    r = subprocess.run([exe, "samples"], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    tok = np.array(r.stdout.split(), dtype=np.int64)
    out, at = [], 0
    for _ in points:
        s = int(tok[at])
        out.append(tok[at + 1:at + 1 + s * 7].astype(np.int32).reshape(s, 7))
        at += 1 + s * 7
    assert at == len(tok)
    return out


@pytest.fixture(scope="module")
def small_graph(hip_ctx):
    g = GC.small()
    rg = ResidentGraph(hip_ctx, g["n_frames"], g["pairs"], g["counts"], g["offsets"], g["q"], g["t"], g["n_kp"])
    rg.set_keypoints(g["xy"])
    yield g, rg
    rg.close()


@pytest.mark.parametrize("iterations", [0, 3, 40])
@pytest.mark.parametrize("sampling", ["opencv", "counter"])
def test_graph_verify_equals_the_host_composition(hip_ctx, small_graph, host_exe, sampling, iterations):
    g, rg = small_graph
    pts = GC.gather(g)
    samples = host_samples(host_exe, pts, sampling, iterations, g["seeds"])
    lb = hip_ctx.lmeds_batch("fundamental", [a for a, _ in pts], [b for _, b in pts], samples)
    masks = np.zeros(g["n_src"], dtype=np.uint8)
    for p, mk in enumerate(lb.masks):
        masks[int(g["offsets"][p]):int(g["offsets"][p]) + len(mk)] = mk
    fixed, n_samples = GC.fixed_stride(samples, iterations, 7)
    want = dict(models=lb.models, medians=lb.medians, thresholds=lb.thresholds, inliers=lb.inliers, masks=masks, winner=lb.winner,
                n_candidates=lb.n_candidates, n_samples=n_samples, samples=fixed)
    got = rg.verify("fundamental", None, sampling, iterations, g["seeds"], retain=True, want_samples=True)
    for name, w in want.items():
        a = getattr(got, name)
        assert a.dtype == w.dtype and a.shape == w.shape and a.tobytes() == w.tobytes(), f"{sampling}/{iterations}: {name}"
    draws = (g["counts"] >= 7) & (iterations > 0)
    if sampling == "opencv":
        draws[GC.COLLINEAR] = False                                                 # checkSubset refuses every subset: getSubset gives up
    assert np.array_equal(got.n_samples, np.where(draws, iterations, 0))
    if iterations == 40:
        assert got.winner[3, 0] >= 0 and got.winner[8, 0] >= 0 and 0 < got.inliers[3] <= 64
    # the retained mask is the `keep` of the track builder
    for policy in (0, 1):
        a, b = rg.tracks_verified(conflict_policy=policy), rg.tracks(keep=got.masks, conflict_policy=policy)
        assert all(getattr(a, f).tobytes() == getattr(b, f).tobytes() and getattr(a, f).shape == getattr(b, f).shape
                   for f in ("track_ptr", "obs_frame", "obs_kp", "flags", "node_track"))


def test_graph_verify_still_refuses_seven_as_a_kind(hip_ctx, small_graph):
    _, rg = small_graph
    with pytest.raises(capi.EachamError) as e:
        rg._verify_raw(7, 7, None, capi.SAMPLING_COUNTER, 3, None, False, False)
    assert e.value.code == capi.ERR_INVALID and "kind" in str(e.value)


# ---- 5. the C++ adapters -------------------------------------------------------------------------------------------------------------------

def test_cpp_adapters_agree_with_each_other(tmp_path):
    exe = str(tmp_path / "fundamental_driver")
    lib = os.path.join(ROOT, "eacham_amd", "lib")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + CPP,
                        os.path.join(CPP, "fundamental_driver.cpp"), "-L" + lib, "-leacham_hip", "-Wl,-rpath," + lib, "-o", exe, "-lpthread"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    g = GC.small()
    case = str(tmp_path / "case.bin")
    with open(case, "wb") as f:                                                      # (the layout of test_graph_verify_gpu.py: write_case)
        f.write(struct.pack("i", g["n_frames"]) + np.asarray(g["n_kp"], dtype=np.int64).tobytes())
        f.write(struct.pack("i", len(g["counts"])) + g["pairs"].astype(np.int32).tobytes() + g["counts"].astype(np.int32).tobytes())
        f.write(g["offsets"].astype(np.int64).tobytes() + struct.pack("q", g["n_src"]) + g["q"].tobytes() + g["t"].tobytes())
        f.write(np.ascontiguousarray(g["xy"], dtype=np.float64).tobytes() + GC.K4.tobytes() + g["seeds"].astype(np.uint64).tobytes())
        f.write(np.ascontiguousarray(FC.scene(3, 1)["F"], dtype=np.float64).tobytes() + FC.K4.tobytes())
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and not [ln for ln in lines if ln.startswith("DIFFERENT")], r.stdout[-3000:] + r.stderr[-2000:]
    with_model = [int(ln.split("pairs_with_a_model")[1].split()[0]) for ln in lines if "pairs_with_a_model" in ln]
    assert len(with_model) == 2 and all(v >= 2 for v in with_model)
    assert sum(ln.startswith("same") for ln in lines) >= 2 * (2 + 3 * len(g["counts"])) + 1
