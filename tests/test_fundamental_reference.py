"""CPU: the reference of the fundamental-matrix kind (tests/cpp/fundamental_reference.c — the seven-point solver, the error and the
LMedS rule written step for step as the kernels run them) held against independent float64 numpy, on the scenes of
tests/fundamental_cases.py; and cv_check_subset_fundamental of include/eacham/CvSampling.hpp through a small driver.
tests/test_fundamental_gpu.py holds the device to this reference bit for bit.

Measured here (200 scenes, exact correspondences): worst held-out symmetric epipolar error 5.4e-15 px^2 (bound 1e-6), worst |det F|
1.0e-18 (bound 1e-12), worst |x2' F x1| on the sample's own points 2.6e-12 (bound 1e-9); 29 samples have one model, 171 three."""
import os
import subprocess

import numpy as np
import pytest

import fundamental_cases as FC
import fundamental_reference as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def solved():
    uv1, uv2, samples, per = FC.minimal_scenes()
    models, counts, cubic, roots = FR.solve_minimal(uv1, uv2, samples, want_cubic=True)
    return uv1, uv2, samples, per, models, counts, cubic, roots


def test_some_root_of_every_sample_fits_the_held_out_points(solved):
    uv1, uv2, samples, per, models, counts, _, _ = solved
    assert len(samples) == 200
    worst = 0.0
    for k in range(len(samples)):
        a, b = uv1[per * k + 7:per * (k + 1)], uv2[per * k + 7:per * (k + 1)]
        assert len(a) == FC.HELD_OUT and counts[k] >= 1, k
        best = min(FC.epipolar_sym(models[k, r].reshape(3, 3), a, b).max() for r in range(counts[k]))
        worst = max(worst, best)
        assert best <= 1e-6, (k, best)
    print(f"worst held-out symmetric epipolar error {worst:.3e} px^2")


def test_every_model_is_a_fundamental_matrix_of_its_seven_points(solved):
    uv1, uv2, samples, _, models, counts, cubic, _ = solved
    wdet = wres = 0.0
    for k in range(len(samples)):
        x1 = np.concatenate([uv1[samples[k]], np.ones((7, 1))], axis=1)
        x2 = np.concatenate([uv2[samples[k]], np.ones((7, 1))], axis=1)
        for r in range(3):
            F = models[k, r].reshape(3, 3)
            if r >= counts[k]:
                assert not F.any(), (k, r)                       # the slots behind n_models are zero
                continue
            assert abs(np.linalg.norm(F) - 1.0) <= 1e-14
            det, res = abs(np.linalg.det(F)), np.abs(np.sum(x2 * (x1 @ F.T), axis=1)).max()
            wdet, wres = max(wdet, det), max(wres, res)
            assert det <= 1e-12 and res <= 1e-9, (k, r, det, res)
        # as many models as the cubic has real roots, on scenes that are not near a double root (where the count is a coin toss)
        rr = np.roots(cubic[k])
        assert len(rr) == 3
        for i in range(3):
            for j in range(i):
                assert abs(rr[i] - rr[j]) > 1e-4 * (1.0 + abs(rr[i])), f"scene {k} is within 1e-4 of a double root: choose another"
        assert int(np.sum(np.abs(rr.imag) <= 1e-7 * (1.0 + np.abs(rr.real)))) == counts[k], k
    print(f"worst |det F| {wdet:.3e}, worst |x2' F x1| {wres:.3e}")
    assert set(np.unique(counts)) == {1, 3}                       # both kinds of cubic occur


def test_the_true_matrix_is_among_the_models(solved):
    """Not only small residuals: up to sign, one model of every sample is the scene's F."""
    _, _, samples, per, models, counts, _, _ = solved
    for k in range(0, len(samples), 10):
        F = FC.scene(1000 + FC.SCENES[k], per)["F"].ravel()
        d = min(min(np.abs(models[k, r] - F).max(), np.abs(models[k, r] + F).max()) for r in range(counts[k]))
        assert d <= 1e-9, (k, d)


def test_degenerate_samples_give_no_model():
    uv1, uv2, _, _ = FC.minimal_scenes()
    same = np.zeros((3, 7), np.int32) + np.array([[0], [5], [9]], np.int32)           # all seven indices equal
    models, counts = FR.solve_minimal(uv1, uv2, same)
    assert not counts.any() and not models.any()
    a = uv1[:7].copy()
    a[:] = a[0]                                                                      # image 1 alone collapses
    models, counts = FR.solve_minimal(a, uv2[:7], np.arange(7, dtype=np.int32)[None])
    assert counts[0] == 0 and not models.any()


def test_error_function_against_float64_numpy():
    rng = np.random.default_rng(5)
    n = 1000
    F = np.stack([FC.scene(9000 + i, 1)["F"] for i in range(n)]) + rng.normal(scale=1e-7, size=(n, 3, 3))
    a, b = rng.uniform(0, FC.W, (n, 2)), rng.uniform(0, FC.H, (n, 2))
    worst = 0
    for i in range(n):                                                                # item i: model i on point i
        got = FR.score_hypotheses(a[i:i + 1], b[i:i + 1], F[i])[0][0, 0]
        want = FC.epipolar_max(F[i], a[i:i + 1], b[i:i + 1])[0]
        ulp = np.spacing(np.float32(want))
        worst = max(worst, abs(float(got) - want) / float(ulp))
        assert abs(float(got) - want) <= 4 * float(ulp), (i, got, want)
    print(f"worst error-function deviation {worst:.2f} float ulps")


def test_medians_and_counts_of_the_scorer():
    c = FC.lmeds_problem()
    for n in (200, 199):                                                        # an even and an odd count
        a, b = c["uv1"][:n], c["uv2"][:n]
        err, cnt, med = FR.score_hypotheses(a, b, c["F"], threshold=1.0)
        s = np.sort(err[0])
        want = s[n // 2] if n % 2 else np.float32((s[n // 2 - 1] + s[n // 2]) * np.float32(0.5))
        assert med[0] == want and cnt[0] == int((err[0] <= np.float32(1.0)).sum())


def test_lmeds_keeps_the_inliers_and_cuts_the_outliers():
    c = FC.lmeds_problem()
    assert c["outlier"].sum() == 60 and len(c["uv1"]) == 200 and c["samples"].shape == (301, 7)
    assert any(not c["outlier"][s].any() for s in c["samples"]), "no outlier-free sample in the stream (chance below 1e-10)"
    # the scene is one where no outlier happens to lie on its epipolar line: farther than a pixel for the true F
    assert FC.epipolar_max(c["F"], c["uv1"], c["uv2"])[c["outlier"]].min() > 1.0
    r = FR.lmeds(c["uv1"], c["uv2"], c["samples"])
    assert r["winner"][0] >= 0 and r["inliers"] == 140
    assert r["mask"][~c["outlier"]].all() and not r["mask"][c["outlier"]].any()
    assert r["inliers"] == int(r["mask"].sum())
    # the rule, restated: the winner's median is the smallest of all candidates', its threshold follows from it
    models, counts = FR.solve_minimal(c["uv1"], c["uv2"], c["samples"])
    cand = np.array([models[s, k] for s in range(len(counts)) for k in range(counts[s])])
    _, _, med = FR.score_hypotheses(c["uv1"], c["uv2"], cand)
    assert r["candidates"] == len(cand) and r["winner"][0] == int(np.nanargmin(med)) and r["median"] == med[r["winner"][0]]
    sigma = max(2.5 * 1.4826 * (1.0 + 5.0 / (200 - 7)) * np.sqrt(float(r["median"])), 0.001)
    assert r["threshold"] == np.float32(sigma * sigma)


def test_lmeds_none_records():
    c = FC.lmeds_problem()
    few = FR.lmeds(c["uv1"][:6], c["uv2"][:6], c["samples"][:3])                      # fewer than 7 points: samples not looked at
    empty = FR.lmeds(c["uv1"], c["uv2"], np.zeros((0, 7), np.int32))
    degenerate = FR.lmeds(c["uv1"], c["uv2"], np.full((4, 7), 3, np.int32))
    for r in (few, empty, degenerate):
        assert r["winner"] == (-1, -1, -1) and np.isnan(r["median"]) and r["threshold"] == 0 and r["inliers"] == 0
        assert not r["model"].any() and not r["mask"].any() and r["candidates"] == 0


# ---- cv_check_subset_fundamental (include/eacham/CvSampling.hpp) ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fund") / "fundamental_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-DFUNDAMENTAL_HOST_ONLY", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "fundamental_driver.cpp"), "-o", out], check=True, capture_output=True)
    return out


def test_fundamental_check_subset(exe):
    rng = np.random.default_rng(8)
    cases, want = [], []
    for c in range(120):
        src = np.rint(rng.uniform(0, 800, (7, 2)))
        dst = np.rint(rng.uniform(0, 800, (7, 2)))
        kind = c % 4
        if kind in (1, 2):                          # the seventh point on the line through two earlier ones, in image 1 / image 2
            p = src if kind == 1 else dst
            j, k = rng.choice(6, 2, replace=False)
            p[k] = p[j] + 2 * np.rint(rng.uniform(5, 60, 2))
            p[6] = (p[j] + p[k]) / 2               # integers: the collinearity is exact in float
        if kind == 3:                               # three EARLIER points on a line: only the last point is tested
            d = np.rint(rng.uniform(5, 60, 2))
            src[1], src[2] = src[0] + 2 * d, src[0] + d
        cases.append(" ".join(repr(float(v)) for v in np.concatenate([src.ravel(), dst.ravel()])))
        want.append(int(kind in (0, 3)))
    r = subprocess.run([exe, "check"], input="\n".join(cases) + "\n", capture_output=True, text=True, check=True)
    assert [int(x) for x in r.stdout.split()] == want


def test_fundamental_sample_stream_refuses_collinear_subsets(exe):
    """lmeds_samples with the fundamental check: every subset it returns passes the check as numpy states it, a pair whose image-1
    points all lie on one line draws nothing, and without a refusal the stream is the plain getSubset stream."""
    import graph_verify_cases as GC

    def collinear_last(p):
        p = np.float32(p)
        for j in range(6):
            d1 = (p[j] - p[6]).astype(np.float64)
            for k in range(j):
                d2 = (p[k] - p[6]).astype(np.float64)
                if abs(d2[0] * d1[1] - d2[1] * d1[0]) <= np.finfo(np.float32).eps * (abs(d1).sum() + abs(d2).sum()):
                    return True
        return False
    pts = GC.gather(GC.small())
    lines = [f"0 40 {len(pts)}"]
    for a, b in pts:
        lines.append(f"{len(a)} 1")
        lines += [f"{x1!r} {y1!r} {x2!r} {y2!r}" for (x1, y1), (x2, y2) in zip(a.tolist(), b.tolist())]
    r = subprocess.run([exe, "samples"], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    tok = np.array(r.stdout.split(), dtype=np.int64)
    at, got = 0, []
    for _ in pts:
        s = int(tok[at])
        got.append(tok[at + 1:at + 1 + 7 * s].reshape(s, 7))
        at += 1 + 7 * s
    assert at == len(tok)
    assert [len(g) for g in got] == [40 if len(a) >= 7 and p != GC.COLLINEAR else 0 for p, (a, _) in enumerate(pts)]
    for (a, b), g in zip(pts, got):
        for s in g:
            assert len(set(s.tolist())) == 7 and not collinear_last(a[s]) and not collinear_last(b[s])
    plain, _ = GC.py_subsets(64, 7, 40)                                              # pair 3: a general scene, nothing refused
    assert np.array_equal(got[3], plain)
    refusing, _ = GC.py_subsets(8, 7, 40)                                            # pair 7: four image-1 points on a line
    assert not np.array_equal(got[GC.REFUSING], refusing)
