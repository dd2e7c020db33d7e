"""GPU: the five-point kernel (essential5_wave, eacham_amd/csrc/solve_dev.hpp) on the samples of tests/golden/essential5_golden.npz —
generic, outliers, forward motion, near-planar and short-baseline scenes with their solution sets at 60 digits (the file is all
this test reads; tests/test_essential5_reference.py holds the CPU restatement to it):

  one eacham_solve_minimal call on all 512 samples, with K and with points normalised by the caller and K = None: counts and
      models bit for bit the restatement's, and on every decided sample exactly the 60-digit solutions within the file's bound;
  the same samples through eacham_lmeds_batch and eacham_ransac_batch, one problem per scene: n_candidates is the sum of the
      60-digit counts over the samples consumed (the kernel's own count where a sample is undecided);
  every call twice on one context: the same bytes."""
import numpy as np
import pytest

from eacham_amd import score
import essential5_cases as EC
import oracle_api as O

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def golden():
    g = EC.load()
    g["n1"], g["n2"] = (g["uv1"] - g["K"][2:]) / g["K"][:2], (g["uv2"] - g["K"][2:]) / g["K"][:2]
    return g


@pytest.fixture(scope="module")
def solved(hip_ctx, golden):
    """The kernel's models and counts on all samples (with K): computed once, shared, never written to."""
    return score.solve_minimal(hip_ctx, "essential5", golden["uv1"], golden["uv2"], golden["samples"], golden["K"])


def expected_candidates(g, counts, k):
    """Sum over the scene's samples of the 60-digit count where the sample is decided, of the kernel's own count elsewhere."""
    of = g["scene"] == k
    dec = g["decided"].astype(bool)
    return int(g["mp_count"][of & dec].sum() + counts[of & ~dec].sum())


@pytest.mark.parametrize("with_K", [True, False])
def test_solve_minimal_is_the_restatement_and_the_60_digit_solution_set(hip_ctx, golden, with_K):
    g = golden
    a, b, K = (g["uv1"], g["uv2"], g["K"]) if with_K else (g["n1"], g["n2"], None)
    models, counts = score.solve_minimal(hip_ctx, "essential5", a, b, g["samples"], K)
    want, wcounts = O.solve_minimal("essential5", a, b, g["samples"], K)
    assert np.array_equal(counts, wcounts) and np.array_equal(bits(models), bits(want))
    worst = EC.assert_solution_sets(g, models, counts, "kernel, K" if with_K else "kernel, K = None")
    print(f"worst distance from the 60-digit sets {worst:.3e}, bound {float(g['bound']):.3e}, counts {np.bincount(counts).tolist()}")
    again, acounts = score.solve_minimal(hip_ctx, "essential5", a, b, g["samples"], K)
    assert np.array_equal(acounts, counts) and np.array_equal(bits(again), bits(models))


@pytest.mark.parametrize("with_K", [True, False])
def test_lmeds_batch_sees_every_solution(hip_ctx, golden, solved, with_K):
    """LMedS has no budget: every sample of a problem is solved and every model is a candidate."""
    g = golden
    P = g["problems"]
    uv1, uv2 = ([p[0] for p in P], [p[1] for p in P]) if with_K else ([(p[0] - g["K"][2:]) / g["K"][:2] for p in P], [(p[1] - g["K"][2:]) / g["K"][:2] for p in P])
    run = lambda: hip_ctx.lmeds_batch("essential", uv1, uv2, [p[2] for p in P], g["K"] if with_K else None)   # noqa: E731
    got, again = run(), run()
    assert got.n_candidates.tolist() == [expected_candidates(g, solved[1], k) for k in range(len(P))]
    assert (got.winner[:, 0] >= 0).all()
    for x, y in zip(got[:4] + got[5:7], again[:4] + again[5:7]):
        assert x.tobytes() == y.tobytes()
    assert all(np.array_equal(x, y) for x, y in zip(got.masks, again.masks))
    for p in range(len(P)):                                    # the winner is the kernel's model of that sample and root (the caller's
        _, s, r = got.winner[p]                                # normalisation is the kernel's own two operations: the same bits)
        assert np.array_equal(bits(got.models[p]), bits(solved[0][EC.S * p + s, r]))


@pytest.mark.parametrize("with_K", [True, False])
def test_ransac_batch_sees_every_solution_of_the_samples_it_consumes(hip_ctx, golden, solved, with_K):
    """All 64 samples of every problem are consumed, by this argument: the loop ends early only when a record shrinks the budget, a
    record needs a candidate with more inliers than max(best, 4), i.e. at least five points with err <= threshold, and with
    threshold = 0 that is five points whose float32 error is exactly +0 — the five points of the candidate's own sample have
    residuals of rounding size, 1e-30 and more after squaring, far above the smallest float32. n_used == 64 is asserted all the
    same, so the argument is checked and not relied on. stage1 = 64 solves all samples in the first pass, the default in two."""
    from eacham_amd import ransac
    g = golden
    P = g["problems"]
    uv1, uv2 = ([p[0] for p in P], [p[1] for p in P]) if with_K else ([(p[0] - g["K"][2:]) / g["K"][:2] for p in P], [(p[1] - g["K"][2:]) / g["K"][:2] for p in P])
    for stage1 in (EC.S, 0):
        run = lambda: ransac.ransac_batch(hip_ctx, "essential", uv1, uv2, [p[2] for p in P], 0.0, 0.99, stage1, g["K"] if with_K else None)   # noqa: E731
        got, again = run(), run()
        assert got.n_used.tolist() == [EC.S] * len(P), stage1
        assert got.n_candidates.tolist() == [expected_candidates(g, solved[1], k) for k in range(len(P))], stage1
        for x, y in zip(got[:2] + got[3:6], again[:2] + again[3:6]):
            assert x.tobytes() == y.tobytes()
        assert all(np.array_equal(x, y) for x, y in zip(got.masks, again.masks))
