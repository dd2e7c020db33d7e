"""GPU: the estimator entry points whose solver kernels are ONE source for the one-problem and the list form
(eacham_amd/csrc/solve.hip: solve_h4_kernel / solve_e5_kernel / solve_pnp_front_kernel / solve_pnp_back_kernel<LIST>, and
pnp_refit_body under solve_pnp_big_kernel and pb_refit_kernel) against the CPU ORACLES directly, as bytes. The list tests of
tests/test_lmeds_batch_gpu.py / tests/test_pnp_batch_gpu.py hold a list call to the composition of the one-problem calls of the
same library: with one kernel on both sides of that comparison, this file is what ties the solve stage to something else.

  eacham_lmeds_batch            every case of tests/lmeds_batch_cases.py in the three variants, and multi_root, against
                                test_lmeds_batch_reference.oracle_compose
  eacham_pnp_hypotheses_batch   HYP_CASES against compose_hypotheses over O.solve_pnp / oracle_score
  eacham_pnp_refit_batch        refit_case() against compose_refit over the same
  eacham_solve_minimal          both kinds, 40 points, n_samples at the edges of SOLVE_WAVES = 4 samples per workgroup
  eacham_solve_pnp              five-point samples at those counts and at the edges of the back half's 64 samples per workgroup;
                                sample sizes 6, 63, 64, 65, 129 (the front half's LDS row stride; the three-wave form on both
                                sides of one term per lane)
  a problem smaller than a sample: the one-problem call solves whatever valid indices it is given (repeated ones here), the
  list call answers "none" without running the solver."""
import numpy as np
import pytest

from eacham_amd import score
import lmeds_batch_cases as LC
import oracle_api as O
import pnp_batch_cases as PC
import score_cases as SC
import test_lmeds_batch_gpu as LG
import test_lmeds_batch_reference as LREF
import test_pnp_batch_gpu as PG
import test_pnp_batch_reference as PREF

pytestmark = pytest.mark.gpu

bits = PREF.bits
COUNTS = [1, 3, 4, 5, 64, 65]


def same_bytes(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


LMEDS = [(n, v) for n in LC.CASES for v in LG.VARIANTS] + [("multi_root", v) for v in LG.VARIANTS[1:]]   # (multi_root: essential only)


@pytest.mark.parametrize("name,variant", LMEDS, ids=[f"{n}-{v}" for n, v in LMEDS])
def test_lmeds_batch_equals_the_oracle_composition(hip_ctx, name, variant):
    case = LG.build(name, variant)
    LG.assert_same(LG.run(hip_ctx, case), LREF.oracle_compose(case), f"{name}/{variant}")


@pytest.mark.parametrize("name", list(PC.HYP_CASES))
def test_pnp_hypotheses_batch_equals_the_oracle_composition(hip_ctx, name):
    c = PC.HYP_CASES[name]()
    want = PREF.compose_hypotheses(O.solve_pnp, PREF.oracle_score, c["X"], c["uv"], c["K"], c["samples"], PC.THR)
    PG.assert_same_hypotheses(hip_ctx.pnp_hypotheses_batch(c["X"], c["uv"], c["K"], c["samples"], PC.THR), want, name)


def test_pnp_refit_batch_equals_the_oracle_composition(hip_ctx):
    c = PC.refit_case()
    want = PREF.compose_refit(O.solve_pnp, PREF.oracle_score, c["X"], c["uv"], c["K"], c["models"], c["has_model"], PC.THR)
    PG.assert_same_refit(hip_ctx.pnp_refit_batch(c["X"], c["uv"], c["K"], c["models"], c["has_model"], PC.THR), want)


@pytest.mark.parametrize("kind", ["homography4", "essential5"])
def test_solve_minimal_at_the_workgroup_edges(hip_ctx, kind):
    c = SC.two_view_case(n=40, n_models=1, seed=3, outliers=0.25, planar=kind == "homography4", facing=True)
    for count in COUNTS:
        rows = LC.draw(40, 4 if kind == "homography4" else 5, count, 100 + count)
        got, gn = score.solve_minimal(hip_ctx, kind, c["uv1"], c["uv2"], rows, c["K"])
        want, wn = O.solve_minimal(kind, c["uv1"], c["uv2"], rows, c["K"])
        assert same_bytes(gn, wn) and same_bytes(got, want), count
        assert gn.any()


def test_solve_pnp_five_point_samples_at_the_workgroup_edges(hip_ctx):
    X, uv, _, _ = PC.problem(40, 0, 7)
    for count in COUNTS:
        rows = PC.draw(40, count, 200 + count)
        got, gok = score.solve_pnp(hip_ctx, X, uv, PC.K, rows)
        want, wok = O.solve_pnp(X, uv, PC.K, rows)
        assert same_bytes(gok, wok) and same_bytes(got, want), count
        assert gok.any()


@pytest.mark.parametrize("m", [6, 63, 64, 65, 129])
def test_solve_pnp_sample_sizes_around_a_wave(hip_ctx, m):
    X, uv, _, _ = PC.problem(200, 0, 9, outliers=0.0)
    rng = np.random.default_rng(m)
    rows = np.array([rng.choice(200, size=m, replace=False) for _ in range(3)], np.int32)
    got, gok = score.solve_pnp(hip_ctx, X, uv, PC.K, rows)
    want, wok = O.solve_pnp(X, uv, PC.K, rows)
    assert same_bytes(gok, wok) and same_bytes(got, want) and gok.all()


SMALL = [("homography", 1, [[0, 0, 0, 0]]), ("homography", 2, [[0, 1, 0, 1], [1, 1, 0, 0]]), ("homography", 3, [[0, 1, 2, 0], [2, 2, 1, 0]]),
         ("essential", 1, [[0, 0, 0, 0, 0]]), ("essential", 4, [[0, 1, 2, 3, 0], [3, 2, 1, 0, 3]])]


@pytest.mark.parametrize("kind,n,rows", SMALL, ids=[f"{k}-{n}" for k, n, _ in SMALL])
def test_a_problem_smaller_than_a_sample(hip_ctx, kind, n, rows):
    """The n < m rule belongs to the list call alone: eacham_solve_minimal validates the indices against n_points and solves the
    sample (what tests/test_solve_gpu.py compares: the counts and the models, against the oracle); eacham_lmeds_batch gives the
    problem the "none" record with no candidates."""
    c = SC.two_view_case(n=8, n_models=1, seed=5, outliers=0.0, planar=kind == "homography", facing=True)
    uv1, uv2, rows = c["uv1"][:n].copy(), c["uv2"][:n].copy(), np.array(rows, np.int32)
    got, gn = score.solve_minimal(hip_ctx, LREF.SOLVER[kind], uv1, uv2, rows, c["K"])
    want, wn = O.solve_minimal(LREF.SOLVER[kind], uv1, uv2, rows, c["K"])
    assert np.array_equal(gn, wn) and np.array_equal(got, want)
    g = hip_ctx.lmeds_batch(kind, [uv1], [uv2], [rows], c["K"])
    assert int(g.n_candidates[0]) == 0
    LG.assert_same(g, [LREF.none_record(n)], f"{kind} {n} points")
