"""GPU: the bundle-adjustment kernels against the CPU oracle on the ragged problems of tests/ba_ragged_cases.py — track lengths
with a heavy tail (landmarks of 1, 2, 3, 7, 9 observations leave lanes of linearize_landmark / ba_step_landmarks without
work), cameras of 0 to 5, 255 / 256 / 257 and 1023 / 1024 / 1025 observations (empty segments, the validity mask and the second
trip of linearize_camera_segment), global observer counts that differ from the local degree, mixed run lengths inside one
landmark group. The tolerances are those of tests/test_ba_gpu.py; tests/test_ba_ragged_reference.py holds the oracle itself on
these problems. Every test prints the figures it asserts on (`pytest -s`)."""
import dataclasses
import functools

import numpy as np
import pytest

from eacham_amd import ba
import ba_ragged_cases as RC
import oracle_api as O
from ba_helpers import backward_error, rel, ctx_with

pytestmark = pytest.mark.gpu
POSE_POINT_RTOL = 1e-5  # north_star tolerance
CFG = ba.OptimizerConfig.refine_ba()


@functools.lru_cache(maxsize=None)
def oracle_step(name, lam):
    ref = O.ba_step(RC.case(name), lam, 0)
    assert ref[-1]
    return ref


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    return O.ba_solve(RC.case(name), CFG)


def step_matches(ctx, A, ref, label):
    """One damped step on `ctx` against the oracle's (S, g, dc, dl, error, lin_change, ok): the bars of
    tests/test_ba_gpu.py::test_every_elimination_order_solves_the_same_system. Returns the camera step."""
    lam = label[1]
    So, go, dco, dlo, erro, lino, ok = ref
    S, g, dc, dl, err, lin = ba.debug_step(ctx, A, lam)
    bw, bw_ref = backward_error(So, go, dc), backward_error(So, go, dco)
    print("RAGGED step", *label, f"S {rel(S, So):.2e} g {rel(g, go):.2e} (< 1e-11)  dc {rel(dc, dco):.2e} dl {rel(dl, dlo):.2e} (< 1e-8)  "
          f"error {abs(err / erro - 1):.1e} lin {abs(lin / lino - 1):.1e}  backward error {bw:.2e} / oracle {bw_ref:.2e} = {bw / bw_ref:.2f}")
    assert rel(S, So) < 1e-11 and rel(g, go) < 1e-11, label
    assert rel(dc, dco) < 1e-8 and rel(dl, dlo) < 1e-8, label
    assert np.isclose(err, erro, rtol=1e-12) and np.isclose(lin, lino, rtol=1e-9), label
    assert bw <= 10 * bw_ref, (label, bw, bw_ref)
    assert not dl[RC.degree(A) == 0].any(), label      # an unobserved landmark does not move
    return dc


def run_matches(ctx, A, ref, label):
    """A whole LM run on `ctx` against the oracle's, and a second run bit for bit."""
    out = ba.RefineBA(ctx, A, CFG)
    assert out.status == ref.status == 0
    assert (out.outer_iterations, out.inner_iterations) == (ref.outer_iterations, ref.inner_iterations), label
    print("RAGGED run", *label, f"{out.outer_iterations} / {out.inner_iterations} iterations  trace {np.abs(out.trace[:, :3] / ref.trace[:, :3] - 1).max():.1e} "
          f"(1e-6)  poses {rel(out.cam_T_wc, ref.cam_T_wc):.1e} points {rel(out.points, ref.points):.1e} (< 1e-7)  K {np.abs(out.K / ref.K - 1).max():.1e} (1e-9)")
    assert np.array_equal(out.trace[:, 3:], ref.trace[:, 3:]) and np.allclose(out.trace[:, :3], ref.trace[:, :3], rtol=1e-6), label
    assert rel(out.cam_T_wc, ref.cam_T_wc) < 1e-7 and rel(out.points, ref.points) < 1e-7, label
    assert np.allclose(out.K, ref.K, rtol=1e-9), label
    assert np.isclose(out.initial_error, ref.initial_error, rtol=1e-12) and np.isclose(out.final_error, ref.final_error, rtol=1e-9), label
    again = ba.RefineBA(ctx, A, CFG)
    assert np.array_equal(out.points, again.points) and np.array_equal(out.cam_T_wc, again.cam_T_wc) and np.array_equal(out.trace, again.trace), label
    return out


@pytest.mark.parametrize("lam", [0.0, 1e-3])
@pytest.mark.parametrize("name", RC.CASES)
def test_damped_step_matches_oracle(hip_ctx, name, lam):
    step_matches(hip_ctx, RC.case(name), oracle_step(name, lam), (name, lam, "default"))


@pytest.mark.parametrize("name", RC.CASES)
def test_whole_run_matches_oracle(hip_ctx, name):
    run_matches(hip_ctx, RC.case(name), oracle_run(name), (name, "default"))


def _structure(ctx, A, want_groups):
    """Every structure array of the problem as prepared on `ctx`, and the group statistics where the groups were built."""
    pb = ba.PreparedBA(ctx, A)
    try:
        arrays = {n: pb.structure(n) for n in ba.PreparedBA.STRUCTURE}
        assert (len(arrays["g_groups"]) > 0) == want_groups and (len(arrays["blocks"]) == 0) == want_groups
        return arrays, (RC.group_stats_of(pb, len(A.cam_T_wc)) if want_groups else None)
    finally:
        pb.close()


PATHS = {"pairs": [dict(EACHAM_BA_SCHUR="pairs")],
         "groups": [dict(EACHAM_BA_SCHUR="groups"), dict(EACHAM_BA_SCHUR="groups", EACHAM_BA_GROUP_ROWS="64"),
                    dict(EACHAM_BA_SCHUR="groups", EACHAM_BA_GROUP_ROWS="480")]}


@pytest.mark.parametrize("schur", list(PATHS))
@pytest.mark.parametrize("name", RC.CASES)
def test_every_path_builds_and_solves_the_same_problem(name, schur):
    """Host loops and device sorts + scans (EACHAM_BA_PREPARE) under the pair lists and under the landmark groups of 128 (the
    size these problems select), 64 and 480 rows: the two constructions build every structure array byte for byte alike, every
    context returns the oracle's step and run, and the runs agree between contexts to 1e-9. The group structure must hold what
    the cases are for: runs of at most four entries and runs longer than a slice at every size, segments of fewer than
    GRP_SEG lanes, a block of more than GRP_LONG partials at 64 rows and full segments at 480."""
    A = RC.case(name)
    outs = []
    for env in PATHS[schur]:
        built = {}
        for prepare in ("host", "device"):
            ctx = ctx_with(EACHAM_BA_PREPARE=prepare, **env)
            try:
                label = (name, 1e-3, prepare, schur, env.get("EACHAM_BA_GROUP_ROWS", "-"))
                built[prepare], stats = _structure(ctx, A, schur == "groups")
                if stats:
                    print("RAGGED groups", *label, stats)
                    assert stats["rows"] == int(env.get("EACHAM_BA_GROUP_ROWS", 128)), label
                    assert stats["short_runs"] > 0 and stats["long_runs"] > 0 and stats["short_segments"] > 0, (label, stats)
                    assert stats["max_run"] > RC.GRP_SLICE * RC.GRP_SEG or stats["rows"] != 480, (label, stats)   # a run of several segments
                    assert stats["long_blocks"] > 0 or stats["rows"] != 64, (label, stats)
                    assert stats["full_segments"] > 0 or stats["rows"] != 480, (label, stats)
                step_matches(ctx, A, oracle_step(name, 1e-3), label)
                outs.append(run_matches(ctx, A, oracle_run(name), label))
            finally:
                ctx.close()
        for n in ba.PreparedBA.STRUCTURE:
            x, y = built["host"][n], built["device"][n]
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{name} {env}: structure array {n} differs ({x.shape} vs {y.shape})"
    for o in outs[1:]:
        assert rel(o.points, outs[0].points) < 1e-9 and rel(o.cam_T_wc, outs[0].cam_T_wc) < 1e-9


@pytest.mark.parametrize("name", ["tail_small", "camera_counts"])
def test_dogleg_parity(hip_ctx, name):
    """tests/test_ba_gpu.py::test_dogleg_parity (delta = 10) on the ragged cases."""
    A = RC.case(name)
    cfg = ba.OptimizerConfig("DogLeg", 100, 1e-5, 10.0, False)
    out = ba.RefineBA(hip_ctx, A, cfg)
    ref = O.ba_solve(A, cfg)
    lm = oracle_run(name)
    assert out.status == ref.status == 0
    assert (out.outer_iterations, out.inner_iterations) == (ref.outer_iterations, ref.inner_iterations)
    print("RAGGED dogleg", name, out.outer_iterations, "iterations  trace", np.abs(out.trace[:, :3] / ref.trace[:, :3] - 1).max(), "poses",
          rel(out.cam_T_wc, ref.cam_T_wc), "points", rel(out.points, ref.points))
    assert np.array_equal(out.trace[:, 3:], ref.trace[:, 3:]) and np.allclose(out.trace[:, :3], ref.trace[:, :3], rtol=1e-6)
    assert rel(out.cam_T_wc, ref.cam_T_wc) < 1e-7 and rel(out.points, ref.points) < 1e-7
    assert np.allclose(out.K, ref.K, rtol=1e-9) and np.isclose(out.final_error, ref.final_error, rtol=1e-9)
    assert np.isclose(out.final_lambda, ref.final_lambda, rtol=1e-6)          # the final trust radius
    assert np.isclose(out.final_error, lm.final_error, rtol=1e-4)             # same optimum as LM


def test_pcg_block_jacobi_parity_on_the_cut_window(hip_ctx):
    """tests/test_ba_gpu.py::test_pcg_block_jacobi_parity on window_cut: every damped system by PCG + block-Jacobi."""
    A = RC.case("window_cut")
    cfg = ba.OptimizerConfig("LM", 100, 1e-5, 10.0, True)
    out = ba.RefineBA(hip_ctx, A, cfg)
    ref = O.ba_solve(A, cfg)
    direct = ba.RefineBA(hip_ctx, A, ba.OptimizerConfig("LM", 100, 1e-5, 10.0, False))
    print("RAGGED pcg", out.inner_iterations, "LM iterations", out.reserved, "PCG iterations, oracle", ref.reserved, " poses", rel(out.cam_T_wc, ref.cam_T_wc),
          "points", rel(out.points, ref.points))
    assert out.status == ref.status == 0 and out.reserved > 20 * out.inner_iterations and direct.reserved == 0
    assert abs(out.reserved - ref.reserved) <= 0.05 * ref.reserved + 5
    assert (out.outer_iterations, out.inner_iterations) == (ref.outer_iterations, ref.inner_iterations)
    assert np.array_equal(out.trace[:, 3:], ref.trace[:, 3:]) and np.allclose(out.trace[:, :3], ref.trace[:, :3], rtol=1e-5)
    for other in (ref, direct):
        assert rel(out.cam_T_wc, other.cam_T_wc) < POSE_POINT_RTOL and rel(out.points, other.points) < POSE_POINT_RTOL
        assert np.isclose(out.final_error, other.final_error, rtol=1e-7)


def test_elimination_orders_on_the_large_tail(hip_ctx):
    """tests/test_ba_gpu.py::test_every_elimination_order_solves_the_same_system for the caller's order and nested dissection on
    tail_large, whose reduced system has two empty camera blocks (cameras of 0 and 1 observations) in it."""
    A = RC.case("tail_large")
    ref = oracle_step("tail_large", 1e-3)
    steps = {}
    for order in ("natural", "nd"):
        B = dataclasses.replace(A, ordering=order)
        pb = ba.PreparedBA(hip_ctx, B)
        info = pb.plan_info()
        pb.close()
        assert info["ordering"] == order
        steps[order] = step_matches(hip_ctx, B, ref, ("tail_large", 1e-3, order, info["panels"], info["levels"]))
    assert rel(steps["nd"], steps["natural"]) < 1e-9
