"""CPU: the bundle-adjustment oracle on the ragged problems of tests/ba_ragged_cases.py, before any kernel is judged by it
(tests/test_ba_ragged_gpu.py). Per case: the properties the case exists for, a damped step that exists at lambda 0 and 1e-3,
the Schur step against a dense solve of ALL variables (the check of tests/test_ba_oracle.py on these shapes), the camera step
against numpy's solve of the oracle's own reduced system, and what ba_groups.hpp's host statement builds for the case."""
import numpy as np
import pytest

import ba_ragged_cases as RC
import oracle_api as O
from ba_helpers import backward_error, rel, schur_step_equals_dense_step

LAMBDAS = [0.0, 1e-3]


@pytest.fixture(scope="module")
def stats_driver(tmp_path_factory):
    return RC.build_stats_driver(tmp_path_factory.mktemp("groups_stats"))


@pytest.mark.parametrize("name", RC.CASES)
def test_case_holds_what_it_is_for(name):
    """The generators assert their own properties; here the ones every case shares."""
    A = RC.case(name)
    deg, load = RC.degree(A), RC.camera_load(A)
    assert A.cam_fixed.sum() == 1 and (A.cam_fixed[0] == 1 or name == "window_cut")    # (the window's fixed node is its second frame)
    assert len(A.obs_cam) == len(A.obs_point) == len(A.obs_uv) <= 20_000
    assert (deg == 1).any() and deg.max() >= 7 and len(np.unique(deg[deg > 0])) >= 6     # a tail, not one degree
    assert (len(A.points) > 8192) == (name == "tail_large")     # two lanes per landmark there, eight everywhere else
    # degrees that leave lanes of a landmark's 8 (or 2) without work, and in the tail cases one that wraps
    assert {1, 2, 3, 7} <= set(deg) and (9 in deg or name in ("camera_counts", "window_cut"))
    if name in ("tail_large", "camera_counts"):                 # a near-idle camera beside busy ones
        assert load.min() == 0 and np.sort(load)[1] == 1 and load.max() > 500


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("name", RC.CASES)
def test_oracle_step_on_ragged_cases(name, lam):
    """The dense form holds (6 n_cams + 5 + 3 n_points)^2 doubles: tail_large (27 149 unknowns, 5.9 GB) goes through it as the
    problem of its first 1500 landmarks — same cameras, same degree law, cameras 5 and 9 idle — and through the other checks whole."""
    A = RC.case(name)
    if name == "tail_large":
        part = RC.first_landmarks(A, 1500)
        assert {0, 1, 2, 3, 7, 9} <= set(RC.degree(part)) and (RC.camera_load(part) == 0).sum() >= 2
        schur_step_equals_dense_step(part, lam)
        S, g, dc, dl, err, lin, ok = O.ba_step(A, lam, 0)
        assert ok
    else:
        S, g, dc, dl, err, lin, ok = schur_step_equals_dense_step(A, lam)
    bw = backward_error(S, g, dc)
    dense = np.linalg.solve(S, g)
    print(f"{name} lambda {lam}: backward error {bw:.2e}, dc against numpy's solve of S {rel(dc, dense):.2e}")
    assert bw < 1e-16                          # below fp64 round-off: the bar the device step is held to (10 x this) is a real one
    assert rel(dc, dense) < 1e-10              # worse: change the case (fewer near-idle cameras), not the GPU tolerance
    assert not dl[RC.degree(A) == 0].any()     # an unobserved landmark sits at its prior's mean: no step


@pytest.mark.parametrize("name", RC.CASES)
def test_oracle_solve_converges(name):
    from eacham_amd import ba
    A = RC.case(name)
    out = O.ba_solve(A, ba.OptimizerConfig.refine_ba())
    assert out.status == 0 and 2 <= out.outer_iterations <= 30 and out.final_error < out.initial_error


def test_group_structure_reaches_every_size_class(stats_driver):
    """ba_groups.hpp's host statement on the cases, at the group size each problem selects and at the two sizes the GPU tests
    force: every case has a run of at most four entries (the group's last lanes) and one longer than a slice; over all cases
    there are segments of fewer than GRP_SEG lanes and blocks with more than GRP_LONG partials."""
    total = {"short_segments": 0, "long_blocks": 0}
    for name in RC.CASES:
        for rows in (0, 64, 480):
            st = RC.host_group_stats(stats_driver, RC.case(name), rows)
            print(name, rows, st)
            assert st["built"] and st["entries_ok"], (name, rows, st)
            assert st["short_runs"] > 0 and st["long_runs"] > 0, (name, rows, st)
            if rows == 0:
                for k in total:
                    total[k] += st[k]
    assert total["short_segments"] > 0 and total["long_blocks"] > 0, total
