"""CPU: the restatement of eacham_pnp_refine_batch (tests/cpp/pnp_refine_reference.c, which the kernel is held to as bytes by
tests/test_pnp_refine_gpu.py) held to what it restates: its Jacobian to a 60-digit derivative, its converged poses to the 60-digit
minimisers of tests/golden/pnp_refine_golden.npz (bound: 8 x the restatement's own largest deviation, recorded when the file is made),
the true pose on exact pixels, a cost that never rises, a final cost at or below EPnP's on the same rows, the share of problems that
reach the cap, the not-refined cases, and a run of the whole case list under the address and undefined-behaviour sanitizers."""
import subprocess

import numpy as np
import pytest

import oracle_api as O
import p3p_cases as PC
import pnp_refine_cases as RC
import pnp_refine_reference as R

# exact pixels: the loop stops at a step of 1e-10 it has not taken, under Gauss-Newton's quadratic convergence on a zero residual the
# step still to go is about the error; |R|, |t| entries of a scene are below 10 and the pixels' own rounding (1e-13 px over 960 px
# of focal length) is far below: 1e-8 leaves a factor 10 for the flattest scenes of the list.
TRUTH_BOUND = 1e-8


@pytest.fixture(scope="module")
def seeded():
    cases = RC.seeded()
    X, uv, T0, has = RC.lists(cases)
    out, trace = R.refine_batch(X, uv, RC.K, T0, has, want_trace=True)
    return cases, out, trace


def test_the_jacobian_is_the_60_digit_derivative_of_the_residual():
    MP = pytest.importorskip("pnp_refine_mp_reference")
    worst = 0.0
    for c in RC.seeded()[2:40:3]:
        for i in (0, c["n"] - 1):
            J, _ = R.jacobian(c["X"][i], c["uv"][i], c["T0"], RC.K)
            want = MP.jacobian(c["X"][i], c["uv"][i], c["T0"], RC.K)
            rel = np.abs(J - want).max(1) / np.abs(want).max(1)
            worst = max(worst, float(rel.max()))
            assert (rel <= 1e-9).all(), (c["n"], i, rel)
    print(f"largest relative deviation of a Jacobian row: {worst:.3e}")


def test_converged_problems_lie_within_the_bound_of_the_60_digit_minimiser():
    g = np.load(RC.GOLDEN)
    P = len(g["T0"])
    ptr = g["point_ptr"]
    X, uv = [g["X"][ptr[p]:ptr[p + 1]] for p in range(P)], [g["uv"][ptr[p]:ptr[p + 1]] for p in range(P)]
    cases = RC.seeded()[:P]
    for p, c in enumerate(cases):   # the file holds the problems the generator still makes
        assert np.array_equal(c["X"], X[p]) and np.array_equal(c["uv"], uv[p]) and np.array_equal(c["T0"], g["T0"][p]), p
    out = R.refine_batch(X, uv, g["K"], g["T0"], np.ones(P, np.uint8))
    conv = out.status == R.CONVERGED
    dev = np.abs(out.refined - g["minimiser"]).max(1)
    print(f"{int(conv.sum())} of {P} converged; largest distance from the minimiser {dev[conv].max():.3e}, bound {float(g['bound']):.3e}")
    assert conv.sum() >= 0.98 * P
    assert float(g["bound"]) == 8 * float(g["deviation"]) and float(g["bound"]) <= 1e-5
    assert (dev[conv] <= float(g["bound"])).all(), np.nonzero(conv & (dev > float(g["bound"])))[0]


def test_the_minimiser_is_rederived_at_60_digits():
    MP = pytest.importorskip("pnp_refine_mp_reference")
    g = np.load(RC.GOLDEN)
    cases = RC.seeded()
    for p in (2, 6):   # 5 and 20 noisy points
        M, cost, it, size = MP.minimise(cases[p]["X"], cases[p]["uv"], RC.K, cases[p]["T"])
        assert size < 1e-50 and np.array_equal(M, g["minimiser"][p]) and cost == g["min_cost"][p], p


def test_exact_pixels_give_the_true_pose(seeded):
    cases, out, _ = seeded
    exact = np.array([c["noise"] == 0 for c in cases])
    err = PC.pose_error(out.refined, np.array([c["T"] for c in cases]))
    print(f"{int(exact.sum())} exact problems: largest pose error {err[exact].max():.3e}, largest final cost {out.cost[exact, 1].max():.3e}")
    assert exact.sum() >= 100 and (out.status[exact] == R.CONVERGED).all()
    assert (err[exact] <= TRUTH_BOUND).all(), np.nonzero(exact & (err > TRUTH_BOUND))[0]


def test_the_cost_never_rises_over_accepted_steps(seeded):
    cases, out, trace = seeded
    far = [RC.problem(n, seed, off, planar=planar, noise=1.0) for n, seed, off, planar in RC.FAR_STARTS]
    fo, ft = R.refine_batch([p[0] for p in far], [p[1] for p in far], RC.K, [p[2] for p in far], np.ones(len(far), np.uint8), want_trace=True)
    rejected = 0
    for o, tr in ((out, trace), (fo, ft)):
        for p in range(len(o.tries)):
            rows = tr[p, :o.tries[p]]
            acc = rows[rows[:, 1] == 1, 0]
            chain = np.concatenate([[o.cost[p, 0]], acc])
            assert (np.diff(chain) < 0).all(), p                                   # every accepted cost is below the one before it
            assert o.cost[p, 1] == chain[-1] and o.cost[p, 1] <= o.cost[p, 0], p   # and the last one is what is reported
            lam = rows[:, 2]
            assert (lam >= 1e-12).all() and (lam <= 1e12).all()
            rejected += int((rows[:, 1] == 0).sum())
    assert rejected >= 27                                                          # the far starts alone reject 9 tries each


def test_the_final_cost_is_at_or_below_epnp_s_on_the_same_rows():
    cases = [c for c in RC.seeded() if c["noise"] > 0 and c["n"] >= 6]
    assert len(cases) >= 60
    poses = []
    for c in cases:
        m, ok = O.solve_pnp(c["X"], c["uv"], RC.K, np.arange(c["n"], dtype=np.int32)[None])
        assert ok[0], c["n"]
        poses.append(m[0])
    out = R.refine_batch([c["X"] for c in cases], [c["uv"] for c in cases], RC.K, np.array(poses), np.ones(len(cases), np.uint8))
    assert (out.status != R.NOT_REFINED).all()
    assert (out.cost[:, 1] <= out.cost[:, 0]).all()
    gain = out.cost[:, 0] / out.cost[:, 1]
    print(f"{len(cases)} noisy problems from EPnP's pose: cost EPnP / refined, median {np.median(gain):.3f}, smallest {gain.min():.4f}, "
          f"largest {gain.max():.1f}; tries median {int(np.median(out.tries))}, most {int(out.tries.max())}")


def test_at_most_two_percent_of_the_seeded_problems_reach_the_cap(seeded):
    cases, out, _ = seeded
    cap = int((out.status == R.CAP).sum())
    print(f"{cap} of {len(cases)} problems at the cap of {RC.MAX_TRIES}; most tries {int(out.tries.max())}, mean {out.tries.mean():.2f}")
    assert len(cases) >= 200 and (out.status != R.NOT_REFINED).all()
    assert cap <= 0.02 * len(cases)


def test_not_refined_problems_copy_through_and_leave_their_neighbours_alone():
    X, uv, T0, has, use, notes = RC.gpu_list()
    out, trace = R.refine_batch(X, uv, RC.K, T0, has, use, RC.MAX_TRIES, RC.THR, want_trace=True)
    by = {n: p for p, n in enumerate(notes)}
    for note in ("empty", "no pose", "mask none", "only the last row", "two rows", "behind", "nan used"):
        p = by[note]
        assert 0 < p < len(X) - 1, note                                            # in the middle of the list
        assert out.status[p] == R.NOT_REFINED and out.tries[p] == 0, note
        want = T0[p] if has[p] else np.zeros(12)
        assert np.array_equal(out.refined[p].view(np.uint64), want.view(np.uint64)), note
        assert np.array_equal(out.cost[p, :1].view(np.uint64), out.cost[p, 1:].view(np.uint64)), note
    assert out.cost[by["no pose"]].tolist() == [0, 0] and not out.masks[by["no pose"]].any() and out.n_inliers[by["no pose"]] == 0
    assert out.cost[by["mask none"]].tolist() == [0, 0] and out.cost[by["two rows"], 0] > 0 and out.cost[by["behind"], 0] > 0
    assert out.cost[by["nan used"]].view(np.uint64).tolist() == [0x7ff8000000000000] * 2
    assert out.status[by["nan unused"]] == R.CONVERGED and out.status[by["planar"]] == R.CONVERGED
    # a problem alone gives what it gives in the list: the neighbours of the not-refined ones included
    for p in (by["empty"] - 1, by["no pose"] + 1, by["nan used"] - 1, by["nan used"] + 1, by["behind"] - 1):
        one = R.refine_batch([X[p]], [uv[p]], RC.K, T0[p:p + 1], has[p:p + 1], [use[p]], RC.MAX_TRIES, RC.THR)
        assert np.array_equal(one.refined[0], out.refined[p]) and np.array_equal(one.cost[0], out.cost[p]) and one.tries[0] == out.tries[p]
        assert np.array_equal(one.masks[0], out.masks[p])
    # what the list of the GPU test is meant to cover
    used = [int(m.sum()) for m in use]
    assert len(used) == 67
    for m in RC.USED_COUNTS:   # every count once with every row used and once with gaps
        assert any(u == m and len(k) == m for u, k in zip(used, use)) and any(u == m and len(k) > m for u, k in zip(used, use)), m
    far = [p for p, n in enumerate(notes) if n == "far start"]
    assert min(int((trace[p, :out.tries[p], 1] == 0).sum()) for p in far) >= 9
    assert out.status[far[0]] == R.CONVERGED and out.status[far[-1]] == R.CAP
    live = out.status != R.NOT_REFINED
    one_try = R.refine_batch(X, uv, RC.K, T0, has, use, 1, RC.THR)
    three = R.refine_batch(X, uv, RC.K, T0, has, use, 3, RC.THR)
    assert (one_try.status[live] == R.CAP).all() and (one_try.tries[live] == 1).all()      # nothing is done after one try
    assert (three.status[live] == R.CAP).sum() >= 50 and (three.cost[live, 1] > out.cost[live, 1]).sum() >= 50   # a cap of 3: in mid-descent


def test_the_case_lists_run_clean_under_the_sanitizers(tmp_path):
    exe = R.build_program(("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))
    X, uv, T0, has, use, _ = RC.gpu_list()
    cases = RC.seeded()
    runs = {"list": (X, uv, T0, has, use, 20), "list3": (X, uv, T0, has, use, 3), "list null mask": (X, uv, T0, has, None, 20),
            "seeded": (*RC.lists(cases), None, 20)}
    for name, (x, u, t0, h, m, cap) in runs.items():
        path = str(tmp_path / "cases.bin")
        R.write_cases(path, x, u, RC.K, t0, h, m, cap, RC.THR)
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, f"{name}: {r.stderr[-2000:]}"
        want = R.refine_batch(x, u, RC.K, t0, h, m, cap, RC.THR)
        lines = [ln.split() for ln in r.stdout.splitlines()]
        assert len(lines) == len(h), name
        assert [int(ln[1]) for ln in lines] == want.status.tolist() and [int(ln[2]) for ln in lines] == want.tries.tolist(), name
        assert [int(ln[3]) for ln in lines] == want.n_inliers.tolist(), name
