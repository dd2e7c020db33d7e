"""CPU: the restatement of eacham_triangulate_refine_tracks (tests/cpp/tri_refine_reference.c, which the kernel is held to as bytes by
tests/test_tri_refine_gpu.py) held to what it restates: its Jacobian to a 60-digit derivative, its converged points to the 60-digit
minimisers of tests/golden/tri_refine_golden.npz (bound: 8 x the restatement's own largest deviation, recorded when the file is made),
the true point on exact pixels, a cost that never rises, the not-refined cases, caps hit in mid-descent, and a run of the whole case
list under the address and undefined-behaviour sanitizers (a stand-alone program)."""
import subprocess

import numpy as np
import pytest

import tri_refine_cases as RC
import tri_refine_reference as R

# exact pixels: the loop stops at a step of 1e-10 (1 + max |X|) it has not taken; under Gauss-Newton's quadratic convergence on a zero
# residual the step still to go is far below the one just found: 1e-8 leaves a factor of 100.
TRUTH_BOUND = 1e-8


def distance(X, Xref):
    return np.abs(X - Xref).max(1) / (1 + np.abs(Xref).max(1))


@pytest.fixture(scope="module")
def seeded():
    cases = RC.seeded()
    out, trace = R.refine_tracks(*RC.args(RC.pack(cases), with_mask=False), want_trace=True)
    return cases, out, trace


@pytest.fixture(scope="module")
def listed():
    c, notes = RC.gpu_list()
    out, trace = R.refine_tracks(*RC.args(c), RC.MAX_TRIES, RC.THR, want_trace=True)
    return c, notes, out, trace


def test_the_jacobian_is_the_60_digit_derivative_of_the_residual():
    MP = pytest.importorskip("tri_refine_mp_reference")
    worst = 0.0
    for c in RC.seeded()[2:60:3]:
        for i in (0, c["m"] - 1):
            J, _ = R.jacobian(c["T"][i], c["uv"][i], c["X0"], RC.K)
            want = MP.jacobian(c["T"][i], c["uv"][i], c["X0"], RC.K)
            rel = np.abs(J - want).max(1) / np.abs(want).max(1)
            worst = max(worst, float(rel.max()))
            assert (rel <= 1e-9).all(), (c["m"], i, rel)
    print(f"largest relative deviation of a Jacobian row: {worst:.3e}")


def test_converged_tracks_lie_within_the_bound_of_the_60_digit_minimiser():
    g = np.load(RC.GOLDEN)
    n = len(g["X0"])
    ptr = g["track_ptr"]
    cases = RC.seeded()[:n]
    for p, c in enumerate(cases):   # the file holds the tracks the generator still makes
        assert np.array_equal(c["T"], g["T"][ptr[p]:ptr[p + 1]]) and np.array_equal(c["uv"], g["uv"][ptr[p]:ptr[p + 1]]), p
        assert np.array_equal(c["X0"], g["X0"][p]), p
    out = R.refine_tracks(g["T"], ptr, np.arange(ptr[-1]), g["uv"], g["K"], g["X0"], np.ones(n, np.uint8))
    conv = out.status == R.CONVERGED
    dev = distance(out.refined, g["minimiser"])
    print(f"{int(conv.sum())} of {n} converged; largest distance from the minimiser {dev[conv].max():.3e}, bound {float(g['bound']):.3e}; "
          f"most tries {int(out.tries.max())}")
    assert conv.sum() >= 0.98 * n
    assert float(g["bound"]) == 8 * float(g["deviation"]) and float(g["bound"]) <= 1e-6
    assert (dev[conv] <= float(g["bound"])).all(), np.nonzero(conv & (dev > float(g["bound"])))[0]


def test_the_minimiser_is_rederived_at_60_digits():
    MP = pytest.importorskip("tri_refine_mp_reference")
    g = np.load(RC.GOLDEN)
    cases = RC.seeded()
    for p in (2, 18):   # 4 and 16 noisy views
        assert cases[p]["noise"] > 0
        X, cost, it, size = MP.minimise(cases[p]["T"], cases[p]["uv"], RC.K, cases[p]["X"])
        assert size < 1e-50 and np.array_equal(X, g["minimiser"][p]) and cost == g["min_cost"][p], p


def test_exact_pixels_give_the_true_point(seeded):
    cases, out, _ = seeded
    exact = np.array([c["noise"] == 0 for c in cases])
    err = distance(out.refined, np.array([c["X"] for c in cases]))
    print(f"{int(exact.sum())} exact tracks: largest distance from the truth {err[exact].max():.3e}, largest final cost {out.cost[exact, 1].max():.3e}")
    assert exact.sum() >= 100 and (out.status[exact] == R.CONVERGED).all()
    assert (err[exact] <= TRUTH_BOUND).all(), np.nonzero(exact & (err > TRUTH_BOUND))[0]


def test_the_cost_never_rises_over_accepted_steps(seeded, listed):
    _, out, trace = seeded
    _, notes, lo, lt = listed
    rejected = 0
    for o, tr in ((out, trace), (lo, lt)):
        for p in range(len(o.tries)):
            rows = tr[p, :o.tries[p]]
            acc = rows[rows[:, 1] == 1, 0]
            chain = np.concatenate([[o.cost[p, 0]], acc])
            assert (np.diff(chain) < 0).all(), p                                   # every accepted cost is below the one before it
            if o.status[p] != R.NOT_REFINED:
                assert o.cost[p, 1] == chain[-1] and o.cost[p, 1] <= o.cost[p, 0], p   # and the last one is what is reported
            lam = rows[:, 2]
            assert (lam >= 1e-12).all() and (lam <= 1e12).all()
            rejected += int((rows[:, 1] == 0).sum())
    far = [p for p, n in enumerate(notes) if n == "far start"]
    assert len(far) == 2 and min(int((lt[p, :lo.tries[p], 1] == 0).sum()) for p in far) >= 5    # the far starts reject tries
    assert rejected >= 10


def test_at_most_two_percent_of_the_seeded_tracks_reach_the_cap(seeded):
    cases, out, _ = seeded
    cap = int((out.status == R.CAP).sum())
    print(f"{cap} of {len(cases)} tracks at the cap of {RC.MAX_TRIES}; most tries {int(out.tries.max())}, mean {out.tries.mean():.2f}")
    assert len(cases) >= 200 and (out.status != R.NOT_REFINED).all()
    assert cap <= 0.02 * len(cases)


def test_not_refined_tracks_copy_through_and_leave_their_neighbours_alone(listed):
    c, notes, out, trace = listed
    ptr, use = c["track_ptr"], c["use_mask"]
    by = {n: p for p, n in enumerate(notes)}
    for note in ("all 0", "all 1", "one of 9", "one of 17", "one of 65", "no point", "behind", "nan used"):
        p = by[note]
        assert out.status[p] == R.NOT_REFINED and out.tries[p] == 0, note
        want = c["points"][p] if c["has_point"][p] else np.zeros(3)
        assert np.array_equal(out.refined[p].view(np.uint64), want.view(np.uint64)), note
        assert np.array_equal(out.cost[p, :1].view(np.uint64), out.cost[p, 1:].view(np.uint64)), note
    for note in ("one of 9", "no point", "behind", "nan used"):
        assert 0 < by[note] < len(notes) - 1                                       # in the middle of the list
    p = by["no point"]
    assert out.cost[p].tolist() == [0, 0] and not out.masks[ptr[p]:ptr[p + 1]].any() and out.n_inliers[p] == 0
    assert out.cost[by["all 0"]].tolist() == [0, 0] and out.cost[by["all 1"], 0] > 0 and out.cost[by["behind"], 0] > 0
    assert out.cost[by["nan used"]].view(np.uint64).tolist() == [0x7ff8000000000000] * 2
    assert out.status[by["nan unused"]] == R.CONVERGED and out.status[by["two of 65"]] == R.CONVERGED
    assert out.status[by["no parallax"]] != R.NOT_REFINED and out.tries[by["no parallax"]] >= 1
    # a track alone gives what it gives in the list: the neighbours of the not-refined ones included
    for p in (by["no point"] - 1, by["no point"], by["behind"], by["nan used"], by["nan used"] + 1, by["no parallax"], len(notes) - 1):
        one = R.refine_tracks(*RC.args(RC.sublist(c, [p])), RC.MAX_TRIES, RC.THR)
        assert np.array_equal(one.refined[0].view(np.uint64), out.refined[p].view(np.uint64)), p
        assert np.array_equal(one.cost[0].view(np.uint64), out.cost[p].view(np.uint64)) and one.tries[0] == out.tries[p], p
        assert np.array_equal(one.masks, out.masks[ptr[p]:ptr[p + 1]]) and one.n_inliers[0] == out.n_inliers[p], p
    # what the list of the GPU test is meant to cover
    assert len(notes) == 70
    lengths = np.diff(ptr)
    used = np.array([int(use[ptr[p]:ptr[p + 1]].sum()) for p in range(len(notes))])
    for m in RC.LENGTHS:
        assert ((lengths == m) & (used == m)).any(), m
    for m in RC.LENGTHS[3:]:
        assert ((lengths == m) & (used == (m + 1) // 2)).any(), m
    assert ((used == 2) & (lengths > 2)).sum() >= 3 and ((used == 1) & (lengths > 1)).sum() >= 3
    wave = range(RC.WAVE_AT, RC.WAVE_AT + 8)                                        # rejected tries beside tracks done after one try
    assert RC.WAVE_AT % 8 == 0 and sorted(notes[p] for p in wave) == ["far start"] * 2 + ["one try"] * 6
    assert all(out.tries[p] == 1 and out.status[p] == R.CONVERGED for p in wave if notes[p] == "one try")
    assert all(out.tries[p] >= 10 for p in wave if notes[p] == "far start")
    live = out.status != R.NOT_REFINED
    busy = live & (out.tries > 1)
    one_try = R.refine_tracks(*RC.args(c), 1, RC.THR)
    three = R.refine_tracks(*RC.args(c), 3, RC.THR)
    assert (one_try.status[busy] == R.CAP).all() and (one_try.tries[live] == 1).all()       # nothing is done after one try
    assert (one_try.status[~live] == R.NOT_REFINED).all() and (three.status[~live] == R.NOT_REFINED).all()
    assert (three.status[live] == R.CAP).sum() >= 20 and (three.cost[live, 1] > out.cost[live, 1]).sum() >= 20   # a cap of 3: in mid-descent


def test_the_case_lists_run_clean_under_the_sanitizers(tmp_path):
    exe = R.build_program(("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))
    c, _ = RC.gpu_list()
    s = RC.pack(RC.seeded())
    runs = {"list": (RC.args(c), 20), "list3": (RC.args(c), 3), "list null mask": (RC.args(c, with_mask=False), 20),
            "seeded": (RC.args(s, with_mask=False), 20)}
    for name, (a, cap) in runs.items():
        path = str(tmp_path / "cases.bin")
        R.write_cases(path, *a, cap, RC.THR)
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, f"{name}: {r.stderr[-2000:]}"
        want = R.refine_tracks(*a, cap, RC.THR)
        lines = [ln.split() for ln in r.stdout.splitlines()]
        assert len(lines) == len(want.status), name
        assert [int(ln[1]) for ln in lines] == want.status.tolist() and [int(ln[2]) for ln in lines] == want.tries.tolist(), name
        assert [int(ln[3]) for ln in lines] == want.n_inliers.tolist(), name
