"""GPU: eacham_pnp_refine_batch (eacham_amd/csrc/pnp_refine.hip) against the CPU restatement (tests/cpp/pnp_refine_reference.c through
tests/pnp_refine_reference.py), EVERY output compared as bytes, on the list of tests/pnp_refine_cases.py: gpu_list — used-row counts
on either side of the kernel's 64-row trip under every kind of mask, empty and not-refined problems in the middle, far starts whose
tries are rejected, a planar scene — at the default cap and at caps of 1 and 3 (hit in mid-descent); the list against its problems
one at a time; a NULL mask against all ones; the recount against eacham_pnp_refit_batch; the error returns."""
import ctypes as C

import numpy as np
import pytest

from eacham_amd import capi, pnp
import pnp_refine_cases as RC
import pnp_refine_reference as R

pytestmark = pytest.mark.gpu
FIELDS = ("refined", "cost", "tries", "status", "n_inliers")


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def assert_same(got, want, label=""):
    for name in FIELDS:
        a, b = getattr(got, name), getattr(want, name)
        where = np.nonzero((bits(a) != bits(b)).reshape(len(b), -1).any(1))[0]
        assert len(where) == 0, f"{label}: {name} differs at problems {where.tolist()[:8]}: {a[where[:2]]} != {b[where[:2]]}"
    for p, (a, b) in enumerate(zip(got.masks, want.masks)):
        assert np.array_equal(a, b), f"{label}: mask of problem {p} differs"


@pytest.fixture(scope="module")
def case():
    X, uv, T0, has, use, notes = RC.gpu_list()
    ref = {t: R.refine_batch(X, uv, RC.K, T0, has, use, t, RC.THR) for t in (RC.MAX_TRIES, 1, 3)}
    return dict(X=X, uv=uv, T0=T0, has=has, use=use, notes=notes, ref=ref)   # (tests/test_pnp_refine_reference.py says what the list covers)


@pytest.mark.parametrize("max_tries", [RC.MAX_TRIES, 1, 3])
def test_every_output_equals_the_restatement(hip_ctx, case, max_tries):
    want = case["ref"][max_tries]
    got = hip_ctx.pnp_refine_batch(case["X"], case["uv"], RC.K, case["T0"], case["has"], case["use"], max_tries, RC.THR)
    assert_same(got, want, f"cap {max_tries}")
    again = hip_ctx.pnp_refine_batch(case["X"], case["uv"], RC.K, case["T0"], case["has"], case["use"], max_tries, RC.THR)
    assert_same(again, got, "second call")


@pytest.mark.parametrize("rows", [[5], [19, 20], [12, 3, 30, 31]])
def test_short_lists(hip_ctx, case, rows):
    """Lists of 1, 2 and 4 problems (the last one workgroup exactly), in another order than the long list has them."""
    pick = lambda xs: [xs[p] for p in rows]   # noqa: E731
    got = hip_ctx.pnp_refine_batch(pick(case["X"]), pick(case["uv"]), RC.K, case["T0"][rows], case["has"][rows], pick(case["use"]), RC.MAX_TRIES, RC.THR)
    want = R.refine_batch(pick(case["X"]), pick(case["uv"]), RC.K, case["T0"][rows], case["has"][rows], pick(case["use"]), RC.MAX_TRIES, RC.THR)
    assert_same(got, want, f"rows {rows}")
    whole = case["ref"][RC.MAX_TRIES]
    for k, p in enumerate(rows):
        assert np.array_equal(bits(got.refined[k]), bits(whole.refined[p])) and np.array_equal(bits(got.cost[k]), bits(whole.cost[p]))


def test_the_list_equals_its_problems_one_at_a_time(hip_ctx, case):
    whole = hip_ctx.pnp_refine_batch(case["X"], case["uv"], RC.K, case["T0"], case["has"], case["use"], RC.MAX_TRIES, RC.THR)
    for p in range(len(case["X"])):
        one = hip_ctx.pnp_refine_batch([case["X"][p]], [case["uv"][p]], RC.K, case["T0"][p:p + 1], case["has"][p:p + 1], [case["use"][p]],
                                       RC.MAX_TRIES, RC.THR)
        for name in FIELDS:
            assert np.array_equal(bits(getattr(one, name)[0]), bits(getattr(whole, name)[p])), (p, case["notes"][p], name)
        assert np.array_equal(one.masks[0], whole.masks[p]), p


def test_a_null_mask_equals_all_ones_and_the_recount_is_optional(hip_ctx, case):
    rows = [p for p, m in enumerate(case["use"]) if m.all()]
    assert len(rows) >= 12
    pick = lambda xs: [xs[p] for p in rows]   # noqa: E731
    args = (pick(case["X"]), pick(case["uv"]), RC.K, case["T0"][rows], case["has"][rows])
    ones = hip_ctx.pnp_refine_batch(*args, pick(case["use"]), RC.MAX_TRIES, RC.THR)
    null = hip_ctx.pnp_refine_batch(*args, None, RC.MAX_TRIES, RC.THR)
    assert_same(null, ones, "NULL mask")
    assert_same(null, R.refine_batch(*args, None, RC.MAX_TRIES, RC.THR), "NULL mask, restatement")
    lean = hip_ctx.pnp_refine_batch(*args, None, RC.MAX_TRIES, RC.THR, want_recount=False)
    assert lean.masks is None and lean.n_inliers is None
    for name in FIELDS[:4]:
        assert np.array_equal(bits(getattr(lean, name)), bits(getattr(ones, name))), name
    # one of the two optional outputs alone
    pp, A, B = pnp.pack_points(args[0], args[1])
    P = len(rows)
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731
    for want_mask in (True, False):
        ref_, cost, tries, status = np.zeros((P, 12)), np.zeros((P, 2)), np.zeros(P, np.int32), np.zeros(P, np.int32)
        mask, ni = np.zeros(len(B), np.uint8), np.zeros(P, np.int32)
        poses, has = np.ascontiguousarray(case["T0"][rows]), np.ascontiguousarray(case["has"][rows])
        hip_ctx._check(capi.lib().eacham_pnp_refine_batch(hip_ctx.handle, P, vp(pp), vp(A), vp(B), vp(RC.K), vp(poses), vp(has), None, RC.MAX_TRIES, RC.THR,
                                                          vp(ref_), vp(cost), vp(tries), vp(status), vp(mask) if want_mask else None,
                                                          None if want_mask else vp(ni)))
        assert np.array_equal(bits(ref_), bits(ones.refined))
        if want_mask:
            assert np.array_equal(mask, np.concatenate(ones.masks)) and not ni.any()
        else:
            assert np.array_equal(ni, ones.n_inliers) and not mask.any()


def test_the_recount_is_the_refit_entry_s_mask_and_count(hip_ctx, case):
    got = hip_ctx.pnp_refine_batch(case["X"], case["uv"], RC.K, case["T0"], case["has"], case["use"], RC.MAX_TRIES, RC.THR)
    refit = hip_ctx.pnp_refit_batch(case["X"], case["uv"], RC.K, got.refined, case["has"], RC.THR)
    assert np.array_equal(refit.n_inliers, got.n_inliers)
    for p, (a, b) in enumerate(zip(refit.masks, got.masks)):
        assert np.array_equal(a, b), p
    assert got.n_inliers.sum() > 2000


SENTINEL_F, SENTINEL_I = -7.25, -77


def test_error_returns_leave_the_outputs_untouched(hip_ctx, case):
    pp, X, uv = pnp.pack_points(case["X"], case["uv"])
    P, NP = len(pp) - 1, len(uv)
    poses, has, use = np.ascontiguousarray(case["T0"]), np.ascontiguousarray(case["has"]), np.concatenate(case["use"])
    L = capi.lib()
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731

    def changed(t, k, v):
        t = t.copy()
        t[k] = v
        return t

    def call(code, *words, n_problems=P, point_ptr=pp, Xa=X, uva=uv, Ka=RC.K, pa=poses, ha=has, max_tries=20, thr=RC.THR, null_out=None,
             recount=True):
        out = dict(refined=np.full((P, 12), SENTINEL_F), cost=np.full((P, 2), SENTINEL_F), tries=np.full(P, SENTINEL_I, np.int32),
                   status=np.full(P, SENTINEL_I, np.int32), mask=np.full(NP, 7, np.uint8), ni=np.full(P, SENTINEL_I, np.int32))
        a = {k: (None if k == null_out or (not recount and k in ("mask", "ni")) else vp(v)) for k, v in out.items()}
        rc = L.eacham_pnp_refine_batch(hip_ctx.handle, n_problems, vp(point_ptr), vp(Xa), vp(uva), vp(Ka), vp(pa), vp(ha), vp(use), max_tries, thr,
                                       a["refined"], a["cost"], a["tries"], a["status"], a["mask"], a["ni"])
        msg = L.eacham_last_error(hip_ctx.handle).decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)
        if code != capi.OK:
            assert (out["refined"] == SENTINEL_F).all() and (out["cost"] == SENTINEL_F).all() and (out["tries"] == SENTINEL_I).all(), msg
            assert (out["status"] == SENTINEL_I).all() and (out["mask"] == 7).all() and (out["ni"] == SENTINEL_I).all(), msg
        return out

    call(capi.ERR_INVALID, "negative", n_problems=-1)
    call(capi.ERR_INVALID, "null", point_ptr=None)
    call(capi.ERR_INVALID, "start at 0", point_ptr=changed(pp, 0, 1))
    call(capi.ERR_INVALID, "problem 1", "decreases", point_ptr=changed(pp, 2, pp[1] - 1))
    call(capi.ERR_CAPACITY, "2^31", point_ptr=changed(pp, len(pp) - 1, 1 << 31))
    for name in ("Xa", "uva", "Ka", "pa", "ha"):
        call(capi.ERR_INVALID, "null array", **{name: None})
    for name in ("refined", "cost", "tries", "status"):
        call(capi.ERR_INVALID, "null array", null_out=name)
    call(capi.ERR_INVALID, "max_tries", max_tries=0)
    call(capi.ERR_INVALID, "max_tries", max_tries=-3)
    call(capi.ERR_INVALID, "threshold", thr=float("nan"))
    call(capi.ERR_INVALID, "threshold", thr=-1.0)
    call(capi.ERR_INVALID, "threshold", thr=-1.0, null_out="mask")                   # the count alone still asks for the recount
    # without the recount the threshold is not looked at; and the context is still usable, same bytes
    out = call(capi.OK, thr=float("nan"), recount=False)
    want = case["ref"][RC.MAX_TRIES]
    assert np.array_equal(bits(out["refined"]), bits(want.refined)) and np.array_equal(bits(out["cost"]), bits(want.cost))
    assert np.array_equal(out["tries"], want.tries) and np.array_equal(out["status"], want.status)
    assert (out["mask"] == 7).all() and (out["ni"] == SENTINEL_I).all()
    r = np.full((1, 12), SENTINEL_F)                                                 # nothing to do: success, nothing written
    assert L.eacham_pnp_refine_batch(hip_ctx.handle, 0, None, None, None, None, None, None, None, 20, RC.THR, vp(r), None, None, None, None, None) == capi.OK
    assert (r == SENTINEL_F).all()
