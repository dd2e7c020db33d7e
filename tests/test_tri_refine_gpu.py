"""GPU: eacham_triangulate_refine_tracks (eacham_amd/csrc/tri_refine.hip) against the CPU restatement (tests/cpp/tri_refine_reference.c
through tests/tri_refine_reference.py), EVERY output compared as bytes, on the list of tests/tri_refine_cases.py: gpu_list — track
lengths on either side of the kernel's 8-lane trip under every kind of mask, not-refined tracks in the middle, far starts whose tries
are rejected in one wave with tracks that are done after one try, a pair with next to no parallax — at the default cap and at caps of
1 and 3 (hit in mid-descent); short lists around the wave and workgroup edges; the list against its tracks one at a time; a NULL mask
against all ones; each optional output alone; the error returns."""
import ctypes as C

import numpy as np
import pytest

from eacham_amd import capi
import tri_refine_cases as RC
import tri_refine_reference as R

pytestmark = pytest.mark.gpu
FIELDS = ("refined", "cost", "tries", "status", "n_inliers", "masks")


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def assert_same(got, want, label=""):
    for name in FIELDS:
        a, b = getattr(got, name), getattr(want, name)
        if name == "masks":
            assert np.array_equal(a, b), f"{label}: masks differ at observations {np.nonzero(a != b)[0].tolist()[:8]}"
            continue
        where = np.nonzero((bits(a) != bits(b)).reshape(len(b), -1).any(1))[0]
        assert len(where) == 0, f"{label}: {name} differs at tracks {where.tolist()[:8]}: {a[where[:2]]} != {b[where[:2]]}"


@pytest.fixture(scope="module")
def case():
    c, notes = RC.gpu_list()
    ref = {t: R.refine_tracks(*RC.args(c), t, RC.THR) for t in (RC.MAX_TRIES, 1, 3)}
    return dict(c=c, notes=notes, ref=ref)   # (tests/test_tri_refine_reference.py says what the list covers)


@pytest.mark.parametrize("max_tries", [RC.MAX_TRIES, 1, 3])
def test_every_output_equals_the_restatement(hip_ctx, case, max_tries):
    want = case["ref"][max_tries]
    got = hip_ctx.refine_tracks(*RC.args(case["c"]), max_tries, RC.THR)
    assert_same(got, want, f"cap {max_tries}")
    again = hip_ctx.refine_tracks(*RC.args(case["c"]), max_tries, RC.THR)
    assert_same(again, got, "second call")


@pytest.mark.parametrize("count", [1, 7, 8, 9, 31, 32, 33])
def test_short_lists(hip_ctx, case, count):
    """Lists around the edges of a wave (8 tracks) and of a workgroup (32), taken from the far end of the long list backwards, so a
    track sits in another lane group, wave and workgroup than it has there."""
    rows = list(range(len(case["notes"]) - 1, -1, -2))[:count] if count < 33 else list(range(40, 8, -1)) + [0]
    assert len(rows) == count
    sub = RC.sublist(case["c"], rows)
    got = hip_ctx.refine_tracks(*RC.args(sub), RC.MAX_TRIES, RC.THR)
    assert_same(got, R.refine_tracks(*RC.args(sub), RC.MAX_TRIES, RC.THR), f"{count} tracks")
    whole = case["ref"][RC.MAX_TRIES]
    for k, p in enumerate(rows):
        assert np.array_equal(bits(got.refined[k]), bits(whole.refined[p])) and np.array_equal(bits(got.cost[k]), bits(whole.cost[p])), p
        assert got.tries[k] == whole.tries[p] and got.status[k] == whole.status[p] and got.n_inliers[k] == whole.n_inliers[p], p


def test_the_list_equals_its_tracks_one_at_a_time(hip_ctx, case):
    c = case["c"]
    whole = hip_ctx.refine_tracks(*RC.args(c), RC.MAX_TRIES, RC.THR)
    ptr = c["track_ptr"]
    for p in range(len(case["notes"])):
        one = hip_ctx.refine_tracks(*RC.args(RC.sublist(c, [p])), RC.MAX_TRIES, RC.THR)
        for name in FIELDS[:5]:
            assert np.array_equal(bits(getattr(one, name)[0]), bits(getattr(whole, name)[p])), (p, case["notes"][p], name)
        assert np.array_equal(one.masks, whole.masks[ptr[p]:ptr[p + 1]]), p


def test_a_null_mask_equals_all_ones_and_the_recount_is_optional(hip_ctx, case):
    c, ptr = case["c"], case["c"]["track_ptr"]
    rows = [p for p in range(len(case["notes"])) if c["use_mask"][ptr[p]:ptr[p + 1]].all()]
    assert len(rows) >= 20
    sub = RC.sublist(c, rows)
    ones = hip_ctx.refine_tracks(*RC.args(sub), RC.MAX_TRIES, RC.THR)
    null = hip_ctx.refine_tracks(*RC.args(sub, with_mask=False), RC.MAX_TRIES, RC.THR)
    assert_same(null, ones, "NULL mask")
    assert_same(null, R.refine_tracks(*RC.args(sub, with_mask=False), RC.MAX_TRIES, RC.THR), "NULL mask, restatement")
    lean = hip_ctx.refine_tracks(*RC.args(sub, with_mask=False), RC.MAX_TRIES, RC.THR, want_recount=False)
    assert lean.masks is None and lean.n_inliers is None
    for name in FIELDS[:4]:
        assert np.array_equal(bits(getattr(lean, name)), bits(getattr(ones, name))), name
    # one of the two optional outputs alone
    P, NO = len(rows), int(sub["track_ptr"][-1])
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731
    T, of, uv = np.ascontiguousarray(sub["transforms"]), np.ascontiguousarray(sub["obs_frame"]), np.ascontiguousarray(sub["obs_uv"])
    pts, has = np.ascontiguousarray(sub["points"]), np.ascontiguousarray(sub["has_point"])
    for want_mask in (True, False):
        ref_, cost, tries, status = np.zeros((P, 3)), np.zeros((P, 2)), np.zeros(P, np.int32), np.zeros(P, np.int32)
        mask, ni = np.zeros(NO, np.uint8), np.zeros(P, np.int32)
        hip_ctx._check(capi.lib().eacham_triangulate_refine_tracks(
            hip_ctx.handle, vp(T), len(T), P, vp(sub["track_ptr"]), vp(of), vp(uv), vp(RC.K), vp(pts), vp(has), None, RC.MAX_TRIES, RC.THR,
            vp(ref_), vp(cost), vp(tries), vp(status), vp(mask) if want_mask else None, None if want_mask else vp(ni)))
        assert np.array_equal(bits(ref_), bits(ones.refined)) and np.array_equal(bits(cost), bits(ones.cost))
        if want_mask:
            assert np.array_equal(mask, ones.masks) and not ni.any()
        else:
            assert np.array_equal(ni, ones.n_inliers) and not mask.any()
    assert ones.n_inliers.sum() > 300


SENTINEL_F, SENTINEL_I = -7.25, -77


def test_error_returns_leave_the_outputs_untouched(hip_ctx, case):
    c = case["c"]
    tp, T, of, uv = c["track_ptr"], np.ascontiguousarray(c["transforms"]), np.ascontiguousarray(c["obs_frame"]), np.ascontiguousarray(c["obs_uv"])
    pts, has, use = np.ascontiguousarray(c["points"]), np.ascontiguousarray(c["has_point"]), np.ascontiguousarray(c["use_mask"])
    P, NO, F = len(tp) - 1, len(of), len(T)
    L = capi.lib()
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731

    def changed(t, k, v):
        t = t.copy()
        t[k] = v
        return t

    def call(code, *words, n_tracks=P, n_frames=F, ptr=tp, Ta=T, ofa=of, uva=uv, Ka=RC.K, pa=pts, ha=has, max_tries=20, thr=RC.THR,
             null_out=None, recount=True):
        out = dict(refined=np.full((P, 3), SENTINEL_F), cost=np.full((P, 2), SENTINEL_F), tries=np.full(P, SENTINEL_I, np.int32),
                   status=np.full(P, SENTINEL_I, np.int32), mask=np.full(NO, 7, np.uint8), ni=np.full(P, SENTINEL_I, np.int32))
        a = {k: (None if k == null_out or (not recount and k in ("mask", "ni")) else vp(v)) for k, v in out.items()}
        rc = L.eacham_triangulate_refine_tracks(hip_ctx.handle, vp(Ta), n_frames, n_tracks, vp(ptr), vp(ofa), vp(uva), vp(Ka), vp(pa), vp(ha), vp(use),
                                                max_tries, thr, a["refined"], a["cost"], a["tries"], a["status"], a["mask"], a["ni"])
        msg = L.eacham_last_error(hip_ctx.handle).decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)
        if code != capi.OK:
            assert (out["refined"] == SENTINEL_F).all() and (out["cost"] == SENTINEL_F).all() and (out["tries"] == SENTINEL_I).all(), msg
            assert (out["status"] == SENTINEL_I).all() and (out["mask"] == 7).all() and (out["ni"] == SENTINEL_I).all(), msg
        return out

    call(capi.ERR_INVALID, "negative", n_tracks=-1)
    call(capi.ERR_INVALID, "negative", n_frames=-1)
    call(capi.ERR_INVALID, "null", ptr=None)
    call(capi.ERR_INVALID, "start at 0", ptr=changed(tp, 0, 1))
    call(capi.ERR_INVALID, "track 2", "decreases", ptr=changed(tp, 3, tp[2] - 1))
    call(capi.ERR_CAPACITY, "2^31", ptr=changed(tp, len(tp) - 1, 1 << 31))
    for name in ("Ta", "ofa", "uva", "Ka", "pa", "ha"):
        call(capi.ERR_INVALID, "null array", **{name: None})
    for name in ("refined", "cost", "tries", "status"):
        call(capi.ERR_INVALID, "null array", null_out=name)
    call(capi.ERR_INVALID, "max_tries", max_tries=0)
    call(capi.ERR_INVALID, "max_tries", max_tries=-3)
    call(capi.ERR_INVALID, "max_repr_error", thr=float("nan"))
    call(capi.ERR_INVALID, "max_repr_error", thr=-1.0)
    call(capi.ERR_INVALID, "max_repr_error", thr=-1.0, null_out="mask")          # the count alone still asks for the recount
    # an observation that names a frame that is not there: the message names its track
    k = int(tp[5]) + 2
    call(capi.ERR_INVALID, "track 5", "observation 2", f"frame {F}", ofa=changed(of, k, F))
    call(capi.ERR_INVALID, "track 5", ofa=changed(of, k, 0xFFFFFFFF))
    call(capi.ERR_INVALID, "track 1", "observation 0", n_frames=0)                 # (track 0 holds no observation)
    # without the recount the threshold is not looked at; and the context is still usable, same bytes
    out = call(capi.OK, thr=float("nan"), recount=False)
    want = case["ref"][RC.MAX_TRIES]
    assert np.array_equal(bits(out["refined"]), bits(want.refined)) and np.array_equal(bits(out["cost"]), bits(want.cost))
    assert np.array_equal(out["tries"], want.tries) and np.array_equal(out["status"], want.status)
    assert (out["mask"] == 7).all() and (out["ni"] == SENTINEL_I).all()
    r = np.full((1, 3), SENTINEL_F)                                              # nothing to do: success, nothing written
    assert L.eacham_triangulate_refine_tracks(hip_ctx.handle, None, 0, 0, None, None, None, None, None, None, None, 20, RC.THR, vp(r), None, None,
                                              None, None, None) == capi.OK
    assert (r == SENTINEL_F).all()
