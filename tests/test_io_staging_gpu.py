"""GPU: the copy rules of the staging helper under the host-pointer entry points (IoStage, eacham_amd/csrc/context.hpp), driven
through entry points that are already held to the oracles. eacham_score_hypotheses with 3 homography models and the errors asked
for stands for all of them: at 16 384 points a point array is exactly PACK_MAX = 262 144 bytes and still travels in the packed
span; at 16 385 it is copied on its own while the models and the counts stay packed around it (a packed span must not cover a
directly copied array); a large call between two small ones grows the staging buffer and its pinned mirror. Null inputs and null
results, a refused call before a good one, and eacham_two_view_points (which shares the path) at 0 and 1 matches. Every comparison
is exact, except two_view_points against the oracle, which keeps the rtol 1e-9 of tests/test_tri_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from eacham_amd import capi, lmeds, score, triangulate as tri, EachamError
import lmeds_batch_cases as LC
import oracle_api as O
import score_cases as SC
import test_lmeds_batch_reference as REF
import test_two_view_batch_gpu as TVB
import two_view_batch_cases as TC

pytestmark = pytest.mark.gpu

PACK_MAX = 256 * 1024
THR = 16.0


def _same(got, want):
    assert got[0].shape == want[0].shape
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))


@pytest.fixture(scope="module")
def cases():
    """n -> (uv1, uv2, 3 homographies, the oracle's (errors, counts, medians)); computed once, never changed"""
    out = {}
    for n in (8, 16384, 16385):
        c = SC.two_view_case(n=n, n_models=3, planar=True, seed=13)
        out[n] = (c["uv1"], c["uv2"], c["H"], O.score_hypotheses("homography", c["uv1"], c["uv2"], c["H"], None, THR))
    return out


def _score(ctx, case):
    return score.score_hypotheses(ctx, "homography", case[0], case[1], case[2], None, THR)


@pytest.mark.parametrize("n", [16384, 16385])
def test_point_arrays_at_and_above_pack_max(hip_ctx, cases, n):
    assert (cases[n][0].nbytes <= PACK_MAX) == (n == 16384) and cases[n][0].nbytes == 16 * n
    _same(_score(hip_ctx, cases[n]), cases[n][3])


def test_small_large_small_on_one_context(hip_ctx, cases):
    first = _score(hip_ctx, cases[8])
    _same(_score(hip_ctx, cases[16385]), cases[16385][3])
    third = _score(hip_ctx, cases[8])
    _same(first, cases[8][3])
    for a, b in zip(first, third):
        assert a.tobytes() == b.tobytes()


def test_null_input_and_null_results(hip_ctx):
    c = SC.two_view_case(n=63)
    K = c["K"]
    x = np.stack([(c["uv1"][:, 0] - K[2]) / K[0], (c["uv1"][:, 1] - K[3]) / K[1]], 1)
    y = np.stack([(c["uv2"][:, 0] - K[2]) / K[0], (c["uv2"][:, 1] - K[3]) / K[1]], 1)
    thr = (1.5 / K[0]) ** 2
    _same(score.score_hypotheses(hip_ctx, "essential", x, y, c["E"], None, thr), O.score_hypotheses("essential", x, y, c["E"], None, thr))
    # every result of eacham_lmeds_batch but the medians left out
    case = LC.CASES["single"]("homography")
    pp, a, b, sp, idx = lmeds.pack("homography", case["uv1"], case["uv2"], case["samples"])
    med = np.zeros(1, np.float32)
    vp = C.c_void_p
    hip_ctx._check(capi.lib().eacham_lmeds_batch(hip_ctx.handle, capi.SOLVE_HOMOGRAPHY4, 1, vp(pp.ctypes.data), vp(a.ctypes.data), vp(b.ctypes.data),
                                                 None, vp(sp.ctypes.data), vp(idx.ctypes.data), None, vp(med.ctypes.data), None, None, None, None, None))
    full = hip_ctx.lmeds_batch(case["kind"], case["uv1"], case["uv2"], case["samples"], case["K"])
    assert REF.bits(med[0], np.float32) == REF.bits(full.medians[0], np.float32)


def test_a_refused_call_then_a_good_one(hip_ctx, cases):
    c = SC.pnp_case(n=50, n_models=3)
    with pytest.raises(EachamError) as e:
        score.score_hypotheses(hip_ctx, "pnp", c["X"], c["uv"], c["models"], None, THR)    # PnP needs K
    assert e.value.code == capi.ERR_INVALID
    _same(_score(hip_ctx, cases[8]), cases[8][3])


def test_two_view_points_with_no_match_and_with_one(hip_ctx):
    uv1, uv2, T = TC.problem(1, 4, 11)
    pts, keep, counts = tri.two_view_points(hip_ctx, uv1[:0], uv2[:0], TC.K, T, TC.MAX_ERR, TC.MIN_ANGLE, True)
    assert pts.shape == (4, 0, 3) and keep.shape == (4, 0) and counts.tolist() == [0, 0, 0, 0]
    for strict in (True, False):
        pts, keep, counts = tri.two_view_points(hip_ctx, uv1, uv2, TC.K, T, TC.MAX_ERR, TC.MIN_ANGLE, strict)
        opts, okeep, ocounts = O.two_view_points(uv1, uv2, TC.K, T, TC.MAX_ERR, TC.MIN_ANGLE, strict)
        assert np.array_equal(keep, okeep) and np.array_equal(counts, ocounts)
        fin = np.isfinite(opts).all(2)
        assert np.allclose(pts[fin], opts[fin], rtol=1e-9, atol=1e-11)
    for rule in ("poses", "solutions"):                      # the same single problem through eacham_two_view_batch: every byte
        case = TC._case([(uv1, uv2, T)], [rule])
        TVB.assert_same(TVB.run(hip_ctx, case), TVB.device_compose(hip_ctx, case), rule)
