"""CPU: what the scenes of the screened dot-product matcher prove (tests/dot_screen_cases.py), with numpy's float16 and the CPU
reference of the exact matcher (tests/dot_reference.py): the input-rounding part of the bound holds on every scene, and every
scene reaches the branch it is named for."""
import numpy as np
import pytest

from eacham_amd import synth
import dot_cases as DC
import dot_reference as R
import dot_screen_cases as SC

NEG_INF = float("-inf")


@pytest.fixture(scope="module")
def scenes():
    return SC.scenes()


def _screened_pairs(descs, pairs):
    return [(int(a), int(b)) for a, b in pairs if SC.screenable(descs[a]) and SC.screenable(descs[b])]


def test_input_rounding_part_of_the_bound_on_every_scene(scenes):
    """|S~ - S| <= (2^-10 + 2^-22) N'_a N'_b <= E, S~ and S the real dot products of the images and of the rows (float64 here: its
    own error, 2^-53 D per unit of |a||b|, is 2^-30 of the bound). Unique pairs i < j: (j, i) is the transpose."""
    seen = 0
    for name, (descs, pairs) in scenes.items():
        worst = 0.0
        for a, b in _screened_pairs(descs, pairs):
            if a > b or not descs[a].size or not descs[b].size:
                continue
            ia, na, _ = SC.image16(descs[a])
            ib, nb, _ = SC.image16(descs[b])
            S = descs[a].astype(np.float64) @ descs[b].astype(np.float64).T
            err = np.abs(ia @ ib.T - S)
            bound = (2.0 ** -10 + 2.0 ** -22) * na[:, None] * nb[None, :]
            assert (err <= bound).all(), (name, a, b)
            _, row_E, col_E = SC.coarse(descs[a], descs[b])
            assert (bound <= row_E[:, None] * (1 + 1e-12)).all() and (bound <= col_E[None, :] * (1 + 1e-12)).all()
            worst = max(worst, float((err / np.minimum(row_E[:, None], col_E[None, :])).max()))
            seen += 1
        print(f"{name}: input rounding / E <= {worst:.3f}")
        if name.startswith("a_"):
            assert 0.03 < worst < 0.30          # Cauchy-Schwarz is loose by a factor 5 to 15 on unit-norm rows
    assert seen >= 30


@pytest.mark.parametrize("name", sorted(DC.SCENES))
def test_the_four_scenes_are_decided_at_the_threshold_and_leave_a_few_rows_open_without_one(scenes, name):
    descs, pairs = scenes["a_" + name]
    tot = {DC.MIN_SCORE: np.zeros(3, int), NEG_INF: np.zeros(3, int)}
    wrong = 0
    for a, b in pairs:
        S, row_E, _ = SC.coarse(descs[a], descs[b])
        for ms in tot:
            st, best = SC.classify(S, row_E, ms)
            tot[ms] += np.bincount(st, minlength=3)
        true_best, _ = R.argmax(descs[a], descs[b])
        st, best = SC.classify(S, row_E, NEG_INF)
        assert (best[st == 1] == true_best[st == 1]).all()          # a settled row's coarse arg-max IS the arg-max
        wrong += int((best != true_best).sum())
    rows = int(tot[NEG_INF].sum())
    assert tot[DC.MIN_SCORE][2] == 0 and tot[DC.MIN_SCORE][0] > 0 and tot[DC.MIN_SCORE][1] > 0      # dead or settled, none open
    # the model is deterministic: a change to the image, the norm bound or kappa moves these counts (2.2 - 4.9 % of the rows)
    assert tot[NEG_INF][0] == 0 and int(tot[NEG_INF][2]) == {"d64": 52, "d100": 70, "d128": 86, "d256": 40}[name]
    print(f"{name}: open rows without a threshold {tot[NEG_INF][2]} of {rows}; coarse arg-max wrong for {wrong}")


def test_near_duplicates_need_the_exact_pass(scenes):
    A, B, (hi, lo, tie) = SC.near_duplicates()
    n0 = B.shape[0] - 3
    true_best, _ = R.argmax(A, B)
    S, row_E, _ = SC.coarse(A, B)
    st, best = SC.classify(S, row_E, NEG_INF)
    for k, q in enumerate((hi, lo, tie)):
        copy, orig = n0 + k, int(best[q])
        assert S[q, copy] == S[q, orig] and orig < n0 and st[q] == 2          # the two tie in fp16: the row is open
        assert np.array_equal(np.float16(B[copy]), np.float16(B[orig]))
        diff = int((B[copy] != B[orig]).sum())
        assert diff == (0 if q == tie else 1)
        if diff:
            k0 = int(np.flatnonzero(B[copy] != B[orig])[0])
            assert abs(int(B[copy, k0:k0 + 1].view(np.int32)[0]) - int(B[orig, k0:k0 + 1].view(np.int32)[0])) == 1   # one fp32 ulp
    assert true_best[hi] == n0 and best[hi] != true_best[hi]                  # fp32 picks the HIGHER index; fp16's arg-max is wrong
    assert true_best[lo] == best[lo] < n0 and true_best[tie] == best[tie] < n0
    # and the matches survive the threshold, so the difference reaches the output
    q, t, s, _ = R.match_mutual(A, B, DC.MIN_SCORE, 0, -1)
    assert t[q == hi].tolist() == [n0]


def test_fallback_scene_reaches_the_fallback(scenes):
    descs, pairs = scenes["c_fallback"]
    flags = [SC.screenable(d) for d in descs]
    assert flags == [True, False, False, True]
    assert np.isinf(descs[1]).any() and (np.abs(descs[1][np.isfinite(descs[1])]) > 65504).any() and np.isnan(descs[2]).any()
    assert len(_screened_pairs(descs, pairs)) == 2


def test_tiny_value_scene_has_flushed_elements_and_a_flushed_row(scenes):
    descs, _ = scenes["d_tiny_values"]
    for f, X in enumerate(descs):
        img, n, flushed = SC.image16(X)
        assert flushed.sum() >= 3 and (img[np.abs(X) < 2.0 ** -14] == 0).all()
        assert (img[np.abs(X) == 2.0 ** -14] == 2.0 ** -14).all() and (np.abs(X) == 2.0 ** -14).any()
        assert (n >= np.linalg.norm(X.astype(np.float64), axis=1)).all()
    img, n, flushed = SC.image16(descs[0])
    assert (img[30] == 0).all() and flushed[30] == 64 and n[30] >= 1.0          # the whole row is flushed: N' carries the absolute term


def test_negative_pair_and_tiny_shapes(scenes):
    (a, b), _ = scenes["e_negative"]
    S, row_E, _ = SC.coarse(a, b)
    assert S.max() < 0 and a.shape[0] == 70
    st, _ = SC.classify(S, row_E, -2.0)
    assert (st > 0).all()                                                       # nothing is dead below every similarity
    descs, pairs = scenes["f_tiny_shapes"]
    assert [d.shape[0] for d in descs] == [33, 70, 1, 2, 0]
    S, row_E, _ = SC.coarse(descs[0], descs[2])
    assert (SC.classify(S, row_E, NEG_INF)[0] == 2).all()                       # a train frame of one row: no second value, open
    S, row_E, _ = SC.coarse(descs[0], descs[4])
    assert (SC.classify(S, row_E, NEG_INF)[0] == 0).all()                       # no train row: dead
