"""GPU: the screen form of the row sweep above 128-D (match_screen_kernel, eacham_amd/csrc/matcher.hip). The rows are swept on the
FP6 (e2m3) image of the frames; a rigorous bound (eacham_amd/csrc/match_screen.hpp) finishes the rows that cannot pass the ratio
test, every other row gets exact numbers from the int8 pass. Held here: the matcher's output stays the oracle's bit for bit at
129 / 160 / 255 / 256-D; the default context at 256-D returns the bytes of the exact sweep; the sweep's quantised minimum equals the
numpy integer min_j |M_a - M_b_j|^2 (the operand layout and the exactness of the accumulation); its bounds enclose the true
minimum and runner-up; and the screen leaves open every passing row and at most the passing rows + 5 % of the real rows."""
import os

import numpy as np
import pytest

from eacham_amd import synth
import oracle_api as O

pytestmark = pytest.mark.gpu
ENV = "EACHAM_MATCH_SWEEP_FORM"


def _ctx(form=None):
    """A context of its own created under EACHAM_MATCH_SWEEP_FORM=form (read once, at eacham_ctx_create); None: the default."""
    from eacham_amd import HipContext
    old = os.environ.get(ENV)
    try:
        if form is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = form
        return HipContext(0)
    finally:
        if old is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = old


def _upload(ctx, descs):
    ctx.clear_descriptors()
    for f, d in enumerate(descs):
        ctx.upload_descriptors(f, d)


def _with_norm_parity(D, parity):
    """Forces the parity of every row's centred squared norm (the parity of its count of odd values): 0 / 1 per row, None leaves it."""
    D = D.copy()
    odd = (D.astype(np.int64) % 2).sum(1) % 2
    for r in range(D.shape[0]):
        if parity[r] is not None and odd[r] != parity[r]:
            D[r, 0] += 1 if D[r, 0] < 255 else -1
    return D


def _frame_set(dim):
    """The frames of test_both_forms_of_the_row_sweep_at_every_dimension (tests/test_match_gpu.py) at `dim`: ragged tile counts with
    every position of the parity boundary, the two-row train frames (a pair that passes, a duplicate), and the row whose runner-up
    sits in the minimum's own subset."""
    sizes = [1, 2, 33, 64, 97, 160, 257, 350, 480]
    base = synth.random_u8_descriptors(max(sizes) + 8, dim, 321, 0)
    descs = []
    for k, n in enumerate(sizes):
        D = np.clip(base[:n] + np.rint(6 * synth.rng_normal(321, 20 + k, (n, dim))), 0, 255).astype(np.float32)
        mode = k % 4
        par = [None] * n if mode == 0 else [0] * n if mode == 1 else [1] * n if mode == 2 else [0] * (n - 1) + [1]
        descs.append(_with_norm_parity(D, par))
    near = np.clip(base[5:6] + np.rint(2 * synth.rng_normal(321, 90, (1, dim))), 0, 255).astype(np.float32)
    far = np.clip(255 - base[5:6], 0, 255).astype(np.float32)
    descs.append(_with_norm_parity(np.vstack([near, far]), [0, 0]))
    descs.append(_with_norm_parity(np.vstack([near, near.copy()]), [0, 0]))
    D = descs[4].copy()
    D[1] = np.clip(D[0] + np.rint(1.5 * synth.rng_normal(321, 91, (dim,))), 0, 255)
    descs.append(D)
    return descs


# ---- the numpy model of the grid (match_screen.hpp restated) ----
def _grid_m():
    """M of every value 0..255: the nearest of 64 + 4 M over M in +-{0..15, 16..30 step 2, 32..60 step 4}, the smaller magnitude on a tie."""
    mags = np.array(list(range(16)) + list(range(16, 32, 2)) + list(range(32, 64, 4)))
    ms = np.unique(np.concatenate([mags, -mags]))
    ms = ms[np.argsort(np.abs(ms), kind="stable")]              # ties: the first of the smallest distances = the smaller magnitude
    x = np.arange(256)[:, None]
    return ms[np.argmin(np.abs(x - (64 + 4 * ms[None, :])), axis=1)].astype(np.int64)


_M = _grid_m()


def _codes(D):
    return _M[D.astype(np.int64)]


def _sq_dists(X, Y):
    X, Y = X.astype(np.int64), Y.astype(np.int64)
    return (X * X).sum(1)[:, None] + (Y * Y).sum(1)[None, :] - 2 * (X @ Y.T)


def _ratio_pass(d1, d2, ratio=0.8):
    """FeatureMatcherFlann.cpp:23 as the library restates it: fp32 square roots, fp32 quotient, compared as double."""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.sqrt(d1.astype(np.float32)) / np.sqrt(d2.astype(np.float32))
    return q.astype(np.float64) < ratio


def _top2(D2):
    s = np.sort(D2, axis=1)
    return s[:, 0], s[:, 1]


@pytest.mark.parametrize("dim", [129, 160, 255, 256])
def test_screen_form_matches_the_oracle_bit_for_bit(dim):
    ctx = _ctx("screen")
    try:
        descs = _frame_set(dim)
        _upload(ctx, descs)
        nf = len(descs)
        pairs = np.array([[a, b] for a in range(nf) for b in range(nf) if a != b], dtype=np.int32)
        for md, mm in ((1, 0), (2, 1), (30, 30)):
            got = ctx.match_all_pairs(pairs, min_dir=md, min_mutual=mm)
            want = O.match_all_pairs(descs, pairs, min_dir=md, min_mutual=mm)
            for name, g, w in zip(["counts", "offsets", "q", "t", "stats"], got[:5], want[:5]):
                assert np.array_equal(g, w), f"{name} differs"
            lean = ctx.match_all_pairs(pairs, min_dir=md, min_mutual=mm, stats=False)     # the screen sweep itself
            for name, g, w in zip(["counts", "offsets", "q", "t"], lean[:4], want[:4]):
                assert np.array_equal(g, w), f"{name} differs"
            rows, left_open = ctx.match_screen()
            assert rows == sum(descs[a].shape[0] for a, _ in pairs) and 0 < left_open < rows   # the screen ran, and closed rows
        assert got[0].sum() > 0
        for a, b, ratio in ((0, 9, 0.8), (4, 9, 0.8), (5, 10, 0.8), (11, 4, 0.8), (4, 11, 0.8), (9, 3, 0.8), (5, 10, 1.5), (4, 11, 1.2), (7, 6, 1.5)):
            q, t = ctx.match_pair(a, b, ratio)
            wq, wt = O.match_directed(descs[a], descs[b], ratio)
            assert np.array_equal(q, wq) and np.array_equal(t, wt), (a, b, ratio)
    finally:
        ctx.close()


def test_default_at_256d_returns_the_bytes_of_the_exact_sweep():
    descs = _frame_set(256)
    nf = len(descs)
    pairs = np.array([[a, b] for a in range(nf) for b in range(nf) if a != b], dtype=np.int32)
    out = {}
    for form in (None, "exact"):
        ctx = _ctx(form)
        try:
            _upload(ctx, descs)
            out[form] = ctx.match_all_pairs(pairs, min_dir=2, min_mutual=1, stats=False)
            out[form, "tally"] = ctx.match_screen()
        finally:
            ctx.close()
    for g, w in zip(out[None][:4], out["exact"][:4]):
        assert g.tobytes() == w.tobytes()
    assert out[None][0].sum() > 0
    assert out[None, "tally"][0] > 0 and out["exact", "tally"] == (0, 0)   # the default above 128-D is the screen form


@pytest.fixture(scope="module")
def swept():
    """The sweep's own numbers (the debug entry, before any exact pass) on ordered pairs of the frame set at every dimension, with
    the numpy references: [(dim, a, b, train rows, n1, L1, U2, quantised minimum, true v1, true v2)]."""
    ctx = _ctx("screen")
    res = []
    try:
        for dim in (129, 160, 255, 256):
            descs = _frame_set(dim)
            _upload(ctx, descs)
            for a, b in ((4, 7), (7, 4), (8, 5), (2, 8), (3, 6), (6, 11), (0, 5), (5, 9), (8, 10), (1, 3), (4, 0)):
                n1, l1, u2 = ctx.match_screen_pair(a, b)
                d2 = _sq_dists(descs[a], descs[b])
                v1, v2 = _top2(d2) if d2.shape[1] > 1 else (d2[:, 0], None)
                res.append((dim, a, b, d2.shape[1], n1, l1, u2, _sq_dists(_codes(descs[a]), _codes(descs[b])).min(1), v1, v2))
    finally:
        ctx.close()
    return res


def test_quantised_minimum_equals_the_numpy_integer(swept):
    """n1 of every real row is min_j |M_a - M_b_j|^2 exactly: pins the FP6 operand layout and the exactness of the accumulation."""
    for dim, a, b, _, n1, _, _, want, _, _ in swept:
        assert np.array_equal(n1.astype(np.int64), want), (dim, a, b)


def test_bounds_enclose_the_true_minimum_and_runner_up(swept):
    seen = 0
    for dim, a, b, nb, _, l1, u2, _, v1, v2 in swept:
        assert np.all(l1 >= 0) and np.all(l1 <= v1), (dim, a, b)
        if v2 is None:
            assert np.all(u2 == -1)                       # one train row: no runner-up, the bound form's padding value
            continue
        has = u2 >= 0
        assert np.all(u2[has] >= v2[has]), (dim, a, b)
        if nb >= 64:
            assert has.all(), (dim, a, b)                 # train rows in more than one subset: every row has a bound
        seen += int(has.sum())
    assert seen > 1000


def test_tally_every_passing_row_open_and_few_others():
    """Four frames of the S200 scene + two unstructured ones, 320 rows at 256-D, all 30 ordered pairs: every row that passes the
    ratio test (numpy) must be left open by the screen, and the open rows may number at most the passing rows + 5 % of the real
    rows (the numpy model of the bound: 384 open against 366 passing of 9600 — a screen that closes nothing would fail the cap
    by a factor of ten)."""
    descs, _ = synth.make_frame_descriptors(synth.make_scene(200, 50000, 10), 320, 256, frames=[3, 4, 5, 90])
    descs = [np.asarray(d, dtype=np.float32) for d in descs]
    descs += [synth.random_u8_descriptors(320, 256, 7, 0), synth.random_u8_descriptors(320, 256, 7, 1)]
    pairs = np.array([[a, b] for a in range(6) for b in range(6) if a != b], dtype=np.int32)
    ctx = _ctx("screen")
    try:
        _upload(ctx, descs)
        ctx.match_all_pairs(pairs, stats=False)
        rows, left_open = ctx.match_screen()
        passing = open_by_entry = 0
        for a, b in pairs:
            v1, v2 = _top2(_sq_dists(descs[a], descs[b]))
            ok = _ratio_pass(v1, v2)
            _, l1, u2 = ctx.match_screen_pair(int(a), int(b))
            is_open = (u2 < 0) | _ratio_pass(l1, np.maximum(u2, 0))
            assert np.all(is_open[ok]), (a, b)            # no passing row is ever closed
            passing += int(ok.sum())
            open_by_entry += int(is_open.sum())
    finally:
        ctx.close()
    real = sum(descs[a].shape[0] for a, _ in pairs)
    print(f"screen tally: rows {rows} open {left_open} (by the debug entry {open_by_entry}) passing {passing}")
    assert rows == real == 9600
    assert left_open == open_by_entry                      # match_rowpick_kernel listed exactly the rows the bounds leave open
    assert passing <= left_open <= passing + 0.05 * real
