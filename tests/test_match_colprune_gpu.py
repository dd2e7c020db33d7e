"""GPU: candidate columns settled from the row sweep's minima (match_argmin_kernel) against the CPU oracle.

A candidate (q, t) — a query row that passes the ratio test, and its best train row — survives the mutual check iff no other
query row comes close enough to t to take the column or to break its ratio test. The arg-min pass settles a candidate without
computing a distance when the lower bounds the row sweep left behind rule every other row out; the rest go through
match_colverify_kernel as before. Every case below is built so that ONE branch of that decision gives the result, and checks on the
CPU first that the case is not soft: the oracle must drop a candidate that "settle everything" would keep. Every case runs at
64 / 128 / 256-D under both forms of the row sweep, bit for bit against the oracle and against a context created with
EACHAM_MATCH_COLPRUNE=0 (every candidate down the column pass)."""
import functools
import os

import numpy as np
import pytest

import oracle_api as O

pytestmark = pytest.mark.gpu

DIMS = [64, 128, 256]
FORMS = ["exact", "bound"]
MD, MM = 1, 0   # thresholds of every case: a pair with one passing row is live, and the library runs its lean form


# ---- contexts: one per (form of the sweep, switch), created once ----------------------------------------------------
_CTX = {}


def _ctx(form, prune):
    key = (form, prune)
    if key not in _CTX:
        from eacham_amd import HipContext
        env = {"EACHAM_MATCH_SWEEP_FORM": form}
        if not prune:
            env["EACHAM_MATCH_COLPRUNE"] = "0"
        old = {k: os.environ.get(k) for k in ("EACHAM_MATCH_SWEEP_FORM", "EACHAM_MATCH_COLPRUNE")}
        try:
            os.environ.pop("EACHAM_MATCH_COLPRUNE", None)
            os.environ.update(env)   # read once, at eacham_ctx_create
            _CTX[key] = HipContext(0)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()


# ---- building blocks ---------------------------------------------------------------------------------------------------
def _rows(rng, n, dim):
    """Random integer descriptors away from 0 and 255, so that the offsets below never clip: d2 between two of them is ~ dim * 6000."""
    return rng.integers(40, 216, size=(n, dim)).astype(np.float32)


def _off(row, **coords):
    """`row` with integer offsets on single coordinates (c0=20 adds 20 to coordinate 0): d2 to `row` is the sum of their squares."""
    r = row.copy()
    for k, v in coords.items():
        r[int(k[1:])] += v
    assert r.min() >= 0 and r.max() <= 255
    return r


def _stored_tile(D):
    """Tile (32 rows) of every row of a frame in the library's stored order: rows with an even squared norm of the centred values
    first, each parity class padded to whole tiles (matcher.hip: partition_kernel)."""
    odd = (((D.astype(np.int64) - 128) ** 2).sum(axis=1) & 1).astype(bool)
    pos = np.empty(len(D), dtype=np.int64)
    pos[~odd] = np.arange((~odd).sum())
    pos[odd] = ((~odd).sum() + 31) // 32 * 32 + np.arange(odd.sum())
    return pos // 32


def _case_a(dim):
    """Clean matches only: every candidate is settled, nothing is verified."""
    rng = np.random.default_rng(100 + dim)
    A, B = _rows(rng, 150, dim), _rows(rng, 170, dim)
    for i in range(40):
        B[3 * i + 1] = _off(A[2 * i], **{f"c{i % dim}": 6, f"c{(i + 7) % dim}": -5})
    return [A, B], [[0, 1], [1, 0]]


def _case_b(dim):
    """Two query rows equally near one train row: the column has no unique minimum, neither is a mutual match."""
    rng = np.random.default_rng(200 + dim)
    A, B = _rows(rng, 70, dim), _rows(rng, 90, dim)
    A[11] = _off(B[40], c0=3)
    A[52] = _off(B[40], c1=-3)
    for i in range(8):
        A[20 + i] = _off(B[60 + i], c2=4)   # clean matches beside them
    return [A, B], [[0, 1]]


def _case_c(dim):
    """The v1 bound: query row 7 is no candidate (two near-equal train neighbours, 30 and 31) but lies at d2 = 100 of train row 12,
    the best column of candidate 3 (d2 = 400): the column's best is row 7, candidate 3 is not mutual."""
    rng = np.random.default_rng(300 + dim)
    A, B = _rows(rng, 70, dim), _rows(rng, 90, dim)
    A[3] = _off(B[12], c0=20)
    A[7] = _off(B[12], c0=-10)
    B[30] = _off(A[7], c1=2)
    B[31] = _off(A[7], c2=2, c3=1)
    for i in range(8):
        A[20 + i] = _off(B[60 + i], c2=4)
    return [A, B], [[0, 1]]


def _case_d(dim):
    """The v2 bound: candidate 9 (best column 50 at d2 = 100) has its runner-up, d2 = 500, at train row 12, the best column of
    candidate 3 (d2 = 400): column 12 fails its ratio test (400 / 500) and candidate 3 is not mutual. Rows 12 and 50 lie in
    different train tiles, so row 9 is not in candidate 3's arg-min item."""
    rng = np.random.default_rng(400 + dim)
    A = _rows(rng, 70, dim)
    for seed in range(64):   # (seeded: the first train frame whose rows 12 and 50 fall into different tiles)
        B = _rows(np.random.default_rng(4000 + 64 * dim + seed), 90, dim)
        A[3] = _off(B[12], c0=20)
        A[9] = _off(B[12], c0=-20, c1=10)
        B[50] = _off(A[9], c2=10)
        tiles = _stored_tile(B)
        if tiles[12] != tiles[50]:
            break
    assert tiles[12] != tiles[50]
    for i in range(8):
        A[20 + i] = _off(B[60 + i], c2=4)
    return [A, B], [[0, 1]]


def _case_e(dim):
    """More than 32 candidates with their minima in one train tile (a second arg-min item, whose rows the first item's wave does
    not hold), six of its columns with a second query row at d2 = 484 against the candidate's 400: those columns fail their ratio test."""
    rng = np.random.default_rng(500 + dim)
    A, B = _rows(rng, 120, dim), _rows(rng, 200, dim)
    tiles = _stored_tile(B)
    full = [k for k in range(tiles.max() + 1) if (tiles == k).sum() == 32]
    cols = np.flatnonzero(tiles == full[0])
    for i, t in enumerate(cols):
        A[3 * i] = _off(B[t], **{f"c{i}": 20})
    for i in range(6):
        A[100 + i] = _off(B[cols[5 * i]], **{f"c{40 + i}": -22})
    return [A, B], [[0, 1]]


def _case_f(dim):
    """The exact block: two candidates with the same best column (d2 = 400 and 484) sit in one arg-min item; every lower bound of
    the sweep is far away, only the item's own distances show that the column fails its ratio test."""
    rng = np.random.default_rng(600 + dim)
    A, B = _rows(rng, 70, dim), _rows(rng, 90, dim)
    A[11] = _off(B[40], c0=20)
    A[52] = _off(B[40], c1=-22)
    for i in range(8):
        A[20 + i] = _off(B[60 + i], c2=4)
    return [A, B], [[0, 1]]


def _case_g(dim):
    """Query frames of 0, 1 and 2 rows against a train frame of 2 rows (and a larger one): a column needs two query rows to have
    a second neighbour, so with fewer nothing may be settled — and nothing matches."""
    rng = np.random.default_rng(700 + dim)
    T2, big = _rows(rng, 2, dim), _rows(rng, 60, dim)
    q1 = _off(T2[0], c0=5)[None]
    q2 = np.stack([_off(T2[0], c0=5), _off(T2[1], c1=-6)])
    for i in range(6):
        big[10 + i] = _off(T2[i % 2], **{f"c{2 + i}": 30 + i})
    descs = [np.zeros((0, dim), np.float32), q1, q2, T2, big]
    pairs = [[a, b] for a in range(5) for b in range(5) if a != b]
    return descs, pairs


def _case_h(dim):
    """A seeded mix: four frames of ~250 noisy copies of one landmark set, every row at one of several noise levels between
    clean and as far as an unrelated row: row and column ratios straddle 0.8, so some candidates are settled, some are verified
    and kept, and some are dropped at the mutual check."""
    rng = np.random.default_rng(800 + dim)
    L = _rows(rng, 260, dim)
    levels = np.array([2.0, 8.0, 20.0, 30.0, 38.0, 46.0])
    descs = []
    for n in (250, 241, 256, 233):
        keep = np.sort(rng.permutation(260)[:n])
        sigma = levels[rng.integers(0, len(levels), n)][:, None]
        descs.append(np.clip(L[keep] + np.rint(sigma * rng.normal(0, 1, (n, dim))), 0, 255).astype(np.float32))
    return descs, [[a, b] for a in range(4) for b in range(4) if a != b]


CASES = {"a": _case_a, "b": _case_b, "c": _case_c, "d": _case_d, "e": _case_e, "f": _case_f, "g": _case_g, "h": _case_h}


@functools.lru_cache(maxsize=None)
def _reference(case, dim):
    """(descs, pairs, the oracle's CSR, candidates the oracle dropped at the mutual check) — computed once per case and dimension."""
    descs, pairs = CASES[case](dim)
    pairs = np.array(pairs, dtype=np.int32)
    want = O.match_all_pairs(descs, pairs, min_dir=MD, min_mutual=MM)
    # "settle everything" keeps every passing row of a live pair: stats = {|m12|, |m21|, |mutual|, edge}
    live = (want[4][:, 0] >= MD) & (want[4][:, 0] > MM)
    dropped = int((want[4][live, 0] - want[4][live, 2]).sum())
    return descs, pairs, want, dropped


def _run(ctx, descs, pairs):
    ctx.clear_descriptors()
    for f, d in enumerate(descs):
        ctx.upload_descriptors(f, d)
    got = ctx.match_all_pairs(pairs, min_dir=MD, min_mutual=MM, stats=False)
    return got, ctx.match_colprune()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_settled_columns_match_the_oracle(case, dim, form):
    descs, pairs, want, dropped = _reference(case, dim)
    if case != "a":   # the named branch decides: the oracle drops candidates that settling everything would keep
        assert dropped > 0, "soft case: the oracle keeps every passing row"
    else:
        assert dropped == 0 and want[0].sum() >= 40
    got, (settled, verified) = _run(_ctx(form, True), descs, pairs)
    old, (settled0, verified0) = _run(_ctx(form, False), descs, pairs)
    print(f"case {case} {dim}-D {form}: settled {settled} verified {verified}; switch at 0: settled {settled0} verified {verified0}; "
          f"oracle matches {int(want[0].sum())}, dropped at the mutual check {dropped}")
    for name, g, o, w in zip(["counts", "offsets", "q", "t"], got[:4], old[:4], want[:4]):
        assert np.array_equal(g, w), f"{name} differs from the oracle"
        assert np.array_equal(o, w), f"{name} differs from the oracle with EACHAM_MATCH_COLPRUNE=0"
    assert settled0 == 0 and settled + verified == verified0
    if case == "a":
        assert settled > 0 and verified == 0
    elif case == "g":
        pass   # (the frames with fewer than two rows: below)
    else:
        assert verified > 0
    if case == "h":
        assert settled > 0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dim", DIMS)
def test_nothing_is_settled_with_fewer_than_two_query_rows(dim, form):
    """Case (g), the single-row query frame alone: its row passes the ratio test against the two-row train frame (a candidate),
    but the column has one neighbour only — the candidate is verified, never settled, and is no match. The two-row query frame
    beside it may be settled."""
    descs, _, _, _ = _reference("g", dim)
    for qf, may_settle in ((1, False), (2, True), (0, False)):
        pairs = np.array([[qf, 3]], dtype=np.int32)
        want = O.match_all_pairs(descs, pairs, min_dir=MD, min_mutual=MM)
        got, (settled, verified) = _run(_ctx(form, True), descs, pairs)
        print(f"query frame of {len(descs[qf])} rows, {dim}-D {form}: settled {settled} verified {verified}, oracle |m12| {want[4][0, 0]} mutual {want[4][0, 2]}")
        for name, g, w in zip(["counts", "offsets", "q", "t"], got[:4], want[:4]):
            assert np.array_equal(g, w), f"{name} differs from the oracle"
        assert settled + verified == want[4][0, 0]
        if not may_settle:
            assert settled == 0
        if qf == 1:
            assert verified == 1 and want[0][0] == 0
        if qf == 2:
            assert want[0][0] == 2
