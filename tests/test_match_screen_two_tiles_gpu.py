"""GPU: the call structure of the screen sweep above 128-D (match_screen_kernel, eacham_amd/csrc/matcher.hip): how many train tiles
a call covers, how the ring slots, the fragment ring and the two accumulator sets rotate, where the prologue stops and which tail
takes the last tiles. None of that may show in a result, so every case holds, on train frames of T = 1 .. 9 tiles (odd and even,
below and above the ring's depth, each with a full and a ragged last tile) and query frames of 1 .. 300 rows (a wave with one
sub-tile, an inactive wave that still stages, a second workgroup):

  * the match graph against the CPU oracle and against a context created under EACHAM_MATCH_SWEEP_FORM=exact, bytes for bytes;
  * {n1, L1, U2} of eacham_match_debug_screen_pair against the numpy statement of the bound: the two smallest of the minima over the
    sixteen subsets (tile parity x group of four stored train rows) of a query row, through screen::lower_d2 / upper_d2;
  * the tally of eacham_match_debug_screen (rows met, rows left open) and the item count of eacham_match_debug_screen_items against
    the numbers that statement gives: the open-row masks and the packed list are what they were, not only the final graph.

A train frame's rows are forced to one parity of the centred squared norm, so that its stored order is its own and its tile count
is ceil(rows / 32); the query frames keep mixed parities (both classes, a partly filled last tile in each)."""
import numpy as np
import pytest

from eacham_amd import synth
import ham_cases as HC
import ham_reference as R
import oracle_api as O
import test_match_open_pack_gpu as P
import test_match_screen_gpu as S
import test_match_screen_list_gpu as L

pytestmark = pytest.mark.gpu
SEED = 1207
TRAIN = [1, 2, 32, 33, 64, 65, 96, 97, 128, 160, 161, 192, 193, 224, 225, 257]
QUERY = [1, 63, 64, 65, 255, 256, 257, 300]
MAX_D2 = 256 * 255 * 255


def _model(Da, Db):
    """(n1, L1, U2) per row of Da against Db as the sweep's tail computes them (match_screen.hpp): n = |M_a - M_b|^2 over the grid
    codes (a padded dimension is code 0 on both sides), n1 and u the two smallest of the minima over the sixteen subsets of the
    STORED train rows, the bounds in double. Every product and sum is an integer below 2^53: float64 is exact."""
    Ma, Mb = L._M[Da.astype(np.int64)], L._M[Db.astype(np.int64)]
    s_a = ((Da.astype(np.int64) - (64 + 4 * Ma)) ** 2).sum(1)
    e_b = ((Db.astype(np.int64) - (64 + 4 * Mb)) ** 2).sum(1).max()
    Fa, Fb = Ma.astype(np.float64), Mb.astype(np.float64)
    n = (Fa * Fa).sum(1)[:, None] + (Fb * Fb).sum(1)[None, :] - 2.0 * (Fa @ Fb.T)
    pos = L._stored_pos(Db)
    subset = ((pos >> 5) & 1) * 8 + ((pos & 31) >> 2)
    mins = np.full((Da.shape[0], 16), np.inf)
    for k in range(16):
        if np.any(subset == k):
            mins[:, k] = n[:, subset == k].min(1)
    mins.sort(axis=1)
    n1, u = mins[:, 0], mins[:, 1]
    slack = np.sqrt(s_a.astype(np.float64)) + np.sqrt(float(e_b))
    lo = 4.0 * np.sqrt(n1) - slack
    l1 = np.where(lo > 0, np.clip(np.floor(lo * lo) - 1.0, 0.0, MAX_D2), 0.0)
    has = np.isfinite(u)
    hi = 4.0 * np.sqrt(np.where(has, u, 0.0)) + slack
    u2 = np.where(has, np.minimum(np.ceil(hi * hi) + 1.0, MAX_D2), -1.0)
    return n1.astype(np.uint32), l1.astype(np.int32), u2.astype(np.int32)


def _open(l1, u2, ratio=0.8, hamming=False):
    """match_rowpick_kernel's predicate on the bounds: a real minimum, and no bound on the runner-up or a pair that passes."""
    test = R.ratio_pass(l1, np.maximum(u2, 0), ratio) if hamming else L._ratio_pass(l1, np.maximum(u2, 0), ratio)
    return (l1 >= 0) & ((u2 < 0) | test)


def _tiles(D):
    """Stored tiles of a frame: whole tiles of its even rows, then of its odd rows."""
    even = int((((D.astype(np.int64) - 128) ** 2).sum(1) % 2 == 0).sum())
    return -(-even // 32) + -(-(D.shape[0] - even) // 32)


def _frames(dim):
    """Frames 0 .. 15: the train sizes, noisy copies of one base frame, all rows even (k even) or all odd (k odd). Frames 16 .. 23:
    the query sizes, noisy copies of the same base with the parities they happen to have."""
    base = synth.random_u8_descriptors(max(TRAIN + QUERY), dim, SEED, 0)
    descs = []
    for k, n in enumerate(TRAIN + QUERY):
        D = np.clip(base[:n] + np.rint(6.0 * synth.rng_normal(SEED, 20 + k, (n, dim))), 0, 255).astype(np.float32)
        descs.append(S._with_norm_parity(D, [k % 2] * n) if k < len(TRAIN) else D)
    return descs


def _pairs():
    """(query, train): the 257-row query frame against every train size; every other query size against three train sizes, a
    different three each; six pairs the other way round (a query frame of mixed parities as the train frame), grouped by train frame."""
    nt, q257 = len(TRAIN), len(TRAIN) + QUERY.index(257)
    pairs = [[q257, t] for t in range(nt)]
    for i, n in enumerate(QUERY):
        if n != 257:
            pairs += [[nt + i, (5 * i + 7 * j + 1) % nt] for j in range(3)]
    pairs += [[t, nt + i] for i, t in ((7, 3), (7, 14), (5, 0), (5, 9), (1, 6), (0, 15))]
    pairs = np.array(pairs, dtype=np.int32)
    return pairs[np.argsort(pairs[:, 1], kind="stable")]


def _bytes_equal(got, want, what):
    for name, g, w in zip(["counts", "offsets", "q", "t"], got[:4], want[:4]):
        w = np.asarray(w)
        assert g.shape == w.shape and g.tobytes() == w.astype(g.dtype).tobytes() and np.array_equal(g, w), f"{what}: {name} differs"


def _check_sweep(ctx, descs, pairs, tally, starts, ratio=0.8, hamming=False, embed=None):
    """The debug entry's numbers of every pair against the model, and the call's tally against what the model leaves open."""
    emb = embed or (lambda d: d)
    opens = []
    for a, b in pairs:
        n1, l1, u2 = ctx.match_screen_pair(int(a), int(b))
        w1, wl, wu = _model(emb(descs[a]), emb(descs[b]))
        assert np.array_equal(n1, w1), ("n1", a, b)
        assert np.array_equal(l1, wl), ("L1", a, b)
        assert np.array_equal(u2, wu), ("U2", a, b)
        opens.append(int(_open(wl, wu, ratio, hamming).sum()))
    want = (sum(descs[a].shape[0] for a, _ in pairs), sum(opens), P._expected_items(pairs, opens, starts))
    print(f"open rows per pair {opens}, launches at {list(starts)}: (rows, open, items) {tally}, expected {want}")
    assert tally == want
    return opens


def test_the_cases_cover_what_they_claim():
    """(no GPU needed) T = 1 .. 9 among the train frames, full and ragged last tiles; every size of both lists in a pair; T = 1 .. 7
    each against the 257-row query frame; train frames of mixed parities among the reversed pairs."""
    descs, pairs = _frames(256), _pairs()
    T = [_tiles(d) for d in descs]
    assert T[:len(TRAIN)] == [-(-n // 32) for n in TRAIN] and set(T[:len(TRAIN)]) == set(range(1, 10))
    assert {descs[a].shape[0] for a, _ in pairs} >= set(QUERY) and {descs[b].shape[0] for _, b in pairs} >= set(TRAIN)
    q257 = len(TRAIN) + QUERY.index(257)
    assert {T[b] for a, b in pairs if a == q257} >= set(range(1, 8))
    assert any(b >= len(TRAIN) and T[b] > -(-descs[b].shape[0] // 32) for _, b in pairs)


@pytest.mark.parametrize("dim", [129, 192, 256])
def test_every_tile_count_and_query_shape(dim):
    descs, pairs = _frames(dim), _pairs()
    want = O.match_all_pairs(descs, pairs, min_dir=1, min_mutual=0)
    with L._context(EACHAM_MATCH_SWEEP_FORM="exact") as ctx:
        L._upload(ctx, descs)
        exact = ctx.match_all_pairs(pairs, min_dir=1, min_mutual=0, stats=False)
        assert ctx.match_screen() == (0, 0)
    with L._context() as ctx:                                    # the default above 128-D is the screen form
        L._upload(ctx, descs)
        got = ctx.match_all_pairs(pairs, min_dir=1, min_mutual=0, stats=False)
        tally = ctx.match_screen() + (ctx.match_screen_items(),)
        starts, _ = ctx.match_batches(len(pairs), stats=False)
        _bytes_equal(got, want, "oracle")
        _bytes_equal(got, exact, "exact form")
        opens = _check_sweep(ctx, descs, pairs, tally, starts)
    assert got[0].sum() > 1000 and 0 < sum(opens) < tally[0]    # rows do match, and the screen closes rows


def test_binary_frames_under_hamming():
    """Packed rows of 200 and of 256 bits: METRIC = 1 of the same loop. Train frames of 1 .. 7 tiles (an even number of set bits in
    every row: one parity class), query frames of 257 and 65 rows."""
    for nbytes in (25, 32):
        sizes = [33, 97, 161, 224, 1, 130, 192, 257, 65]
        base = HC._bytes(SEED, nbytes, (257, nbytes))
        descs = []
        for k, n in enumerate(sizes):
            rows = base[:n] ^ HC._flips(SEED, 40 + 16 * nbytes + k, (n, nbytes), 0.04)
            if k < 7:
                rows[:, 0] ^= (R.popcount(rows) & 1).astype(np.uint8)     # an even popcount: the parity of the centred norm
            descs.append(rows)
        assert [_tiles(R.embed(d)) for d in descs[:7]] == [2, 4, 6, 7, 1, 5, 6]
        pairs = np.array([[7, t] for t in range(7)] + [[8, 1], [8, 3], [3, 7]], dtype=np.int32)
        pairs = pairs[np.argsort(pairs[:, 1], kind="stable")]
        want = R.Scene(descs).match_all_pairs(pairs, 0.8, 1, 0)
        out = {}
        for form in ("exact", None):
            with L._context(**({"EACHAM_MATCH_SWEEP_FORM": form} if form else {})) as ctx:
                ctx.clear_descriptors()
                for f, d in enumerate(descs):
                    ctx.upload_descriptors_bits(f, d)
                out[form] = ctx.match_all_pairs_hamming(pairs, 0.8, 1, 0, stats=False)
                tally = ctx.match_screen() + (ctx.match_screen_items(),)
                if form is None:
                    starts, _ = ctx.match_batches(len(pairs), stats=False)
                    _check_sweep(ctx, descs, pairs, tally, starts, hamming=True, embed=R.embed)
                else:
                    assert tally == (0, 0, 0)
        for g, w, e in zip(out[None][:5], want[:5], out["exact"][:5]):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes() == e.tobytes()
        assert out[None][0].sum() > 300


def test_ties_across_the_tiles_of_a_call():
    """A train frame of seven tiles (all rows even: stored as given) with equal rows 32 apart in every neighbouring pair of tiles and
    copies of one row at row 0 of tiles 2 .. 6; the query rows are noisy copies, so the tied rows are their minimum AND their
    runner-up. Under ratio 1.5 (the directed call takes it) a tie passes: the lowest train index must come back, through the screen
    and the exact pass. The graph is held at ratio 1, the largest it takes, where the tied rows fail and every other row passes."""
    n = 224
    base = synth.random_u8_descriptors(n, 256, SEED, 5).astype(np.float32)
    train = S._with_norm_parity(base, [0] * n)
    lower = {}
    for t in range(6):
        for r in (3 + t, 31):
            train[32 * (t + 1) + r] = train[32 * t + r]
            lower[32 * (t + 1) + r] = lower.get(32 * t + r, 32 * t + r)
    for t in range(2, 7):
        train[32 * t] = train[7]
        lower[32 * t] = 7
    assert _tiles(train) == 7 and np.array_equal(L._stored_pos(train), np.arange(n))
    query = np.clip(train + np.rint(2.0 * synth.rng_normal(SEED, 6, (n, 256))), 0, 255).astype(np.float32)
    descs = [query, train]
    pairs = np.array([[0, 1]], dtype=np.int32)
    wq, wt = O.match_directed(query, train, 1.5)
    want = O.match_all_pairs(descs, pairs, ratio=1.0, min_dir=1, min_mutual=0)   # (the graph takes ratios up to 1: a tie fails there)
    with L._context(EACHAM_MATCH_SWEEP_FORM="exact") as ctx:
        directed_exact = ctx.match_pairs_directed(descs, pairs, ratio=1.5)[0]
        exact = ctx.match_all_pairs(pairs, ratio=1.0, min_dir=1, min_mutual=0, stats=False)
    with L._context() as ctx:
        directed = ctx.match_pairs_directed(descs, pairs, ratio=1.5)[0]
        tally = ctx.match_screen() + (ctx.match_screen_items(),)
        opens = _check_sweep(ctx, descs, pairs, tally, [0], ratio=1.5)
        got = ctx.match_all_pairs(pairs, ratio=1.0, min_dir=1, min_mutual=0, stats=False)
        tally = ctx.match_screen() + (ctx.match_screen_items(),)
        _check_sweep(ctx, descs, pairs, tally, [0], ratio=1.0)
    assert directed == dict(zip(wq.tolist(), wt.tolist())) == directed_exact and len(directed) == n
    for row, first in lower.items():
        assert directed[row] == first and directed[first] == first, (row, first)
    _bytes_equal(got, want, "oracle")
    _bytes_equal(got, exact, "exact form")
    assert opens[0] == n                                          # every row is left to the exact pass


def test_launches_through_two_slots():
    """EACHAM_MATCH_BUDGET_MB=16 with one resident frame of 2000 rows that no pair names (a launch's workspace is sized by the
    largest resident frame): the 276 pairs of the 24 frames go through at least two launches and both workspace slots."""
    descs = _frames(256)
    big = synth.random_u8_descriptors(2000, 256, SEED, 9).astype(np.float32)
    nf = len(descs)
    pairs = synth.all_pairs(nf)
    pairs = pairs[np.argsort(pairs[:, 1], kind="stable")]
    want = O.match_all_pairs(descs, pairs, min_dir=1, min_mutual=0)
    with L._context(EACHAM_MATCH_BUDGET_MB=16, EACHAM_MATCH_SWEEP_FORM="exact") as ctx:
        L._upload(ctx, descs + [big])
        exact = ctx.match_all_pairs(pairs, min_dir=1, min_mutual=0, stats=False)
    with L._context(EACHAM_MATCH_BUDGET_MB=16) as ctx:
        L._upload(ctx, descs + [big])
        got = ctx.match_all_pairs(pairs, min_dir=1, min_mutual=0, stats=False)
        again = ctx.match_all_pairs(pairs, min_dir=1, min_mutual=0, stats=False)
        tally = ctx.match_screen() + (ctx.match_screen_items(),)
        starts, slots = ctx.match_batches(len(pairs), stats=False)
        assert len(starts) >= 2 and slots == 2, (starts, slots)
        _check_sweep(ctx, descs, pairs, tally, starts)
    _bytes_equal(got, want, "oracle")
    _bytes_equal(got, exact, "exact form")
    _bytes_equal(again, got, "second call")
