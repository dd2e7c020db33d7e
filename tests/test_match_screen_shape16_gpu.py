"""GPU: the inside of a train tile of the screen sweep above 128-D (match_screen_kernel, eacham_amd/csrc/matcher.hip): which lanes
hold which query rows and which K blocks, in which registers the groups of four train rows land, which constants start a chain.
The chains work on sub-tiles of 16 query rows, halves of 16 train rows and K blocks of 32 codes, so the shapes here sit on those
edges: query frames of 1 .. 65 rows around every multiple of 16, train frames of 1 .. 8 and 13 real tiles of both parity classes
(odd and even counts: with and without the tile swept ahead of the calls), dimensions that end inside a K block, binary frames of
160 and 256 bits, minima and runners-up planted in chosen positions of the stored train frame, and train rows whose constants
differ by level between rows r, r + 4 and r + 16. None of the inside may show, so every case holds

  * {n1, L1, U2} of eacham_match_debug_screen_pair (the words the sweep stores per row) against the numpy statement below of the
    sixteen subsets (tile parity x group of four stored train rows);
  * the match graph against the CPU oracle and a context under EACHAM_MATCH_SWEEP_FORM=exact, bytes for bytes;
  * the tally of eacham_match_debug_screen and the item count against what that statement leaves open."""
import numpy as np
import pytest

from eacham_amd import synth
import ham_cases as HC
import ham_reference as R
import oracle_api as O
import test_match_open_pack_gpu as P
import test_match_screen_gpu as S
import test_match_screen_list_gpu as L
import test_match_screen_two_tiles_gpu as T

pytestmark = pytest.mark.gpu
SEED = 16128
QUERY = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65]
# (rows of even, rows of odd centred norm) of a train frame: 1 .. 8 and 13 stored tiles, the classes' last tiles ragged or full
TRAIN = [(20, 0), (20, 10), (40, 30), (33, 40), (70, 50), (96, 65), (100, 90), (128, 100), (200, 190)]
TRAIN_TILES = [1, 2, 3, 4, 5, 6, 7, 8, 13]
MAX_D2 = 256 * 255 * 255


def _subset_minima(Da, Db):
    """n = |M_a - M_b|^2 over the grid codes (match_screen.hpp) for every row of Da against every row of Db, and its minima over
    the sixteen subsets of the STORED train rows: stored position p lies in tile p >> 5 at row p & 31; the subset is (parity of the
    tile, row >> 2). Integers below 2^53 throughout: float64 is exact."""
    Ma, Mb = L._M[Da.astype(np.int64)].astype(np.float64), L._M[Db.astype(np.int64)].astype(np.float64)
    n = (Ma * Ma).sum(1)[:, None] + (Mb * Mb).sum(1)[None, :] - 2.0 * (Ma @ Mb.T)
    pos = L._stored_pos(Db)
    tile, row = pos >> 5, pos & 31
    subset = 8 * (tile & 1) + (row >> 2)
    mins = np.full((Da.shape[0], 16), np.inf)
    for k in range(16):
        if np.any(subset == k):
            mins[:, k] = n[:, subset == k].min(1)
    return n, mins


def _model(Da, Db):
    """(n1, L1, U2) per row of Da as the tail computes them: the two smallest subset minima through screen::lower_d2 / upper_d2."""
    _, mins = _subset_minima(Da, Db)
    mins = np.sort(mins, axis=1)
    n1, u = mins[:, 0], mins[:, 1]
    err = lambda D: ((D.astype(np.int64) - (64 + 4 * L._M[D.astype(np.int64)])) ** 2).sum(1)
    slack = np.sqrt(err(Da).astype(np.float64)) + np.sqrt(float(err(Db).max()))
    lo = 4.0 * np.sqrt(n1) - slack
    l1 = np.where(lo > 0, np.clip(np.floor(lo * lo) - 1.0, 0.0, MAX_D2), 0.0)
    has = np.isfinite(u)
    hi = 4.0 * np.sqrt(np.where(has, u, 0.0)) + slack
    u2 = np.where(has, np.minimum(np.ceil(hi * hi) + 1.0, MAX_D2), -1.0)
    return n1.astype(np.uint32), l1.astype(np.int32), u2.astype(np.int32)


def _check_sweep(ctx, descs, pairs, tally, starts, ratio=0.8, hamming=False, embed=None):
    """Every pair's stored words against the model; the call's (rows, open rows, items) against what the model leaves open."""
    emb = embed or (lambda d: d)
    opens = []
    for a, b in pairs:
        got = ctx.match_screen_pair(int(a), int(b))
        want = _model(emb(descs[a]), emb(descs[b]))
        for name, g, w in zip(("n1", "L1", "U2"), got, want):
            assert np.array_equal(g, w), (name, int(a), int(b), np.flatnonzero(g != w)[:8], g[g != w][:8], w[g != w][:8])
        opens.append(int(T._open(want[1], want[2], ratio, hamming).sum()))
    want = (sum(descs[a].shape[0] for a, _ in pairs), sum(opens), P._expected_items(pairs, opens, starts))
    print(f"open rows per pair {opens}, launches at {list(starts)}: (rows, open, items) {tally}, expected {want}")
    assert tally == want
    return opens


def _three_ways(descs, pairs, ratio=0.8):
    """The graph of the screen form against the oracle and the exact form, and the sweep's words and tally against the model."""
    want = O.match_all_pairs(descs, pairs, ratio=ratio, min_dir=1, min_mutual=0)
    with L._context(EACHAM_MATCH_SWEEP_FORM="exact") as ctx:
        L._upload(ctx, descs)
        exact = ctx.match_all_pairs(pairs, ratio=ratio, min_dir=1, min_mutual=0, stats=False)
        assert ctx.match_screen() == (0, 0)
    with L._context() as ctx:
        L._upload(ctx, descs)
        got = ctx.match_all_pairs(pairs, ratio=ratio, min_dir=1, min_mutual=0, stats=False)
        tally = ctx.match_screen() + (ctx.match_screen_items(),)
        starts, _ = ctx.match_batches(len(pairs), stats=False)
        T._bytes_equal(got, want, "oracle")
        T._bytes_equal(got, exact, "exact form")
        opens = _check_sweep(ctx, descs, pairs, tally, starts, ratio=ratio)
    return got, opens, tally


def _mixed(n_even, n_odd):
    """A parity per row, the two classes interleaved while both last: the stored order is not the given one."""
    par, left = [], [n_even, n_odd]
    while left[0] or left[1]:
        c = 0 if left[0] and (not left[1] or len(par) % 2 == 0) else 1
        par.append(c)
        left[c] -= 1
    return par


def _frames(dim):
    """Frames 0 .. 8: the train frames, noisy copies of the first rows of one base frame with the parities of _mixed. Frames 9 .. 21:
    the query sizes, noisy copies of base rows spread over the base (stride 7 from an offset of their own), all of even parity: stored
    as given, so a frame of m rows is m rows of its first wave-block. Frame 22: 65 rows with the parities they happen to have."""
    nmax = max(e + o for e, o in TRAIN)
    base = synth.random_u8_descriptors(nmax, dim, SEED, 0)
    noisy = lambda rows, k: np.clip(base[rows] + np.rint(6.0 * synth.rng_normal(SEED, 20 + k, (len(rows), dim))), 0, 255).astype(np.float32)
    descs = [S._with_norm_parity(noisy(np.arange(e + o), k), _mixed(e, o)) for k, (e, o) in enumerate(TRAIN)]
    for i, m in enumerate(QUERY):
        rows = (11 * i + 7 * np.arange(m)) % nmax
        descs.append(S._with_norm_parity(noisy(rows, 40 + i), [0] * m))
    descs.append(noisy((5 + 3 * np.arange(65)) % nmax, 60))
    return descs


def _pairs(full):
    """(query, train) grouped by train frame. Every query size against train frames of an odd and of an even tile count (no tile
    and one tile swept ahead of the calls): four train frames each when full, two otherwise, rotating through the list. The 65-row
    frame of mixed parities against every train frame either way."""
    nt, nq = len(TRAIN), len(QUERY)
    pairs = [[nt + i, t] for i in range(nq) for t in sorted({(i + j) % 8 for j in ((0, 1, 4, 5) if full else (0, 1))} | ({8} if full and i % 3 == 0 else set()))]
    pairs += [[nt + nq, t] for t in range(nt)]
    pairs = np.array(pairs, dtype=np.int32)
    return pairs[np.argsort(pairs[:, 1], kind="stable")]


def test_the_cases_are_what_they_claim():
    """(no GPU needed) the tile counts of the train frames, both classes present; the query frames stored as given; this file's
    statement of the subsets gives the numbers of the two-tiles test's."""
    descs = _frames(256)
    assert [T._tiles(d) for d in descs[:len(TRAIN)]] == TRAIN_TILES
    for d, (e, o) in zip(descs, TRAIN):
        assert int((((d.astype(np.int64) - 128) ** 2).sum(1) % 2 == 0).sum()) == e and d.shape[0] == e + o
    for d, m in zip(descs[len(TRAIN):], QUERY):
        assert d.shape[0] == m and np.array_equal(L._stored_pos(d), np.arange(m))
    for a, b in ((len(TRAIN) + 8, 8), (len(TRAIN) + 12, 4), (len(TRAIN) + 13, 7)):
        for mine, theirs in zip(_model(descs[a], descs[b]), T._model(descs[a], descs[b])):
            assert np.array_equal(mine, theirs)
    for full in (False, True):
        met = {}
        for a, b in _pairs(full):
            met.setdefault(int(a), set()).add(TRAIN_TILES[b])
        assert set(met) == set(range(len(TRAIN), len(descs)))
        assert all({t & 1 for t in ts} == {0, 1} for ts in met.values())              # every query frame meets both peel cases
        assert set().union(*met.values()) == set(TRAIN_TILES)


@pytest.mark.parametrize("dim", [129, 160, 192, 224, 255, 256])
def test_every_query_edge_and_tile_count(dim):
    """At 256-D every query size against four or five tile counts; below, where the last K blocks are partly or wholly code 0 on both
    sides, against two."""
    descs, pairs = _frames(dim), _pairs(dim == 256)
    got, opens, tally = _three_ways(descs, pairs)
    assert got[0].sum() > 300 and 0 < sum(opens) < tally[0]     # rows do match, and the screen closes rows


BINARY_TRAIN = [(40, 0), (33, 30), (70, 50), (96, 65)]      # (rows of even, rows of odd popcount): 2, 3, 5 and 6 stored tiles


def _binary_frames(nbytes):
    """Frames 0 .. 3: train frames of both parity classes interleaved (the parity of a row's centred norm is that of its popcount).
    Frames 4 .. 6: query frames of 17, 49 and 65 rows with the parities they happen to have."""
    sizes = [e + o for e, o in BINARY_TRAIN] + [17, 49, 65]
    base = HC._bytes(SEED, nbytes, (max(sizes), nbytes))
    descs = [base[:n] ^ HC._flips(SEED, 40 + 16 * nbytes + k, (n, nbytes), 0.04) for k, n in enumerate(sizes)]
    for d, (e, o) in zip(descs, BINARY_TRAIN):
        d[:, 0] ^= ((R.popcount(d) & 1) ^ np.array(_mixed(e, o))).astype(np.uint8)
    pairs = np.array([[q, t] for q in (4, 5, 6) for t in range(4)] + [[3, 6]], dtype=np.int32)
    return descs, pairs[np.argsort(pairs[:, 1], kind="stable")]


def test_binary_frames_of_160_and_256_bits():
    """METRIC = 1 of the same loop. Train frames of both parity classes (2, 3, 5 and 6 tiles), query frames around the sub-tile edges."""
    for nbytes in (20, 32):
        descs, pairs = _binary_frames(nbytes)
        assert [T._tiles(R.embed(d)) for d in descs[:4]] == [2, 3, 5, 6]
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
        assert out[None][0].sum() > 50


# stored positions (tile, row) of a planted minimum and runner-up; every pair is planted in both orders
PLANTS = [
    ((3, 8), (3, 10)),      # the same group of four
    ((4, 1), (4, 3)),
    ((3, 21), (3, 25)),     # rows r and r + 4: neighbouring groups
    ((5, 2), (5, 6)),
    ((4, 15), (4, 16)),     # both sides of row 15 / 16: the two row halves
    ((6, 13), (6, 18)),
    ((1, 5), (3, 5)),       # tiles of equal parity: the same subset when the groups agree
    ((2, 30), (8, 29)),
    ((1, 12), (2, 12)),     # tiles of opposite parity
    ((7, 0), (10, 17)),
    ((0, 9), (6, 9)),       # across a ring wrap: tiles v and v + 6 share a slot (with the front peel: v - 1 and v + 5)
    ((5, 27), (11, 24)),
    ((0, 16), (12, 15)),    # the first tile (peeled when the count is even) and the last
]


def _planted(ntiles):
    """A train frame of `ntiles` full tiles, all rows of even parity (stored as given), and two query rows per entry of PLANTS. The
    two positions of an entry hold two neighbours of one random vector (noise of 5 per value); query row 2 k is a close copy (noise
    of 1.5) of the row at the first position, so that one is its minimum and the other position its runner-up, and query row
    2 k + 1 a close copy of the row at the second position: the same two with the roles swapped. Unrelated random rows are far from
    everything (several times the neighbours' distance)."""
    n, dim = 32 * ntiles, 256
    train = synth.random_u8_descriptors(n, dim, SEED, 3)
    centre = synth.random_u8_descriptors(len(PLANTS), dim, SEED, 4)
    near = lambda v, k, amp: np.clip(v + np.rint(amp * synth.rng_normal(SEED, 100 + k, (dim,))), 0, 255)
    query = np.zeros((2 * len(PLANTS), dim))
    for k, (p, q) in enumerate(PLANTS):
        for i, (tile, row) in enumerate((p, q)):
            train[32 * tile + row] = near(centre[k], 4 * k + i, 5.0)
    train = S._with_norm_parity(train.astype(np.float32), [0] * n)
    for k, (p, q) in enumerate(PLANTS):
        for i, (tile, row) in enumerate((p, q)):
            query[2 * k + i] = near(train[32 * tile + row], 4 * k + 2 + i, 1.5)
    return S._with_norm_parity(query.astype(np.float32), [0] * query.shape[0]), train


@pytest.mark.parametrize("ntiles", [13, 14])
def test_planted_minimum_and_runner_up(ntiles):
    """Both peel cases. The model's own n says the plants are where they were put; the sweep's words then say that the two rows were
    folded into the right subsets: equal subsets leave u to a third row far away, different ones give u = the runner-up's n
    (a runner-up folded into the wrong subset shows as the other value of u, a minimum as another n1)."""
    query, train = _planted(ntiles)
    assert T._tiles(train) == ntiles and np.array_equal(L._stored_pos(train), np.arange(train.shape[0]))
    n, mins = _subset_minima(query, train)
    order = np.argsort(n, axis=1, kind="stable")
    same = 0
    for k, (p, q) in enumerate(PLANTS):
        for swap in (0, 1):
            first, second = (q, p) if swap else (p, q)
            r = 2 * k + swap
            assert (order[r, 0], order[r, 1]) == (32 * first[0] + first[1], 32 * second[0] + second[1]), (k, swap)
            sub = lambda t: 8 * (t[0] & 1) + (t[1] >> 2)
            u = np.sort(mins[r])[1]
            if sub(first) == sub(second):
                same += 1
                assert u > 4 * n[r, order[r, 1]]
            else:
                assert u == n[r, order[r, 1]]
    assert same >= 6
    descs = [query, train]
    pairs = np.array([[0, 1], [1, 0]], dtype=np.int32)
    got, opens, _ = _three_ways(descs, pairs)
    assert opens[0] >= 2 * len(PLANTS) - same


def _level_frames(ntiles):
    """[query, train]: train rows of `ntiles` full tiles (even parity: stored as given) whose values lie at an amplitude about the
    centre that grows fourfold per level, the level 1 + (bit 2 of the row) + 2 (bit 4 of the row); 64 query rows, noisy copies of
    train rows of every level."""
    n, dim = 32 * ntiles, 256
    row = np.arange(n) & 31
    level = 1 + ((row >> 2) & 1) + 2 * ((row >> 4) & 1)
    amp = np.array([0.0, 3.0, 12.0, 48.0, 160.0])[level]
    sign = np.where(synth.rng_uniform(SEED, 7, (n, dim)) < 0.5, -1.0, 1.0)
    mag = amp[:, None] * (0.5 + 0.5 * synth.rng_uniform(SEED, 8, (n, dim)))
    train = S._with_norm_parity(np.clip(np.rint(64.0 + sign * mag), 0, 255).astype(np.float32), [0] * n)
    rows = (3 + 7 * np.arange(64)) % n
    query = np.clip(train[rows] + np.rint(2.0 * synth.rng_normal(SEED, 9, (64, dim))), 0, 255).astype(np.float32)
    return [S._with_norm_parity(query, [0] * 64), train]


def test_constants_that_differ_by_level():
    """Train rows whose |M_b|^2 / 2 — the constant a chain starts on — grows more than eightfold per level (_level_frames): rows r,
    r + 4 and r + 16 never share one. A constant taken from the wrong group or row half moves n of that row by more than any true
    distance between neighbours here, so n1 of the rows nearest to it changes. Three tiles and five (odd counts) and four (the
    peeled tile too)."""
    for ntiles in (3, 4, 5):
        descs = _level_frames(ntiles)
        train, n = descs[1], 32 * ntiles
        m2 = (L._M[train.astype(np.int64)].astype(np.int64) ** 2).sum(1)
        for r in range(n - 16):
            if (r & 31) < 12 and not (r & 4):
                assert 8 * m2[r] < m2[r + 4] and 8 * m2[r + 4] < m2[r + 16], r
        assert np.array_equal(L._stored_pos(train), np.arange(n))
        got, opens, _ = _three_ways(descs, np.array([[0, 1]], dtype=np.int32))
        assert got[0].sum() > 20
