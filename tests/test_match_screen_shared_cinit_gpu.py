"""GPU: the constants that start the chains of the screen sweep above 128-D (match_screen_kernel, eacham_amd/csrc/matcher.hip).
A chain on a train tile starts from |M_b|^2 / 2 of its 32 rows; a lane's sixteen values depend on the tile and on the lane's half
alone, so the kernel reads ONE set per train tile and hands it to the first MFMA of both query sub-tiles of the wave. What that can
get wrong, and a result must show: a sub-tile starting on the constants of another tile (a wrong ring slot), on those of the other
half (rows r and r ^ 4), on registers whose read had not landed, or on registers already given away.

So every case here runs on train frames whose constants differ strongly between the rows r and r + 4 of every group of eight and
between every tile and the six tiles behind it (a ring of six slots), of T = 1 .. 13 tiles with a full and a ragged last tile each
(T = 10 .. 13: a whole trip of three calls followed by two, by none and by one tail call), all rows forced to one parity of the
centred squared norm so that stored order is given order; against query frames of 1, 32, 33, 64, 65, 97, 129 and 257 rows of mixed
parities (second sub-tile absent, partly filled, a wave with its first sub-tile only, a second workgroup). Per pair and dimension:

  * {n1, L1, U2} of eacham_match_debug_screen_pair for every row against the numpy statement of the bound, and the tally and item
    count of the call (test_match_screen_two_tiles_gpu._model / _check_sweep);
  * the match graph against the CPU oracle and against a context under EACHAM_MATCH_SWEEP_FORM=exact, bytes for bytes;
  * one binary case under Hamming (256 bits, T = 11): METRIC = 1 of the same loop.

test_the_frames_can_see_wrong_constants (no GPU) proves that these inputs see each of the errors: it recomputes the model's n1 with
the constants of tile t taken from tile t + 1, from tile t + 2 (the ring's own rule past the end: the last tile again), with rows r
and r ^ 4 swapped, and with zeros, and holds that each of the four changes n1 for more than half of the query rows of every pair
with T >= 2, counted separately over the rows of first sub-tiles (stored row % 64 < 32) and of second sub-tiles."""
import functools

import numpy as np
import pytest

from eacham_amd import synth
import ham_reference as R
import oracle_api as O
import test_match_screen_gpu as S
import test_match_screen_list_gpu as L
import test_match_screen_two_tiles_gpu as W

SEED = 1913
TMAX = 13
RAGGED = [1, 5, 9, 13, 17, 21, 25, 29, 31, 3, 7, 11, 30]          # rows of the ragged last tile of the frame of T tiles
TRAIN = [n for T in range(1, TMAX + 1) for n in (32 * T, 32 * (T - 1) + RAGGED[T - 1])]
QUERY = [1, 32, 33, 64, 65, 97, 129, 257]
# |M_b|^2 of a row as a share of the base frame's median: fourteen levels in steps of 6 % of the largest
LEVEL2 = np.linspace(0.2, 1.0, 14)


def _level(rows):
    """Level of a stored train row: its tile modulo seven (no two of seven consecutive tiles share one) and bit 2 of its row (rows
    r and r + 4 of a group of eight are seven levels apart)."""
    rows = np.asarray(rows)
    return (rows >> 5) % 7 + 7 * ((rows >> 2) & 1)


def _source(i):
    """The train row that query row i copies: every third one a row of tile 0, the others spread over all thirteen tiles (a last
    tile keeps its own constants under the tile shifts, so a frame of two tiles needs more than half of the minima in its first)."""
    i = np.asarray(i)
    return np.where(i % 3 == 0, (11 * i) % 32, (37 * i + 5) % (32 * TMAX))


def _scaled_to_level(base):
    """Every row scaled about the grid's zero (value 64) so that its |M|^2 is its level's share of the median |M|^2 of the unscaled
    rows: bisection on the scale (|M|^2 does not fall as the scale grows), which lands within a code step or two of the target."""
    def m2(x):
        m = L._M[x.astype(np.int64)]
        return (m * m).sum(1)

    def at(scale):
        return np.clip(np.rint(64.0 + scale[:, None] * (base - 64.0)), 0, 255)
    target = LEVEL2[_level(np.arange(base.shape[0]))] * np.median(m2(base))
    lo, hi = np.zeros(base.shape[0]), np.full(base.shape[0], 2.0)
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        below = m2(at(mid)) < target
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return at(hi).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _frames(dim):
    """Frames 0 .. 25: the first n rows of one base frame scaled to its rows' levels, all rows even (k even) or all odd.
    Frames 26 .. 33: the query sizes, noisy copies of the rows _source names, with the parities they happen to have."""
    base = synth.random_u8_descriptors(32 * TMAX, dim, SEED, 0).astype(np.float64)
    scaled = _scaled_to_level(base)
    descs = [S._with_norm_parity(scaled[:n], [k % 2] * n) for k, n in enumerate(TRAIN)]
    for k, n in enumerate(QUERY):
        noise = np.rint(6.0 * synth.rng_normal(SEED, 20 + k, (n, dim)))
        descs.append(np.clip(scaled[_source(np.arange(n))] + noise, 0, 255).astype(np.float32))
    for d in descs:
        d.setflags(write=False)
    return tuple(descs)


@functools.lru_cache(maxsize=None)
def _pairs():
    """(query, train), grouped by train frame: every train frame against the 257-row query frame; the other seven query sizes
    against the two frames of every tile count between them (three the full one, four the ragged one)."""
    nt, q257 = len(TRAIN), len(TRAIN) + QUERY.index(257)
    others = [len(TRAIN) + i for i, n in enumerate(QUERY) if n != 257]
    pairs = [[q, t] for t in range(nt) for q in [q257] + [others[(3 * t + j) % 7] for j in range(3 + t % 2)]]
    return np.array(pairs, dtype=np.int32)


def _minimum(Da, Db, constants):
    """n1 of every row of Da against the train frame Db (stored as given) with `constants`[t, r] in the place of |M_b|^2 of stored
    row 32 t + r: inf drops the row, as a padding row's constant does."""
    Fa, Fb = L._M[Da.astype(np.int64)].astype(np.float64), L._M[Db.astype(np.int64)].astype(np.float64)
    n = (Fa * Fa).sum(1)[:, None] + constants.reshape(-1)[None, :Db.shape[0]] - 2.0 * (Fa @ Fb.T)
    return n.min(1)


def _constants(Db):
    """|M_b|^2 by [tile, row], inf on the padding rows of the last tile."""
    Fb = L._M[Db.astype(np.int64)].astype(np.float64)
    T = -(-Db.shape[0] // 32)
    c = np.full(32 * T, np.inf)
    c[:Db.shape[0]] = (Fb * Fb).sum(1)
    return c.reshape(T, 32)


def _wrong_constants(c):
    """The four errors: the constants of the next tile, of the tile after next (past the end the last tile again, as the ring holds
    it), of the other half, and none."""
    T = c.shape[0]
    t = np.arange(T)
    return {"tile t + 1": c[np.minimum(t + 1, T - 1)], "tile t + 2": c[np.minimum(t + 2, T - 1)],
            "rows r ^ 4": c[:, np.arange(32) ^ 4], "zero": np.where(np.isfinite(c), 0.0, np.inf)}


def _shares_changed(Da, Db):
    """{error: (share of the first sub-tiles' rows whose n1 changes, share of the second sub-tiles' rows)}; nan for no such row."""
    assert np.array_equal(L._stored_pos(Db), np.arange(Db.shape[0]))
    c = _constants(Db)
    right = _minimum(Da, Db, c)
    assert np.array_equal(right.astype(np.uint32), W._model(Da, Db)[0])     # the statement the GPU cases are held to
    second = L._stored_pos(Da) % 64 >= 32
    out = {}
    for what, wrong in _wrong_constants(c).items():
        changed = _minimum(Da, Db, wrong) != right
        out[what] = tuple(float(changed[sel].mean()) if sel.any() else float("nan") for sel in (~second, second))
    return out


def _bits_frames():
    """Packed rows of 256 bits: a train frame of T = 11 tiles (340 rows, even popcounts: one parity class) whose rows have a bit
    density by their level, so that |M_b|^2 = 256 zeros + 2304 ones differs as the float frames' does; queries of 257 and 65 rows."""
    n = 340
    density = np.linspace(0.15, 0.85, 14)[_level(np.arange(32 * TMAX))]
    bits = synth.rng_uniform(SEED, 70, (32 * TMAX, 256)) < density[:, None]
    train = np.packbits(bits[:n], axis=-1)
    train[:, 0] ^= (R.popcount(train) & 1).astype(np.uint8)
    descs = [train]
    for k, nq in enumerate((257, 65)):
        src = bits[_source(np.arange(nq)) % n]
        flips = synth.rng_uniform(SEED, 80 + k, (nq, 256)) < 0.04
        descs.append(np.packbits(src ^ flips, axis=-1))
    return descs


def test_the_cases_cover_what_they_claim():
    """(no GPU needed) T = 1 .. 13, full and ragged; every query size against T = 10 .. 13; constants of rows r and r + 4 and of a
    tile and the six behind it more than 4 % of the largest apart (the levels are 6 % apart, a row is within a per cent of its level)."""
    descs, pairs = _frames(256), _pairs()
    T = [W._tiles(d) for d in descs[:len(TRAIN)]]
    assert T == [-(-n // 32) for n in TRAIN] and sorted(set(T)) == list(range(1, TMAX + 1))
    assert {n % 32 == 0 for n in TRAIN} == {True, False}
    for tiles in range(10, TMAX + 1):
        assert {descs[a].shape[0] for a, b in pairs if T[b] == tiles} == set(QUERY)
    assert any(len({int(x) for x in (((d.astype(np.int64) - 128) ** 2).sum(1) % 2)}) == 2 for d in descs[len(TRAIN):])
    c = _constants(descs[TRAIN.index(32 * TMAX)])
    step = 0.04 * c.max()
    assert np.abs(c - c[:, np.arange(32) ^ 4]).min() > step
    for k in range(1, 7):
        assert np.abs(c[k:] - c[:-k]).min() > step


@pytest.mark.parametrize("dim", [129, 192, 256])
def test_the_frames_can_see_wrong_constants(dim):
    """(no GPU needed) each of the four errors changes n1 for more than half of the rows of either kind of sub-tile, in every pair
    with T >= 2."""
    descs, pairs = _frames(dim), _pairs()
    low = {}
    for a, b in pairs:
        if descs[b].shape[0] <= 32:
            continue
        for what, shares in _shares_changed(descs[a], descs[b]).items():
            for kind, share in zip(("first", "second"), shares):
                if share == share:
                    low[what, kind] = min(low.get((what, kind), 1.0), share)
                    assert share > 0.5, (what, kind, descs[a].shape[0], descs[b].shape[0], share)
    print(f"dim {dim}: smallest share of rows whose n1 changes, over the pairs: "
          + ", ".join(f"{w} / {k} sub-tiles {s:.3f}" for (w, k), s in sorted(low.items())))
    assert len(low) == 8


def test_the_binary_frames_can_see_wrong_constants():
    """(no GPU needed) the same for the Hamming case's frames."""
    descs = [R.embed(d) for d in _bits_frames()]
    for q in (1, 2):
        for what, shares in _shares_changed(descs[q], descs[0]).items():
            print(f"{descs[q].shape[0]} rows, {what}: {shares}")
            assert min(shares) > 0.5, (what, shares)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [129, 192, 256])
def test_every_tile_count_against_every_query_shape(dim):
    descs, pairs = list(_frames(dim)), _pairs()
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
        W._bytes_equal(got, want, "oracle")
        W._bytes_equal(got, exact, "exact form")
        opens = W._check_sweep(ctx, descs, pairs, tally, starts)
    assert got[0].sum() > 1000 and 0 < sum(opens) < tally[0]    # rows do match, and the screen closes rows


@pytest.mark.gpu
def test_binary_frames_under_hamming():
    descs = _bits_frames()
    assert W._tiles(R.embed(descs[0])) == 11
    pairs = np.array([[1, 0], [2, 0]], dtype=np.int32)
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
                W._check_sweep(ctx, descs, pairs, tally, starts, hamming=True, embed=R.embed)
            else:
                assert tally == (0, 0, 0)
    for g, w, e in zip(out[None][:5], want[:5], out["exact"][:5]):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes() == e.tobytes()
    assert out[None][0].sum() > 100
