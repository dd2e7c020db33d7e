"""GPU: the train tiles of the screen sweep above 128-D (match_screen_kernel, eacham_amd/csrc/matcher.hip). A frame's rows are stored
sorted by the parity of their centred squared norm, each class in whole 32-row tiles, and the tiles in use (meta[1]) are rounded up
to whole wave-blocks of two tiles. The sweep covers a train frame's tiles up to the last one that holds a real row (meta[2],
finish_screen_kernel): where the two differ the last tile is padding alone. None of that may show in a result. Held here on frames
whose rows have forced parities, as (even, odd) row counts:

    (1, 1) (32, 32) (48, 49) (40, 0) (0, 40)   real tiles 2, 2, 4, 2, 2: nothing rounded
    (33, 31) (31, 33) (1, 0)                   real tiles 3, 3, 1 of 4, 4, 2 in use: the last tile is padding alone
    an empty frame, on either side
    one class of 32 k - 3 rows, k = 1 .. 8, 13 every real tile count of that list: each call instantiation, both remainders of the
                                               trip of three calls, odd counts (a padding tile behind them) and even ones

and on copies of a train row of the LAST real tile (its first and its last real position) planted in the boundary rows of a query
frame (its last even row, its first and its last odd row in the stored order). On every pair:

  * counts and edges are those of a context under EACHAM_MATCH_SWEEP_FORM=exact and of the CPU oracle, byte for byte;
  * n1 of eacham_match_debug_screen_pair is the numpy integer minimum of |M_a - M_b|^2 for every real query row, in the caller's
    numbering; 0 <= L1 <= the true minimum; U2 >= the true runner-up, or -1 exactly where the train frame's rows lie in one of the
    sweep's subsets (tile parity x group of four stored rows);
  * match_screen() counts exactly the real query rows, and every row that passes the ratio test in numpy is left open;
  * on the S200-derived frames of tests/test_match_screen_gpu.py the open rows number at most the passing rows + 5 % of the real
    rows (that test's cap);
  * binary frames of 160 and of 256 bits through the Hamming calls.

Every assertion holds with the padding tile swept too: the file passes on a library from before the change."""
import contextlib
import os

import numpy as np
import pytest

from eacham_amd import synth
import ham_reference as R
import oracle_api as O

pytestmark = pytest.mark.gpu
SEED = 2311
SHAPES = [(1, 1), (32, 32), (48, 49), (40, 0), (0, 40), (33, 31), (31, 33), (1, 0), (0, 0)]
COUNTS = [1, 2, 3, 4, 5, 6, 7, 8, 13]
QUERIES = [2, 5, 0, 7, 8, len(SHAPES) + len(COUNTS) - 1]      # (48, 49), (33, 31), (1, 1), (1, 0), empty, 13 tiles (two workgroups)


@contextlib.contextmanager
def _context(form=None):
    """A context of its own created under EACHAM_MATCH_SWEEP_FORM=form (read once, at eacham_ctx_create); None: the default."""
    from eacham_amd import HipContext
    old = os.environ.get("EACHAM_MATCH_SWEEP_FORM")
    os.environ.pop("EACHAM_MATCH_SWEEP_FORM", None)
    if form is not None:
        os.environ["EACHAM_MATCH_SWEEP_FORM"] = form
    try:
        ctx = HipContext(0)
    finally:
        os.environ.pop("EACHAM_MATCH_SWEEP_FORM", None)
        if old is not None:
            os.environ["EACHAM_MATCH_SWEEP_FORM"] = old
    try:
        yield ctx
    finally:
        ctx.close()


def _with_norm_parity(D, parity):
    """Forces the parity of every row's centred squared norm (the parity of its count of odd values): 0 / 1 per row."""
    D = D.copy()
    odd = (D.astype(np.int64) % 2).sum(1) % 2
    for r in range(D.shape[0]):
        if odd[r] != parity[r]:
            D[r, 0] += 1 if D[r, 0] < 255 else -1
    return D


def _parities(even, odd, stream):
    """`even` zeros and `odd` ones in a fixed shuffled order: the caller's numbering is not the stored one."""
    par = np.array([0] * even + [1] * odd, dtype=np.int64)
    return par[np.argsort(synth.rng_uniform(SEED, 300 + stream, (even + odd,)), kind="stable")]


def _class_sizes():
    return SHAPES + [((32 * k - 3, 0) if k % 2 == 0 else (0, 32 * k - 3)) for k in COUNTS]


def _frames(dim):
    """Frame k = noisy copies of the first rows of one base frame with the parities of _class_sizes()[k]: frames that match one another."""
    sizes = _class_sizes()
    base = synth.random_u8_descriptors(max(e + o for e, o in sizes), dim, SEED, 0)
    descs = []
    for k, (e, o) in enumerate(sizes):
        n = e + o
        D = np.clip(base[:n] + np.rint(6.0 * synth.rng_normal(SEED, 20 + k, (n, dim))), 0, 255).astype(np.float32)
        descs.append(_with_norm_parity(D, _parities(e, o, k)))
    return descs


def _pairs(nf, queries):
    pairs = np.array([[a, b] for a in queries for b in range(nf) if a != b], dtype=np.int32)
    return pairs[np.argsort(pairs[:, 1], kind="stable")]


def _even(D):
    return ((D.astype(np.int64) - 128) ** 2).sum(1) % 2 == 0


def _stored_pos(D):
    """Stored position of every row (partition_kernel): the rows of even centred squared norm first, in order, in whole tiles."""
    even = _even(D)
    even_pad = (int(even.sum()) + 31) // 32 * 32
    return np.where(even, np.cumsum(even) - 1, even_pad + np.cumsum(~even) - 1)


def _tiles(D):
    """(tiles that hold a real row, tiles in use) of a frame."""
    even = int(_even(D).sum())
    real = -(-even // 32) + -(-(D.shape[0] - even) // 32)
    return real, (real + 1) // 2 * 2


def _grid_m():
    """M of every value 0..255 (match_screen.hpp): the nearest of 64 + 4 M over the e2m3 grid, the smaller magnitude on a tie."""
    mags = np.array(list(range(16)) + list(range(16, 32, 2)) + list(range(32, 64, 4)))
    ms = np.unique(np.concatenate([mags, -mags]))
    ms = ms[np.argsort(np.abs(ms), kind="stable")]
    x = np.arange(256)[:, None]
    return ms[np.argmin(np.abs(x - (64 + 4 * ms[None, :])), axis=1)].astype(np.int64)


_M = _grid_m()


def _sq_dists(X, Y):
    X, Y = X.astype(np.int64), Y.astype(np.int64)
    return (X * X).sum(1)[:, None] + (Y * Y).sum(1)[None, :] - 2 * (X @ Y.T)


def _ratio_pass(d1, d2, ratio=0.8):
    """FeatureMatcherFlann.cpp:23 as the library restates it: fp32 square roots, fp32 quotient, compared as double."""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.sqrt(d1.astype(np.float32)) / np.sqrt(d2.astype(np.float32))
    return q.astype(np.float64) < ratio


def _check_pair(ctx, Da, Db, a, b, hamming=False):
    """The debug entry's {n1, L1, U2} of the ordered pair against numpy; returns (rows the bounds leave open, rows that pass)."""
    n1, l1, u2 = ctx.match_screen_pair(int(a), int(b))
    d2 = _sq_dists(Da, Db)
    assert n1.shape == l1.shape == u2.shape == (Da.shape[0],)
    assert np.array_equal(n1.astype(np.int64), _sq_dists(_M[Da.astype(np.int64)], _M[Db.astype(np.int64)]).min(1)), ("n1", a, b)
    s = np.sort(d2, axis=1)
    assert np.all(l1 >= 0) and np.all(l1 <= s[:, 0]), ("L1", a, b)
    pos = _stored_pos(Db)
    subsets = len(set((((pos >> 5) & 1) * 8 + ((pos & 31) >> 2)).tolist()))
    if subsets < 2:
        assert np.all(u2 == -1), ("U2 of one subset", a, b)
    else:
        assert np.all(u2 >= s[:, 1]), ("U2", a, b)
    test = (lambda x, y: R.ratio_pass(x, y, 0.8)) if hamming else _ratio_pass
    is_open = (u2 < 0) | test(l1, np.maximum(u2, 0))
    ok = test(s[:, 0], s[:, 1]) if Db.shape[0] > 1 else np.zeros(Da.shape[0], bool)
    assert np.all(is_open[ok]), ("a passing row is closed", a, b)
    return int(is_open.sum()), int(ok.sum())


def _bytes_equal(got, want, what):
    for name, g, w in zip(["counts", "offsets", "q", "t"], got[:4], want[:4]):
        w = np.asarray(w)
        assert g.shape == w.shape and g.tobytes() == w.astype(g.dtype).tobytes(), f"{what}: {name} differs"


def _run(descs, pairs, upload="upload_descriptors", match="match_all_pairs", embed=None, hamming=False):
    """The job under the exact form and under the default (the screen form above 128-D); the debug entry on every pair of real frames."""
    emb = embed or (lambda d: d)
    out = {}
    for form in ("exact", None):
        with _context(form) as ctx:
            ctx.clear_descriptors()
            for f, d in enumerate(descs):
                getattr(ctx, upload)(f, d)
            out[form] = getattr(ctx, match)(pairs, 0.8, 1, 0, stats=False)
            tally = ctx.match_screen()
            if form is None:
                assert tally[0] == sum(descs[a].shape[0] for a, _ in pairs), tally      # exactly the real query rows
                opens = passing = 0
                for a, b in pairs:
                    if descs[a].shape[0] and descs[b].shape[0]:
                        o, p = _check_pair(ctx, emb(descs[a]), emb(descs[b]), a, b, hamming)
                        opens, passing = opens + o, passing + p
                    elif descs[a].shape[0]:                                              # no train row: no minimum, no open row
                        _, l1, _ = ctx.match_screen_pair(int(a), int(b))
                        assert np.all(l1 == -1), (a, b)
                assert tally[1] == opens, (tally, opens)
                print(f"rows {tally[0]} open {tally[1]} passing {passing}")
            else:
                assert tally == (0, 0)
    return out[None], out["exact"]


def test_the_cases_cover_what_they_claim():
    """(no GPU needed) the (real, in use) tile counts of the frames; real counts 1 .. 9 and 13 among the train frames, odd ones with
    a padding tile behind them; a mixed frame whose last tile is padding, and mixed frames without one."""
    descs = _frames(256)
    tiles = [_tiles(d) for d in descs]
    assert tiles[:len(SHAPES)] == [(2, 2), (2, 2), (4, 4), (2, 2), (2, 2), (3, 4), (3, 4), (1, 2), (0, 0)]
    assert tiles[len(SHAPES):] == [(k, (k + 1) // 2 * 2) for k in COUNTS]
    assert [(int(_even(d).sum()), int((~_even(d)).sum())) for d in descs] == _class_sizes()
    assert not np.array_equal(_stored_pos(descs[2]), np.arange(97))                     # (the caller's numbering is not the stored one)
    assert descs[QUERIES[-1]].shape[0] > 256 and descs[QUERIES[4]].shape[0] == 0


@pytest.mark.parametrize("dim", [256, 129, 255])
def test_every_real_tile_count(dim):
    descs = _frames(dim)
    queries = QUERIES if dim == 256 else QUERIES[:2]
    pairs = _pairs(len(descs), queries)
    got, exact = _run(descs, pairs)
    _bytes_equal(got, exact, "exact form")
    _bytes_equal(got, O.match_all_pairs(descs, pairs, min_dir=1, min_mutual=0), "oracle")
    assert got[0].sum() > 300                                                            # rows do match


def _planted(dim=256):
    """Train frames (33, 31) (three real tiles of four in use: the last real tile is the odd class's) and (48, 49) (four of four);
    per train frame and per train row at the first / the last real position of its last real tile a query frame (33, 31) whose last
    even row, first odd row and last odd row (stored order) are that train row, up to the one value that sets their parity.
    Returns (descs, pairs, [(query frame, query row, train frame, train row)])."""
    descs = _frames(dim)
    trains, planted = [5, 2], []
    out = [descs[5], descs[2]]
    for ti, t in enumerate(trains):
        T = descs[t]
        pos = _stored_pos(T)
        last = pos >> 5 == (pos >> 5).max()
        for tr in (int(np.argmin(np.where(last, pos, 1 << 30))), int(np.argmax(pos))):
            par = (~_even(descs[5])).astype(np.int64)
            Q = np.clip(descs[5] + np.rint(40.0 * synth.rng_normal(SEED, 70 + len(out), descs[5].shape)), 0, 255).astype(np.float32)
            Q = _with_norm_parity(Q, par)
            qpos, even = _stored_pos(Q), _even(Q)
            rows = [int(np.argmax(np.where(even, qpos, -1))), int(np.argmin(np.where(~even, qpos, 1 << 30))), int(np.argmax(qpos))]
            for r in rows:
                Q[r] = T[tr]
                planted.append((len(out), r, ti, tr))
            out.append(_with_norm_parity(Q, par))
    pairs = np.array(sorted({(q, t) for q, _, t, _ in planted}, key=lambda x: (x[1], x[0])), dtype=np.int32)
    return out, pairs, planted


def test_planted_rows_of_the_last_real_tile():
    descs, pairs, planted = _planted()
    assert [_tiles(d) for d in descs[:2]] == [(3, 4), (4, 4)] and len(pairs) == 4
    for q, r, t, tr in planted:                                                          # the plant is the row's minimum, at distance 0 or 1
        d2 = _sq_dists(descs[q][r:r + 1], descs[t])[0]
        assert int(np.argmin(d2)) == tr and d2[tr] <= 1 and np.sort(d2)[1] > 1000
        assert (_stored_pos(descs[t])[tr] >> 5) == _tiles(descs[t])[0] - 1
    got, exact = _run(descs, pairs)
    _bytes_equal(got, exact, "exact form")
    _bytes_equal(got, O.match_all_pairs(descs, pairs, min_dir=1, min_mutual=0), "oracle")
    with _context() as ctx:                                                              # (three rows share a plant: the directed form keeps all)
        directed = ctx.match_pairs_directed(descs, pairs)
    for p, (a, b) in enumerate(pairs):
        wq, wt = O.match_directed(descs[a], descs[b], 0.8)
        assert directed[p] == dict(zip(wq.tolist(), wt.tolist())), (a, b)
    for qf, r, tf, tr in planted:
        p = int(np.flatnonzero((pairs[:, 0] == qf) & (pairs[:, 1] == tf))[0])
        assert directed[p].get(r) == tr, (qf, r, tf, tr)


def test_open_rows_within_the_cap_of_the_s200_frames():
    """The frames and the cap of test_tally_every_passing_row_open_and_few_others (tests/test_match_screen_gpu.py): four frames of the
    S200 scene + two unstructured ones, 320 rows, all 30 ordered pairs; open rows <= passing rows + 5 % of the real rows."""
    descs, _ = synth.make_frame_descriptors(synth.make_scene(200, 50000, 10), 320, 256, frames=[3, 4, 5, 90])
    descs = [np.asarray(d, dtype=np.float32) for d in descs]
    descs += [synth.random_u8_descriptors(320, 256, 7, 0), synth.random_u8_descriptors(320, 256, 7, 1)]
    pairs = np.array([[a, b] for a in range(6) for b in range(6) if a != b], dtype=np.int32)
    with _context() as ctx:
        for f, d in enumerate(descs):
            ctx.upload_descriptors(f, d)
        ctx.match_all_pairs(pairs, stats=False)
        rows, left_open = ctx.match_screen()
        opens = passing = 0
        for a, b in pairs:
            o, p = _check_pair(ctx, descs[a], descs[b], a, b)
            opens, passing = opens + o, passing + p
    print(f"rows {rows} open {left_open} passing {passing}")
    assert rows == 9600 and left_open == opens
    assert passing <= left_open <= passing + 0.05 * rows


@pytest.mark.parametrize("nbytes", [20, 32])
def test_binary_frames_under_hamming(nbytes):
    """Packed rows of 160 and of 256 bits with forced popcount parities (the parity of the centred norm of a row of 0 / 255)."""
    sizes = [(33, 31), (48, 49), (40, 0), (1, 1), (0, 93), (31, 33)]
    n = max(e + o for e, o in sizes)
    w = synth.rng_u64(SEED, 500 + nbytes, np.arange(n * nbytes, dtype=np.uint64))
    base = (w >> np.uint64(56)).astype(np.uint8).reshape(n, nbytes)
    descs = []
    for k, (e, o) in enumerate(sizes):
        flips = np.packbits(synth.rng_uniform(SEED, 520 + 8 * nbytes + k, (e + o, nbytes, 8)) < 0.04, axis=-1).reshape(e + o, nbytes)
        rows = base[:e + o] ^ flips
        rows[:, 0] ^= ((R.popcount(rows) & 1) ^ _parities(e, o, 40 + k)).astype(np.uint8)
        descs.append(rows)
    assert [_tiles(R.embed(d)) for d in descs] == [(3, 4), (4, 4), (2, 2), (2, 2), (3, 4), (3, 4)]
    pairs = _pairs(len(descs), [0, 1])
    got, exact = _run(descs, pairs, upload="upload_descriptors_bits", match="match_all_pairs_hamming", embed=R.embed, hamming=True)
    want = R.Scene(descs).match_all_pairs(pairs, 0.8, 1, 0)
    for g, w, e in zip(got[:5], want[:5], exact[:5]):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes() == e.tobytes()
    assert got[0].sum() > 100
