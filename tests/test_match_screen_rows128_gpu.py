"""GPU: the screen sweep above 128-D with 128 query rows per wave (match_screen_kernel, eacham_amd/csrc/matcher.hip): a wave owns two
wave-blocks of 64 rows and eight sub-tiles, a workgroup 512 rows, and there is one set of accumulators whose row halves are
consumed under the step behind the one that ended their chains. None of that may show in a result — the tail still runs per
wave-block — so every case holds what tests/test_match_screen_two_tiles_gpu.py holds, on the shapes at which this form takes another
path:

  * query frames of 1 .. 600 rows: a wave with one real sub-tile (1, 16), a sub-tile boundary (17), a wave-block boundary (64, 65:
    the wave's second wave-block has no tile of the frame), a wave boundary (127, 128, 129), a workgroup boundary (511, 512, 513:
    the second workgroup has inactive waves that still stage) and a frame of mixed parities past it (600);
  * train frames of meta[2] = 1, 2, 3, 6, 7, 8 tiles: the front peel and none, fewer tiles than the prologue stages, no call at all
    (1, 2: the prologue's plain minima and last() alone), one call (3, 4 behind the peel), the ring wrapping once (7, 8);
  * dimensions 129, 160, 255, 256, binary rows of 160 and 256 bits, and one job through two workspace slots.

Each case: the match graph byte for byte that of a context under EACHAM_MATCH_SWEEP_FORM=exact and the CPU oracle's; {n1, L1, U2}
of eacham_match_debug_screen_pair against the numpy statement of the sixteen subsets; (rows, open, items) of the call against what
that statement leaves open."""
import numpy as np
import pytest

from eacham_amd import synth
import ham_cases as HC
import ham_reference as R
import oracle_api as O
import test_match_screen_gpu as S
import test_match_screen_list_gpu as L
from test_match_screen_two_tiles_gpu import _bytes_equal, _check_sweep, _model, _tiles  # noqa: F401  (_model: what _check_sweep holds the entry to)

pytestmark = pytest.mark.gpu
SEED = 1311
TRAIN = [20, 64, 90, 192, 200, 256]                                  # 1, 2, 3, 6, 7, 8 tiles (one parity class each)
QUERY = [1, 16, 17, 64, 65, 127, 128, 129, 511, 512, 513, 600]
TRAIN_TILES = [1, 2, 3, 6, 7, 8]


def _frames(dim):
    """Frames 0 .. 5: the train sizes, noisy copies of one base frame, all rows even (k even) or all odd (k odd). Frames 6 .. 17: the
    query sizes, noisy copies of the same base with the parities they happen to have."""
    base = synth.random_u8_descriptors(max(TRAIN + QUERY), dim, SEED, 0)
    descs = []
    for k, n in enumerate(TRAIN + QUERY):
        D = np.clip(base[:n] + np.rint(6.0 * synth.rng_normal(SEED, 20 + k, (n, dim))), 0, 255).astype(np.float32)
        descs.append(S._with_norm_parity(D, [k % 2] * n) if k < len(TRAIN) else D)
    return descs


def _pairs():
    """Every query size against every train tile count, grouped by train frame."""
    nt = len(TRAIN)
    pairs = np.array([[nt + i, t] for t in range(nt) for i in range(len(QUERY))], dtype=np.int32)
    return pairs[np.argsort(pairs[:, 1], kind="stable")]


def test_the_cases_cover_what_they_claim():
    """(no GPU needed) the train frames have the tile counts named above, and every query size meets every one of them."""
    descs, pairs = _frames(256), _pairs()
    assert [_tiles(d) for d in descs[:len(TRAIN)]] == TRAIN_TILES
    assert [d.shape[0] for d in descs[len(TRAIN):]] == QUERY
    assert {(descs[a].shape[0], _tiles(descs[b])) for a, b in pairs} == {(q, t) for q in QUERY for t in TRAIN_TILES}


@pytest.mark.parametrize("dim", [129, 160, 255, 256])
def test_every_query_shape_against_every_tile_count(dim):
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
    """Packed rows of 160 and of 256 bits: METRIC = 1 of the same loop. Train frames of 1 .. 8 tiles (an even number of set bits in
    every row: one parity class), query frames of 513, 129 and 65 rows."""
    for nbytes in (20, 32):
        sizes = TRAIN + [513, 129, 65]
        nt = len(TRAIN)
        base = HC._bytes(SEED, nbytes, (max(sizes), nbytes))
        descs = []
        for k, n in enumerate(sizes):
            rows = base[:n] ^ HC._flips(SEED, 40 + 16 * nbytes + k, (n, nbytes), 0.04)
            if k < nt:
                rows[:, 0] ^= (R.popcount(rows) & 1).astype(np.uint8)     # an even popcount: the parity of the centred norm
            descs.append(rows)
        assert [_tiles(R.embed(d)) for d in descs[:nt]] == TRAIN_TILES
        pairs = np.array([[nt + i, t] for t in range(nt) for i in range(3)] + [[3, nt]], dtype=np.int32)
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


def test_a_job_through_two_slots():
    """EACHAM_MATCH_BUDGET_MB=16 with one resident frame of 4000 rows that no pair names (a launch's workspace is sized by the
    largest resident frame: about 210 KB per pair, so a launch holds fewer than 80): the 153 pairs of the 18 frames go through at
    least two launches and both workspace slots, and the grid of a launch is that of workgroups of 512 rows over a stride of 4000
    rows and more."""
    descs = _frames(256)
    big = synth.random_u8_descriptors(4000, 256, SEED, 9).astype(np.float32)
    pairs = synth.all_pairs(len(descs))
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
