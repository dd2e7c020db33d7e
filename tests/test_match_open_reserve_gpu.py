"""GPU: the screen sweep reserves room for its open rows itself (eacham_amd/csrc/matcher.hip: the tail of match_screen_kernel adds a
wave's open rows to its segment's counter, writes its candidates at the position the add returned and creates the item whose first
candidate lies in its range; match_openprep_kernel sets the segment heads and zeroes the counters once per call), and the exact pass
(match_sweep_kernel<8, false, true>) takes a workgroup per item of the dense list.

What may go wrong is the list, not the arithmetic: a candidate lost or written twice, an item missing or doubled where a
reservation straddles a multiple of 256, a counter that survives a call, an item of a long list never visited. Any of these
changes a row's exact {v1, tile, v2} or leaves the screen's bounds in its place, so every case holds the graph (thresholds 30/30 and
min_dir=1, min_mutual=0) and the directed lists byte for byte against a context under EACHAM_MATCH_SWEEP_FORM=exact and against the
CPU oracle, and the call's item tally against sum over launches and segments of ceil(open rows / 256), derived from
eacham_match_debug_screen_pair and eacham_match_debug_batches (test_match_open_pack_gpu._run does all of that).

Inputs are the open-pack test's: a train frame plus query frames with k noisy copied rows; where a case needs an exact number of open
rows, every row of a query is a noisy copy (sigma 3) of a train row: such a row passes the ratio test, so it cannot be closed, and the
pair's open rows are its query rows. Nothing here names an entry point the parent commit lacks."""
import numpy as np
import pytest

from eacham_amd import shard, synth
import ham_cases as HC
import ham_reference as R
import oracle_api as O
import test_match_open_pack_gpu as P
import test_match_screen_list_gpu as L

pytestmark = pytest.mark.gpu
SEED = 930
WIDTH = P.WIDTH


def _copies(sizes, dim=256, seed=SEED):
    """Frame k = the first sizes[k] rows of one base frame + rounded N(0, 3): every row of a pair's smaller frame stays open."""
    return L._noisy_copies(sizes, dim, seed, 3.0)


def _segment_totals(pairs, opens, starts):
    bounds = [int(s) for s in starts] + [len(pairs)]
    totals = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        run = 0
        for p in range(lo, hi):
            run += int(opens[p])
            if p + 1 == hi or pairs[p + 1][1] != pairs[p][1]:
                totals.append(run)
                run = 0
    return totals


@pytest.mark.parametrize("dim", [256, 129])
def test_one_segment_of_many_light_pairs(dim):
    """Sixty pairs (k, T) with a handful of open rows each, query frames of 64 to 200 rows: one segment, its rows in ceil(n / 256)
    items whichever waves reserved first."""
    n = 60
    sizes = [(64, 97, 130, 200)[k % 4] for k in range(n)]
    shared = [1 + k % 7 for k in range(n)]
    descs = P._frames(sizes, shared, dim)
    pairs = [[k, n] for k in range(n)]
    opens, starts, items = P._run(descs, pairs)
    assert len(starts) == 1 and np.all(opens >= np.array(shared)) and opens.max() < 64
    assert items == -(-int(opens.sum()) // WIDTH) and items < (opens > 0).sum() / 8


def test_segment_totals_around_a_multiple_of_256():
    """Segments of 255, 256, 257 and 320 open rows (two train frames alternated, every query row open): the reservation that holds
    candidate 256 creates the second item — none at 255 and 256, one row of it at 257."""
    q = [100, 155, 100, 156, 100, 157, 64, 256]
    descs = _copies(q + [400, 400])
    pairs = [[k, 8 + (k // 2) % 2] for k in range(8)]
    opens, starts, items = P._run(descs, pairs)
    assert opens.tolist() == q and len(starts) == 1
    assert _segment_totals(pairs, opens, starts) == [255, 256, 257, 320]
    assert items == 1 + 1 + 2 + 2


def test_several_items_from_one_pair():
    """One pair of 600-row frames with every row open: ten waves reserve in one segment, three items."""
    descs = _copies([600, 600])
    opens, _, items = P._run(descs, [[0, 1]])
    assert opens.tolist() == [600] and items == 3


def test_unsorted_pair_list():
    """An unsorted list: segments of one pair, a pair given twice in a row, a pair with no open row in the middle of a segment, a
    one-row train frame (no runner-up: every query row open) and an empty frame on either side."""
    descs = L._frames_with_a_dead_pair()                          # 0..2 match one another, (3, 4) leaves no row open
    for k, n in enumerate((64, 100)):                             # 5, 6: noisy copies of rows of frame 4
        descs.append(np.clip(descs[4][:n] + np.rint(6.0 * synth.rng_normal(SEED, 80 + k, (n, 256))), 0, 255).astype(np.float32))
    descs.append(descs[0][5:6].copy())                            # 7: one row
    descs.append(np.zeros((0, 256), np.float32))                  # 8: empty
    pairs = [[0, 2], [5, 4], [3, 4], [6, 4], [1, 2], [0, 1], [2, 1], [2, 1], [0, 7], [8, 0], [1, 0], [0, 8], [2, 0], [7, 0]]
    opens, starts, items = P._run(descs, pairs)
    assert len(starts) == 1
    assert opens[2] == 0 and opens[1] > 0 and opens[3] > 0       # the dead pair inside the segment onto frame 4
    assert opens[6] == opens[7] > 0                               # the pair given twice
    assert opens[8] == descs[0].shape[0] and opens[9] == 0 and opens[11] == 0 and opens[13] == 1
    want = sum(-(-t // WIDTH) for t in _segment_totals(pairs, opens, starts))
    assert items == want >= 7


def test_counters_are_zeroed_per_call_across_launches():
    """EACHAM_MATCH_BUDGET_MB=16 and 56 frames of 600 rows ordered by train frame: at least three launches through two slots and a
    segment cut by a launch boundary. The call runs twice in one context: the same bytes, those of the exact form, and the same
    three tallies — a segment or item counter that survived the first call would double the second call's."""
    nf = 56
    descs, _ = synth.make_frame_descriptors(synth.make_scene(nf, 14000, 10), 600, 256)
    descs = [np.asarray(d, dtype=np.float32) for d in descs]
    pairs = shard.order_pairs(synth.all_pairs(nf))
    with L._context(EACHAM_MATCH_BUDGET_MB=16, EACHAM_MATCH_SWEEP_FORM="exact") as ctx:
        L._upload(ctx, descs)
        exact = ctx.match_all_pairs(pairs, stats=False)
    runs, tallies = [], []
    with L._context(EACHAM_MATCH_BUDGET_MB=16) as ctx:
        L._upload(ctx, descs)
        for _ in range(2):
            runs.append(ctx.match_all_pairs(pairs, stats=False))
            tallies.append(ctx.match_screen() + (ctx.match_screen_items(),))
        starts, slots = ctx.match_batches(len(pairs), stats=False)
        opens = np.array([int(L._open_by_entry(ctx, a, b).sum()) for a, b in pairs])
    assert len(starts) >= 3 and slots == 2, (starts, slots)
    assert any(pairs[s - 1][1] == pairs[s][1] for s in starts[1:])            # a boundary inside a run of one train frame
    want = (sum(descs[a].shape[0] for a, _ in pairs), int(opens.sum()), P._expected_items(pairs, opens, starts))
    print(f"launches at {list(starts)}: (rows, open, items) {tallies}, expected {want}")
    assert tallies[0] == want and tallies[1] == want
    for run in runs:
        for g, w in zip(run[:4], exact[:4]):
            assert g.tobytes() == w.tobytes()
    sample = sorted({0, len(pairs) - 1, *[int(s) - 1 for s in starts[1:]], *[int(s) for s in starts[1:]]})
    ref = O.match_all_pairs(descs, pairs[sample])
    assert np.array_equal(runs[0][0][sample], ref[0]) and runs[0][0].sum() > 30 * nf


def test_more_items_than_one_round_of_workgroups():
    """36 frames of 64 rows, every row open, the 630 pairs in shuffled order: (nearly) every pair is a segment and an item of its own,
    more than 512 items in the one launch — more than one round of the chip's workgroups, the size a persistent exact pass would
    loop at. (The committed exact pass is a workgroup per item, so the case checks the list: hundreds of segments, items of 64 and 128.)"""
    nf = 36
    descs = _copies([64] * nf)
    pairs = synth.all_pairs(nf)[synth.rng_permutation(SEED, 3, nf * (nf - 1) // 2)]
    opens, starts, items = P._run(descs, pairs)
    assert len(starts) == 1 and np.all(opens == 64)
    assert 512 < items <= len(pairs)


def test_the_same_job_three_times():
    """The order of the list is whatever the waves' adds made it; the outputs are not: three runs of the job around the multiple of
    256 in one context give identical bytes, graph and directed lists."""
    q = [100, 155, 100, 156, 100, 157, 64, 256]
    descs = _copies(q + [400, 400])
    pairs = np.array([[k, 8 + (k // 2) % 2] for k in range(8)], np.int32)
    with L._context() as ctx:
        L._upload(ctx, descs)
        graphs = [ctx.match_all_pairs(pairs, min_dir=1, min_mutual=0, stats=False) for _ in range(3)]
        tallies = [ctx.match_screen() + (ctx.match_screen_items(),)]
        directed = [ctx.match_pairs_directed(descs, pairs) for _ in range(3)]
        tallies.append(ctx.match_screen() + (ctx.match_screen_items(),))
    for g in graphs[1:]:
        for x, w in zip(g[:4], graphs[0][:4]):
            assert x.tobytes() == w.tobytes()
    assert directed[1] == directed[0] and directed[2] == directed[0]
    assert graphs[0][0].tolist() == q                             # every query row matches
    assert tallies[0] == tallies[1] == (sum(q), sum(q), 6)


@pytest.mark.parametrize("nbytes", [32, 20])
def test_binary_frames(nbytes):
    """Packed binary rows of 256 and of 160 bits (the Hamming instantiation of the screen kernel): query frames whose every row is a
    train row with 4 % of its bits flipped, one segment of more than 256 open rows; graph (mode 0) and directed lists (mode 1)
    against ham_reference."""
    sizes = [64, 97, 130, 200]
    T = HC._bytes(SEED, 0, (200, nbytes))
    descs = []
    for k, n in enumerate(sizes):
        descs.append(T[(7 * np.arange(n) + 3 * k) % 200] ^ HC._flips(SEED, 40 + k, (n, nbytes), 0.04))
    descs.append(T)
    pairs = np.array([[k, 4] for k in range(4)], np.int32)
    ref = R.Scene(descs)
    with L._context() as ctx:
        ctx.clear_descriptors()
        for f, d in enumerate(descs):
            ctx.upload_descriptors_bits(f, d)
        directed = ctx.match_pairs_directed_hamming(pairs, 0.8)
        tally = ctx.match_screen() + (ctx.match_screen_items(),)
        graphs = [ctx.match_all_pairs_hamming(pairs, 0.8, md, mm, stats=False) for md, mm in P.THRESHOLDS]
        tally_graph = ctx.match_screen() + (ctx.match_screen_items(),)
        opens = np.array([int(P._open_by_entry_hamming(ctx, a, b).sum()) for a, b in pairs])
    for g, w in zip(directed, ref.match_pairs_directed(pairs, 0.8)):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    for got, (md, mm) in zip(graphs, P.THRESHOLDS):
        for g, w in zip(got[:5], ref.match_all_pairs(pairs, 0.8, md, mm)[:5]):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    want = (sum(sizes), int(opens.sum()), -(-int(opens.sum()) // WIDTH))
    print(f"open rows per pair {opens.tolist()}: (rows, open, items) {tally}, expected {want}")
    assert tally == want and tally_graph == want
    assert opens.sum() > WIDTH and directed[0].sum() > WIDTH     # the copied rows do match
