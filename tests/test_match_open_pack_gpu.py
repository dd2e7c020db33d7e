"""GPU: the exact pass behind the screen sweep takes the open rows of MANY pairs per work item (eacham_amd/csrc/matcher.hip:
match_opencount_kernel / match_openscan_kernel / match_openfill_kernel build one packed candidate list per launch and cut it into
items of 256 per run of consecutive pairs onto one train frame; match_sweep_kernel<8, false, true>, the exact sweep with gathered
query rows, reads them, a workgroup per item and 64 candidates per wave).

Every test holds the graph (thresholds 30/30 and min_dir=1, min_mutual=0) and the directed lists byte for byte against a context
created under EACHAM_MATCH_SWEEP_FORM=exact and against the CPU oracle, and the number of items of the call
(eacham_match_debug_screen_items) against the number derived from the per-pair open rows of eacham_match_debug_screen_pair and the
launches of eacham_match_debug_batches: sum over launches, over runs of equal train frame, of ceil(open rows of the run / 256).

Inputs: one train frame T of 200 random rows; query frame k is random rows whose first s_k rows are noisy copies (sigma 6, rounded,
clipped) of rows (7 i + 3 k) mod 200 of T. What a case says about its own shape (a single item for six pairs, a pair cut by an
item boundary, ...) is asserted from those open counts, and where the numpy model of the bound is quick, from the model too."""
import numpy as np
import pytest

from eacham_amd import shard, synth
import ham_cases as HC
import ham_reference as R
import oracle_api as O
import test_match_screen_list_gpu as L

pytestmark = pytest.mark.gpu
SEED = 900
WIDTH = 256         # candidates per item: a workgroup of the gathered exact sweep, 64 per wave
PER_PAIR_WIDTH = 64 # ... and of the per-pair items this list replaces
THRESHOLDS = ((30, 30), (1, 0))


def _train(dim, stream=0):
    return synth.random_u8_descriptors(200, dim, SEED, stream)


def _query(T, k, n, shared, dim):
    """n random rows; the first `shared` are rows (7 i + 3 k) mod 200 of T + rounded N(0, 6), clipped."""
    q = synth.random_u8_descriptors(n, dim, SEED, 10 + k).astype(np.float32)
    src = (7 * np.arange(shared) + 3 * k) % T.shape[0]
    q[:shared] = np.clip(T[src] + np.rint(6.0 * synth.rng_normal(SEED, 40 + k, (shared, dim))), 0, 255)
    return q.astype(np.float32)


def _frames(sizes, shared, dim=256):
    """[query 0, .., query m-1, T]"""
    T = _train(dim).astype(np.float32)
    return [_query(T, k, n, s, dim) for k, (n, s) in enumerate(zip(sizes, shared))] + [T]


def _expected_items(pairs, opens, starts):
    """Items the packed list of a job has: per launch, per maximal run of consecutive pairs with one train frame."""
    bounds = [int(s) for s in starts] + [len(pairs)]
    total = 0
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        run = 0
        for p in range(lo, hi):
            run += int(opens[p])
            if p + 1 == hi or pairs[p + 1][1] != pairs[p][1]:
                total += -(-run // WIDTH)
                run = 0
    return total


def _per_pair_items(opens):
    """What one list per pair costs: the items of the form this one replaces."""
    return int(sum(-(-int(o) // PER_PAIR_WIDTH) for o in opens))


def _run(descs, pairs, env=None):
    """The job through match_pairs_directed and match_all_pairs (both threshold sets) on the screen form (the default above 128-D)
    and on the exact form: the same bytes, the oracle's results. Returns (open rows per pair by the debug entry, launch starts,
    items of the directed call, items of a graph call)."""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    env = env or {}
    out = {}
    for form in ("screen", "exact"):
        with L._context(EACHAM_MATCH_SWEEP_FORM=form, **env) as ctx:
            out[form, "directed"] = ctx.match_pairs_directed(descs, pairs)
            out[form, "tally"] = ctx.match_screen() + (ctx.match_screen_items(),)
            for th in THRESHOLDS:
                out[form, th] = ctx.match_all_pairs(pairs, min_dir=th[0], min_mutual=th[1], stats=False)
            out[form, "tally_graph"] = ctx.match_screen() + (ctx.match_screen_items(),)
            if form == "screen":
                starts, _ = ctx.match_batches(len(pairs), stats=False)
                opens = np.array([int(L._open_by_entry(ctx, a, b).sum()) for a, b in pairs])
    assert out["screen", "directed"] == out["exact", "directed"]
    for k, (a, b) in enumerate(pairs):
        wq, wt = O.match_directed(descs[a], descs[b], 0.8)
        assert out["screen", "directed"][k] == dict(zip(wq.tolist(), wt.tolist())), (a, b)
    for th in THRESHOLDS:
        L._same_graph(out["screen", th], O.match_all_pairs(descs, pairs, min_dir=th[0], min_mutual=th[1]), f"oracle {th}")
        for g, w in zip(out["screen", th][:4], out["exact", th][:4]):
            assert g.tobytes() == w.tobytes()
    rows = sum(descs[a].shape[0] for a, _ in pairs)
    want = (rows, int(opens.sum()), _expected_items(pairs, opens, starts))
    print(f"open rows per pair {opens.tolist()}, launches at {list(starts)}: (rows, open, items) {out['screen', 'tally']}, "
          f"expected {want}, one list per pair {_per_pair_items(opens)} items")
    assert out["screen", "tally"] == want and out["screen", "tally_graph"] == want
    assert out["exact", "tally"] == (0, 0, 0) and out["exact", "tally_graph"] == (0, 0, 0)
    return opens, starts, want[2]


def _cut_by_a_boundary(opens, width):
    """Pairs of ONE run whose candidates [start, start + open) have a multiple of `width` strictly inside: cut by an item boundary."""
    ends = np.cumsum(opens)
    return [p for p, (s, e) in enumerate(zip(ends - opens, ends)) if e > s and (e - 1) // width > s // width and s % width != 0]


@pytest.mark.parametrize("dim", [256, 129])
def test_many_light_pairs_share_one_item(dim):
    """Six pairs (k, T) with one to seven open rows each, six frame sizes from 1 to 200 rows: one item where one list per pair needs six."""
    sizes, shared = [1, 40, 70, 97, 130, 200], [1, 3, 5, 2, 7, 4]
    descs = _frames(sizes, shared, dim)
    pairs = [[k, 6] for k in range(6)]
    if dim == 256:                                              # the premise, from the numpy model of the bound (which restates 256-D)
        model = np.array([int(L._model_open(descs[k], descs[6]).sum()) for k in range(6)])
        assert np.all(model >= 1) and model.sum() <= WIDTH
    opens, _, items = _run(descs, pairs)
    assert np.all(opens >= 1) and opens.sum() <= WIDTH
    assert items == 1 and _per_pair_items(opens) == 6
    assert np.all(opens >= np.array(shared))                    # every shared row matches: it cannot be closed


def test_a_pair_straddles_an_item_boundary():
    """About 200 candidates of six pairs in one run: the 64-candidate boundaries between the waves of an item fall inside pairs."""
    sizes, shared = [40, 70, 97, 130, 200, 200], [20, 30, 25, 40, 35, 50]
    descs = _frames(sizes, shared)
    pairs = [[k, 6] for k in range(6)]
    opens, _, items = _run(descs, pairs)
    assert np.all(opens < 64) and len(_cut_by_a_boundary(opens, 64)) >= 2          # pairs that fit a wave and are cut all the same
    assert items == -(-int(opens.sum()) // WIDTH) and opens.sum() % 64 != 0 and items < _per_pair_items(opens)


def test_a_run_beyond_256_candidates():
    """More than 256 candidates in one run of five pairs, three of them with more than 64 each."""
    sizes, shared = [200, 200, 200, 130, 97], [90, 80, 70, 60, 50]
    descs = _frames(sizes, shared)
    pairs = [[k, 5] for k in range(5)]
    opens, _, items = _run(descs, pairs)
    assert opens.sum() > 256 and (opens > 64).sum() >= 3
    assert len(_cut_by_a_boundary(opens, 256)) == 1             # one pair holds candidate 256 of the run
    assert items == -(-int(opens.sum()) // WIDTH) < _per_pair_items(opens)


def test_pairs_of_many_items():
    """Near-identical frames of 600, 600 and 97 rows: every shared row stays open, so a pair alone fills more than two items, and the
    runs of two pairs (ordered by train frame) start their second pair inside an item."""
    sizes = [600, 600, 97]
    descs = L._noisy_copies(sizes, 256, 7, 3.0)
    pairs = shard.order_pairs(L._ordered(3))
    opens, _, items = _run(descs, pairs)
    assert np.all(opens >= [min(sizes[a], sizes[b]) for a, b in pairs])          # a shared row matches: it cannot be closed
    assert opens.max() > 2 * WIDTH and items >= 3 + 3 + 1
    assert opens[0] > 2 * WIDTH and opens[0] % WIDTH != 0                         # the run onto frame 0: its second pair starts inside an item


def test_list_order():
    """Orders of the pair list that cut the runs: every run of length one (two train frames interleaved), the same pair twice in
    a row, a pair without an open row in the middle of a run, and the reversed pairs (T, k) — a 1-row train frame leaves all 200
    rows open with no runner-up."""
    sizes, shared = [1, 40, 70, 97, 130, 200], [1, 3, 5, 2, 7, 4]
    descs = _frames(sizes, shared)
    descs.append(np.clip(_train(256, 1) + 0.0, 0, 255).astype(np.float32))       # frame 7: a second train frame, unrelated
    descs[2][40:48] = np.clip(descs[7][:8] + np.rint(6.0 * synth.rng_normal(SEED, 70, (8, 256))), 0, 255)   # (rows of it seen by query 2)
    inter = [[k, t] for k in range(6) for t in (6, 7)]
    opens, _, items = _run(descs, inter)
    assert items == sum(-(-int(o) // WIDTH) for o in opens) == (opens > 0).sum() >= 7   # runs of one pair: nothing to share
    twice = [[0, 6], [3, 6], [3, 6], [5, 6], [5, 6], [1, 6]]
    opens, _, items = _run(descs, twice)
    assert opens[1] == opens[2] > 0 and items == 1
    opens, _, items = _run(descs, [[6, k] for k in range(6)])
    assert opens[0] == 200 and np.all(opens[1:] >= 1) and items == sum(-(-int(o) // WIDTH) for o in opens)
    # a pair with no open row inside a run: the train frame of _frames_with_a_dead_pair (every row five times) closes every row
    # of an unrelated query, while noisy copies of its own rows stay open (their lower bound is far below the bound on the runner-up)
    dead = L._frames_with_a_dead_pair()
    for k, n in enumerate((60, 100)):
        dead.append(np.clip(dead[4][:n] + np.rint(6.0 * synth.rng_normal(SEED, 80 + k, (n, 256))), 0, 255).astype(np.float32))
    opens, _, items = _run(dead, [[0, 2], [5, 4], [3, 4], [6, 4], [1, 2]])
    assert opens[2] == 0 and opens[1] > 0 and opens[3] > 0
    assert items == -(-int(opens[0]) // WIDTH) + -(-int(opens[1] + opens[3]) // WIDTH) + -(-int(opens[4]) // WIDTH)


def test_a_run_cut_by_a_launch_boundary():
    """EACHAM_MATCH_BUDGET_MB=16 and 56 frames of 600 rows ordered by train frame: at least three launches through two slots, and
    runs that a launch boundary cuts. The call queued twice with no synchronisation in between gives the same bytes, those of the
    exact form; the oracle's pairs on both sides of every boundary; fewer items than one list per pair."""
    import torch
    nf = 56
    descs, _ = synth.make_frame_descriptors(synth.make_scene(nf, 14000, 10), 600, 256)
    descs = [np.asarray(d, dtype=np.float32) for d in descs]
    pairs = shard.order_pairs(synth.all_pairs(nf))
    with L._context(EACHAM_MATCH_BUDGET_MB=16, EACHAM_MATCH_SWEEP_FORM="exact") as ctx:
        L._upload(ctx, descs)
        exact = ctx.match_all_pairs(pairs, stats=False)
    with L._context(EACHAM_MATCH_BUDGET_MB=16) as ctx:
        L._upload(ctx, descs)
        a = ctx.match_all_pairs(pairs, stats=False)
        tally = ctx.match_screen() + (ctx.match_screen_items(),)
        starts, slots = ctx.match_batches(len(pairs), stats=False)
        assert len(starts) >= 3 and slots == 2, (starts, slots)
        assert any(pairs[s - 1][1] == pairs[s][1] for s in starts[1:])            # a boundary inside a run
        counts, offsets, q, t = a[:4]
        dev = torch.device("cuda", 0)
        with torch.cuda.stream(torch.cuda.ExternalStream(ctx.stream, device=dev)):
            pd = torch.from_numpy(pairs).to(dev)
            outs = [{"counts": torch.zeros(len(pairs), dtype=torch.int32, device=dev),
                     "offsets": torch.zeros(len(pairs) + 1, dtype=torch.int64, device=dev),
                     "edges": torch.zeros(max(len(q), 1) * 2, dtype=torch.int32, device=dev),
                     "total": torch.zeros(1, dtype=torch.int64, device=dev)} for _ in range(2)]
            ctx.sync()
            for o in outs:
                ctx.match_all_pairs_dev(pd.data_ptr(), len(pairs), o["counts"].data_ptr(), o["offsets"].data_ptr(), o["edges"].data_ptr(),
                                        len(q), o["total"].data_ptr())
            ctx.sync()
        for o in outs:
            assert int(o["total"].item()) == len(q)
            assert o["counts"].cpu().numpy().tobytes() == counts.tobytes() and o["offsets"].cpu().numpy().tobytes() == offsets.tobytes()
            e = o["edges"].cpu().numpy().view(np.uint32).reshape(-1, 2)
            assert np.array_equal(e[:len(q), 0], q) and np.array_equal(e[:len(q), 1], t)
        opens = np.array([int(L._open_by_entry(ctx, a_, b_).sum()) for a_, b_ in pairs])
    for x, w in zip(a[:4], exact[:4]):
        assert x.tobytes() == w.tobytes()
    want = (sum(descs[i].shape[0] for i, _ in pairs), int(opens.sum()), _expected_items(pairs, opens, starts))
    print(f"launches at {list(starts)}: (rows, open, items) {tally}, expected {want}, one list per pair {_per_pair_items(opens)} items")
    assert tally == want and tally[2] < _per_pair_items(opens)
    sample = sorted({0, len(pairs) - 1, *[int(s) - 1 for s in starts[1:]], *[int(s) for s in starts[1:]]})
    want = O.match_all_pairs(descs, pairs[sample])
    assert np.array_equal(counts[sample], want[0])
    assert np.array_equal(np.concatenate([q[offsets[p]:offsets[p + 1]] for p in sample]), want[2])
    assert np.array_equal(np.concatenate([t[offsets[p]:offsets[p + 1]] for p in sample]), want[3])
    assert len(q) > 30 * nf


def _open_by_entry_hamming(ctx, a, b):
    """The rows of a binary pair the sweep leaves open: a real minimum and either no bound on the runner-up or bounds that pass the
    Hamming form of the ratio test, (float) L1 / (float) U2 < ratio in double."""
    _, l1, u2 = ctx.match_screen_pair(int(a), int(b))
    return (l1 >= 0) & ((u2 < 0) | R.ratio_pass(l1, np.maximum(u2, 0), 0.8))


def test_binary_frames_of_256_bits():
    """The first case's shape as packed binary rows of 32 bytes (the screen path under the Hamming ratio test), against ham_reference."""
    sizes, shared = [1, 40, 70, 97, 130, 200], [1, 3, 5, 2, 7, 4]
    T = HC._bytes(SEED, 0, (200, 32))
    descs = []
    for k, (n, s) in enumerate(zip(sizes, shared)):
        q = HC._bytes(SEED, 10 + k, (n, 32))
        q[:s] = T[(7 * np.arange(s) + 3 * k) % 200] ^ HC._flips(SEED, 40 + k, (s, 32), 0.04)
        descs.append(q)
    descs.append(T)
    pairs = np.array([[k, 6] for k in range(6)], np.int32)
    ref = R.Scene(descs)
    with L._context() as ctx:
        ctx.clear_descriptors()
        for f, d in enumerate(descs):
            ctx.upload_descriptors_bits(f, d)
        directed = ctx.match_pairs_directed_hamming(pairs, 0.8)
        tally = ctx.match_screen() + (ctx.match_screen_items(),)
        graphs = [ctx.match_all_pairs_hamming(pairs, 0.8, md, mm, stats=False) for md, mm in THRESHOLDS]
        opens = np.array([int(_open_by_entry_hamming(ctx, a, b).sum()) for a, b in pairs])
    for g, w in zip(directed, ref.match_pairs_directed(pairs, 0.8)):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    assert directed[0].sum() >= sum(shared) - 2                  # the shared rows do match
    for got, (md, mm) in zip(graphs, THRESHOLDS):
        for g, w in zip(got[:5], ref.match_all_pairs(pairs, 0.8, md, mm)[:5]):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    want = (sum(sizes), int(opens.sum()), _expected_items(pairs, opens, [0]))
    print(f"open rows per pair {opens.tolist()}: (rows, open, items) {tally}, expected {want}")
    assert tally == want
    assert want[2] < _per_pair_items(opens) and np.all(opens >= 1)    # shared
