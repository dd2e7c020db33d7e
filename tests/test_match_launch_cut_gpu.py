"""The cut of a matching job into launches, and the pairs the row pass drops on their open count (eacham_amd/csrc/matcher.hip:
make_plan / next_batch, match_rows2_kernel<METRIC_L2, true>).

The plan. A job that needs more than one launch goes through two workspace slots as n equal full launches and one short last
launch, planned as a whole. With batch, round and tail as eacham_match_debug_plan gives them for the job:
  1. no launch exceeds batch;
  2. the full launches are whole rounds and differ by at most one round;
  3. with two or more launches the last holds between 1 and tail + round pairs — never the budget's remnant;
  4. the launches sum to the job.
Held over a ladder of job sizes around every boundary of the rule, under a 16 MiB budget with a 600-row frame resident (a launch
holds less than one round of workgroups there: the unit is one pair), under 64 MiB (three rounds of 512 pairs) and with a 2000-row
frame under the default 1 GiB (rounds of 64 pairs, and the headline job itself: 19 900 = 9 344 + 9 344 + 1 212). The plan is that of
the frame table as the last matching call left it, so every case runs one pair first.

A job across the new boundaries: 56 frames x 600 rows x 256-D ordered by train frame, 1 540 pairs under 16 MiB — the default form
gives the bytes of EACHAM_MATCH_SWEEP_FORM=exact, the oracle's pairs on both sides of every boundary, and two calls queued with no
synchronisation the same bytes.

Pairs at the threshold: behind the screen sweep (above 128-D, mutual matching) a pair with no more than min_mutual open rows leaves
match_rows2_kernel before it reads a row. Frames of 64-160 random integer rows with k rows of one copied into the other, k = 0, 1,
29, 30, 31, 32, 64: the oracle alone first shows that such a pair has exactly k mutual matches, (nearly) no other passing row, count 0
up to k = 30 and 31 at k = 31; then one device job over all k, an empty frame and a one-row frame, against the oracle and the exact
form, also as directed lists (no pair may be dropped) and under min_mutual 0 and (min_dir, min_mutual) = (6, 5).

On the library of the parent commit the five plan cases fail (it has no eacham_match_debug_plan, and its cut leaves remnants: a job
of 2 x batch + 1 pairs is batch + batch + 1, with the whole tail of the second launch open behind a sweep of one pair);
every other test of the file passes there: nothing observable changes."""
import numpy as np
import pytest

from eacham_amd import shard, synth
import oracle_api as O
import test_match_screen_list_gpu as L

gpu = pytest.mark.gpu
SEED = 1207
KS = (0, 1, 29, 30, 31, 32, 64)


# ---------------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------------
def _check_cut(ctx, npairs):
    starts, slots = ctx.match_batches(npairs, stats=False)
    batch, rnd, tail = ctx.match_plan(npairs, stats=False)
    sizes = np.diff(np.concatenate([starts, [npairs]]).astype(np.int64))
    what = f"npairs {npairs}: launches {sizes.tolist()}, slots {slots}, batch {batch}, round {rnd}, tail {tail}"
    assert starts[0] == 0 and np.all(sizes > 0) and sizes.sum() == npairs, what          # 4
    assert sizes.max() <= batch, what                                                    # 1
    if len(sizes) > 1:
        assert slots == 2, what
        full = sizes[:-1]
        assert np.all(full % rnd == 0) and full.max() - full.min() <= rnd, what          # 2
        assert 1 <= sizes[-1] <= tail + rnd, what                                        # 3
        assert len(full) == -(-int(full.sum()) // batch), what                           # as few full launches as the budget allows
    return sizes


def _resident(ctx, rows):
    """One frame of `rows` rows at 256-D, seen by a matching call: the plan is that of the frame table as the last call left it."""
    L._upload(ctx, [synth.random_u8_descriptors(rows, 256, SEED, 0)])
    ctx.match_all_pairs(np.array([[0, 0]], np.int32), stats=False)


def _ladder(ctx):
    batch, rnd, tail = ctx.match_plan(10 ** 6, stats=False)     # the budget's launch, whatever the job
    return batch, rnd, tail, sorted({1, rnd, batch - 1, batch, batch + 1, batch + tail - 1, batch + tail, batch + tail + 1,
                                     2 * batch - 1, 2 * batch, 2 * batch + 1, 2 * batch + rnd, 1540})


@gpu
@pytest.mark.parametrize("budget_mb, rows", [(16, 600), (64, 600), (1024, 2000)])
def test_the_cut_over_a_ladder_of_jobs(budget_mb, rows):
    with L._context(EACHAM_MATCH_BUDGET_MB=budget_mb) as ctx:
        _resident(ctx, rows)
        batch, rnd, tail, ladder = _ladder(ctx)
        print(f"budget {budget_mb} MiB, {rows}-row frames: batch {batch}, round {rnd}, tail {tail}")
        assert batch >= 2 and 1 <= tail <= max(batch // 8, rnd) and (batch % rnd == 0)
        if budget_mb == 16:
            assert 2 * batch < 1540                                  # 1 540 pairs are at least three launches
        for n in ladder:
            sizes = _check_cut(ctx, n)
            print(f"  {n}: {sizes.tolist()}")
            if n > batch + rnd:                                      # (up to a round more may fit the budget as one launch)
                assert len(sizes) >= 2
        for m in (3, 5):                                             # no remnant near a further multiple of the budget's launch
            for d in range(-2, 3):
                _check_cut(ctx, m * batch + d)


@gpu
def test_the_cut_of_the_headline_job():
    """S200: 19 900 pairs of 2000-row frames under the default 1 GiB — two equal launches and a short one, where a budget that
    gives 9 792 pairs per launch once left 9 792 + 9 792 + 316."""
    with L._context(EACHAM_MATCH_BUDGET_MB=1024) as ctx:
        _resident(ctx, 2000)
        batch, rnd, tail = ctx.match_plan(19900, stats=False)
        sizes = _check_cut(ctx, 19900)
        print(f"batch {batch}, round {rnd}, tail {tail}: {sizes.tolist()}")
        assert len(sizes) == 3 and sizes[0] == sizes[1] and tail - rnd < sizes[2] <= tail
        if (batch, rnd, tail) == (9792, 64, 1216):
            assert sizes.tolist() == [9344, 9344, 1212]


@gpu
def test_the_plan_of_the_full_column_form():
    """The form the per-pair statistics select has its own bytes per pair, the same rule."""
    with L._context(EACHAM_MATCH_BUDGET_MB=16) as ctx:
        _resident(ctx, 600)
        batch, rnd, tail = ctx.match_plan(10 ** 6, stats=True)
        for n in (1, batch, batch + 1, batch + tail + 1, 2 * batch + 1, 1540):
            starts, slots = ctx.match_batches(n, stats=True)
            b, r, t = ctx.match_plan(n, stats=True)
            sizes = np.diff(np.concatenate([starts, [n]]).astype(np.int64))
            assert sizes.sum() == n and sizes.max() <= b and (len(sizes) == 1 or (slots == 2 and 1 <= sizes[-1] <= t + r)), (n, sizes)
            assert len(sizes) == 1 or (np.all(sizes[:-1] % r == 0) and np.ptp(sizes[:-1]) <= r), (n, sizes)


# ---------------------------------------------------------------------------------------------------------------------------
# a job across the new boundaries
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_job_across_the_boundaries():
    import torch
    nf = 56
    descs, _ = synth.make_frame_descriptors(synth.make_scene(nf, 14000, 10), 600, 256)
    descs = [np.asarray(d, dtype=np.float32) for d in descs]
    pairs = shard.order_pairs(synth.all_pairs(nf))
    assert len(pairs) == 1540
    with L._context(EACHAM_MATCH_BUDGET_MB=16, EACHAM_MATCH_SWEEP_FORM="exact") as ctx:
        L._upload(ctx, descs)
        exact = ctx.match_all_pairs(pairs, stats=False)
    with L._context(EACHAM_MATCH_BUDGET_MB=16) as ctx:
        L._upload(ctx, descs)
        a = ctx.match_all_pairs(pairs, stats=False)
        rows, left_open = ctx.match_screen()
        starts, slots = ctx.match_batches(len(pairs), stats=False)
        print(f"launches at {list(starts)}, {slots} slots; {left_open} of {rows} rows open")
        assert len(starts) >= 3 and slots == 2, (starts, slots)
        assert 0 < left_open < rows                                      # the screen form ran
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
    for x, w in zip(a[:4], exact[:4]):
        assert x.tobytes() == w.tobytes()
    sample = sorted({0, len(pairs) - 1, *[int(s) - 1 for s in starts[1:]], *[int(s) for s in starts[1:]]})
    want = O.match_all_pairs(descs, pairs[sample])
    assert np.array_equal(counts[sample], want[0])
    assert np.array_equal(np.concatenate([q[offsets[p]:offsets[p + 1]] for p in sample]), want[2])
    assert np.array_equal(np.concatenate([t[offsets[p]:offsets[p + 1]] for p in sample]), want[3])
    assert len(q) > 30 * nf and (counts == 0).sum() > 0               # live pairs and dead pairs


# ---------------------------------------------------------------------------------------------------------------------------
# pairs at the threshold
# ---------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _threshold_frames(dim):
    """Frames 2i, 2i + 1: 64 + 13 i and 160 - 11 i random rows, KS[i] rows of the first copied to scattered rows of the second;
    then an empty frame and a one-row frame (a copy of row 5 of frame 0). Built once per dimension, never changed."""
    if dim not in _CACHE:
        descs = []
        # (at 129-D the screen's slack is a larger share of a distance: a wider spread keeps it from leaving random rows open)
        spread = 48.0 if dim > 192 else 140.0
        for i, k in enumerate(KS):
            A = synth.random_u8_descriptors(64 + 13 * i, dim, SEED, 2 * i, spread)
            B = synth.random_u8_descriptors(160 - 11 * i, dim, SEED, 2 * i + 1, spread)
            src = synth.rng_permutation(SEED, 50 + i, A.shape[0])[:k]
            dst = synth.rng_permutation(SEED, 70 + i, B.shape[0])[:k]
            B[dst] = A[src]
            descs += [A, B]
        descs.append(np.zeros((0, dim), np.float32))
        descs.append(descs[0][5:6].copy())
        e, s = 2 * len(KS), 2 * len(KS) + 1
        pairs = [[2 * i, 2 * i + 1] for i in range(len(KS))] + [[2 * i + 1, 2 * i] for i in range(len(KS))]
        pairs += [[e, 0], [0, e], [s, 0], [0, s], [e, s]]
        for d in descs:
            d.setflags(write=False)
        _CACHE[dim] = descs, np.array(pairs, np.int32)
    return _CACHE[dim]


@pytest.mark.parametrize("dim", [256, 129])
def test_the_threshold_inputs_by_the_oracle_alone(dim):
    descs, pairs = _threshold_frames(dim)
    for i, k in enumerate(KS):
        for a, b in ((2 * i, 2 * i + 1), (2 * i + 1, 2 * i)):
            q, t, stats = O.match_mutual(descs[a], descs[b], 0.8, 0, -1)
            assert len(q) == stats[2] == k, (dim, k, stats)                       # exactly k mutual matches
            assert np.all(np.abs(descs[a][q] - descs[b][t]).sum(1) == 0)          # ... the copied rows
            assert k <= stats[0] <= k + 2 and k <= stats[1] <= k + 2, (dim, k, stats)   # nearly no random row passes
            cnt = len(O.match_mutual(descs[a], descs[b], 0.8, 30, 30)[0])
            assert cnt == (k if k >= 31 else 0), (dim, k, cnt)
            # the numpy model of the screen's bound: the copied rows stay open and at most two more, so k <= 30 means <= 30 open rows
            model = int(L._model_open(descs[a], descs[b]).sum())
            assert k <= model <= k + 2 and (k > 30 or model <= 30), (dim, k, model)
    assert list(KS[2:5]) == [29, 30, 31]


def _bytes_equal(got, want, what):
    for name, g, w in zip(["counts", "offsets", "q", "t"], got[:4], want[:4]):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"{what}: {name} differs"


@gpu
@pytest.mark.parametrize("dim", [256, 129])
def test_pairs_at_the_threshold(dim):
    descs, pairs = _threshold_frames(dim)
    thresholds = ((30, 30), (0, 0), (1, 0), (6, 5))
    want = {th: O.match_all_pairs(descs, pairs, min_dir=th[0], min_mutual=th[1]) for th in thresholds}
    got, directed = {}, {}
    for form in ("screen", "exact"):
        with L._context(EACHAM_MATCH_SWEEP_FORM=form) as ctx:
            directed[form] = ctx.match_pairs_directed(descs, pairs)          # (uploads the frames)
            for th in thresholds:
                got[form, th] = ctx.match_all_pairs(pairs, min_dir=th[0], min_mutual=th[1], stats=False)
            if form == "screen":
                rows, left_open = ctx.match_screen()
                assert rows == sum(descs[a].shape[0] for a, _ in pairs) and 0 < left_open < rows       # the screen sweep ran
                opens = []
                for p in pairs:                                              # a job of one pair: its open rows, its count
                    one = ctx.match_all_pairs(p[None, :], stats=False)
                    opens.append(ctx.match_screen()[1])
                    assert one[0][0] == want[30, 30][0][len(opens) - 1]
    opens = np.array(opens)
    print(f"{dim}-D: open rows per pair {opens.tolist()}, counts {got['screen', (30, 30)][0].tolist()}")
    for th in thresholds:
        _bytes_equal(got["screen", th], want[th], f"oracle {th}")
        _bytes_equal(got["screen", th], got["exact", th], f"exact form {th}")
    # the pairs the new branch takes under 30 / 30: no more than 30 open rows, and every copied row is open
    for i, k in enumerate(KS):
        for p in (i, len(KS) + i):
            assert opens[p] >= k, (k, opens[p])
            if k <= 30:
                assert opens[p] <= 30, (k, opens[p])
    e = 2 * len(KS)                                                          # [e, 0], [0, e], [s, 0], [0, s], [e, s]
    assert opens[e] == 0 and opens[e + 1] == 0 and opens[e + 2] == 1 and opens[e + 4] == 0
    assert opens[e + 3] == descs[0].shape[0]                                 # a one-row train frame: no runner-up, every row open
    counts = got["screen", (30, 30)][0]
    assert counts.tolist() == [k if k >= 31 else 0 for k in KS] * 2 + [0] * 5
    assert got["screen", (0, 0)][0].tolist()[:2 * len(KS)] == list(KS) * 2
    assert got["screen", (6, 5)][0].tolist()[:2 * len(KS)] == [k if k > 5 else 0 for k in KS] * 2
    # directed lists: no pair may be dropped
    assert directed["screen"] == directed["exact"]
    for p, (a, b) in enumerate(pairs):
        wq, wt = O.match_directed(descs[a], descs[b], 0.8)
        assert directed["screen"][p] == dict(zip(wq.tolist(), wt.tolist())), (a, b)
        if p < 2 * len(KS):
            assert len(directed["screen"][p]) >= KS[p % len(KS)]
