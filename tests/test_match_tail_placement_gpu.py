"""GPU: the tail of a matching launch (rows -> arg-min -> candidate columns -> finalize -> scan -> compaction) beside the next launch's
sweep, whatever share of the chip the driver gives it (eacham_amd/csrc/matcher.hip: run_match_metric, launch_lean_tail; match_plan.hpp:
argmin_grid). Nothing observable may depend on it: edges and counts are held byte for byte against the CPU oracle and against a
context created under EACHAM_MATCH_SWEEP_FORM=exact.

The job: ten frames of 96 .. 600 rows (noisy copies of one base frame, so that pairs do match), their 45 pairs ordered by train frame,
under EACHAM_MATCH_BUDGET_MB=16 with one resident frame of 16 000 rows that no pair names (a launch's workspace is sized by the largest
resident frame: 1.6 MB per pair and more), so that the job falls into four or more launches through both workspace slots and every
tail but the last runs beside a sweep. A launch of this job is about ten pairs, so argmin_grid's caps do not bind in it: the half
round beside a sweep is run by one more job, 1 540 pairs of 600-row frames under 48 MiB, whose first launch passes 8 x CUs. At 256-D and 129-D (the screen form), mutual matching and the directed lists; at 128-D (the
bound form, whose tail also carries match_rowpick_kernel and the exact pass); with per-pair statistics (the full-column form); packed
rows of 256 bits under Hamming distance; one context used for three calls in a row; a call that fits one launch; and one
eacham_ba_prepare + solve (device construction, which uses the second stream) on the same context between two matching calls, its
result equal to a fresh context's.

The file passes on the parent commit's library as well: nothing observable changes."""
import numpy as np
import pytest

from eacham_amd import ba, synth
import ham_cases as HC
import ham_reference as R
import oracle_api as O
import test_match_screen_list_gpu as L

pytestmark = pytest.mark.gpu
SEED = 2207
SIZES = [96, 130, 200, 257, 320, 384, 450, 512, 577, 600]
BIG_ROWS = 16000
BUDGET = {"EACHAM_MATCH_BUDGET_MB": 16}
_CACHE = {}


def _pairs():
    p = synth.all_pairs(len(SIZES))
    return p[np.argsort(p[:, 1], kind="stable")]


def _job(dim):
    """(frames, the big frame no pair names, the oracle's graphs under 30 / 30 and 1 / 0) — built once per dimension, never changed."""
    if dim not in _CACHE:
        descs = L._noisy_copies(SIZES, dim, SEED + dim, 6.0)
        big = synth.random_u8_descriptors(BIG_ROWS, dim, SEED, 9).astype(np.float32)
        for d in descs + [big]:
            d.setflags(write=False)
        pairs = _pairs()
        want = {th: O.match_all_pairs(descs, pairs, min_dir=th[0], min_mutual=th[1]) for th in ((30, 30), (1, 0))}
        _CACHE[dim] = descs, big, want
    return _CACHE[dim]


def _bytes_equal(got, want, what, n=4):
    for k, (g, w) in enumerate(zip(got[:n], want[:n])):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"{what}: array {k} differs"


def _launches(ctx, npairs, stats=False, at_least=4):
    starts, slots = ctx.match_batches(npairs, stats=stats)
    assert len(starts) >= at_least and slots == 2, (list(starts), slots)
    return starts


@pytest.mark.parametrize("dim", [256, 129, 128])
def test_mutual_matching_and_directed_lists(dim):
    """256-D and 129-D run the screen form, 128-D the bound form; each against the oracle and the exact form."""
    descs, big, want = _job(dim)
    pairs = _pairs()
    got, directed = {}, {}
    for form in (None, "exact"):
        with L._context(**BUDGET, **({"EACHAM_MATCH_SWEEP_FORM": form} if form else {})) as ctx:
            directed[form] = ctx.match_pairs_directed(descs + [big], pairs)       # (uploads the frames)
            _launches(ctx, len(pairs))
            for th in want:
                got[form, th] = ctx.match_all_pairs(pairs, min_dir=th[0], min_mutual=th[1], stats=False)
            if form is None:
                rows, left_open = ctx.match_screen()
                print(f"{dim}-D: {left_open} of {rows} rows open")
                # which sweep ran (the frames are copies of one another: the screen may have to leave every row open)
                assert (0 < left_open <= rows) if dim > 128 else (rows, left_open) == (0, 0)
    for th in want:
        _bytes_equal(got[None, th], want[th], f"{dim}-D oracle {th}")
        _bytes_equal(got[None, th], got["exact", th], f"{dim}-D exact form {th}")
    assert got[None, (1, 0)][0].sum() > 2000 and (got[None, (30, 30)][0] > 0).sum() >= 20      # pairs do match
    assert directed[None] == directed["exact"]
    for p, (a, b) in enumerate(pairs):
        wq, wt = O.match_directed(descs[a], descs[b], 0.8)
        assert directed[None][p] == dict(zip(wq.tolist(), wt.tolist())), (dim, a, b)


def test_a_launch_whose_arg_min_grid_is_capped():
    """In the jobs above a launch is about ten pairs: nb x wgs_per_pair is a few hundred and argmin_grid never reaches a cap, so the
    arg-min pass runs the same grid beside a sweep or not. Here it binds: 56 frames x 600 rows (three workgroups per pair), 1 540
    pairs under 48 MiB — a first launch of 700 pairs or more, over 8 x CUs workgroups' worth of items' bound, with the second launch's
    sweep beside its tail; then a shorter launch and the last one."""
    import torch
    from eacham_amd import shard
    nf = 56
    descs, _ = synth.make_frame_descriptors(synth.make_scene(nf, 14000, 10), 600, 256)
    descs = [np.asarray(d, dtype=np.float32) for d in descs]
    pairs = shard.order_pairs(synth.all_pairs(nf))
    out = {}
    for form in (None, "exact"):
        with L._context(EACHAM_MATCH_BUDGET_MB=48, **({"EACHAM_MATCH_SWEEP_FORM": form} if form else {})) as ctx:
            L._upload(ctx, descs)
            out[form] = ctx.match_all_pairs(pairs, stats=False)
            if form is None:
                starts = _launches(ctx, len(pairs), at_least=2)
                rows, left_open = ctx.match_screen()
                assert 0 < left_open < rows                                  # the screen form ran
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    first = int(starts[1] - starts[0])
    print(f"launches at {list(starts)}, {cus} CUs: {3 * first} workgroups' bound in the first launch, cap {8 * cus} beside a sweep")
    assert 3 * first > 8 * cus, (list(starts), cus)                          # the half round binds
    _bytes_equal(out[None], out["exact"], "exact form")
    sample = sorted({0, len(pairs) - 1, *[int(s) - 1 for s in starts[1:]], *[int(s) for s in starts[1:]], 100, 700, 1300})
    want = O.match_all_pairs(descs, pairs[sample])
    counts, offsets, q, t = out[None][:4]
    assert np.array_equal(counts[sample], want[0])
    assert np.array_equal(np.concatenate([q[offsets[p]:offsets[p + 1]] for p in sample]), want[2])
    assert np.array_equal(np.concatenate([t[offsets[p]:offsets[p + 1]] for p in sample]), want[3])
    assert len(q) > 30 * nf


def test_per_pair_statistics():
    """The full-column form: every launch is a pair or two under this budget, the tail is match_finalize_kernel."""
    descs, big, want = _job(256)
    pairs = _pairs()
    out = {}
    for form in (None, "exact"):
        with L._context(**BUDGET, **({"EACHAM_MATCH_SWEEP_FORM": form} if form else {})) as ctx:
            L._upload(ctx, descs + [big])
            out[form] = ctx.match_all_pairs(pairs, stats=True)
            _launches(ctx, len(pairs), stats=True)
    _bytes_equal(out[None], want[30, 30], "oracle", n=5)
    _bytes_equal(out[None], out["exact"], "exact form", n=5)


def test_binary_rows_of_256_bits():
    nbytes = 32
    base = HC._bytes(SEED, nbytes, (max(SIZES), nbytes))
    descs = [base[:n] ^ HC._flips(SEED, 300 + k, (n, nbytes), 0.04) for k, n in enumerate(SIZES)]
    big = HC._bytes(SEED + 1, nbytes, (BIG_ROWS, nbytes))
    pairs = _pairs()
    ref = R.Scene(descs)
    want = ref.match_all_pairs(pairs, 0.8, 1, 0)
    out, directed = {}, {}
    for form in (None, "exact"):
        with L._context(**BUDGET, **({"EACHAM_MATCH_SWEEP_FORM": form} if form else {})) as ctx:
            ctx.clear_descriptors()
            for f, d in enumerate(descs + [big]):
                ctx.upload_descriptors_bits(f, d)
            out[form] = ctx.match_all_pairs_hamming(pairs, 0.8, 1, 0, stats=False)
            directed[form] = ctx.match_pairs_directed_hamming(pairs, 0.8)
            _launches(ctx, len(pairs))
    _bytes_equal(out[None], want, "reference", n=5)
    _bytes_equal(out[None], out["exact"], "exact form", n=5)
    _bytes_equal(directed[None], ref.match_pairs_directed(pairs, 0.8), "directed, reference", n=5)
    _bytes_equal(directed[None], directed["exact"], "directed, exact form", n=5)
    assert out[None][0].sum() > 1000


def test_three_calls_in_a_row_on_one_context():
    """No synchronisation of the caller's between them: the slots, the events and the tail's stream are the context's."""
    descs, big, want = _job(256)
    pairs = _pairs()
    with L._context(**BUDGET) as ctx:
        L._upload(ctx, descs + [big])
        a = ctx.match_all_pairs(pairs, min_dir=1, min_mutual=0, stats=False)
        b = ctx.match_all_pairs(pairs, stats=False)
        c = ctx.match_all_pairs(pairs, min_dir=1, min_mutual=0, stats=False)
        _launches(ctx, len(pairs))                              # (the plan is that of the frame table as the last call left it)
    _bytes_equal(a, want[1, 0], "first call")
    _bytes_equal(b, want[30, 30], "second call")
    _bytes_equal(c, want[1, 0], "third call")


def test_a_call_that_fits_one_launch():
    descs, big, want = _job(256)
    pairs = _pairs()
    with L._context() as ctx:                                   # the default budget
        L._upload(ctx, descs + [big])
        got = ctx.match_all_pairs(pairs, min_dir=1, min_mutual=0, stats=False)
        starts, slots = ctx.match_batches(len(pairs), stats=False)
        assert len(starts) == 1 and slots == 1, (list(starts), slots)
        one = ctx.match_all_pairs(pairs[7:8], stats=False)
    _bytes_equal(got, want[1, 0], "one launch")
    assert one[0][0] == want[30, 30][0][7]


def test_bundle_adjustment_between_two_matching_calls():
    """eacham_ba_prepare's device construction runs its second half on the second stream, the matching tails beside the sweeps: one
    after the other on one context, each gives what it gives alone."""
    descs, big, want = _job(256)
    pairs = _pairs()
    arrays = ba.BaArrays.from_scene(synth.make_scene(6, 200, 4, seed=5))
    cfg = ba.OptimizerConfig.refine_ba()

    def solve(ctx):
        prep = ba.PreparedBA(ctx, arrays)
        try:
            return prep.run(cfg)
        finally:
            prep.close()

    env = dict(BUDGET, EACHAM_BA_PREPARE="device")
    with L._context(**env) as ctx:
        alone = solve(ctx)
    with L._context(**env) as ctx:
        L._upload(ctx, descs + [big])
        first = ctx.match_all_pairs(pairs, min_dir=1, min_mutual=0, stats=False)
        between = solve(ctx)
        second = ctx.match_all_pairs(pairs, min_dir=1, min_mutual=0, stats=False)
        _launches(ctx, len(pairs))
    _bytes_equal(first, want[1, 0], "before the solve")
    _bytes_equal(second, want[1, 0], "behind the solve")
    assert (between.outer_iterations, between.inner_iterations) == (alone.outer_iterations, alone.inner_iterations)
    assert between.points.tobytes() == alone.points.tobytes() and between.cam_T_wc.tobytes() == alone.cam_T_wc.tobytes()
    assert between.final_error == alone.final_error and between.final_error < between.initial_error
