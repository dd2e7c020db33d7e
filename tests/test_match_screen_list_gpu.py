"""GPU: the screen sweep above 128-D lists its own open rows (match_screen_kernel's masks + match_openlist_kernel) and the exact
pass over them runs behind the sweep on the sweep's stream (eacham_amd/csrc/matcher.hip). Held here, bit for bit against the CPU
oracle and against a context created under EACHAM_MATCH_SWEEP_FORM=exact: every shape of a pair's mask words (a wave-block with one
sub-tile, an inactive wave, one and two workgroups per pair, a train frame without a runner-up, a last word that is partly padding);
pairs whose every row stays open (items of 64, 64, 64, 8 and of 64, 32: the boundary of the empty second group in
match_colverify_kernel<8, true>); a pair with no open row beside ordinary ones; several launches through the two workspace slots,
also queued without a synchronisation; and the tally against the debug entry's own bounds."""
import contextlib
import os

import numpy as np
import pytest

from eacham_amd import synth
import oracle_api as O

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _context(**env):
    """A context of its own with the switches eacham_ctx_create reads from the environment."""
    from eacham_amd import HipContext
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        ctx = HipContext(0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        yield ctx
    finally:
        ctx.close()


def _upload(ctx, descs):
    ctx.clear_descriptors()
    for f, d in enumerate(descs):
        ctx.upload_descriptors(f, d)


def _noisy_copies(sizes, dim, seed, noise):
    """Frame k = the first sizes[k] rows of one base frame + rounded N(0, noise): frames that match one another."""
    base = synth.random_u8_descriptors(max(sizes), dim, seed, 0)
    return [np.clip(base[:n] + np.rint(noise * synth.rng_normal(seed, 20 + k, (n, dim))), 0, 255).astype(np.float32)
            for k, n in enumerate(sizes)]


def _ordered(nf):
    return np.array([[a, b] for a in range(nf) for b in range(nf) if a != b], dtype=np.int32)


def _ratio_pass(d1, d2, ratio=0.8):
    """FeatureMatcherFlann.cpp:23 as the library restates it: fp32 square roots, fp32 quotient, compared as double."""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.sqrt(d1.astype(np.float32)) / np.sqrt(d2.astype(np.float32))
    return q.astype(np.float64) < ratio


def _open_by_entry(ctx, a, b):
    """Rows of the ordered pair that do not fail the ratio test on the sweep's own (L1, U2) (eacham_match_debug_screen_pair): a row
    with a real minimum and either no bound on its runner-up or a pair of bounds that passes."""
    _, l1, u2 = ctx.match_screen_pair(int(a), int(b))
    return (l1 >= 0) & ((u2 < 0) | _ratio_pass(l1, np.maximum(u2, 0)))


# ---- the numpy model of the screen's bound (match_screen.hpp and the sweep's sixteen subsets restated) ----
def _grid_m():
    mags = np.array(list(range(16)) + list(range(16, 32, 2)) + list(range(32, 64, 4)))
    ms = np.unique(np.concatenate([mags, -mags]))
    ms = ms[np.argsort(np.abs(ms), kind="stable")]
    x = np.arange(256)[:, None]
    return ms[np.argmin(np.abs(x - (64 + 4 * ms[None, :])), axis=1)].astype(np.int64)


_M = _grid_m()


def _stored_pos(D):
    """Stored position of every row (partition_kernel): the rows of even centred squared norm first, in order, in whole tiles."""
    even = ((D.astype(np.int64) - 128) ** 2).sum(1) % 2 == 0
    even_pad = (int(even.sum()) + 31) // 32 * 32
    return np.where(even, np.cumsum(even) - 1, even_pad + np.cumsum(~even) - 1)


def _model_open(Da, Db, ratio=0.8):
    """Which rows of Da the screen leaves open against Db: n1 and u from the minima over the sixteen subsets of the stored train
    rows (tile parity x groups of four rows), L1 / U2 as screen::lower_d2 / upper_d2 compute them in double."""
    Ma, Mb = _M[Da.astype(np.int64)], _M[Db.astype(np.int64)]
    s_a = ((Da.astype(np.int64) - (64 + 4 * Ma)) ** 2).sum(1)
    e_b = ((Db.astype(np.int64) - (64 + 4 * Mb)) ** 2).sum(1).max()
    n = (Ma * Ma).sum(1)[:, None] + (Mb * Mb).sum(1)[None, :] - 2 * (Ma @ Mb.T)
    pos = _stored_pos(Db)
    subset = ((pos >> 5) & 1) * 8 + ((pos & 31) >> 2)
    mins = np.full((Da.shape[0], 16), np.inf)
    for k in range(16):
        if np.any(subset == k):
            mins[:, k] = n[:, subset == k].min(1)
    mins.sort(axis=1)
    n1, u = mins[:, 0], mins[:, 1]
    slack = np.sqrt(s_a.astype(np.float64)) + np.sqrt(float(e_b))
    lo = 4.0 * np.sqrt(n1) - slack
    l1 = np.where(lo > 0, np.maximum(np.floor(lo * lo) - 1.0, 0.0), 0.0)
    has = np.isfinite(u)
    hi = 4.0 * np.sqrt(np.where(has, u, 0.0)) + slack
    u2 = np.minimum(np.ceil(hi * hi) + 1.0, 256.0 * 255 * 255)
    return ~has | _ratio_pass(l1, u2, ratio)


def _same_graph(got, want, what):
    for name, g, w in zip(["counts", "offsets", "q", "t"], got[:4], want[:4]):
        assert np.array_equal(g, w), f"{what}: {name} differs"


@pytest.mark.parametrize("dim", [256, 129])
def test_shapes_of_a_pair(dim):
    """Frames of 1, 40, 70, 97, 130 and 200 rows in one job: a wave-block with one sub-tile, an inactive wave, pairs with one and
    with two workgroups, a train frame with no runner-up, a last mask word that is partly padding. Every ordered pair through
    match_pairs_directed, every unordered one through match_all_pairs."""
    descs = _noisy_copies([1, 40, 70, 97, 130, 200], dim, 611, 6.0)
    nf = len(descs)
    ordered, unordered = _ordered(nf), synth.all_pairs(nf)
    out = {}
    for form in ("screen", "exact"):
        with _context(EACHAM_MATCH_SWEEP_FORM=form) as ctx:
            out[form, "directed"] = ctx.match_pairs_directed(descs, ordered)
            out[form, "tally_directed"] = ctx.match_screen()
            if form == "screen":
                by_entry = sum(int(_open_by_entry(ctx, a, b).sum()) for a, b in ordered)
            for md, mm in ((2, 1), (30, 30)):
                out[form, md] = ctx.match_all_pairs(unordered, min_dir=md, min_mutual=mm, stats=False)
    for k, (a, b) in enumerate(ordered):
        wq, wt = O.match_directed(descs[a], descs[b], 0.8)
        assert out["screen", "directed"][k] == dict(zip(wq.tolist(), wt.tolist())), (a, b)
    assert out["screen", "directed"] == out["exact", "directed"]
    assert sum(len(m) for m in out["screen", "directed"]) > 200
    rows = sum(descs[a].shape[0] for a, _ in ordered)
    assert out["screen", "tally_directed"] == (rows, by_entry) and 0 < by_entry < rows
    assert out["exact", "tally_directed"] == (0, 0)
    for md, mm in ((2, 1), (30, 30)):
        _same_graph(out["screen", md], O.match_all_pairs(descs, unordered, min_dir=md, min_mutual=mm), f"oracle {md}/{mm}")
        for g, w in zip(out["screen", md][:4], out["exact", md][:4]):
            assert g.tobytes() == w.tobytes()
    assert out["screen", 2][0].sum() > 200


@pytest.mark.parametrize("n", [200, 96])
def test_every_row_open(n):
    """Near-identical frames (the heavy-candidate case): every row passes the ratio test, so every row stays open and goes through
    the exact pass — items of 64, 64, 64 and 8 candidates at 200 rows, of 64 and 32 at 96 (the last item's second group is empty
    from 32 candidates down)."""
    descs = _noisy_copies([n, n, n], 256, 7, 3.0)
    ordered, unordered = _ordered(3), synth.all_pairs(3)
    out = {}
    for form in ("screen", "exact"):
        with _context(EACHAM_MATCH_SWEEP_FORM=form) as ctx:
            out[form, "directed"] = ctx.match_pairs_directed(descs, ordered)
            out[form, "tally"] = ctx.match_screen()
            out[form] = ctx.match_all_pairs(unordered, stats=False)
            out[form, "tally_mutual"] = ctx.match_screen()
    assert out["screen", "tally"] == (6 * n, 6 * n) and out["screen", "tally_mutual"] == (3 * n, 3 * n)   # open == rows
    assert out["exact", "tally"] == (0, 0)
    for k, (a, b) in enumerate(ordered):
        wq, wt = O.match_directed(descs[a], descs[b], 0.8)
        assert len(wq) == n and out["screen", "directed"][k] == dict(zip(wq.tolist(), wt.tolist())), (a, b)
    assert out["screen", "directed"] == out["exact", "directed"]
    _same_graph(out["screen"], O.match_all_pairs(descs, unordered), "oracle")
    for g, w in zip(out["screen"][:4], out["exact"][:4]):
        assert g.tobytes() == w.tobytes()
    assert np.all(out["screen"][0] == n)


def _frames_with_a_dead_pair():
    """Frames 0..2 match one another (130 / 97 / 200 rows); frame 3 is unrelated to them (130 rows); frame 4 holds 24 rows five times
    each, the copies adjacent: five consecutive stored rows always lie in two of the sweep's subsets, so the bound on every
    runner-up against frame 4 is the bound on the minimum, and (3, 4) leaves no row open."""
    descs = _noisy_copies([130, 97, 200], 256, 612, 6.0)
    descs.append(synth.random_u8_descriptors(130, 256, 613, 1))
    descs.append(np.repeat(synth.random_u8_descriptors(24, 256, 613, 2), 5, axis=0))
    return descs


def test_the_numpy_bound_closes_every_row_of_the_dead_pair():
    """(no GPU needed for this one: the premise of test_no_row_open, from the numpy model of the bound)"""
    descs = _frames_with_a_dead_pair()
    assert not _model_open(descs[3], descs[4]).any()
    assert _model_open(descs[0], descs[2]).sum() > 60           # the model does leave rows open where rows match


def test_no_row_open():
    """A train frame of duplicated rows (every row's two nearest are equal) beside ordinary pairs in the same launch: that pair has
    zero items and zero matches, its neighbours are what they are without it."""
    descs = _frames_with_a_dead_pair()
    pairs = np.array([[0, 1], [3, 4], [0, 2], [3, 4], [1, 2], [2, 0]], dtype=np.int32)
    dead = [1, 3]
    with _context(EACHAM_MATCH_SWEEP_FORM="screen") as ctx:
        _upload(ctx, descs)
        assert not _open_by_entry(ctx, 3, 4).any()              # the sweep's own bounds close every row
        ctx.match_all_pairs(pairs[dead], min_dir=1, min_mutual=0, stats=False)
        assert ctx.match_screen() == (2 * 130, 0)               # a launch with no item at all
        got = ctx.match_all_pairs(pairs, min_dir=1, min_mutual=0, stats=False)
        tally = ctx.match_screen()
        by_entry = sum(int(_open_by_entry(ctx, a, b).sum()) for a, b in pairs)
        directed = ctx.match_pairs_directed(descs, pairs)
    with _context(EACHAM_MATCH_SWEEP_FORM="exact") as ctx:
        _upload(ctx, descs)
        exact = ctx.match_all_pairs(pairs, min_dir=1, min_mutual=0, stats=False)
    _same_graph(got, O.match_all_pairs(descs, pairs, min_dir=1, min_mutual=0), "oracle")
    for g, w in zip(got[:4], exact[:4]):
        assert g.tobytes() == w.tobytes()
    assert np.all(got[0][dead] == 0) and np.all(np.delete(got[0], dead) > 60)
    assert tally == (sum(descs[a].shape[0] for a, _ in pairs), by_entry) and by_entry > 0
    for k, (a, b) in enumerate(pairs):
        wq, wt = O.match_directed(descs[a], descs[b], 0.8)
        assert directed[k] == dict(zip(wq.tolist(), wt.tolist())), (a, b)
        assert (len(wq) == 0) == (k in dead)


def test_several_launches_through_two_slots():
    """EACHAM_MATCH_BUDGET_MB=16 and 56 frames of 600 rows: 1540 pairs in at least three launches through the two workspace slots.
    Oracle pairs from both sides of every boundary; the call twice back to back and twice more through match_all_pairs_dev with no
    synchronisation between them: the same bytes four times, and those of the exact sweep."""
    import torch
    nf = 56
    descs, _ = synth.make_frame_descriptors(synth.make_scene(nf, 14000, 10), 600, 256)
    descs = [np.asarray(d, dtype=np.float32) for d in descs]
    pairs = synth.all_pairs(nf)
    with _context(EACHAM_MATCH_BUDGET_MB=16, EACHAM_MATCH_SWEEP_FORM="exact") as ctx:
        _upload(ctx, descs)
        exact = ctx.match_all_pairs(pairs, stats=False)
    with _context(EACHAM_MATCH_BUDGET_MB=16) as ctx:
        _upload(ctx, descs)
        a = ctx.match_all_pairs(pairs, stats=False)
        b = ctx.match_all_pairs(pairs, stats=False)
        starts, slots = ctx.match_batches(len(pairs), stats=False)   # (the plan of the frames as the calls above saw them)
        assert len(starts) >= 3 and slots == 2, (starts, slots)
        rows, left_open = ctx.match_screen()
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
    for x, y, w in zip(a[:4], b[:4], exact[:4]):
        assert x.tobytes() == y.tobytes() == w.tobytes()
    assert rows == sum(descs[i].shape[0] for i, _ in pairs) and 0 < left_open < rows // 4
    sample = sorted({0, len(pairs) - 1, *[int(s) - 1 for s in starts[1:]], *[int(s) for s in starts[1:]]})
    assert len(sample) == 2 * len(starts)
    want = O.match_all_pairs(descs, pairs[sample])
    assert np.array_equal(counts[sample], want[0])
    assert np.array_equal(np.concatenate([q[offsets[p]:offsets[p + 1]] for p in sample]), want[2])
    assert np.array_equal(np.concatenate([t[offsets[p]:offsets[p + 1]] for p in sample]), want[3])
    assert len(q) > 30 * nf                                      # neighbouring frames of the helix do match


def test_tally_is_the_open_rows_of_the_debug_entry():
    """match_screen() after a job = (real rows, rows that do not fail the ratio test on (L1, U2) of match_screen_pair), summed over
    the job's pairs: ragged frames, an unrelated frame, the duplicated-row frame, both orders."""
    descs = _frames_with_a_dead_pair() + _noisy_copies([1, 40, 70], 256, 614, 6.0)
    pairs = _ordered(len(descs))
    with _context() as ctx:                                      # the default above 128-D is the screen form
        _upload(ctx, descs)
        for sub in (pairs, pairs[::3], pairs[5:6]):
            ctx.match_all_pairs(sub, min_dir=1, min_mutual=0, stats=False)
            tally = ctx.match_screen()
            want_open = sum(int(_open_by_entry(ctx, a, b).sum()) for a, b in sub)
            assert tally == (sum(descs[a].shape[0] for a, _ in sub), want_open), len(sub)
        model_open = sum(int(_model_open(descs[a], descs[b]).sum()) for a, b in pairs[5:6])
        assert model_open == want_open                           # and the numpy model of the bound says the same of that pair
