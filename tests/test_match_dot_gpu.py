"""GPU: the dot-product matcher (eacham_match_pair_dot / _pairs_directed_dot / _all_pairs_dot, eacham_amd/csrc/matcher_dot.hip)
against its CPU reference (tests/dot_reference.py): indices, counts, offsets, stats and the BITS of every score."""
import os
import struct
import subprocess

import numpy as np
import pytest

from eacham_amd import HipContext, capi, synth
import dot_cases as DC
import dot_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    names = ["counts", "offsets", "q", "t", "scores", "stats"]
    for name, g, w in zip(names, got, want):
        if name == "scores":
            assert np.array_equal(_bits(g), _bits(w)), f"{what}: score bits differ"
        else:
            assert np.array_equal(g, w), f"{what}: {name} differ"


def _upload(ctx, descs):
    ctx.clear_descriptors()
    for f, d in enumerate(descs):
        ctx.upload_descriptors_f32(f, d)


@pytest.mark.parametrize("name", sorted(DC.SCENES))
def test_directed_and_mutual_forms_against_the_reference(name):
    descs = DC.scene(name)
    ordered = DC.ordered_pairs(len(descs))
    want_d = R.match_pairs_directed(descs, ordered, DC.MIN_SCORE)
    rows = sum(descs[a].shape[0] for a, _ in ordered)
    assert 0.10 * rows <= want_d[0].sum() <= 0.90 * rows        # both branches of the threshold are exercised
    pairs = synth.all_pairs(len(descs))
    with HipContext(0) as ctx:
        _upload(ctx, descs)
        _same(ctx.match_pairs_directed_dot(ordered, DC.MIN_SCORE), want_d, "directed")
        for a, b in ordered[:3]:
            q, t, s = ctx.match_pair_dot(int(a), int(b), DC.MIN_SCORE)
            wq, wt, ws = R.match_directed(descs[a], descs[b], DC.MIN_SCORE)
            assert np.array_equal(q, wq) and np.array_equal(t, wt) and np.array_equal(_bits(s), _bits(ws))
        # every pair an edge; then thresholds that drop some pairs and keep others
        loose = R.match_all_pairs(descs, pairs, DC.MIN_SCORE, 0, -1)
        _same(ctx.match_all_pairs_dot(pairs, DC.MIN_SCORE, 0, -1), loose, "mutual, no thresholds")
        mut = np.sort(loose[5][:, 2])
        cut = int(mut[len(mut) // 2])                              # |mutual| > cut holds for some pairs and fails for others
        tight = R.match_all_pairs(descs, pairs, DC.MIN_SCORE, 5, cut)
        assert 0 < (tight[0] > 0).sum() < len(pairs) or mut[0] == mut[-1]
        got = ctx.match_all_pairs_dot(pairs, DC.MIN_SCORE, 5, cut)
        _same(got, tight, "mutual with thresholds")
        nostats = ctx.match_all_pairs_dot(pairs, DC.MIN_SCORE, 5, cut, stats=False)
        assert nostats[5] is None
        _same(nostats[:5], tight[:5], "mutual without stats")


def test_padding_rows_and_columns_are_excluded_by_index():
    """All true similarities are negative: a padded row or column (zero fragments, similarity exactly 0) would beat every real
    one. n = 70 leaves 26 padded rows in the last tile and a whole padded tile behind it."""
    a, b = DC.negative_pair()
    n = a.shape[0]
    assert n == 70 and (a.astype(np.float64) @ b.astype(np.float64).T).max() < 0
    with HipContext(0) as ctx:
        _upload(ctx, [a, b])
        q, t, s = ctx.match_pair_dot(0, 1, -2.0)
        assert np.array_equal(q, np.arange(n)) and t.max() < n and (s < 0).all()   # every row matches a REAL row
        wq, wt, ws = R.match_directed(a, b, -2.0)
        assert np.array_equal(t, wt) and np.array_equal(_bits(s), _bits(ws))
        for pairs in ([[0, 1]], [[1, 0]]):
            got = ctx.match_all_pairs_dot(pairs, -2.0, 0, -1)
            assert got[5][0, 0] == n and got[5][0, 1] == n                          # both directions: all 70, none of them padding
            assert len(got[2]) and got[2].max() < n and got[3].max() < n
            _same(got, R.match_all_pairs([a, b], pairs, -2.0, 0, -1), "negative scene, mutual")


def test_one_row_and_zero_row_train_frames_and_ties():
    A = DC.scene("d64")[0]
    one, empty = A[5:6].copy(), np.zeros((0, A.shape[1]), np.float32)
    dup = np.concatenate([A[:40], A[:40]])                                          # duplicate train rows -> lower index
    descs = [A, one, empty, dup]
    ordered = [[0, 1], [1, 0], [0, 2], [2, 0], [0, 3], [3, 0]]
    with HipContext(0) as ctx:
        _upload(ctx, descs)
        for ms in (0.9, -2.0):
            _same(ctx.match_pairs_directed_dot(ordered, ms), R.match_pairs_directed(descs, ordered, ms), f"directed {ms}")
            _same(ctx.match_all_pairs_dot(ordered, ms, 0, -1), R.match_all_pairs(descs, ordered, ms, 0, -1), f"mutual {ms}")
        q, t, s = ctx.match_pair_dot(0, 3, 0.9)
        assert len(q) == 40 and t.max() < 40
        # a similarity exactly equal to min_score is rejected: take a score the device itself reports as the threshold
        q, t, s = ctx.match_pair_dot(0, 1, -2.0)
        thr = float(s[7])
        q2, _, _ = ctx.match_pair_dot(0, 1, thr)
        wq2, _, _ = R.match_directed(A, one, thr)
        assert 7 not in q2.tolist() and np.array_equal(q2, wq2)


def test_job_cut_into_more_than_one_launch():
    """33 frames of 2000 rows: 528 pairs against the 500 per launch that the planner's per_pair formula gives at 2000-row frames.
    Reference samples on both sides of the launch boundary (and both ends of the job)."""
    batch = DC.multi_launch_batch(2000)
    F = 33
    pairs = synth.all_pairs(F)
    assert batch == 500 and len(pairs) > batch
    descs = DC.float_frames(64, [2000] * F, 1200, 77)
    samples = [0, batch - 1, batch, len(pairs) - 1]
    with HipContext(0) as ctx:
        _upload(ctx, descs)
        counts, offsets, q, t, s, st = ctx.match_all_pairs_dot(pairs, DC.MIN_SCORE, 30, 30)
        assert np.array_equal(offsets[1:], np.cumsum(counts)) and offsets[0] == 0 and len(q) == offsets[-1]
        dc, do, dq, dt, ds = ctx.match_pairs_directed_dot(pairs, DC.MIN_SCORE)
        assert np.array_equal(do[1:], np.cumsum(dc))
    for p in samples:
        a, b = pairs[p]
        wq, wt, ws, wst = R.match_mutual(descs[a], descs[b], DC.MIN_SCORE, 30, 30)
        assert 200 < len(wq) < 1800                                    # the threshold cuts both ways
        sl = slice(offsets[p], offsets[p + 1])
        assert np.array_equal(q[sl], wq) and np.array_equal(t[sl], wt) and np.array_equal(_bits(s[sl]), _bits(ws)), p
        assert np.array_equal(st[p], wst), p
        wq, wt, ws = R.match_directed(descs[a], descs[b], DC.MIN_SCORE)
        sl = slice(do[p], do[p + 1])
        assert np.array_equal(dq[sl], wq) and np.array_equal(dt[sl], wt) and np.array_equal(_bits(ds[sl]), _bits(ws)), p


def _repetition(short, idx):
    """The CSR (counts, offsets, q, t, scores, stats) of the pairs of `short` in the order `idx`."""
    per = lambda k: [short[k][short[1][p]:short[1][p + 1]] for p in range(len(short[0]))]     # noqa: E731
    counts = short[0][idx]
    return (counts, np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64),
            *(np.concatenate([per(k)[i] for i in idx]) for k in (2, 3, 4)), None if short[5] is None else short[5][idx])


def test_packed_and_direct_results_in_one_call():
    """IoStage::PACK_MAX (eacham_amd/csrc/context.hpp) is 256 KiB = 262 144 B. At 33 000 pairs the counts (132 000 B) travel through
    the pinned mirror, the offsets (264 008 B) and the stats (528 000 B) lie above it and take their own direct copy: the 12 ordered
    pairs of four 40-row frames (two 32-row tiles, the second mostly padding), repeated cyclically, must give the 12-pair call's
    results (all of them packed) repeated, byte for byte, with the offsets their running sum."""
    descs = DC.float_frames(32, [40] * 4, 25, 311)
    ordered = DC.ordered_pairs(4)
    idx = np.arange(33000) % 12
    want = R.match_all_pairs(descs, ordered, DC.MIN_SCORE, 0, -1)
    assert (want[0] > 0).all() and want[0].min() < 40
    with HipContext(0) as ctx:
        _upload(ctx, descs)
        for stats in (True, False):
            short = ctx.match_all_pairs_dot(ordered, DC.MIN_SCORE, 0, -1, stats=stats)
            _same(short[:5], want[:5], f"12 pairs, stats={stats}")
            assert np.array_equal(short[5], want[5]) if stats else short[5] is None
            long = ctx.match_all_pairs_dot(ordered[idx], DC.MIN_SCORE, 0, -1, stats=stats)
            for name, g, w in zip(["counts", "offsets", "q", "t", "scores", "stats"], long, _repetition(short, idx)):
                assert (g is None and w is None) or np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), (name, stats)


def test_error_paths():
    descs = DC.scene("d64")
    with HipContext(0) as ctx:
        # int8 frames: dot-product needs float frames
        ctx.clear_descriptors()
        u8 = synth.random_u8_descriptors(50, 64, 3)
        ctx.upload_descriptors(0, u8)
        ctx.upload_descriptors(1, u8)
        for call in (lambda: ctx.match_pair_dot(0, 1), lambda: ctx.match_pairs_directed_dot([[0, 1]]),
                     lambda: ctx.match_all_pairs_dot([[0, 1]])):
            with pytest.raises(capi.EachamError) as e:
                call()
            assert e.value.code == capi.ERR_UNSUPPORTED and "float frames" in str(e.value)
        _upload(ctx, descs[:2])
        # a frame that is not resident
        for call in (lambda: ctx.match_pair_dot(0, 9), lambda: ctx.match_pairs_directed_dot([[0, 1], [9, 0]], cap=1000),
                     lambda: ctx.match_all_pairs_dot([[0, 1], [1, 9]], cap=1000)):
            with pytest.raises(capi.EachamError) as e:
                call()
            assert e.value.code == capi.ERR_INVALID and "not resident" in str(e.value)
        # capacity exceeded
        for call in (lambda: ctx.match_pairs_directed_dot([[0, 1]], cap=3), lambda: ctx.match_all_pairs_dot([[0, 1]], 0.5, 0, -1, cap=3)):
            with pytest.raises(capi.EachamError) as e:
                call()
            assert e.value.code == capi.ERR_CAPACITY and "capacity" in str(e.value)
        L, cnt = capi.lib(), __import__("ctypes").c_int(0)
        q = np.zeros(3, np.uint32)
        rc = L.eacham_match_pair_dot(ctx.handle, 0, 1, 0.5, q.ctypes.data, q.ctypes.data, None, 3, __import__("ctypes").byref(cnt))
        assert rc == capi.ERR_CAPACITY and cnt.value > 3 and b"capacity" in L.eacham_last_error(ctx.handle)
        # out_score may be NULL
        want = R.match_directed(descs[0], descs[1], 0.5)
        q, t = np.zeros(len(descs[0]), np.uint32), np.zeros(len(descs[0]), np.uint32)
        rc = L.eacham_match_pair_dot(ctx.handle, 0, 1, 0.5, q.ctypes.data, t.ctypes.data, None, len(q), __import__("ctypes").byref(cnt))
        assert rc == capi.OK and np.array_equal(q[:cnt.value], want[0]) and np.array_equal(t[:cnt.value], want[1])
        # and the context still works after the errors
        _same(ctx.match_pairs_directed_dot([[0, 1]]), R.match_pairs_directed(descs, [[0, 1]], 0.5), "after errors")


def test_l2_float_path_is_unchanged_by_a_dot_call():
    """Shared workspace state: an L2 call on the same resident float frames returns what it returned before."""
    descs = DC.scene("d128")
    pairs = synth.all_pairs(len(descs))
    with HipContext(0) as ctx:
        _upload(ctx, descs)
        before = ctx.match_all_pairs(pairs, min_dir=5, min_mutual=5)
        pair_before = ctx.match_pair(0, 1)
        assert before[0].sum() > 0 and len(pair_before[0]) > 0
        ctx.match_all_pairs_dot(pairs, DC.MIN_SCORE, 0, -1)
        pair_after = ctx.match_pair(0, 1)
        ctx.match_pair_dot(1, 0, DC.MIN_SCORE)
        ctx.match_pairs_directed_dot(DC.ordered_pairs(len(descs)), -2.0)
        after = ctx.match_all_pairs(pairs, min_dir=5, min_mutual=5)
        for g, w in zip(after, before):
            assert np.array_equal(g, w)
        assert np.array_equal(pair_after[0], pair_before[0]) and np.array_equal(pair_after[1], pair_before[1])
        again = ctx.match_pair(0, 1)
        assert np.array_equal(again[0], pair_before[0]) and np.array_equal(again[1], pair_before[1])


def test_python_mirror_of_the_adapter():
    from eacham_amd import FeatureMatcherDotHip
    descs = DC.scene("d64")
    for mutual in (True, False):
        m = FeatureMatcherDotHip(DC.MIN_SCORE, mutual)
        got = m.Match(descs[0], descs[1])
        if mutual:
            wq, wt, ws, _ = R.match_mutual(descs[0], descs[1], DC.MIN_SCORE, 0, -1)
        else:
            wq, wt, ws = R.match_directed(descs[0], descs[1], DC.MIN_SCORE)
        assert got == dict(zip(wq.tolist(), wt.tolist())) and len(got) > 10
        assert m.LastScores() == dict(zip(wq.tolist(), ws.tolist()))
        m.ctx.close()


def _vec(f, dtype):
    n = struct.unpack("q", f.read(8))[0]
    return np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype=dtype).copy()


def test_cpp_adapter_from_16_threads(tmp_path):
    """include/eacham/FeatureMatcherHip.hpp: FeatureMatcherDotHip called from 16 threads on one shared instance, mutual on and
    off, and MatchAllPairsDot — held against the C-ABI's own results (through the ctypes mirror) and the reference."""
    tmp = str(tmp_path)
    exe, lib = os.path.join(tmp, "match_dot_driver"), os.path.join(ROOT, "eacham_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "match_dot_driver.cpp"),
                    "-o", exe, "-L" + lib, "-leacham_hip", "-Wl,-rpath," + lib, "-lpthread"], check=True, capture_output=True)
    descs = DC.scene("d256") + [DC.scene("d256")[0][:1].copy()]      # + a one-row frame
    dim, F = descs[0].shape[1], len(descs)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("ii", F, dim))
        for d in descs:
            f.write(struct.pack("i", d.shape[0]))
            f.write(np.ascontiguousarray(d, np.float32).tobytes())
    r = subprocess.run([exe, fin, fout, "16", repr(DC.MIN_SCORE), "5", "5"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ordered = DC.ordered_pairs(F)
    pairs = synth.all_pairs(F)
    with HipContext(0) as ctx:
        _upload(ctx, descs)
        abi_mut = ctx.match_all_pairs_dot(ordered, DC.MIN_SCORE, 0, -1)
        abi_dir = ctx.match_pairs_directed_dot(ordered, DC.MIN_SCORE)
        abi_all = ctx.match_all_pairs_dot(pairs, DC.MIN_SCORE, 5, 5)
    _same(abi_dir, R.match_pairs_directed(descs, ordered, DC.MIN_SCORE), "C-ABI directed")
    with open(fout, "rb") as f:
        for abi in (abi_mut, abi_dir):
            _, off, q, t, s = abi[:5]
            for p in range(len(ordered)):
                n = struct.unpack("q", f.read(8))[0]
                qt = np.frombuffer(f.read(8 * n), np.uint32).reshape(-1, 2)
                sc = np.frombuffer(f.read(4 * n), np.float32)
                sl = slice(off[p], off[p + 1])
                assert np.array_equal(qt[:, 0], q[sl]) and np.array_equal(qt[:, 1], t[sl]) and np.array_equal(_bits(sc), _bits(s[sl])), p
        counts, gq, gt, gs = _vec(f, np.int32), _vec(f, np.uint32), _vec(f, np.uint32), _vec(f, np.float32)
    assert np.array_equal(counts, abi_all[0]) and np.array_equal(gq, abi_all[2]) and np.array_equal(gt, abi_all[3])
    assert np.array_equal(_bits(gs), _bits(abi_all[4])) and counts.sum() > 0
