"""GPU: binary descriptors of up to 64 bytes per row as frames of the wide kind (eacham_upload_descriptors_bits_wide; the FP4 sweep of
eacham_amd/csrc/matcher_ham_wide.hip behind eacham_match_*_hamming) against the numpy reference (tests/ham_reference.py): the
sweep's top-2 on every row, counts, offsets, q, t, the Hamming distances and stats, as bytes. Every comparison is equality."""
import contextlib
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from eacham_amd import HipContext, capi, synth
import ham_cases as HC
import ham_reference as R
import ham_wide_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NAMES = ["counts", "offsets", "q", "t", "dist", "stats"]


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"{what}: {name} differ"


@contextlib.contextmanager
def _context(**env):
    """A context of its own with the diagnostic switches that eacham_ctx_create reads from the environment."""
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
        ctx.upload_descriptors_bits_wide(f, d)


def _top2_equal(ctx, a, b, D, what):
    best, h0, h1 = ctx.match_debug_hamming_wide_pair(a, b)
    wb, w0, w1 = R.top2(D)
    assert np.array_equal(best, wb), f"{what}: best differ at rows {np.nonzero(best != wb)[0][:8]}"
    assert np.array_equal(h0, w0), f"{what}: h0 differ at rows {np.nonzero(h0 != w0)[0][:8]}"
    assert np.array_equal(h1, w1), f"{what}: h1 differ at rows {np.nonzero(h1 != w1)[0][:8]}"


@pytest.mark.parametrize("name", sorted(W.SCENES))
def test_sweep_top2_every_row(name):
    """The MFMA lane map and the key arithmetic on every row of every ordered pair, not only on rows that pass the ratio test."""
    ref = W.reference(name)
    done = 0
    with HipContext(0) as ctx:
        _upload(ctx, ref.descs)
        for a, b in HC.ordered_pairs(len(ref.descs)):
            if len(ref.descs[b]) < 2:
                continue
            _top2_equal(ctx, int(a), int(b), ref.D(a, b), f"{name} ({a}, {b})")
            done += 1
    assert done >= 6


@pytest.mark.parametrize("name", sorted(W.SCENES))
def test_directed_and_mutual(name):
    ref = W.reference(name)
    ordered = HC.ordered_pairs(len(ref.descs))
    pairs = synth.all_pairs(len(ref.descs))
    with HipContext(0) as ctx:
        _upload(ctx, ref.descs)
        _same(ctx.match_pairs_directed_hamming(ordered, W.RATIO), ref.match_pairs_directed(ordered, W.RATIO), "directed")
        _same(ctx.match_pairs_directed_hamming(ordered, 1.25), ref.match_pairs_directed(ordered, 1.25), "directed, ratio 1.25")
        a, b = (int(v) for v in ordered[-1])
        for g, w in zip(ctx.match_pair_hamming(a, b, W.RATIO), R.directed_from(ref.D(a, b), W.RATIO)):
            assert g.tobytes() == w.tobytes()
        for both in (pairs, ordered):
            for min_dir, min_mutual in ((30, 30), (0, -1)):
                want = ref.match_all_pairs(both, W.RATIO, min_dir, min_mutual)
                _same(ctx.match_all_pairs_hamming(both, W.RATIO, min_dir, min_mutual), want, f"mutual {min_dir}/{min_mutual} with stats")
                lean = ctx.match_all_pairs_hamming(both, W.RATIO, min_dir, min_mutual, stats=False)
                assert lean[5] is None
                _same(lean[:5], want[:5], f"mutual {min_dir}/{min_mutual} without stats")
            assert want[0].sum() > 0
        dbg = ctx.match_debug_hamming_wide()
        assert dbg["batches"] == 1 and dbg["query_rows"] == sum(len(ref.descs[a]) + len(ref.descs[b]) for a, b in ordered)


def test_extremes():
    nb = 64
    zeros, ones = np.zeros((1, nb), np.uint8), np.full((3, nb), 255, np.uint8)
    x, y, z = HC._bytes(77, 1, (3, nb))
    bq, bt, _, expect = HC.boundary_frames(nb)
    frames = [zeros, ones,                                         # 0, 1: h = 512 three times
              np.array([x, y]), np.array([x, x, y, z]),            # 2, 3: 0 / 0 fails; 0 against h1 > 0 passes
              bq, bt]                                              # 4, 5
    cases = [(204, 255, False), (400, 500, False), (408, 510, False), (399, 500, True)]
    for h0, h1, _ in cases:                                        # 6.., two frames per case: one query row, its two train rows
        frames += [x[None].copy(), np.array(W.pair_at(nb, x, h0, h1))]
    far = HC._bytes(78, 1, (260, nb))                              # random rows lie ~256 bits from x
    far[30], far[230] = W.pair_at(nb, x, 7, 7)                     # two holders of the minimum, 200 rows apart
    t_tie = len(frames)
    frames += [x[None].copy(), far]
    ref = R.Scene(frames)
    with HipContext(0) as ctx:
        _upload(ctx, frames)
        best, h0, h1 = ctx.match_debug_hamming_wide_pair(0, 1)
        assert (best.tolist(), h0.tolist(), h1.tolist()) == ([0], [512], [512])
        q, t, d = ctx.match_pair_hamming(0, 1, 0.8)
        assert len(q) == 0
        q, t, d = ctx.match_pair_hamming(0, 1, 1.25)
        assert (q.tolist(), t.tolist(), d.tolist()) == ([0], [0], [512])
        q, t, d = ctx.match_pair_hamming(2, 3, 0.8)
        assert (q.tolist(), t.tolist(), d.tolist()) == ([1], [2], [0])
        _top2_equal(ctx, 2, 3, ref.D(2, 3), "identical rows")
        q, t, d = ctx.match_pair_hamming(4, 5, 0.8)
        assert q.tolist() == [5, 6] and t.tolist() == expect[[5, 6]].tolist() and d.tolist() == [0, 3]
        _top2_equal(ctx, 4, 5, ref.D(4, 5), "boundary_frames")
        _top2_equal(ctx, 5, 4, ref.D(5, 4), "boundary_frames, reverse")
        for k, (c0, c1, passes) in enumerate(cases):
            a, b = 6 + 2 * k, 7 + 2 * k
            best, h0, h1 = ctx.match_debug_hamming_wide_pair(a, b)
            assert (best.tolist(), h0.tolist(), h1.tolist()) == ([0], [c0], [c1])
            q, t, d = ctx.match_pair_hamming(a, b, 0.8)
            assert (q.tolist(), t.tolist(), d.tolist()) == (([0], [0], [c0]) if passes else ([], [], [])), (c0, c1)
        best, h0, h1 = ctx.match_debug_hamming_wide_pair(t_tie, t_tie + 1)
        assert (best.tolist(), h0.tolist(), h1.tolist()) == ([30], [7], [7])
        q, t, d = ctx.match_pair_hamming(t_tie, t_tie + 1, 1.25)
        assert (q.tolist(), t.tolist(), d.tolist()) == ([0], [30], [7])
        ordered = np.array([[0, 1], [2, 3], [3, 2], [4, 5], [5, 4], [6, 7], [8, 9], [10, 11], [12, 13], [t_tie, t_tie + 1], [t_tie + 1, t_tie]], np.int32)
        _same(ctx.match_pairs_directed_hamming(ordered, 0.8), ref.match_pairs_directed(ordered, 0.8), "directed")
        _same(ctx.match_all_pairs_hamming(ordered, 0.8, 0, -1), ref.match_all_pairs(ordered, 0.8, 0, -1), "mutual")


def test_high_train_indices():
    """The 14-bit index field of the key: a train frame of 16384 rows with the neighbours at both ends of it and around 2^13."""
    nb = 64
    qf = HC._bytes(91, 1, (40, nb))
    tf = HC._bytes(91, 2, (16384, nb))
    for k, at in enumerate((31, 32, 8191, 8192, 16383)):
        tf[at] = W.pair_at(nb, qf[k], 3 + k, 0)[0]                 # near-duplicates, 3..7 bits off
    tf[5000] = tf[12000] = qf[5]                                   # an exact duplicate pair: h0 = h1 = 0, the lower index holds it
    D = R.distances(qf, tf)
    wb, w0, w1 = R.top2(D)
    assert wb[:6].tolist() == [31, 32, 8191, 8192, 16383, 5000] and w0[:6].tolist() == [3, 4, 5, 6, 7, 0] and w1[5] == 0
    ref = R.Scene([qf, tf])
    ref._D[(0, 1)] = D
    with HipContext(0) as ctx:
        _upload(ctx, [qf, tf])
        _top2_equal(ctx, 0, 1, D, "16384 train rows")
        want = ref.match_pairs_directed([[0, 1], [1, 0]], W.RATIO)
        assert want[0][0] == 5 and want[0][1] > 0
        _same(ctx.match_pairs_directed_hamming([[0, 1], [1, 0]], W.RATIO), want, "directed")
        _top2_equal(ctx, 1, 0, D.T, "16384 query rows")


@pytest.mark.parametrize("name", sorted(HC.SCENES))
def test_same_bytes_as_the_narrow_kind(name):
    """Two independent arithmetic paths on the same rows: 0 / 255 in the int8 kernels, +-1 on the FP4 matrix cores."""
    descs = HC.reference(name).descs
    ordered = HC.ordered_pairs(len(descs))
    out = []
    for wide in (False, True):
        with HipContext(0) as ctx:
            ctx.clear_descriptors()
            for f, d in enumerate(descs):
                (ctx.upload_descriptors_bits_wide if wide else ctx.upload_descriptors_bits)(f, d)
            out.append((ctx.match_pairs_directed_hamming(ordered, HC.RATIO), ctx.match_all_pairs_hamming(ordered, HC.RATIO, 30, 30),
                        ctx.match_all_pairs_hamming(ordered, HC.RATIO, 0, -1)))
    assert out[0][0][0].sum() > 0 and out[0][2][0].sum() > 0
    for narrow, wide, what in zip(out[0], out[1], ("directed", "mutual 30/30", "mutual 0/-1")):
        _same(wide, narrow, what)


def test_batch_boundaries():
    """28 pairs cut into two launches or more: the same bytes as under the default budget, and as the reference."""
    F = 8
    descs = HC.binary_frames(64, [600] * F, 400, W.SEED, inject=False)
    pairs = synth.all_pairs(F)
    want = R.Scene(descs).match_all_pairs(pairs, W.RATIO, 30, 30)
    assert (want[5][:, 3] == 1).all() and want[0].min() > 100
    with _context(EACHAM_MATCH_BUDGET_MB=0.25) as ctx:
        _upload(ctx, descs)
        cut = ctx.match_all_pairs_hamming(pairs, W.RATIO, 30, 30)
        dbg = ctx.match_debug_hamming_wide()
        assert dbg["batches"] >= 2 and dbg["pairs_per_batch"] < len(pairs) and dbg["sweep_launches"] == dbg["batches"], dbg
        assert dbg["query_rows"] == 2 * 600 * len(pairs)
        cut_lean = ctx.match_all_pairs_hamming(pairs, W.RATIO, 30, 30, stats=False)
        cut_dir = ctx.match_pairs_directed_hamming(pairs, W.RATIO)
        assert ctx.match_debug_hamming_wide()["batches"] >= 2
    with HipContext(0) as ctx:
        _upload(ctx, descs)
        whole = ctx.match_all_pairs_hamming(pairs, W.RATIO, 30, 30)
        assert ctx.match_debug_hamming_wide()["batches"] == 1
        whole_dir = ctx.match_pairs_directed_hamming(pairs, W.RATIO)
    _same(cut, want, "cut against the reference")
    _same(cut, whole, "cut against one launch")
    _same(cut_lean[:5], want[:5], "cut, without stats")
    _same(cut_dir, whole_dir, "directed, cut against one launch")


def test_device_pointer_forms():
    import torch
    ref = W.reference("w64")
    descs = ref.descs
    pairs = np.array([[0, 1], [0, 2], [2, 1], [1, 0]], np.int32)
    dev = torch.device("cuda", 0)
    with HipContext(0) as ctx:
        ext = torch.cuda.ExternalStream(ctx.stream, device=dev)
        with torch.cuda.stream(ext):
            ctx.clear_descriptors()
            keep = [torch.from_numpy(d).to(dev) for d in descs]
            ctx.sync()
            for f, (d, td) in enumerate(zip(descs, keep)):
                ctx.upload_descriptors_bits_wide_dev(f, td.data_ptr(), d.shape[0], d.shape[1])
            host = ctx.match_all_pairs_hamming(pairs, W.RATIO, 5, 5)
            _same(host, ref.match_all_pairs(pairs, W.RATIO, 5, 5), "host form on device uploads")
            cap = len(host[2])
            assert cap > 100
            for with_stats, with_dist in ((True, True), (False, True), (False, False)):
                pd = torch.from_numpy(pairs).to(dev)
                counts = torch.full((len(pairs),), -1, dtype=torch.int32, device=dev)
                offsets = torch.zeros(len(pairs) + 1, dtype=torch.int64, device=dev)
                total = torch.zeros(1, dtype=torch.int64, device=dev)
                edges = torch.zeros(2 * cap, dtype=torch.int32, device=dev)
                dist = torch.full((cap,), -7, dtype=torch.int32, device=dev)
                st = torch.zeros(4 * len(pairs), dtype=torch.int32, device=dev)
                ctx.match_all_pairs_hamming_dev(pd.data_ptr(), len(pairs), counts.data_ptr(), offsets.data_ptr(), edges.data_ptr(), cap,
                                                total.data_ptr(), st.data_ptr() if with_stats else 0, dist.data_ptr() if with_dist else 0,
                                                ratio=W.RATIO, min_dir=5, min_mutual=5)
                ctx.sync()
                assert int(total.item()) == cap
                assert np.array_equal(counts.cpu().numpy(), host[0]) and np.array_equal(offsets.cpu().numpy(), host[1])
                e2 = edges.cpu().numpy().view(np.uint32).reshape(-1, 2)
                assert np.array_equal(e2[:, 0], host[2]) and np.array_equal(e2[:, 1], host[3])
                assert np.array_equal(dist.cpu().numpy(), host[4] if with_dist else np.full(cap, -7, np.int32))
                if with_stats:
                    assert np.array_equal(st.cpu().numpy().reshape(-1, 4), host[5])


def _l2_directed(ctx):
    pr, cnt, off, total = np.array([[0, 1]], np.int32), np.zeros(1, np.int32), np.zeros(2, np.int64), C.c_int64(0)
    ctx._check(ctx._L.eacham_match_pairs_directed(ctx.handle, pr.ctypes.data, 1, 0.8, cnt.ctypes.data, off.ctypes.data, None, None, 0, C.byref(total)))


def test_limits_are_errors():
    ref = W.reference("w64")
    descs = ref.descs
    want = ref.match_pairs_directed([[0, 1]], W.RATIO)
    u8 = synth.random_u8_descriptors(50, 128, 3)
    f32 = synth.unit_float_descriptors(50, 128, 3)
    narrow = HC.reference("b16").descs[0]
    with HipContext(0) as ctx:
        def raises(call, code, text):
            with pytest.raises(capi.EachamError) as e:
                call()
            assert e.value.code == code and text in str(e.value), str(e.value)
            # the next valid call succeeds with the right answer
            _same(ctx.match_pairs_directed_hamming([[0, 1]], W.RATIO), want, f"after: {text}")

        _upload(ctx, descs[:2])
        raises(lambda: ctx.upload_descriptors_bits_wide(2, np.zeros((4, 65), np.uint8)), capi.ERR_UNSUPPORTED, "64")
        raises(lambda: ctx.upload_descriptors_bits_wide(2, np.zeros((16385, 64), np.uint8)), capi.ERR_UNSUPPORTED, "16384")
        raises(lambda: ctx.upload_descriptors_bits_wide(2, np.zeros((4, 0), np.uint8)), capi.ERR_INVALID, "shape")
        raises(lambda: ctx._check(ctx._L.eacham_upload_descriptors_bits_wide(ctx.handle, 2, None, 4, 64)), capi.ERR_INVALID, "null")
        raises(lambda: ctx.upload_descriptors_bits_wide(2, descs[0][:, :48]), capi.ERR_UNSUPPORTED, "bytes per row")
        # other kinds on top of wide frames
        raises(lambda: ctx.upload_descriptors(2, u8), capi.ERR_UNSUPPORTED, "kind")
        raises(lambda: ctx.upload_descriptors_f32(2, f32), capi.ERR_UNSUPPORTED, "kind")
        raises(lambda: ctx.upload_descriptors_bits(2, narrow), capi.ERR_UNSUPPORTED, "kind")
        # the L2 and dot-product calls on wide frames
        for call in (lambda: ctx.match_pair(0, 1), lambda: ctx.match_all_pairs([[0, 1]], stats=False), lambda: ctx.match_all_pairs([[0, 1]]),
                     lambda: _l2_directed(ctx)):
            raises(call, capi.ERR_UNSUPPORTED, "binary")
        for call in (lambda: ctx.match_pair_dot(0, 1), lambda: ctx.match_all_pairs_dot([[0, 1]]),
                     lambda: ctx.match_all_pairs_dot([[0, 1]], screened=True)):
            raises(call, capi.ERR_UNSUPPORTED, "float frames")
        import torch
        z = torch.zeros(64, dtype=torch.int64, device="cuda:0")
        raises(lambda: ctx.match_all_pairs_dev(z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), 4, z.data_ptr()),
               capi.ERR_UNSUPPORTED, "binary")
        # the debug pair call: a one-row train frame, a frame that is not resident, too small a capacity
        ctx.upload_descriptors_bits_wide(2, descs[0][:1])
        raises(lambda: ctx.match_debug_hamming_wide_pair(0, 2), capi.ERR_INVALID, "two or more")
        raises(lambda: ctx.match_debug_hamming_wide_pair(0, 9), capi.ERR_INVALID, "not resident")
        b = np.zeros(4, np.int32)
        raises(lambda: ctx._check(ctx._L.eacham_match_debug_hamming_wide_pair(ctx.handle, 0, 1, b.ctypes.data, b.ctypes.data, b.ctypes.data, 4)),
               capi.ERR_CAPACITY, "capacity")
        raises(lambda: ctx.match_all_pairs_hamming([[0, 1]], 1.25, 0, -1), capi.ERR_INVALID, "ratio")
        raises(lambda: ctx.match_pairs_directed_hamming([[0, 1]], cap=3), capi.ERR_CAPACITY, "capacity")
        # wide frames on top of other kinds; eacham_clear_descriptors resets the kind
        for up in (lambda f: ctx.upload_descriptors(f, u8), lambda f: ctx.upload_descriptors_f32(f, f32), lambda f: ctx.upload_descriptors_bits(f, narrow)):
            ctx.clear_descriptors()
            up(0), up(1)
            with pytest.raises(capi.EachamError) as e:
                ctx.upload_descriptors_bits_wide(2, descs[0])
            assert e.value.code == capi.ERR_UNSUPPORTED and "kind" in str(e.value)
            with pytest.raises(capi.EachamError) as e:
                ctx.match_debug_hamming_wide_pair(0, 1)
            assert e.value.code == capi.ERR_UNSUPPORTED
        _upload(ctx, descs[:2])
        _same(ctx.match_pairs_directed_hamming([[0, 1]], W.RATIO), want, "after clear")
    # the narrow upload still refuses 33 bytes, in the same words
    with HipContext(0) as ctx:
        with pytest.raises(capi.EachamError) as e:
            ctx.upload_descriptors_bits(0, np.zeros((4, 33), np.uint8))
        assert e.value.code == capi.ERR_UNSUPPORTED and "<= 32" in str(e.value)


def test_python_mirror_of_the_adapter_wide():
    from eacham_amd import FeatureMatcherHammingHip
    ref = W.reference("w61")
    for mutual in (False, True):
        m = FeatureMatcherHammingHip(W.RATIO, mutual)
        got = m.Match(ref.descs[0], ref.descs[1])
        wq, wt, wd = (R.mutual_from(ref.D(0, 1), W.RATIO, 0, -1) if mutual else R.directed_from(ref.D(0, 1), W.RATIO))[:3]
        assert got == dict(zip(wq.tolist(), wt.tolist())) and len(got) > 10
        assert m.LastDistances() == dict(zip(wq.tolist(), wd.tolist()))
        m.ctx.close()


def _vec(f, dtype):
    n = struct.unpack("q", f.read(8))[0]
    return np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype=dtype).copy()


def test_cpp_adapter_wide(tmp_path):
    """include/eacham/FeatureMatcherHip.hpp on 64-byte rows: FeatureMatcherHammingHip from 8 threads on one shared instance, directed
    and mutual, and MatchAllPairsHamming (tests/cpp/match_hamming_driver.cpp, which reads the bytes per row from its input)."""
    tmp = str(tmp_path)
    exe, lib = os.path.join(tmp, "match_hamming_driver"), os.path.join(ROOT, "eacham_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "match_hamming_driver.cpp"),
                    "-o", exe, "-L" + lib, "-leacham_hip", "-Wl,-rpath," + lib, "-lpthread"], check=True, capture_output=True)
    ref = W.reference("w64")
    descs = ref.descs
    F = len(descs)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("ii", F, descs[0].shape[1]))
        for d in descs:
            f.write(struct.pack("i", d.shape[0]))
            f.write(d.tobytes())
    r = subprocess.run([exe, fin, fout, "8", repr(W.RATIO), "5", "5"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ordered = HC.ordered_pairs(F)
    want_dir = ref.match_pairs_directed(ordered, W.RATIO)
    want_mut = ref.match_all_pairs(ordered, W.RATIO, 0, -1)
    want_all = ref.match_all_pairs(synth.all_pairs(F), W.RATIO, 5, 5)
    with open(fout, "rb") as f:
        for want in (want_dir, want_mut):
            _, off, q, t, d = want[:5]
            for p in range(len(ordered)):
                n = struct.unpack("q", f.read(8))[0]
                qt = np.frombuffer(f.read(8 * n), np.uint32).reshape(-1, 2)
                dd = np.frombuffer(f.read(4 * n), np.int32)
                sl = slice(off[p], off[p + 1])
                assert np.array_equal(qt[:, 0], q[sl]) and np.array_equal(qt[:, 1], t[sl]) and np.array_equal(dd, d[sl]), p
        counts, gq, gt, gd = _vec(f, np.int32), _vec(f, np.uint32), _vec(f, np.uint32), _vec(f, np.int32)
    assert np.array_equal(counts, want_all[0]) and np.array_equal(gq, want_all[2]) and np.array_equal(gt, want_all[3])
    assert np.array_equal(gd, want_all[4]) and counts.sum() > 0
