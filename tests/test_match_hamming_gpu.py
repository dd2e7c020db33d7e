"""GPU: binary descriptors under Hamming distance (eacham_upload_descriptors_bits, eacham_match_*_hamming;
eacham_amd/csrc/matcher_ham.hip and the metric argument of the int8 kernels of matcher.hip) against the numpy reference
(tests/ham_reference.py): counts, offsets, q, t, the Hamming distances and stats, as bytes."""
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
        ctx.upload_descriptors_bits(f, d)


@pytest.mark.parametrize("colprune", ["1", "0"])
@pytest.mark.parametrize("name", sorted(HC.SCENES))
def test_scene_directed_lean_and_stats_forms(name, colprune):
    ref = HC.reference(name)
    descs = ref.descs
    ordered = HC.ordered_pairs(len(descs))
    pairs = synth.all_pairs(len(descs))
    with _context(EACHAM_MATCH_COLPRUNE=colprune) as ctx:
        _upload(ctx, descs)
        _same(ctx.match_pairs_directed_hamming(ordered, HC.RATIO), ref.match_pairs_directed(ordered, HC.RATIO), "directed")
        # above 1 a tied minimum passes: the lower train index must come out
        _same(ctx.match_pairs_directed_hamming(ordered, 1.25), ref.match_pairs_directed(ordered, 1.25), "directed, ratio 1.25")
        for a, b in ordered[:3]:
            got = ctx.match_pair_hamming(int(a), int(b), HC.RATIO)
            for g, w in zip(got, R.directed_from(ref.D(a, b), HC.RATIO)):
                assert g.tobytes() == w.tobytes(), (a, b)
        for both in (pairs, ordered):                           # (ordered: both roles of every frame)
            loose = ref.match_all_pairs(both, HC.RATIO, 0, -1)
            assert loose[0].sum() > 0
            lean = ctx.match_all_pairs_hamming(both, HC.RATIO, 0, -1, stats=False)
            assert lean[5] is None
            _same(lean[:5], loose[:5], "mutual, lean form")
            if colprune == "1":
                settled, verified = ctx.match_colprune()
                assert settled + verified > 0
            else:
                assert ctx.match_colprune()[0] == 0
            _same(ctx.match_all_pairs_hamming(both, HC.RATIO, 0, -1), loose, "mutual with stats")
        mut = np.sort(loose[5][:, 2])
        cut = int(mut[len(mut) // 2])                           # |mutual| > cut holds for some pairs and fails for others
        tight = ref.match_all_pairs(ordered, HC.RATIO, 2, cut)
        _same(ctx.match_all_pairs_hamming(ordered, HC.RATIO, 2, cut), tight, "mutual with thresholds, stats")
        _same(ctx.match_all_pairs_hamming(ordered, HC.RATIO, 2, cut, stats=False)[:5], tight[:5], "mutual with thresholds, lean")


@pytest.mark.parametrize("nbytes", [16, 32])
def test_boundary_rows(nbytes):
    """(4,5), (8,10), (40,50): 5 h0 = 4 h1 fails under Hamming (the square-root route lets them pass); (0,0), (3,3) fail; (0,3), (3,4) pass."""
    q, t, cases, expect = HC.boundary_frames(nbytes)
    want = R.match_directed(q, t, 0.8)
    assert want[0].tolist() == [5, 6] and want[1].tolist() == expect[[5, 6]].tolist() and want[2].tolist() == [0, 3]
    with HipContext(0) as ctx:
        _upload(ctx, [q, t])
        for g, w in zip(ctx.match_pair_hamming(0, 1, 0.8), want):
            assert g.tobytes() == w.tobytes()
        for stats in (True, False):
            got = ctx.match_all_pairs_hamming([[0, 1], [1, 0]], 0.8, 0, -1, stats=stats)
            _same(got[:5], R.match_all_pairs([q, t], [[0, 1], [1, 0]], 0.8, 0, -1)[:5], f"mutual, stats={stats}")
        # the train rows as queries: every row's nearest is its own anchor, the other row of its anchor lies h0 + h1 away
        _same(ctx.match_pairs_directed_hamming([[1, 0]], 0.8), R.match_pairs_directed([q, t], [[1, 0]], 0.8), "reverse")


def test_train_chunk_boundary():
    """4100 rows cross the 4096-row train chunk of the full-column sweep (7-bit tile field of its keys)."""
    descs = HC.binary_frames(8, [4100, 4100], 2500, 21)
    ref = R.Scene(descs)
    want = ref.match_all_pairs([[0, 1]], HC.RATIO, 30, 30)
    assert want[0][0] > 500
    with HipContext(0) as ctx:
        _upload(ctx, descs)
        _same(ctx.match_all_pairs_hamming([[0, 1]], HC.RATIO, 30, 30), want, "stats form")
        _same(ctx.match_all_pairs_hamming([[0, 1]], HC.RATIO, 30, 30, stats=False)[:5], want[:5], "lean form")
        _same(ctx.match_pairs_directed_hamming([[1, 0]], HC.RATIO), ref.match_pairs_directed([[1, 0]], HC.RATIO), "directed")


@pytest.mark.parametrize("stats", [False, True])
def test_job_cut_into_more_than_one_launch(stats):
    """20 frames of 2000 rows under a 16 MiB batch budget: eacham_match_debug_batches places the launch boundaries, the reference
    is sampled on both sides of each and at both ends of the job."""
    F = 20
    descs = HC.binary_frames(8, [2000] * F, 1200, 31, inject=False)
    pairs = synth.all_pairs(F)
    with _context(EACHAM_MATCH_BUDGET_MB=16) as ctx:
        _upload(ctx, descs)
        got = ctx.match_all_pairs_hamming(pairs, HC.RATIO, 30, 30, stats=stats)
        starts, _ = ctx.match_batches(len(pairs), stats)       # (the plan of the frames as the call above saw them)
        assert len(starts) > 1 and starts[0] == 0
    counts, offsets, q, t, d, st = got
    assert np.array_equal(offsets[1:], np.cumsum(counts)) and offsets[0] == 0 and len(q) == offsets[-1] == len(d)
    samples = sorted({0, len(pairs) - 1, *[int(s) - 1 for s in starts[1:]], *[int(s) for s in starts[1:]]})
    for p in samples:
        a, b = pairs[p]
        wq, wt, wd, wst = R.match_mutual(descs[a], descs[b], HC.RATIO, 30, 30)
        assert 200 < len(wq) < 1800
        sl = slice(offsets[p], offsets[p + 1])
        assert np.array_equal(q[sl], wq) and np.array_equal(t[sl], wt) and np.array_equal(d[sl], wd), p
        assert not stats or np.array_equal(st[p], wst), p


def test_device_pointer_form_equals_the_host_form():
    import torch
    name = "b32"
    descs = HC.reference(name).descs
    pairs = np.array([[0, 1], [0, 2], [2, 1], [1, 0], [0, 7]], np.int32)      # the last names a frame that is not resident
    dev = torch.device("cuda", 0)
    with HipContext(0) as ctx:
        ext = torch.cuda.ExternalStream(ctx.stream, device=dev)
        with torch.cuda.stream(ext):
            ctx.clear_descriptors()
            keep = [torch.from_numpy(d).to(dev) for d in descs]
            ctx.sync()
            for f, (d, td) in enumerate(zip(descs, keep)):
                ctx.upload_descriptors_bits_dev(f, td.data_ptr(), d.shape[0], d.shape[1])
            host = ctx.match_all_pairs_hamming(pairs[:4], HC.RATIO, 5, 5)
            _same(host, HC.reference(name).match_all_pairs(pairs[:4], HC.RATIO, 5, 5), "host form on device uploads")
            cap = len(host[2])
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
                                                ratio=HC.RATIO, min_dir=5, min_mutual=5)
                with pytest.raises(capi.EachamError) as e:          # the pair of the missing frame: no match, reported once
                    ctx.sync()
                assert e.value.code == capi.ERR_INVALID
                ctx.sync()
                assert int(total.item()) == cap
                assert np.array_equal(counts.cpu().numpy(), np.append(host[0], 0))
                assert np.array_equal(offsets.cpu().numpy(), np.append(host[1], host[1][-1]))
                e2 = edges.cpu().numpy().view(np.uint32).reshape(-1, 2)
                assert np.array_equal(e2[:, 0], host[2]) and np.array_equal(e2[:, 1], host[3])
                assert np.array_equal(dist.cpu().numpy(), host[4] if with_dist else np.full(cap, -7, np.int32))
                if with_stats:
                    assert np.array_equal(st.cpu().numpy().reshape(-1, 4)[:4], host[5])


def test_screen_bounds_are_valid_and_the_screen_decides_rows():
    """32-byte rows run the FP6 screen: per row L1 <= the true minimum 65025 h0 and U2 >= the true runner-up 65025 h1; on independent
    random rows (nothing near anything: every row fails the ratio test by far) the screen finishes rows on its own."""
    descs = HC.binary_frames(32, [300, 300], 120, 41)
    _, h0, h1 = R.top2(R.distances(descs[0], descs[1]))
    rand = [HC._bytes(43, f, (300, 32)) for f in range(2)]
    with HipContext(0) as ctx:
        _upload(ctx, descs)
        n1, l1, u2 = ctx.match_screen_pair(0, 1)
        assert (l1 >= 0).all() and (u2 >= 0).all()
        assert (l1 <= 65025 * h0).all() and (u2 >= 65025 * h1).all()
        assert (l1[h0 > 20] > 0).all()                           # and they say something: a far minimum has a positive lower bound
        ctx.match_all_pairs_hamming([[0, 1]], HC.RATIO, 0, -1, stats=False)
        rows, open_ = ctx.match_screen()
        assert rows == 300 and 0 < open_ <= rows                # true matches stay open for the exact pass
        _upload(ctx, rand)
        got = ctx.match_all_pairs_hamming([[0, 1]], HC.RATIO, 0, -1, stats=False)
        _same(got[:5], R.match_all_pairs(rand, [[0, 1]], HC.RATIO, 0, -1)[:5], "random rows")
        rows, open_ = ctx.match_screen()
        assert rows > 0 and open_ < rows


def _l2_directed(ctx):
    """eacham_match_pairs_directed on the resident frames (the mirror's own wrapper uploads frames first)."""
    pr, cnt, off, total = np.array([[0, 1]], np.int32), np.zeros(1, np.int32), np.zeros(2, np.int64), C.c_int64(0)
    ctx._check(ctx._L.eacham_match_pairs_directed(ctx.handle, pr.ctypes.data, 1, 0.8, cnt.ctypes.data, off.ctypes.data, None, None, 0, C.byref(total)))


def test_error_paths():
    descs = HC.reference("b16").descs
    u8 = synth.random_u8_descriptors(50, 128, 3)
    f32 = synth.unit_float_descriptors(50, 128, 3)
    ham_calls = lambda ctx: (lambda: ctx.match_pair_hamming(0, 1), lambda: ctx.match_pairs_directed_hamming([[0, 1]]),   # noqa: E731
                             lambda: ctx.match_all_pairs_hamming([[0, 1]]))
    with HipContext(0) as ctx:
        def raises(call, code, text):
            with pytest.raises(capi.EachamError) as e:
                call()
            assert e.value.code == code and text in str(e.value), str(e.value)

        # binary frames resident: every other kind of upload and of matching call is refused
        _upload(ctx, descs[:2])
        raises(lambda: ctx.upload_descriptors(2, u8), capi.ERR_UNSUPPORTED, "one descriptor kind")
        raises(lambda: ctx.upload_descriptors_f32(2, f32), capi.ERR_UNSUPPORTED, "kind")
        raises(lambda: ctx.upload_descriptors_bits(2, descs[0][:, :8]), capi.ERR_UNSUPPORTED, "dim class")
        for call in (lambda: ctx.match_pair(0, 1), lambda: ctx.match_all_pairs([[0, 1]], stats=False),
                     lambda: _l2_directed(ctx)):
            raises(call, capi.ERR_UNSUPPORTED, "binary")
        for call in (lambda: ctx.match_pair_dot(0, 1), lambda: ctx.match_all_pairs_dot([[0, 1]]),
                     lambda: ctx.match_all_pairs_dot([[0, 1]], screened=True)):
            raises(call, capi.ERR_UNSUPPORTED, "float frames")
        import torch
        z = torch.zeros(64, dtype=torch.int64, device="cuda:0")
        packed = torch.from_numpy(descs[0]).to("cuda:0")
        raises(lambda: ctx.match_all_pairs_dev(z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), 4, z.data_ptr()),
               capi.ERR_UNSUPPORTED, "binary")
        # shape limits
        raises(lambda: ctx.upload_descriptors_bits(2, np.zeros((4, 33), np.uint8)), capi.ERR_UNSUPPORTED, "<= 32")
        raises(lambda: ctx.upload_descriptors_bits(2, np.zeros((4, 0), np.uint8)), capi.ERR_INVALID, "shape")
        # a frame that is not resident; capacity
        raises(lambda: ctx.match_pair_hamming(0, 9), capi.ERR_INVALID, "not resident")
        raises(lambda: ctx.match_all_pairs_hamming([[0, 1], [1, 9]], cap=1000), capi.ERR_INVALID, "not resident")
        raises(lambda: ctx.match_pairs_directed_hamming([[0, 1]], cap=3), capi.ERR_CAPACITY, "capacity")
        raises(lambda: ctx.match_all_pairs_hamming([[0, 1]], HC.RATIO, 0, -1, cap=3), capi.ERR_CAPACITY, "capacity")
        raises(lambda: ctx.match_all_pairs_hamming([[0, 1]], 1.25, 0, -1), capi.ERR_INVALID, "ratio")
        # out_dist may be NULL
        want = R.match_directed(descs[0], descs[1], HC.RATIO)
        q, t, cnt = np.zeros(len(descs[0]), np.uint32), np.zeros(len(descs[0]), np.uint32), C.c_int(0)
        rc = ctx._L.eacham_match_pair_hamming(ctx.handle, 0, 1, HC.RATIO, q.ctypes.data, t.ctypes.data, None, len(q), C.byref(cnt))
        assert rc == capi.OK and np.array_equal(q[:cnt.value], want[0]) and np.array_equal(t[:cnt.value], want[1])
        # the context still works; eacham_clear_descriptors resets the kind, and then the Hamming calls are the ones refused
        _same(ctx.match_pairs_directed_hamming([[0, 1]]), R.match_pairs_directed(descs, [[0, 1]], HC.RATIO), "after errors")
        for up, text in ((lambda f: ctx.upload_descriptors(f, u8), "binary frames"), (lambda f: ctx.upload_descriptors_f32(f, f32), "binary frames")):
            ctx.clear_descriptors()
            up(0), up(1)
            for call in ham_calls(ctx):
                raises(call, capi.ERR_UNSUPPORTED, text)
            raises(lambda: ctx.match_all_pairs_hamming_dev(z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), 4, z.data_ptr(),
                                                           dist_dev=z.data_ptr()), capi.ERR_UNSUPPORTED, text)
            raises(lambda: ctx.upload_descriptors_bits(2, descs[0]), capi.ERR_UNSUPPORTED, "kind")
            raises(lambda: ctx.upload_descriptors_bits_dev(2, packed.data_ptr(), descs[0].shape[0], descs[0].shape[1]),
                   capi.ERR_UNSUPPORTED, "kind")


def test_l2_results_are_unchanged_around_a_hamming_session():
    """An L2 call on the same context before and after a Hamming session gives the same bytes (shared workspace, tables, kind)."""
    A = synth.random_u8_descriptors(300, 128, 31, 0)
    B = synth.random_u8_descriptors(280, 128, 31, 1)
    B[:150] = np.clip(A[:150] + np.rint(4 * synth.rng_normal(3, 3, (150, 128))), 0, 255)
    ref = HC.reference("b16")
    ordered = HC.ordered_pairs(len(ref.descs))

    def l2(ctx):
        ctx.clear_descriptors()
        ctx.upload_descriptors(0, A)
        ctx.upload_descriptors(1, B)
        return (*ctx.match_all_pairs([[0, 1], [1, 0]], min_dir=5, min_mutual=5), *ctx.match_pair(0, 1), *ctx.match_pair(1, 0, 1.5))

    with HipContext(0) as ctx:
        before = l2(ctx)
        assert before[0].sum() > 100
        _upload(ctx, ref.descs)
        _same(ctx.match_all_pairs_hamming(ordered, HC.RATIO, 0, -1), ref.match_all_pairs(ordered, HC.RATIO, 0, -1), "hamming session")
        _same(ctx.match_pairs_directed_hamming(ordered, HC.RATIO), ref.match_pairs_directed(ordered, HC.RATIO), "hamming session")
        after = l2(ctx)
        for g, w in zip(after, before):
            assert g.tobytes() == w.tobytes()


def test_python_mirror_of_the_adapter():
    from eacham_amd import FeatureMatcherHammingHip
    ref = HC.reference("b32")
    for mutual in (False, True):
        m = FeatureMatcherHammingHip(HC.RATIO, mutual)
        got = m.Match(ref.descs[0], ref.descs[1])
        wq, wt, wd = (R.mutual_from(ref.D(0, 1), HC.RATIO, 0, -1) if mutual else R.directed_from(ref.D(0, 1), HC.RATIO))[:3]
        assert got == dict(zip(wq.tolist(), wt.tolist())) and len(got) > 10
        assert m.LastDistances() == dict(zip(wq.tolist(), wd.tolist()))
        m.ctx.close()


def _vec(f, dtype):
    n = struct.unpack("q", f.read(8))[0]
    return np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype=dtype).copy()


def test_cpp_adapter_from_16_threads(tmp_path):
    """include/eacham/FeatureMatcherHip.hpp: FeatureMatcherHammingHip called from 16 threads on one shared instance, directed and
    mutual, and MatchAllPairsHamming — held against the reference."""
    tmp = str(tmp_path)
    exe, lib = os.path.join(tmp, "match_hamming_driver"), os.path.join(ROOT, "eacham_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "match_hamming_driver.cpp"),
                    "-o", exe, "-L" + lib, "-leacham_hip", "-Wl,-rpath," + lib, "-lpthread"], check=True, capture_output=True)
    ref = HC.reference("b32")
    descs = ref.descs + [ref.descs[0][:1].copy()]               # + a one-row frame
    ref = R.Scene(descs)
    F = len(descs)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("ii", F, descs[0].shape[1]))
        for d in descs:
            f.write(struct.pack("i", d.shape[0]))
            f.write(d.tobytes())
    r = subprocess.run([exe, fin, fout, "16", repr(HC.RATIO), "5", "5"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ordered = HC.ordered_pairs(F)
    want_dir = ref.match_pairs_directed(ordered, HC.RATIO)
    want_mut = ref.match_all_pairs(ordered, HC.RATIO, 0, -1)
    want_all = ref.match_all_pairs(synth.all_pairs(F), HC.RATIO, 5, 5)
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
