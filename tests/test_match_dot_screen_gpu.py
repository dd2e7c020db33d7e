"""GPU: the screened dot-product matcher (eacham_match_all_pairs_dot_screened, eacham_amd/csrc/matcher_dot16.hip) returns the BYTES
of eacham_match_all_pairs_dot and of the CPU reference (tests/dot_reference.py); its error bound holds on the device for every
(q, t) of every scene; every branch (dead, settled, open, fp32 fallback) is reached where the scene is built for it."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from eacham_amd import HipContext, capi, synth
import dot_cases as DC
import dot_reference as R
import dot_screen_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NEG_INF = float("-inf")
NAMES = ["counts", "offsets", "q", "t", "scores", "stats"]


@functools.lru_cache(maxsize=None)
def _scenes():
    return SC.scenes()


@functools.lru_cache(maxsize=None)
def _reference(name, min_score, min_dir, min_mutual):
    descs, pairs = _scenes()[name]
    return R.match_all_pairs(descs, pairs, min_score, min_dir, min_mutual)


def _same_bytes(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: {name} differ"


def _upload(ctx, descs):
    ctx.clear_descriptors()
    for f, d in enumerate(descs):
        ctx.upload_descriptors_f32(f, d)


SCENE_NAMES = ["a_d100", "a_d128", "a_d256", "a_d64", "b_near_duplicates", "c_fallback", "d_tiny_values", "e_negative", "f_tiny_shapes"]


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_screened_call_returns_the_bytes_of_the_exact_call_and_of_the_reference(name):
    descs, pairs = _scenes()[name]
    with HipContext(0) as ctx:
        _upload(ctx, descs)
        for ms in (DC.MIN_SCORE, NEG_INF):
            for md, mm in ((0, -1), (30, 30)):
                got = ctx.match_all_pairs_dot(pairs, ms, md, mm, screened=True)
                _same_bytes(got, ctx.match_all_pairs_dot(pairs, ms, md, mm), f"{name} {ms} {md}/{mm} vs the exact call")
                _same_bytes(got, _reference(name, ms, md, mm), f"{name} {ms} {md}/{mm} vs the reference")
                tally = ctx.match_dot_screen()
                rows = sum(descs[a].shape[0] for a, b in pairs)
                if tally["fallback_pairs"] == 0:     # dead + settled + open = the real rows and columns
                    assert sum(tally["rows"]) == rows and sum(tally["cols"]) == sum(descs[b].shape[0] for a, b in pairs)


def test_scene_names_are_complete():
    assert SCENE_NAMES == sorted(_scenes())


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_the_bound_holds_on_the_device(name):
    """|s~ - s| <= E for every (q, t), s~ and E from the device (eacham_match_debug_dot_coarse), s from the reference. A condition,
    not a tolerance. Prints the largest observed ratio of each scene (DESIGN §3.5 is where it is recorded)."""
    descs, pairs = _scenes()[name]
    worst = 0.0
    with HipContext(0) as ctx:
        _upload(ctx, descs)
        for a, b in pairs:
            if a > b or not (SC.screenable(descs[a]) and SC.screenable(descs[b])):
                continue                                   # (b, a) is the transpose: the same products in the same k order
            s, row_E, col_E = ctx.match_dot_coarse(int(a), int(b))
            if s.size == 0:
                continue
            ref = SC.exact_scores(descs[a], descs[b]).astype(np.float64)
            err = np.abs(s.astype(np.float64) - ref)
            E = np.minimum(row_E.astype(np.float64)[:, None], col_E.astype(np.float64)[None, :])
            worst = max(worst, float((err / E).max()))
            assert (err <= E).all(), f"{name} pair ({a},{b}): |s~ - s| exceeds E by a factor {float((err / E).max())}"
            # the device's bounds are no tighter than the CPU model's norms allow (they are built from upper bounds)
            _, mrow, mcol = SC.coarse(descs[a], descs[b])
            assert (row_E >= mrow * (1 - 1e-6)).all() and (col_E >= mcol * (1 - 1e-6)).all()
    print(f"{name}: largest |s~ - s| / E = {worst:.4f}")


def test_branch_coverage_by_the_getter():
    sc = _scenes()
    with HipContext(0) as ctx:
        # (a) at 0.5: nothing open, nothing falls back — a screen that opens everything does not pass
        for name in ("a_d64", "a_d100", "a_d128", "a_d256"):
            descs, pairs = sc[name]
            _upload(ctx, descs)
            ctx.match_all_pairs_dot(pairs, DC.MIN_SCORE, 0, -1, screened=True)
            t = ctx.match_dot_screen()
            assert t["rows"][2] == 0 and t["cols"][2] == 0 and t["fallback_pairs"] == 0, (name, t)
            assert t["rows"][0] > 0 and t["rows"][1] > 0 and t["cols"][0] > 0 and t["cols"][1] > 0, (name, t)
            rows = sum(descs[a].shape[0] for a, b in pairs)
            assert sum(t["rows"]) == rows and sum(t["cols"]) == rows      # ordered pairs: every frame is on both sides
            ctx.match_all_pairs_dot(pairs, NEG_INF, 0, -1, screened=True)
            t = ctx.match_dot_screen()
            assert t["rows"][0] == 0 and 0 < t["rows"][2] <= 0.06 * rows, (name, t)
        # (b): open rows, results right (the bytes are held by the first test)
        descs, pairs = sc["b_near_duplicates"]
        _upload(ctx, descs)
        got = ctx.match_all_pairs_dot(pairs, DC.MIN_SCORE, 0, -1, screened=True)
        t = ctx.match_dot_screen()
        assert t["rows"][2] > 0 and t["fallback_pairs"] == 0, t
        _, _, rows3 = SC.near_duplicates()
        n0 = descs[1].shape[0] - 3
        q, tt = got[2][:got[0][0]], got[3][:got[0][0]]
        assert tt[q == rows3[0]].tolist() == [n0]                 # fp32 picks the copy at the higher index
        # (c): the fallback
        descs, pairs = sc["c_fallback"]
        _upload(ctx, descs)
        ctx.match_all_pairs_dot(pairs, DC.MIN_SCORE, 0, -1, screened=True)
        t = ctx.match_dot_screen()
        assert t["fallback_pairs"] == len(pairs) - 2, t           # all but (0, 3) and (3, 0)
        assert sum(t["rows"]) == descs[0].shape[0] + descs[3].shape[0] == sum(t["cols"])


def test_job_cut_into_more_than_one_launch():
    """Two frames of 2000 x 256 named by 504 pairs: 4 more than the 500 per launch that the planner gives at 2000-row frames."""
    batch = DC.multi_launch_batch(2000)
    descs = DC.float_frames(256, [2000, 2000], 1200, 78)
    pairs = np.array([[0, 1], [1, 0]] * 252, np.int32)
    assert batch == 500 and len(pairs) > batch
    want = [R.match_mutual(descs[a], descs[b], DC.MIN_SCORE, 30, 30) for a, b in ((0, 1), (1, 0))]
    assert 200 < len(want[0][0]) < 1800
    with HipContext(0) as ctx:
        _upload(ctx, descs)
        counts, offsets, q, t, s, st = ctx.match_all_pairs_dot(pairs, DC.MIN_SCORE, 30, 30, screened=True)
        tally = ctx.match_dot_screen()
        assert sum(tally["rows"]) == 2000 * len(pairs) == sum(tally["cols"]) and tally["fallback_pairs"] == 0
    assert np.array_equal(offsets[1:], np.cumsum(counts)) and offsets[0] == 0 and len(q) == offsets[-1]
    for p in (0, 1, batch - 1, batch, batch + 1, len(pairs) - 1):
        wq, wt, ws, wst = want[p % 2]
        sl = slice(offsets[p], offsets[p + 1])
        assert q[sl].tobytes() == wq.tobytes() and t[sl].tobytes() == wt.tobytes() and s[sl].tobytes() == ws.tobytes(), p
        assert np.array_equal(st[p], wst), p


def test_many_tiny_pairs_in_one_launch():
    """66 000 pairs of two frames of 5 and 7 rows (one row of the second twice, so that the exact pass has work): one launch (the planner gives ~95 000 pairs per launch at frames of <= 128
    rows) with more pairs than a grid's y extent may hold."""
    fr = DC.scene("d64")
    descs = [fr[0][:5].copy(), np.concatenate([fr[0][:4], fr[0][3:4], fr[1][:2]])]      # rows 3 and 4 of the second are equal: a tie, open
    pairs = np.array([[0, 1], [1, 0]] * 33000, np.int32)
    want = [R.match_mutual(descs[a], descs[b], NEG_INF, 0, -1) for a, b in ((0, 1), (1, 0))]
    assert len(want[0][0]) >= 4
    with HipContext(0) as ctx:
        _upload(ctx, descs)
        counts, offsets, q, t, s, st = ctx.match_all_pairs_dot(pairs, NEG_INF, 0, -1, screened=True)
        exact = ctx.match_all_pairs_dot(pairs, NEG_INF, 0, -1)
        tally = ctx.match_dot_screen()
    _same_bytes((counts, offsets, q, t, s, st), exact, "66 000 tiny pairs vs the exact call")
    assert sum(tally["rows"]) == 12 * 33000 == sum(tally["cols"]) and tally["rows"][2] > 0
    for p in (0, 1, 65535, 65536, 65537, len(pairs) - 1):
        wq, wt, ws, wst = want[p % 2]
        sl = slice(offsets[p], offsets[p + 1])
        assert q[sl].tobytes() == wq.tobytes() and t[sl].tobytes() == wt.tobytes() and s[sl].tobytes() == ws.tobytes(), p
        assert np.array_equal(st[p], wst), p


def test_packed_and_direct_results_in_one_call():
    """IoStage::PACK_MAX (eacham_amd/csrc/context.hpp) is 256 KiB = 262 144 B. At 33 000 pairs the counts (132 000 B) travel through
    the pinned mirror; the two pair lists and the offsets (264 000 B, 264 008 B) and the stats (528 000 B) lie above it and take their
    own direct copy. The 12 ordered pairs of four 40-row frames (two 32-row tiles, the second mostly padding), repeated cyclically,
    must give the exact call's bytes and the reference's 12-pair results repeated, with the offsets their running sum."""
    descs = DC.float_frames(32, [40] * 4, 25, 311)
    ordered = DC.ordered_pairs(4)
    idx = np.arange(33000) % 12
    want = R.match_all_pairs(descs, ordered, DC.MIN_SCORE, 0, -1)
    assert (want[0] > 0).all() and want[0].min() < 40
    per = lambda k: [want[k][want[1][p]:want[1][p + 1]] for p in range(12)]     # noqa: E731
    rep = (want[0][idx], np.concatenate([[0], np.cumsum(want[0][idx], dtype=np.int64)]).astype(np.int64),
           *(np.concatenate([per(k)[i] for i in idx]) for k in (2, 3, 4)), want[5][idx])
    with HipContext(0) as ctx:
        _upload(ctx, descs)
        _same_bytes(ctx.match_all_pairs_dot(ordered, DC.MIN_SCORE, 0, -1, screened=True), want, "12 pairs, screened")
        got = ctx.match_all_pairs_dot(ordered[idx], DC.MIN_SCORE, 0, -1, screened=True)
        _same_bytes(got, rep, "33 000 pairs, screened, vs the repetition")
        _same_bytes(got, ctx.match_all_pairs_dot(ordered[idx], DC.MIN_SCORE, 0, -1), "33 000 pairs, screened, vs the exact call")
        lean = ctx.match_all_pairs_dot(ordered[idx], DC.MIN_SCORE, 0, -1, stats=False, screened=True)
        assert lean[5] is None
        _same_bytes(lean[:5], rep[:5], "33 000 pairs, screened, without stats")


def test_repeat_and_order_independence():
    descs, pairs = _scenes()["a_d128"]
    with HipContext(0) as ctx:
        _upload(ctx, descs)
        exact = ctx.match_all_pairs_dot(pairs, NEG_INF, 0, -1)
        first = ctx.match_all_pairs_dot(pairs, NEG_INF, 0, -1, screened=True)
        second = ctx.match_all_pairs_dot(pairs, NEG_INF, 0, -1, screened=True)
        _same_bytes(first, exact, "first screened call")
        _same_bytes(second, exact, "second screened call")
        _same_bytes(ctx.match_all_pairs_dot(pairs, NEG_INF, 0, -1), exact, "exact call after screened ones")
        # re-upload of one frame with other rows of the same shape: the stale fp16 image must be gone
        changed = list(descs)
        changed[1] = np.ascontiguousarray(descs[1][::-1])
        ctx.upload_descriptors_f32(1, changed[1])
        want = R.match_all_pairs(changed, pairs, NEG_INF, 0, -1)
        assert want[3].tobytes() != exact[3].tobytes()
        _same_bytes(ctx.match_all_pairs_dot(pairs, NEG_INF, 0, -1, screened=True), want, "screened call after a re-upload")
        # and one whose rows leave the fp16 range: its pairs now fall back
        changed[1] = changed[1].copy()
        changed[1][0, 0] = 1.0e6
        ctx.upload_descriptors_f32(1, changed[1])
        _same_bytes(ctx.match_all_pairs_dot(pairs, DC.MIN_SCORE, 0, -1, screened=True),
                    R.match_all_pairs(changed, pairs, DC.MIN_SCORE, 0, -1), "screened call after a re-upload out of range")
        assert ctx.match_dot_screen()["fallback_pairs"] == sum(1 for a, b in pairs if 1 in (a, b))


def test_an_empty_frame_that_gains_rows_gets_an_image():
    """An empty frame has no allocation of either kind; once rows are uploaded under its id the screen must build their image."""
    descs = DC.scene("d64")[:2]
    empty = np.zeros((0, 64), np.float32)
    with HipContext(0) as ctx:
        _upload(ctx, [descs[0], empty])
        got = ctx.match_all_pairs_dot([[0, 1], [1, 0]], DC.MIN_SCORE, 0, -1, screened=True)
        assert got[0].tolist() == [0, 0]
        ctx.upload_descriptors_f32(1, descs[1])
        _same_bytes(ctx.match_all_pairs_dot([[0, 1], [1, 0]], DC.MIN_SCORE, 0, -1, screened=True),
                    R.match_all_pairs(descs, [[0, 1], [1, 0]], DC.MIN_SCORE, 0, -1), "after the empty frame gained rows")


def test_error_paths():
    import ctypes as C
    descs = DC.scene("d64")
    with HipContext(0) as ctx:
        ctx.clear_descriptors()
        u8 = synth.random_u8_descriptors(50, 64, 3)
        ctx.upload_descriptors(0, u8)
        ctx.upload_descriptors(1, u8)
        with pytest.raises(capi.EachamError) as e:
            ctx.match_all_pairs_dot([[0, 1]], screened=True)
        assert e.value.code == capi.ERR_UNSUPPORTED and "float frames" in str(e.value)
        with pytest.raises(capi.EachamError) as e:
            ctx.match_dot_coarse(0, 1)
        assert e.value.code == capi.ERR_UNSUPPORTED
        _upload(ctx, descs[:2])
        with pytest.raises(capi.EachamError) as e:
            ctx.match_all_pairs_dot([[0, 1], [1, 9]], cap=1000, screened=True)
        assert e.value.code == capi.ERR_INVALID and "not resident" in str(e.value)
        # nothing is written on an error that is found before the launch
        L = capi.lib()
        pr = np.array([[0, 1], [1, 9]], np.int32)
        counts, offsets = np.full(2, -7, np.int32), np.full(3, -7, np.int64)
        q, t, s = np.full(8, 77, np.uint32), np.full(8, 77, np.uint32), np.full(8, 7.0, np.float32)
        total = C.c_int64(-7)
        rc = L.eacham_match_all_pairs_dot_screened(ctx.handle, pr.ctypes.data, 2, 0.5, 0, -1, counts.ctypes.data, offsets.ctypes.data,
                                                   q.ctypes.data, t.ctypes.data, s.ctypes.data, 8, C.byref(total), None)
        assert rc == capi.ERR_INVALID and (counts == -7).all() and (offsets == -7).all() and (q == 77).all() and (s == 7.0).all()
        assert total.value == -7
        # capacity: the same code and the same total as the exact call; q, t and scores untouched
        for screened in (False, True):
            with pytest.raises(capi.EachamError) as e:
                ctx.match_all_pairs_dot([[0, 1]], 0.5, 0, -1, cap=3, screened=screened)
            assert e.value.code == capi.ERR_CAPACITY and "capacity" in str(e.value)
        rc = L.eacham_match_all_pairs_dot_screened(ctx.handle, pr.ctypes.data, 1, 0.5, 0, -1, counts.ctypes.data, offsets.ctypes.data,
                                                   q.ctypes.data, t.ctypes.data, s.ctypes.data, 3, C.byref(total), None)
        assert rc == capi.ERR_CAPACITY and total.value > 3 and (q == 77).all() and (t == 77).all() and (s == 7.0).all()
        # null arguments
        rc = L.eacham_match_all_pairs_dot_screened(ctx.handle, None, 1, 0.5, 0, -1, counts.ctypes.data, offsets.ctypes.data,
                                                   q.ctypes.data, t.ctypes.data, s.ctypes.data, 8, C.byref(total), None)
        assert rc == capi.ERR_INVALID
        out = (C.c_int64 * 7)()
        assert L.eacham_match_debug_dot_screen(ctx.handle, None) == capi.ERR_INVALID
        assert L.eacham_match_debug_dot_screen(None, out) == capi.ERR_INVALID
        # the coarse hook: a frame that is not resident
        with pytest.raises(capi.EachamError) as e:
            ctx.match_dot_coarse(0, 9)
        assert e.value.code == capi.ERR_INVALID
        # and the context still works after the errors
        _same_bytes(ctx.match_all_pairs_dot([[0, 1]], 0.5, 0, -1, screened=True), R.match_all_pairs(descs, [[0, 1]], 0.5, 0, -1), "after errors")


def test_coarse_hook_capacity():
    with HipContext(0) as ctx:
        ctx.clear_descriptors()
        big = np.zeros((4097, 64), np.float32)
        ctx.upload_descriptors_f32(0, big)
        ctx.upload_descriptors_f32(1, big[:10])
        L = capi.lib()
        one = np.zeros(16, np.float32)
        rc = L.eacham_match_debug_dot_coarse(ctx.handle, 0, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data)
        assert rc == capi.ERR_CAPACITY and (one == 0).all()


def _vec(f, dtype):
    n = struct.unpack("q", f.read(8))[0]
    return np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype=dtype).copy()


def test_cpp_adapter_and_python_mirror_with_screened(tmp_path):
    """MatchAllPairsDot(..., screened = true) of include/eacham/FeatureMatcherHip.hpp against the mirror's screened call."""
    tmp = str(tmp_path)
    exe, lib = os.path.join(tmp, "match_dot_screen_driver"), os.path.join(ROOT, "eacham_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "match_dot_screen_driver.cpp"),
                    "-o", exe, "-L" + lib, "-leacham_hip", "-Wl,-rpath," + lib, "-lpthread"], check=True, capture_output=True)
    descs = DC.scene("d256")
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("ii", len(descs), descs[0].shape[1]))
        for d in descs:
            f.write(struct.pack("i", d.shape[0]))
            f.write(np.ascontiguousarray(d, np.float32).tobytes())
    r = subprocess.run([exe, fin, fout, repr(DC.MIN_SCORE), "5", "5"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    pairs = synth.all_pairs(len(descs))
    with HipContext(0) as ctx:
        _upload(ctx, descs)
        mirror = ctx.match_all_pairs_dot(pairs, DC.MIN_SCORE, 5, 5, screened=True)
    _same_bytes(mirror, R.match_all_pairs(descs, pairs, DC.MIN_SCORE, 5, 5), "mirror, screened")
    with open(fout, "rb") as f:
        for k in range(2):                                   # screened, then unscreened: the same graph
            counts, gq, gt, gs = _vec(f, np.int32), _vec(f, np.uint32), _vec(f, np.uint32), _vec(f, np.float32)
            assert counts.tobytes() == mirror[0].tobytes() and gq.tobytes() == mirror[2].tobytes(), k
            assert gt.tobytes() == mirror[3].tobytes() and gs.tobytes() == mirror[4].tobytes() and counts.sum() > 0, k
