"""GPU: eacham_match_guided / eacham_graph_match_guided (eacham_amd/csrc/match_guided.hip) against the sequential CPU reference
(tests/guided_reference.py) on the cases of tests/guided_cases.py. Everything has an exact answer — the gate is the scorer's float
compared with a float, distances are integers — so counts, offsets, q, t, d2 and stats are compared as arrays, no tolerance. Output
arrays are preset to 0x55 before every call: an entry a call should not have written shows."""
import numpy as np
import pytest

import guided_cases as GCS
import guided_reference as GR
from eacham_amd import HipContext, ResidentGraph, capi
from eacham_amd import guided as G

pytestmark = pytest.mark.gpu

PRESET = 0x55
FIELDS = ["counts", "offsets", "q", "t", "d2", "stats"]


def upload(ctx, case):
    ctx.clear_descriptors()
    for f, d in enumerate(case["descs"]):
        ctx.upload_descriptors(f, np.asarray(d, np.float32).reshape(len(d), case["dim"]))
    return G.pack_keypoints(case["xys"])


def cap_of(case):
    return int(sum(len(case["descs"][f]) for f in case["pairs"][:, 0]))


def run(ctx, case, k, kpo, xy, graph=None, cap=None):
    rc, total, g = G.guided_raw(ctx, G.KINDS[case["kind"]], case["models"], case["K"], k["max_error"], k["ratio"], k["max_d2"], int(k["cross_check"]),
                                len(case["pairs"]), cap_of(case) if cap is None else cap, pairs=case["pairs"], kpo=kpo, xy=xy,
                                graph=graph, preset=PRESET)
    return rc, total, g


def assert_equals_reference(got, total, want, label):
    counts, offsets, q, t, d2, stats = want
    assert total == int(offsets[-1]), label
    trimmed = [got.counts, got.offsets, got.q[:total], got.t[:total], got.d2[:total], got.stats]
    for name, a, b in zip(FIELDS, trimmed, want):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{label}: {name}"
        assert np.array_equal(a, b), f"{label}: {name} differs at {np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:8]}"
    assert (got.q[total:] == 0x55555555).all() and (got.t[total:] == 0x55555555).all() and (got.d2[total:] == 0x55555555).all(), f"{label}: wrote past the total"


@pytest.mark.parametrize("name", GCS.CASE_NAMES)
def test_every_case_equals_the_reference(name):
    """The list form on every call of the case, then the graph form on the same context: the list form's bytes."""
    case = GCS.case_by_name(name)
    with HipContext(0) as ctx:
        kpo, xy = upload(ctx, case)
        n_frames = len(case["descs"])
        P = len(case["pairs"])
        rg = ResidentGraph(ctx, n_frames, case["pairs"], np.zeros(P, np.int32), np.zeros(P, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.uint32),
                           [len(d) for d in case["descs"]])
        rg.set_keypoints(xy)
        try:
            for i, k in enumerate(GCS.calls(name)):
                rc, total, got = run(ctx, case, k, kpo, xy)
                assert rc == capi.OK, (name, i, rc)
                assert_equals_reference(got, total, GCS.reference(name, i), f"{name}/call {i}")
                rc2, total2, got2 = run(ctx, case, k, None, None, graph=rg._h)
                assert rc2 == capi.OK and total2 == total
                for f in FIELDS:
                    assert getattr(got2, f).tobytes() == getattr(got, f).tobytes(), f"{name}/call {i}: the graph form's {f} differs from the list form's"
        finally:
            rg.close()


@pytest.mark.parametrize("name", ["twins128", "twinsE_K", "twinsE_norm", "rows128", "multi_pair"])
def test_without_the_screen_the_same_answers(name):
    """EACHAM_GUIDED_SCREEN=0 at eacham_ctx_create: every element goes through the gate's divisions. The screen (on in every other
    test) never decides anything the exact comparison would not: both forms give the reference's arrays."""
    import os
    case = GCS.case_by_name(name)
    old = os.environ.get("EACHAM_GUIDED_SCREEN")
    os.environ["EACHAM_GUIDED_SCREEN"] = "0"
    try:
        ctx = HipContext(0)
    finally:
        if old is None:
            os.environ.pop("EACHAM_GUIDED_SCREEN", None)
        else:
            os.environ["EACHAM_GUIDED_SCREEN"] = old
    with ctx:
        kpo, xy = upload(ctx, case)
        for i, k in enumerate(GCS.calls(name)):
            rc, total, got = run(ctx, case, k, kpo, xy)
            assert rc == capi.OK
            assert_equals_reference(got, total, GCS.reference(name, i), f"{name}/call {i} without the screen")


@pytest.mark.parametrize("name", ["twins128", "rows128", "parity", "dim32", "dim256", "large_train"])
def test_no_gate_no_cross_check_is_match_pairs_directed(name):
    case = GCS.case_by_name(name)
    ok = [p for p, (f1, f2) in enumerate(case["pairs"].tolist()) if len(case["descs"][f2]) >= 2]
    sub = dict(case, pairs=case["pairs"][ok], models=case["models"][ok])
    with HipContext(0) as ctx:
        want = ctx.match_pairs_directed([np.asarray(d, np.float32).reshape(len(d), case["dim"]) for d in case["descs"]], sub["pairs"], 0.8)
        kpo, xy = G.pack_keypoints(case["xys"])
        rc, total, got = run(ctx, sub, GCS.call(np.inf, cross_check=False), kpo, xy)
        assert rc == capi.OK
        for p in range(len(ok)):
            s = slice(int(got.offsets[p]), int(got.offsets[p + 1]))
            assert dict(zip(got.q[s].tolist(), got.t[s].tolist())) == want[p], (name, p)
            assert got.counts[p] == len(want[p])


def untouched(g, total):
    return total == PRESET and all((getattr(g, f).view(np.uint8) == PRESET).all() for f in FIELDS)


def test_error_codes_leave_the_outputs_alone():
    case = GCS.twins(128)
    k = GCS.call(4)
    with HipContext(0) as ctx:
        kpo, xy = upload(ctx, case)
        P, cap = 1, cap_of(case)
        code = G.KINDS["fundamental"]

        def raw(**kw):
            a = dict(kind=code, models=case["models"], K=None, max_error=4.0, ratio=0.8, max_d2=0, cross_check=1, npairs=P, cap=cap, pairs=case["pairs"],
                     kpo=kpo, xy=xy, graph=None)
            a.update(kw)
            return G.guided_raw(ctx, a["kind"], a["models"], a["K"], a["max_error"], a["ratio"], a["max_d2"], a["cross_check"], a["npairs"], a["cap"],
                                pairs=a["pairs"], kpo=a["kpo"], xy=a["xy"], graph=a["graph"], preset=PRESET)

        invalid = {
            "null models": dict(models=None), "null pairs": dict(pairs=None), "null kp_offsets": dict(kpo=None), "null xy": dict(xy=None),
            "kind pnp": dict(kind=capi.SCORE_PNP), "kind 7": dict(kind=7), "negative npairs": dict(npairs=-1), "negative cap": dict(cap=-1),
            "nan max_error": dict(max_error=float("nan")), "negative max_error": dict(max_error=-1.0),
            "ratio above 1 with the cross-check": dict(ratio=1.5), "ratio 0 with the cross-check": dict(ratio=0.0),
            "nan ratio": dict(ratio=float("nan"), cross_check=0), "frame not resident": dict(pairs=np.array([[0, 9]], np.int32)),
            "negative frame": dict(pairs=np.array([[-1, 0]], np.int32)),
        }
        for label, kw in invalid.items():
            rc, total, g = raw(**kw)
            assert rc == capi.ERR_INVALID, label
            assert untouched(g, total), label
        bad_kpo = kpo.copy()
        bad_kpo[2] -= 1                                              # frame 1 now claims 129 keypoints for its 130 rows
        rc, total, g = raw(kpo=bad_kpo)
        assert rc == capi.ERR_INVALID and untouched(g, total)
        assert b"frame 1" in ctx._L.eacham_last_error(ctx.handle)
        # legal: +inf, ratio above 1 without the cross-check
        assert raw(max_error=float("inf"))[0] == capi.OK and raw(ratio=1.5, cross_check=0)[0] == capi.OK
        # capacity: what is needed comes back, nothing else is written
        rc, need, g = raw()
        assert rc == capi.OK and need > 1
        rc, total, g = raw(cap=need - 1)
        assert rc == capi.ERR_CAPACITY and total == need
        assert all((getattr(g, f).view(np.uint8) == PRESET).all() for f in FIELDS)
        rc, total, g = raw(cap=need)
        assert rc == capi.OK and total == need
        # the graph form: keypoints not set
        rg = ResidentGraph(ctx, 2, case["pairs"], np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.uint32), [150, 130])
        try:
            rc, total, g = raw(graph=rg._h)
            assert rc == capi.ERR_INVALID and untouched(g, total)
            rg.set_keypoints(xy)
            assert raw(graph=rg._h)[0] == capi.OK
            rc, total, g = raw(graph=rg._h, models=None)
            assert rc == capi.ERR_INVALID and untouched(g, total)
        finally:
            rg.close()
        # frames of another kind
        ctx.clear_descriptors()
        for f, d in enumerate(case["descs"]):
            ctx.upload_descriptors_f32(f, d)
        rc, total, g = raw()
        assert rc == capi.ERR_UNSUPPORTED and untouched(g, total)


@pytest.fixture(scope="module")
def pipeline_scene():
    """Four frames in the style of graph_verify_cases.eight(): 200 scene points in integer pixels, the first 100 of them 50 pairs of
    twins that share a base descriptor."""
    import graph_verify_cases as GC
    rng = np.random.default_rng(41)
    n = 200
    X = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)], axis=1)
    base = GCS.random_desc(rng, n, 128)
    base[50:100] = base[:50]
    descs, xys = [], []
    for f in range(4):
        perm = rng.permutation(n)
        d, xy = np.zeros((n, 128), np.float32), np.zeros((n, 2))
        d[perm], xy[perm] = GCS.noisy(rng, base), GC._project(X, f)
        descs.append(d), xys.append(xy)
    return descs, xys, np.array([[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]], np.int32)


def test_pipeline_verify_guided_graph_tracks(pipeline_scene):
    """blind eacham_match_all_pairs -> eacham_graph_verify_ransac (F) -> eacham_graph_match_guided -> eacham_graph_create on its
    output -> tracks. The guided step returns what the reference returns for the same models, and finds more than the blind one."""
    descs, xys, pairs = pipeline_scene
    with HipContext(0) as ctx:
        for f, d in enumerate(descs):
            ctx.upload_descriptors(f, d)
        counts, offsets, q, t, _ = ctx.match_all_pairs(pairs, 0.8, 0, -1)
        blind = ResidentGraph(ctx, 4, pairs, counts, offsets, q, t, [200] * 4)
        try:
            blind.set_keypoints(xys)
            ver = blind.verify_ransac("fundamental", 4.0, 0.99, 300, sampling="counter", seeds=np.arange(6, dtype=np.uint64) + 7)
            assert ver.models.any(axis=1).all(), "every pair has a model"
            got = blind.match_guided("fundamental", ver.models, 4.0)
            want = GR.guided("fundamental", descs, xys, pairs, ver.models, None, np.float32(4.0))
            for name, a, b in zip(FIELDS, got, want):
                assert a.dtype == b.dtype and np.array_equal(a, b), name
            assert (want[0] > counts).all() and int(want[0].sum()) >= int(counts.sum()) + 6 * 40, "the twins come back under the model"
            blind_tracks = blind.tracks(keep=ver.masks)
        finally:
            blind.close()
        guided = ResidentGraph(ctx, 4, pairs, got.counts, got.offsets, got.q, got.t, [200] * 4)
        try:
            tracks = guided.tracks()
        finally:
            guided.close()
        assert tracks.obs_frame.size > blind_tracks.obs_frame.size and tracks.n_tracks >= blind_tracks.n_tracks
