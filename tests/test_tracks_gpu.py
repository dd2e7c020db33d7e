"""GPU: eacham_tracks_build and eacham_graph_tracks (csrc/tracks.hip) against the host union-find of tests/tracks_reference.py,
every output identical as bytes, on the cases of tests/tracks_cases.py: the hand-written ones, the seeded 30 x 600 scene (the
three-kernel scan, two radix passes, the staging's direct copies), two depth-stress paths (rounds above 1 and within the cap,
read through eacham_tracks_debug_last), the resident form, the error returns."""
import ctypes as C

import numpy as np
import pytest

import tracks_cases as TC
import tracks_reference as TR
from eacham_amd import HipContext, ResidentGraph, capi
from eacham_amd import tracks as T

pytestmark = pytest.mark.gpu
HAND = TC.hand_written()


@pytest.fixture(scope="module")
def ctx():
    with HipContext(0) as c:
        yield c


def build(ctx, case, keep=None, min_len=2, policy=0, **kw):
    return T.build_tracks(ctx, len(case["kp"]), case["pairs"], case["counts"], case["offsets"], case["q"], case["t"], case["kp"],
                          keep, min_len, policy, **kw)


def resident(ctx, case):
    return ResidentGraph(ctx, len(case["kp"]), case["pairs"], case["counts"], case["offsets"], case["q"], case["t"], case["kp"])


def same(got, want, what):
    for f in TR.FIELDS:
        g = getattr(got, f)
        assert g.dtype == want[f].dtype and g.tobytes() == want[f].tobytes(), f"{what}: {f} differs"


@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written_cases(ctx, name, policy):
    case, _ = HAND[name]
    want = TR.reference_tracks(case, case["keep"], case["min_len"], policy)
    same(build(ctx, case, case["keep"], case["min_len"], policy), want, name)
    g = resident(ctx, case)
    try:
        same(g.tracks(case["keep"], case["min_len"], policy), want, name + " (resident)")
    finally:
        g.close()


@pytest.mark.parametrize("masked,min_len,policy", [(False, 2, 0), (True, 2, 0), (True, 2, 1), (True, 3, 0), (False, 3, 1)])
def test_scene(ctx, masked, min_len, policy):
    case = TC.scene()
    got = build(ctx, case, case["keep"] if masked else None, min_len, policy)
    same(got, TC.scene_reference(masked, min_len, policy), "scene")
    info = T.last_call_info(ctx)
    # launches and read-backs as designed: one read-back per batch of 4 rounds, one for the totals
    assert 1 < info["rounds"] <= info["round_cap"] == 2 * 15 + 1
    assert info["readbacks"] == -(-info["rounds"] // 4) + 1


@pytest.mark.parametrize("comb", [False, True])
def test_depth_stress(ctx, comb):
    case = TC.path64(comb)
    want = TR.reference_tracks(case)
    assert want["track_ptr"].tolist() == [0, 64] and want["obs_frame"].tolist() == list(range(64))
    same(build(ctx, case), want, "path")
    info = T.last_call_info(ctx)
    print("rounds", info)
    assert info["round_cap"] == 2 * 6 + 1                    # 64 touched nodes
    assert 1 < info["rounds"] <= info["round_cap"]
    if comb:
        assert info["rounds"] == 7                           # 64 -> 32 -> ... -> 1 trees, and the round that finds nothing to hook


def test_resident_form_equals_the_one_shot_form(ctx):
    case = TC.scene()
    g = resident(ctx, case)
    try:
        other = case["keep"].copy()
        other[::7] ^= 1
        for keep, policy in ((case["keep"], 0), (None, 0), (other, 1), (case["keep"], 1), (None, 1), (case["keep"], 0)):
            a, b = g.tracks(keep, 2, policy), build(ctx, case, keep, 2, policy)
            for f in TR.FIELDS:
                assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (f, policy, keep is None)
        same(g.tracks(case["keep"], 2, 0), TC.scene_reference(True), "resident scene")
    finally:
        g.close()


def test_resident_form_with_gaps_in_the_offsets(ctx):
    """`keep` is indexed like the q and t the graph was made from, also when the match lists do not lie one behind the other."""
    case, _ = HAND["c_keep_cuts"]
    c = dict(case)
    c["offsets"] = np.array([0, 3, 5], dtype=np.int64)
    q, t, keep = np.full(6, 1, np.uint32), np.full(6, 1, np.uint32), np.zeros(6, np.uint8)
    for p, o in enumerate(c["offsets"]):
        q[o], t[o], keep[o] = case["q"][p], case["t"][p], case["keep"][p]
    c["q"], c["t"] = q, t
    want = TR.reference_tracks(case, case["keep"])
    same(build(ctx, c, keep), want, "gaps")
    g = resident(ctx, c)
    try:
        same(g.tracks(keep), want, "gaps (resident)")
    finally:
        g.close()


SENTINEL = 0x5A


def raw_call(ctx, case, n_frames=None, kpo=None, keep=None, min_len=2, policy=0, cap_obs=None, cap_tracks=None, null=()):
    """eacham_tracks_build with sentinel-filled outputs; returns (code, n_tracks, n_obs, outputs)."""
    kpo = TR.kp_offsets_of(case["kp"]) if kpo is None else np.asarray(kpo, dtype=np.int64)
    n_frames = len(case["kp"]) if n_frames is None else n_frames
    bo, bt = T.output_bounds(int(kpo[-1]), int(np.abs(case["counts"]).sum()))
    cap_obs, cap_tracks = bo if cap_obs is None else cap_obs, bt if cap_tracks is None else cap_tracks
    outs = {"track_ptr": np.full(cap_tracks + 1, SENTINEL, np.int64), "obs_frame": np.full(cap_obs + 1, SENTINEL, np.uint32),
            "obs_kp": np.full(cap_obs + 1, SENTINEL, np.uint32), "flags": np.full(cap_tracks + 1, SENTINEL, np.uint8),
            "node_track": np.full(int(kpo[-1]) + 1, SENTINEL, np.int32)}
    nt, no = C.c_int32(-7), C.c_int64(-7)
    arrays = {"pairs": case["pairs"], "counts": case["counts"], "offsets": case["offsets"], "q": case["q"], "t": case["t"], "kpo": kpo}
    ptr = {k: (None if k in null else v.ctypes.data) for k, v in {**arrays, **outs}.items()}
    rc = ctx._L.eacham_tracks_build(ctx.handle, n_frames, ptr["pairs"], len(case["counts"]), ptr["counts"], ptr["offsets"], ptr["q"], ptr["t"],
                                    ptr["kpo"], None if keep is None else keep.ctypes.data, min_len, policy, cap_obs, cap_tracks,
                                    None if "n_tracks" in null else C.byref(nt), None if "n_obs" in null else C.byref(no),
                                    ptr["track_ptr"], ptr["obs_frame"], ptr["obs_kp"], ptr["flags"], ptr["node_track"])
    return rc, nt.value, no.value, outs


def untouched(outs):
    return all((a == SENTINEL).all() for a in outs.values())


def variant(case, **changes):
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    for k, (i, v) in changes.items():
        c[k][i] = v
    return c


def test_invalid_arguments(ctx):
    case, _ = HAND["a_triangle"]
    bad = {
        "null pairs": dict(null=("pairs",)), "null q": dict(null=("q",)), "null kp_offsets": dict(null=("kpo",)),
        "null track_ptr": dict(null=("track_ptr",)), "null n_obs": dict(null=("n_obs",)), "null obs_kp": dict(null=("obs_kp",)),
        "offsets start": dict(case=variant(case, offsets=(0, 1))), "offsets decrease": dict(case=variant(case, offsets=(2, 0))),
        "kp_offsets start": dict(kpo=[1, 2, 4, 6]), "kp_offsets decrease": dict(kpo=[0, 4, 2, 6]),
        "frame out of range": dict(case=variant(case, pairs=((1, 1), 3))), "negative frame": dict(case=variant(case, pairs=((0, 0), -1))),
        "q beyond": dict(case=variant(case, q=(1, 2))), "t beyond": dict(case=variant(case, t=(2, 2))),
        "min_len": dict(min_len=1), "policy": dict(policy=2),
    }
    for what, kw in bad.items():
        kw = dict(kw)
        rc, nt, no, outs = raw_call(ctx, kw.pop("case", case), **kw)
        assert rc == capi.ERR_INVALID, what
        assert untouched(outs) and (nt, no) == (-7, -7), what
        assert ctx._L.eacham_last_error(ctx.handle), what
    rc, nt, no, outs = raw_call(ctx, case)                                   # and the context is fine afterwards
    assert rc == capi.OK and (nt, no) == (1, 3) and outs["track_ptr"][:2].tolist() == [0, 3]


def test_capacity(ctx):
    case = TC.scene()
    want = TC.scene_reference(True)
    n_t, n_o = want["flags"].size, want["obs_frame"].size
    for caps in (dict(cap_obs=n_o - 1, cap_tracks=n_t), dict(cap_obs=n_o, cap_tracks=n_t - 1)):
        rc, nt, no, outs = raw_call(ctx, case, keep=case["keep"], **caps)
        assert rc == capi.ERR_CAPACITY and (nt, no) == (n_t, n_o) and untouched(outs)
    rc, nt, no, outs = raw_call(ctx, case, keep=case["keep"], cap_obs=n_o, cap_tracks=n_t)   # exactly what was reported fits
    assert rc == capi.OK and (nt, no) == (n_t, n_o)
    assert outs["track_ptr"][:n_t + 1].tobytes() == want["track_ptr"].tobytes() and outs["obs_kp"][:n_o].tobytes() == want["obs_kp"].tobytes()
    assert outs["node_track"][:-1].tobytes() == want["node_track"].tobytes()
    assert all((a[n:] == SENTINEL).all() for a, n in ((outs["track_ptr"], n_t + 1), (outs["obs_frame"], n_o), (outs["flags"], n_t), (outs["node_track"], -1)))


def test_both_staging_paths(ctx):
    """IoStage packs arrays up to 256 KB into one copy through its pinned mirror and copies larger ones directly: the hand-written
    cases are all below, the scene's q and t (and with 4 x the keypoints its node_track) are above."""
    small, _ = HAND["c_keep_cuts"]
    assert max(small[k].nbytes for k in ("pairs", "counts", "offsets", "q", "t", "keep")) < 256 * 1024
    same(build(ctx, small, small["keep"]), TR.reference_tracks(small, small["keep"]), "small")
    big = dict(TC.scene())
    assert big["q"].nbytes > 256 * 1024 and big["keep"].nbytes < 256 * 1024
    big["kp"] = [4 * k for k in big["kp"]]                    # 72 000 nodes: node_track comes back by a direct copy too
    want = TR.reference_tracks(big, big["keep"])
    assert want["node_track"].nbytes > 256 * 1024
    same(build(ctx, big, big["keep"]), want, "big")
