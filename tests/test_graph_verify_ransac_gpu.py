"""GPU: eacham_graph_verify_ransac (eacham_amd/csrc/graph_verify.hip) against the host composition on the same context — the numpy
gather of every pair's matches, the project's own lmeds_samples / draw_samples compiled for the host (tests/graph_verify_cases.py:
host_samples), eacham_ransac_batch — EVERY output compared as bytes, for both samplings and for stage1 on either side of the number of
samples drawn; then the retained mask as the `keep` of the track builder, and LMedS and RANSAC masks replacing each other."""
import numpy as np
import pytest

import graph_verify_cases as GC
from eacham_amd import ResidentGraph, capi, ransac

pytestmark = pytest.mark.gpu

FIELDS = ["models", "inliers", "masks", "winner", "n_candidates", "n_used", "n_samples", "samples"]
CONFIDENCE = {"homography": 0.995, "essential": 0.999}
THRESHOLD = {"homography": 9.0, "essential": float(np.float32((1.0 / 500.0) ** 2)), "essential_noK": float(np.float32(1.0))}   # 3 px; 1 px at f = 500; 1 px on pixels


def resident(ctx, g):
    rg = ResidentGraph(ctx, g["n_frames"], g["pairs"], g["counts"], g["offsets"], g["q"], g["t"], g["n_kp"])
    rg.set_keypoints(g["xy"])
    return rg


@pytest.fixture(scope="module")
def graphs(hip_ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = resident(hip_ctx, getattr(GC, name)())
        return made[name]

    yield get
    for rg in made.values():
        rg.close()


_expected = {}


def expected(ctx, name, variant, sampling, iterations, seeded):
    """The host composition, computed once per combination (single pass) and left unchanged."""
    key = (name, variant, sampling, iterations, seeded)
    if key not in _expected:
        kind = variant.split("_")[0]
        g, m = getattr(GC, name)(), GC.M[kind]
        pts = GC.gather(g)
        seeds = g["seeds"] if seeded else np.full(len(pts), 12345, dtype=np.uint64)
        samples = GC.host_samples(pts, m, kind == "homography", sampling, iterations, seeds)
        rb = ransac.ransac_batch(ctx, kind, [a for a, _ in pts], [b for _, b in pts], samples, THRESHOLD[variant], CONFIDENCE[kind], 1 << 20,
                                 GC.K4 if variant == "essential" else None)
        masks = np.zeros(g["n_src"], dtype=np.uint8)
        for p, mk in enumerate(rb.masks):
            masks[int(g["offsets"][p]):int(g["offsets"][p]) + len(mk)] = mk
        fixed, n_samples = GC.fixed_stride(samples, iterations, m)
        _expected[key] = dict(models=rb.models, inliers=rb.inliers, masks=masks, winner=rb.winner, n_candidates=rb.n_candidates, n_used=rb.n_used,
                              n_samples=n_samples, samples=fixed)
        for v in _expected[key].values():
            v.setflags(write=False)
    return _expected[key]


def verify(rg, g, variant, sampling, iterations, seeded, stage1=0, retain=False):
    kind = variant.split("_")[0]
    return rg.verify_ransac(kind, THRESHOLD[variant], CONFIDENCE[kind], iterations, GC.K4 if variant == "essential" else None, sampling,
                            g["seeds"] if seeded else None, retain, True, stage1)


def assert_same(got, want, label):
    for name in FIELDS:
        a, b = getattr(got, name), want[name]
        assert a.dtype == b.dtype and a.shape == b.shape, f"{label}: {name}"
        assert a.tobytes() == b.tobytes(), f"{label}: {name} differs at {np.flatnonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8))[:8]}"


@pytest.mark.parametrize("seeded", [True, False], ids=["seeds", "seeds_null"])
@pytest.mark.parametrize("iterations", [0, 3, 40])
@pytest.mark.parametrize("sampling", ["opencv", "counter"])
@pytest.mark.parametrize("variant", ["homography", "essential", "essential_noK"])
def test_every_output_equals_the_host_composition(hip_ctx, graphs, variant, sampling, iterations, seeded):
    g, rg = GC.small(), graphs("small")
    kind = variant.split("_")[0]
    want = expected(hip_ctx, "small", variant, sampling, iterations, seeded)
    for stage1 in (0, 1, 3, 1 << 20):
        assert_same(verify(rg, g, variant, sampling, iterations, seeded, stage1), want, f"{variant}/{sampling}/{iterations}/stage1={stage1}")
    draws = (g["counts"] >= GC.M[kind]) & (iterations > 0)
    if kind == "homography" and sampling == "opencv":
        draws[GC.COLLINEAR] = False                                                              # getSubset gives up at once
    assert np.array_equal(want["n_samples"], np.where(draws, iterations, 0))
    for p in np.flatnonzero(~draws):                                                             # the "none" record
        assert want["winner"][p].tolist() == [-1, -1, -1] and not want["models"][p].any() and want["inliers"][p] == 0 and want["n_used"][p] == 0


@pytest.mark.parametrize("variant,sampling", [("homography", "opencv"), ("essential", "opencv"), ("essential", "counter")])
def test_eight_pairs_of_300_matches_stop_early(hip_ctx, graphs, variant, sampling):
    g, rg = GC.eight(), graphs("eight")
    want = expected(hip_ctx, "eight", variant, sampling, 200, True)
    for stage1 in (0, 8, 200):
        assert_same(verify(rg, g, variant, sampling, 200, True, stage1), want, f"eight/{variant}/{sampling}/stage1={stage1}")
    assert (want["winner"][:, 0] >= 0).all() and (want["inliers"] > 0).all() and (want["inliers"] < 300).any()
    assert (want["n_used"] <= want["n_samples"]).all()
    if variant == "essential":
        # 240 of 300 matches are right: a model with more than 153 inliers (0.51^5 > 1 - 0.001^(1 / 200)) ends the loop before 200 samples
        assert (want["inliers"] > 153).all() and (want["n_used"] < 200).all()


def tracks_equal(a, b):
    return all(getattr(a, f).tobytes() == getattr(b, f).tobytes() and getattr(a, f).shape == getattr(b, f).shape
               for f in ("track_ptr", "obs_frame", "obs_kp", "flags", "node_track"))


def test_retained_masks_feed_the_track_builder_and_replace_each_other(hip_ctx):
    g = GC.eight()
    rg = resident(hip_ctx, g)
    try:
        R = verify(rg, g, "essential", "opencv", 200, True, retain=True)
        for policy in (0, 1):
            got, want = rg.tracks_verified(conflict_policy=policy), rg.tracks(keep=R.masks, conflict_policy=policy)
            assert tracks_equal(got, want) and want.n_tracks > 0
            assert not tracks_equal(got, rg.tracks(conflict_policy=policy)), "the mask cuts matches: not the tracks of the whole graph"
        L = rg.verify("essential", GC.K4, "opencv", 89, g["seeds"], retain=True)                 # a later LMedS call replaces the mask
        assert L.masks.tobytes() != R.masks.tobytes()
        assert tracks_equal(rg.tracks_verified(), rg.tracks(keep=L.masks)) and not tracks_equal(rg.tracks_verified(), rg.tracks(keep=R.masks))
        H = verify(rg, g, "homography", "counter", 200, True, retain=True)                       # ... and a RANSAC call the LMedS one
        assert tracks_equal(rg.tracks_verified(), rg.tracks(keep=H.masks)) and not tracks_equal(rg.tracks_verified(), rg.tracks(keep=L.masks))
        verify(rg, g, "essential", "opencv", 200, True, retain=False)                            # without retain the graph keeps what it has
        assert tracks_equal(rg.tracks_verified(), rg.tracks(keep=H.masks))
    finally:
        rg.close()


def test_the_documented_errors_are_errors(hip_ctx, graphs):
    g, rg = GC.small(), graphs("small")
    want = expected(hip_ctx, "small", "essential", "opencv", 3, False)
    for kwargs, word in ((dict(threshold=float("nan")), "threshold"), (dict(threshold=-1.0), "threshold"), (dict(confidence=0.0), "confidence"),
                         (dict(confidence=1.0), "confidence"), (dict(stage1=-1), "stage1"), (dict(iterations=-1), "iterations")):
        args = dict(threshold=THRESHOLD["essential"], confidence=0.999, iterations=3, stage1=0)
        args.update(kwargs)
        with pytest.raises(capi.EachamError) as e:
            rg.verify_ransac("essential", args["threshold"], args["confidence"], args["iterations"], GC.K4, stage1=args["stage1"])
        assert e.value.code == capi.ERR_INVALID and word in str(e.value)
        assert_same(verify(rg, g, "essential", "opencv", 3, False), want, "after " + word)
    bare = ResidentGraph(hip_ctx, g["n_frames"], g["pairs"], g["counts"], g["offsets"], g["q"], g["t"], g["n_kp"])
    try:
        with pytest.raises(capi.EachamError) as e:
            bare.verify_ransac("essential", THRESHOLD["essential"], 0.999, 3, GC.K4)
        assert e.value.code == capi.ERR_INVALID and "keypoint" in str(e.value)
    finally:
        bare.close()
