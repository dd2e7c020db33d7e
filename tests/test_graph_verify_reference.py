"""CPU: the sample streams eacham_graph_verify draws on the device are the host's, stated once (include/eacham/CvSampling.hpp:
CvRNG, cv_get_subset, cv_check_subset_homography, mix, counter_sample — what lmeds_samples / draw_samples of TwoViewHip.hpp now
call). Compiled for the host they must give the subsets the separate host statements gave before they were shared: the streams of
tests/golden/graph_verify_streams.json were recorded from the commit before (tests/golden/make_graph_verify_golden.py). And the cases
of tests/graph_verify_cases.py do what they are for, shown on the host alone."""
import json
import os

import numpy as np
import pytest

import graph_verify_cases as GC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_verify_streams.json")
MASK64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def draw(g, kind, sampling, iterations, check=None):
    return GC.host_samples(GC.gather(g), GC.M[kind], kind == "homography" if check is None else check, sampling, iterations, g["seeds"])


@pytest.mark.parametrize("sampling", ["opencv", "counter"])
@pytest.mark.parametrize("kind", ["homography", "essential"])
def test_shared_streams_give_the_recorded_subsets(golden, kind, sampling):
    for name, g, its in (("small", GC.small(), 72 if kind == "homography" else 89), ("large", GC.large(), 3)):
        want = golden[f"{name}/{kind}/{sampling}/{its}"]
        got = draw(g, kind, sampling, its)
        assert len(got) == len(want) == len(g["counts"])
        for p, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, np.array(b, dtype=np.int32).reshape(-1, GC.M[kind])), f"{name} pair {p}"
    # fewer iterations are a prefix of the same stream
    g = GC.small()
    for p, (a, b) in enumerate(zip(draw(g, kind, sampling, 3), golden[f"small/{kind}/{sampling}/{72 if kind == 'homography' else 89}"])):
        assert np.array_equal(a, np.array(b, dtype=np.int32).reshape(-1, GC.M[kind])[:3]), f"pair {p}"
    assert all(len(a) == 0 for a in draw(g, kind, sampling, 0))


def test_unchecked_streams_equal_the_recording_and_an_independent_statement(golden):
    for n, m, its in ((4, 4, 72), (8, 4, 72), (5, 5, 89)):
        z = [(np.zeros((n, 2)), np.zeros((n, 2)))]
        got = GC.host_samples(z, m, False, "opencv", its, [0])[0]
        assert np.array_equal(got, np.array(golden[f"unchecked/{n}/{m}/{its}"], dtype=np.int32))
        assert np.array_equal(got, GC.py_subsets(n, m, its)[0])


def py_counter(n, m, count, seed):
    """The counter stream stated independently: splitmix64 of seed * 0x100000001B3 + (sample << 20) + draw, modulo n, repeats skipped."""
    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & MASK64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
        return x ^ (x >> 31)
    out = []
    for s in range(count):
        sub, ctr = [], 0
        while len(sub) < m:
            v = mix((seed * 0x100000001B3 + (s << 20) + ctr) & MASK64) % n
            ctr += 1
            if v not in sub:
                sub.append(v)
        out.append(sub)
    return np.array(out, dtype=np.int32).reshape(count, m)


@pytest.mark.parametrize("kind", ["homography", "essential"])
def test_counter_stream_equals_an_independent_statement(kind):
    g, m = GC.small(), GC.M[kind]
    got = draw(g, kind, "counter", 72)
    for p, n in enumerate(g["counts"]):
        want = py_counter(int(n), m, 72, int(g["seeds"][p])) if n >= m else np.zeros((0, m), np.int32)
        assert np.array_equal(got[p], want), f"pair {p}"
    assert not np.array_equal(got[3], got[8][:, :m])   # per-pair seeds and sizes: the pairs do not share a stream


def test_collinear_pair_yields_no_samples_and_its_neighbours_all_of_theirs():
    g = GC.small()
    uv1, _ = GC.gather(g)[GC.COLLINEAR]
    d = uv1 - uv1[0]
    assert len(uv1) == 12 and not (d[:, 0] * d[1, 1] - d[:, 1] * d[1, 0]).any()            # every image-1 point on one line
    got = draw(g, "homography", "opencv", 72)
    assert len(got[GC.COLLINEAR]) == 0
    assert [len(s) for s in got] == [72, 72, 0, 72, 72, 0, 0, 72, 72]
    assert len(draw(g, "essential", "opencv", 89)[GC.COLLINEAR]) == 89                     # no checkSubset: the pair draws like any other


def test_refusing_pair_draws_another_stream_than_the_unchecked_one():
    g = GC.small()
    checked = draw(g, "homography", "opencv", 72)[GC.REFUSING]
    unchecked = draw(g, "homography", "opencv", 72, check=False)[GC.REFUSING]
    assert g["counts"][GC.REFUSING] == 8
    assert checked.shape == unchecked.shape == (72, 4) and not np.array_equal(checked, unchecked)
    assert np.array_equal(unchecked, GC.py_subsets(8, 4, 72)[0])
    # the four collinear image-1 points are the even matches. checkSubset tests the LAST point of a subset against the lines through
    # two earlier ones: no accepted subset ends on a third point of that line, and the unchecked stream has subsets that do
    on_line = lambda row: row[3] % 2 == 0 and int((row[:3] % 2 == 0).sum()) >= 2   # noqa: E731
    assert not any(on_line(row) for row in checked) and any(on_line(row) for row in unchecked)


@pytest.mark.parametrize("kind", ["homography", "essential"])
def test_pairs_of_exactly_m_matches_hit_the_duplicate_rejection(kind):
    g, m = GC.small(), GC.M[kind]
    p = GC.N_EQ_M[kind]
    assert g["counts"][p] == m
    its = 72 if kind == "homography" else 89
    want, rejected = GC.py_subsets(m, m, its)
    assert rejected > its                                                 # more than one thrown-away draw per subset
    got = draw(g, kind, "opencv", its, check=False)[p]
    assert np.array_equal(got, want) and all(sorted(r) == list(range(m)) for r in got.tolist())
    if kind == "essential":                                               # (no checkSubset: the case's own stream is this one)
        assert np.array_equal(draw(g, kind, "opencv", its)[p], want)


def test_the_small_graph_has_the_shapes_it_is_for():
    g = GC.small()
    assert g["n_kp"][1] == 0 and g["counts"].tolist() == [6, 5, 0, 64, 4, 3, 12, 8, 30]
    assert g["pairs"][0].tolist() == g["pairs"][1][::-1].tolist() and g["pairs"][3].tolist() == g["pairs"][4].tolist()
    assert (g["offsets"][1:] - g["offsets"][:-1] - g["counts"][:-1] == 3).all()            # gaps behind every pair's matches
    assert g["n_src"] == int(g["offsets"][-1] + g["counts"][-1])
    for (a, b), n in zip(GC.gather(g), g["counts"]):
        assert a.shape == b.shape == (n, 2)
    big = GC.large()
    assert big["counts"].tolist() == [16400] and big["n_kp"] == [16400, 16400]


def test_iterations_as_lmeds_computes_them():
    from eacham_amd import graph
    import estimator_reference as ER
    assert graph.lmeds_iterations("essential") == ER.lmeds_iterations(0.99, 5, 1000) == 89
    assert graph.lmeds_iterations("homography") == ER.lmeds_iterations(0.999, 4, 100) == 72
    for conf, m, mx, kind in ((0.5, 5, 1000, "essential"), (0.999, 4, 10, "homography"), (0.999999, 5, 1000, "essential"), (0.0, 4, 100, "homography")):
        assert graph.lmeds_iterations(kind, mx, conf) == ER.lmeds_iterations(conf, m, mx)
