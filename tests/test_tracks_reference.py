"""CPU: pins the host reference of the track building (tests/tracks_reference.py) — the definition tests/test_tracks_gpu.py holds
eacham_tracks_build and eacham_graph_tracks to. Hand-written expected outputs for the small cases of tests/tracks_cases.py, and on
the seeded 30 x 600 scene the component partition against scipy.sparse.csgraph.connected_components on the same edges."""
import numpy as np
import pytest

import tracks_cases as TC
import tracks_reference as TR

HAND = TC.hand_written()


@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written_cases(name, policy):
    case, want = HAND[name]
    got = TR.reference_tracks(case, case["keep"], case["min_len"], policy)
    for f in TR.FIELDS:
        assert got[f].dtype == want[policy][f].dtype and np.array_equal(got[f], want[policy][f]), (name, policy, f, got[f])


def test_the_cases_are_what_they_are_for():
    b = HAND["b_conflict"][1]
    assert b[0]["flags"].tolist() == [1] and b[1]["flags"].size == 0 and (b[1]["node_track"] == -1).all()
    assert HAND["g_nothing_kept"][1][0]["track_ptr"].tolist() == [0]
    e = HAND["e_empty_pairs_empty_frame"][0]
    assert e["kp"][1] == 0 and (e["counts"] == 0).sum() == 3 and e["counts"][0] == 0 == e["counts"][-1]
    d = HAND["d_duplicates_reversed"][0]
    assert d["pairs"][1, 0] > d["pairs"][1, 1] and (d["q"][0], d["t"][0]) == (d["q"][1], d["t"][1])


@pytest.mark.parametrize("masked", [False, True])
def test_scene_partition_equals_scipy(masked):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    case = TC.scene()
    keep = case["keep"] if masked else None
    n = int(TR.kp_offsets_of(case["kp"])[-1])
    u, v = TR.kept_edges(case, keep)
    _, comp = connected_components(coo_matrix((np.ones(u.size, np.int8), (u, v)), shape=(n, n)), directed=False)
    ref = TC.scene_reference(masked)
    nt = ref["node_track"]
    touched = np.zeros(n, dtype=bool)
    touched[u] = touched[v] = True
    assert ((nt >= 0) == touched).all()                      # min_len 2, policy 0: every end of a kept edge is in a track
    # same partition: one track per scipy component and one scipy component per track, over the touched nodes
    pairs = np.unique(np.stack([nt[touched], comp[touched]], axis=1), axis=0)
    assert len(pairs) == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1])) == ref["flags"].size
    # canonical order: tracks by smallest node id, nodes ascending inside a track
    kpo = TR.kp_offsets_of(case["kp"])
    node = kpo[ref["obs_frame"]] + ref["obs_kp"]
    firsts = node[ref["track_ptr"][:-1]]
    assert (np.diff(firsts) > 0).all()
    inside = np.ones(node.size, dtype=bool)
    inside[ref["track_ptr"][:-1]] = False
    assert (np.diff(node)[inside[1:]] > 0).all()
    assert (nt[node] == np.repeat(np.arange(ref["flags"].size), np.diff(ref["track_ptr"]))).all()


def test_scene_filters():
    full, dropped, long3 = TC.scene_reference(True), TC.scene_reference(True, 2, 1), TC.scene_reference(True, 3, 0)
    assert dropped["flags"].size == int((full["flags"] == 0).sum()) and not dropped["flags"].any()
    assert long3["flags"].size == int((np.diff(full["track_ptr"]) >= 3).sum())
    assert np.diff(long3["track_ptr"]).min() >= 3
