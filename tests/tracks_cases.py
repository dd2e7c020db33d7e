"""The match graphs the track building is tested on (tests/test_tracks_reference.py on the host reference, tests/test_tracks_gpu.py
on the device). A case is a dict: kp (keypoints per frame), pairs, counts, offsets, q, t — the wire format of the matcher — and,
for the hand-written ones, `keep`, `min_len` and the expected output per conflict policy.
"""
import functools

import numpy as np

import tracks_reference as TR


def make(kp, pair_matches, keep=None, min_len=2):
    """pair_matches: [((f1, f2), [(q, t), ...]), ...] in pair order."""
    pairs = np.array([p for p, _ in pair_matches], dtype=np.int32).reshape(-1, 2)
    counts = np.array([len(m) for _, m in pair_matches], dtype=np.int32)
    offsets = np.zeros(len(pair_matches), dtype=np.int64)
    offsets[1:] = np.cumsum(counts)[:-1]
    flat = [qt for _, m in pair_matches for qt in m]
    q = np.array([a for a, _ in flat], dtype=np.uint32)
    t = np.array([b for _, b in flat], dtype=np.uint32)
    return {"kp": list(kp), "pairs": pairs, "counts": counts, "offsets": offsets, "q": q, "t": t,
            "keep": None if keep is None else np.array(keep, dtype=np.uint8), "min_len": min_len}


def expect(track_ptr, obs_frame, obs_kp, flags, node_track):
    return {"track_ptr": np.array(track_ptr, dtype=np.int64), "obs_frame": np.array(obs_frame, dtype=np.uint32),
            "obs_kp": np.array(obs_kp, dtype=np.uint32), "flags": np.array(flags, dtype=np.uint8),
            "node_track": np.array(node_track, dtype=np.int32)}


def hand_written():
    """name -> (case, {policy: expected}); node ids in the comments are kp_offsets[f] + k."""
    out = {}
    # (a) a triangle over three frames that closes on the keypoint it left from: nodes 0 (f0 k0), 3 (f1 k1), 4 (f2 k0)
    c = make([2, 2, 2], [((0, 1), [(0, 1)]), ((1, 2), [(1, 0)]), ((0, 2), [(0, 0)])])
    e = expect([0, 3], [0, 1, 2], [0, 1, 0], [0], [0, -1, -1, 0, 0, -1])
    out["a_triangle"] = (c, {0: e, 1: e})
    # (b) the triangle comes back to ANOTHER keypoint of frame 0: nodes 0, 1 (both f0), 3, 4 — flagged, or dropped whole
    c = make([2, 2, 2], [((0, 1), [(0, 1)]), ((1, 2), [(1, 0)]), ((0, 2), [(1, 0)])])
    out["b_conflict"] = (c, {0: expect([0, 4], [0, 0, 1, 2], [0, 1, 1, 0], [1], [0, 0, -1, 0, 0, -1]),
                             1: expect([0], [], [], [], [-1] * 6)})
    # (c) {0, 2} and {3, 5}, and an edge 0 - 5 between them whose keep byte is 0
    c = make([2, 2, 2], [((0, 1), [(0, 0)]), ((1, 2), [(1, 1)]), ((0, 2), [(0, 1)])], keep=[1, 1, 0])
    e = expect([0, 2, 4], [0, 1, 1, 2], [0, 0, 1, 1], [0, 0], [0, -1, 0, 1, -1, 1])
    out["c_keep_cuts"] = (c, {0: e, 1: e})
    # (d) the edge 0 - 1 twice, and the pair (2, 1): q indexes frame 2, t frame 1 -> the edge 3 - 1
    c = make([1, 1, 2], [((0, 1), [(0, 0), (0, 0)]), ((2, 1), [(1, 0)])])
    e = expect([0, 3], [0, 1, 2], [0, 0, 1], [0], [0, 0, -1, 0])
    out["d_duplicates_reversed"] = (c, {0: e, 1: e})
    # (e) pairs without matches at the head, in the middle and at the tail; frame 1 has no keypoints: ids 0 1 | | 2 3 | 4
    c = make([2, 0, 2, 1], [((0, 1), []), ((0, 2), [(1, 0)]), ((1, 3), []), ((2, 3), [(0, 0)]), ((0, 3), [])])
    e = expect([0, 3], [0, 2, 3], [1, 0, 0], [0], [-1, 0, 0, -1, 0])
    out["e_empty_pairs_empty_frame"] = (c, {0: e, 1: e})
    # (f) min_len = 3: {0, 2, 4} stays, the 2-track {1, 3} goes
    c = make([2, 2, 2], [((0, 1), [(0, 0), (1, 1)]), ((1, 2), [(0, 0)])], min_len=3)
    e = expect([0, 3], [0, 1, 2], [0, 0, 0], [0], [0, -1, 0, -1, 0, -1])
    out["f_min_len_3"] = (c, {0: e, 1: e})
    # (g) no kept edge at all
    c = make([2, 2], [((0, 1), [(0, 0), (1, 1)])], keep=[0, 0])
    e = expect([0], [], [], [], [-1] * 4)
    out["g_nothing_kept"] = (c, {0: e, 1: e})
    return out


SCENE_FRAMES, SCENE_KP = 30, 600


@functools.lru_cache(maxsize=None)
def scene(seed=7):
    """30 frames x 600 keypoints from landmark visibility: 300 landmarks seen in 20 consecutive frames (cyclically), 3600 seen in 3,
    40 keypoints per frame that see nothing; every pair of frames that shares a landmark lists it as a match; 5 % of the matches
    are rewired to a wrong keypoint of the second frame. `keep` (for the masked runs) drops 4 of 5 rewired matches and 3 % of
    the others, as an inlier mask would."""
    rng = np.random.default_rng(seed)
    F, K = SCENE_FRAMES, SCENE_KP
    seen = [[] for _ in range(F)]                     # per frame: the landmarks it sees
    n_lm = 0
    for count, length in ((300, 20), (3600, 3)):
        for l in range(count):
            for i in range(length):
                seen[(l % F + i) % F].append(n_lm)
            n_lm += 1
    kp_of = []                                        # per frame: landmark -> keypoint index
    for f in range(F):
        assert len(seen[f]) == 560
        slots = rng.permutation(K)[:len(seen[f])]
        kp_of.append(dict(zip(seen[f], slots.tolist())))
    pair_matches = []
    for f1 in range(F):
        for f2 in range(f1 + 1, F):
            common = sorted(set(kp_of[f1]) & set(kp_of[f2]))
            pair_matches.append(((f1, f2), [(kp_of[f1][l], kp_of[f2][l]) for l in common]))
    case = make([K] * F, pair_matches)
    m = case["q"].size
    wrong = rng.permutation(m)[:m // 20]
    case["t"][wrong] = (case["t"][wrong] + rng.integers(1, K, size=wrong.size).astype(np.uint32)) % K   # never the keypoint it was
    keep = np.ones(m, dtype=np.uint8)
    keep[wrong[: 4 * wrong.size // 5]] = 0
    keep[rng.permutation(m)[: 3 * m // 100]] = 0
    case["keep"] = keep
    case["rewired"] = wrong
    # what the scene is for
    kpo = TR.kp_offsets_of(case["kp"])
    assert kpo[-1] > 16384 and int(kpo[-1] - 1).bit_length() > 10          # the three-kernel scan; several radix passes
    assert case["q"].nbytes > 256 * 1024                                    # above what the staging packs: copied directly
    for k in (None, keep):
        ref = TR.reference_tracks(case, k)
        lens = np.diff(ref["track_ptr"])
        assert (ref["flags"] == 1).any() and (ref["flags"] == 0).any() and lens.max() > 10
    return case


@functools.lru_cache(maxsize=None)
def scene_reference(masked, min_len=2, conflict_policy=0):
    c = scene()
    return TR.reference_tracks(c, c["keep"] if masked else None, min_len, conflict_policy)


def bitrev6(i):
    return int(format(i, "06b")[::-1], 2)


def path64(comb):
    """A path over 64 frames of one keypoint each. Plain: the edges (k, k + 1), listed in descending k. Comb: the node at
    position i of the path is frame bitrev6(i) — every odd position carries an id above 32 between two below, so the first round
    can only hook those, and what is left is the same comb over 32 positions: the number of trees halves per round and no faster."""
    if comb:
        edges = [(bitrev6(i), bitrev6(i + 1)) for i in range(63)]
    else:
        edges = [(k, k + 1) for k in range(62, -1, -1)]
    return make([1] * 64, [(e, [(0, 0)]) for e in edges])
