"""The definition the device's track building (eacham_tracks_build / eacham_graph_tracks) is held to: a plain union-find on the
host that emits the canonical output.

  node            a keypoint, global id kp_offsets[f] + k
  edge            a match (q of f1, t of f2) of a pair whose keep byte is non-zero (keep None: every match)
  track           a connected component with at least min_len nodes, labelled by its smallest node id
  order           tracks by label; inside a track nodes ascending (frame-major, then keypoint)
  conflict        two keypoints of one frame in a track: bit 0 of its flag; conflict_policy 1 drops such tracks whole
  node_track      the track of every keypoint, -1 = none
"""
import numpy as np


def kp_offsets_of(kp_counts):
    kpo = np.zeros(len(kp_counts) + 1, dtype=np.int64)
    kpo[1:] = np.cumsum(np.asarray(kp_counts, dtype=np.int64))
    return kpo


def kept_edges(case, keep):
    """(u, v) global node ids of the kept matches, in pair order."""
    kpo = kp_offsets_of(case["kp"])
    us, vs = [], []
    for (f1, f2), c, o in zip(case["pairs"], case["counts"], case["offsets"]):
        if c == 0:
            continue
        sl = slice(int(o), int(o) + int(c))
        k = np.ones(c, dtype=bool) if keep is None else np.asarray(keep[sl]) != 0
        us.append(kpo[f1] + case["q"][sl].astype(np.int64)[k])
        vs.append(kpo[f2] + case["t"][sl].astype(np.int64)[k])
    if not us:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(us), np.concatenate(vs)


def labels_of(n_nodes, u, v):
    """label[i] = smallest node id of i's component, touched[i] = i is an end of a kept edge (sequential union-find)."""
    parent = list(range(n_nodes))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    touched = np.zeros(n_nodes, dtype=bool)
    for a, b in zip(u.tolist(), v.tolist()):
        touched[a] = touched[b] = True
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)   # the smaller root stays the root: a root is its tree's smallest node
    label = np.array([find(i) for i in range(n_nodes)], dtype=np.int64)
    return label, touched


def reference_tracks(case, keep=None, min_len=2, conflict_policy=0):
    kpo = kp_offsets_of(case["kp"])
    n_nodes = int(kpo[-1])
    u, v = kept_edges(case, keep)
    label, touched = labels_of(n_nodes, u, v)
    nodes = np.nonzero(touched)[0]
    order = np.argsort(label[nodes], kind="stable")        # by label; nodes stay ascending inside one label
    nodes = nodes[order]
    lab = label[nodes]
    frame = np.searchsorted(kpo, nodes, side="right") - 1  # (a frame without keypoints owns no id)
    starts = np.nonzero(np.r_[True, lab[1:] != lab[:-1]])[0] if nodes.size else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], nodes.size] if nodes.size else np.zeros(0, np.int64)
    track_ptr, obs_frame, obs_kp, flags = [0], [], [], []
    node_track = np.full(n_nodes, -1, dtype=np.int32)
    for s, e in zip(starts.tolist(), ends.tolist()):
        fr = frame[s:e]
        conflict = bool(np.any(fr[1:] == fr[:-1]))
        if e - s < min_len or (conflict_policy == 1 and conflict):
            continue
        node_track[nodes[s:e]] = len(flags)
        obs_frame.extend(fr.tolist())
        obs_kp.extend((nodes[s:e] - kpo[fr]).tolist())
        flags.append(1 if conflict else 0)
        track_ptr.append(len(obs_frame))
    return {"track_ptr": np.array(track_ptr, dtype=np.int64), "obs_frame": np.array(obs_frame, dtype=np.uint32),
            "obs_kp": np.array(obs_kp, dtype=np.uint32), "flags": np.array(flags, dtype=np.uint8), "node_track": node_track}


FIELDS = ("track_ptr", "obs_frame", "obs_kp", "flags", "node_track")
