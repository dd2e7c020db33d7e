"""Bundle-adjustment problems with the ragged observation structure of real SfM: track lengths with a heavy tail, windows
that cut tracks down to one observation, a freshly registered camera beside cameras with thousands of observations, global
observer counts that differ from the local degree. The scenes of eacham_amd.synth give every landmark the same number of
observations; here observations are REMOVED from such scenes (a kept observation keeps its generated pixel), and every
generator asserts on the CPU what its case is for, so that a later change to synth cannot silently empty it.

`case(name)` builds a case once and hands the same BaArrays to every test: nobody may write to it (dataclasses.replace for
another ordering). `group_stats*` state what ba_groups.hpp's structure holds for a problem (run, segment and block sizes).
numpy + eacham_amd.synth / ba only. Test infrastructure (tests/test_ba_ragged_reference.py, tests/test_ba_ragged_gpu.py)."""
import dataclasses
import functools
import json
import os
import subprocess

import numpy as np

from eacham_amd import ba, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("tail_small", "tail_large", "camera_counts", "window_cut", "mixed")
GRP_SLICE, GRP_SEG, GRP_LONG = 8, 8, 48        # eacham_amd/csrc/ba_groups.hpp
CAMERA_COUNTS = (0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025)   # camera 1 + i holds CAMERA_COUNTS[i]; the last camera >= 2049


def degree(A):
    return np.bincount(A.obs_point, minlength=len(A.points))


def camera_load(A):
    return np.bincount(A.obs_cam, minlength=len(A.cam_T_wc))


def _keep(A, mask):
    A.obs_cam, A.obs_point, A.obs_uv = A.obs_cam[mask].copy(), A.obs_point[mask].copy(), A.obs_uv[mask].copy()


def _rank_within_landmark(obs_point, words):
    """Rank of every observation among those of its landmark, in the order of `words` (one random word per observation)."""
    order = np.lexsort((words, obs_point))
    first = np.searchsorted(obs_point[order], obs_point[order], side="left")
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order)) - first
    return rank


def _tail_degrees(seed, stream, n, dmax):
    """n degrees drawn with P(d) proportional to 1 / d^2, d = 1..dmax."""
    p = 1.0 / np.arange(1, dmax + 1) ** 2
    cdf = np.cumsum(p / p.sum())
    return 1 + np.minimum(np.searchsorted(cdf, synth.rng_uniform(seed, stream, (n,)), side="right"), dmax - 1)


def _cut_to_tail(A, seed, dmax):
    """Keeps of every landmark a random d of its observations, d drawn by _tail_degrees."""
    want = _tail_degrees(seed, 900_001, len(A.points), dmax)
    rank = _rank_within_landmark(A.obs_point, synth.rng_u64(seed, 900_002, np.arange(len(A.obs_point))))
    _keep(A, rank < want[A.obs_point])
    return want


def _cut_camera(A, cam, count, seed):
    """Keeps `count` random observations of camera `cam`."""
    mine = np.nonzero(A.obs_cam == cam)[0]
    assert len(mine) >= count, (cam, len(mine), count)
    drop = mine[synth.rng_permutation(seed, 900_100 + cam, len(mine))[count:]]
    mask = np.ones(len(A.obs_cam), bool)
    mask[drop] = False
    _keep(A, mask)


def tail_small(seed=7):
    """12 cameras, 600 landmarks (<= 8192: eight lanes per landmark), degree 1..12 with a 1 / d^2 tail."""
    A = ba.BaArrays.from_scene(synth.make_scene(12, 600, 12, seed=seed, pixel_noise=1.0))
    _cut_to_tail(A, seed, 12)
    deg = degree(A)
    A.point_observers = deg.astype(np.int32)
    assert len(A.points) <= 8192 and set(deg) == set(range(1, 13)), sorted(set(deg))
    assert (deg == 1).sum() * 2 >= len(deg)
    return A


def tail_large(seed=11):
    """24 cameras, 9000 landmarks (> 8192: two lanes per landmark), degree 1..10 from the ten nearest cameras with a 1 / d^2 tail;
    then camera 5 is cut to one observation, camera 9 to none, camera 14 to 257, which leaves landmarks unobserved (observer
    count 0: the landmark prior then takes sigma = 1)."""
    A = ba.BaArrays.from_scene(synth.make_scene(24, 9000, 10, seed=seed, pixel_noise=1.0))
    _cut_to_tail(A, seed, 10)
    for cam, count in ((5, 1), (9, 0), (14, 257)):
        _cut_camera(A, cam, count, seed)
    deg, load = degree(A), camera_load(A)
    A.point_observers = deg.astype(np.int32)
    assert len(A.points) > 8192 and len(A.obs_cam) <= 20_000
    assert (load[5], load[9], load[14]) == (1, 0, 257) and load.max() > 2 * 257
    assert (deg == 0).any() and set(deg) >= set(range(0, 10))
    return A


def camera_counts(seed=6):
    """Fifteen cameras that all see all 2049 landmarks (as few as a camera of 2049 observations needs), cut per camera: camera 0
    (fixed) keeps 600, cameras 1..12 keep exactly 0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024 and 1025, camera 13 keeps 700,
    camera 14 all 2049. The cameras at the low counts are held by their pose priors: the undamped reduced system is the worst
    conditioned of the cases (numpy's fp64 solve of it agrees with the oracle's step to 6e-11 at this seed, 2e-10 at seed 3;
    tests/test_ba_ragged_reference.py asks for 1e-10 before a kernel is judged on the case)."""
    n_cams, n_lm = 15, 2049
    A = ba.BaArrays.from_scene(synth.make_scene(n_cams, n_lm, n_cams, seed=seed, pixel_noise=1.0))
    for cam, count in [(0, 600)] + [(1 + i, c) for i, c in enumerate(CAMERA_COUNTS)] + [(13, 700)]:
        _cut_camera(A, cam, count, seed)
    deg, load = degree(A), camera_load(A)
    A.point_observers = deg.astype(np.int32)
    assert len(A.points) <= 8192 and A.cam_fixed[0] == 1 and not A.cam_fixed[1:].any()
    assert tuple(load[1:13]) == CAMERA_COUNTS and load[14] == 2049 and load[0] == 600
    assert deg.min() >= 1
    return A


def window_cut(seed=5):
    """The 19-camera local window of a 60-camera scene; point_observers stays at the GLOBAL count (8), which the window's own
    degree reaches for few landmarks; every fourth landmark is further cut to one observation."""
    scene = synth.make_scene(60, 4000, 8, seed=seed, pixel_noise=1.0)
    A = ba.BaArrays.from_scene(synth.local_window(scene, 30, max_neighbours=18))
    assert A.cam_T_wc.shape[0] == 19 and (A.point_observers == 8).all()
    single = synth.rng_uniform(seed, 900_201, (len(A.points),)) < 0.25
    rank = _rank_within_landmark(A.obs_point, synth.rng_u64(seed, 900_202, np.arange(len(A.obs_point))))
    _keep(A, ~single[A.obs_point] | (rank == 0))
    deg = degree(A)
    assert deg.min() >= 1 and (deg == 1).sum() >= 0.2 * len(deg)
    assert (A.point_observers != deg).sum() > 0.5 * len(deg)
    assert camera_load(A).min() >= 1 and len(A.points) >= 50
    return A


def mixed(seed=7):
    """tail_small plus: landmark 3 seen by every camera, one camera seeing landmark 40 twice (the groups then go through the sorting
    entry kernel), landmark 77 behind one of its cameras (cheirality: zero residual and Jacobians), every 13th pixel moved by
    30 px (the Huber branch)."""
    full = ba.BaArrays.from_scene(synth.make_scene(12, 600, 12, seed=seed, pixel_noise=1.0))
    A = ba.BaArrays.from_scene(synth.make_scene(12, 600, 12, seed=seed, pixel_noise=1.0))
    _cut_to_tail(A, seed, 12)
    # every generated observation of landmark 3
    _keep(A, A.obs_point != 3)
    every = full.obs_point == 3
    first = int(np.nonzero(A.obs_point == 40)[0][0])
    A.obs_cam = np.concatenate([A.obs_cam, full.obs_cam[every], A.obs_cam[first:first + 1]]).astype(np.uint32)
    A.obs_point = np.concatenate([A.obs_point, full.obs_point[every], A.obs_point[first:first + 1]]).astype(np.uint32)
    A.obs_uv = np.concatenate([A.obs_uv, full.obs_uv[every], A.obs_uv[first:first + 1] + 0.7])
    A.obs_uv[::13] += 30.0
    behind = int(np.nonzero(A.obs_point == 77)[0][0])
    cam = int(A.obs_cam[behind])
    A.points = A.points.copy()
    A.points[77] = A.points[77] + 50.0 * (np.linalg.inv(A.cam_T_wc[cam])[:3, 3] - A.points[77])
    deg = degree(A)
    A.point_observers = deg.astype(np.int32)
    pairs = A.obs_point.astype(np.int64) * 12 + A.obs_cam
    assert len(np.unique(pairs)) == len(pairs) - 1 and deg[3] == 12 and len(np.unique(A.obs_cam[A.obs_point == 3])) == 12
    assert (A.cam_T_wc[cam] @ np.append(A.points[77], 1.0))[2] <= 0
    assert set(deg) == set(range(1, 13)) and (deg == 1).sum() * 2 >= len(deg)
    return A


def first_landmarks(A, n):
    """The problem of A's first n landmarks: same cameras, the observations of those landmarks."""
    B = dataclasses.replace(A, points=A.points[:n].copy(), point_observers=A.point_observers[:n].copy())
    _keep(B, A.obs_point < n)
    return B


@functools.lru_cache(maxsize=None)
def case(name):
    assert name in CASES, name
    return globals()[name]()


# ---- the landmark-group structure of a problem (eacham_amd/csrc/ba_groups.hpp) ---------------------------------------------

def stats_from_structure(groups, chunks, ent, laneinfo, rowinfo, blk, longblk, n_cams):
    """What the arrays of PreparedBA.structure (g_groups, g_chunks, g_ent, g_laneinfo, g_rowinfo, g_blk, g_longblk) hold: the
    lengths of the runs (entries of one camera block inside one group), of the segments (lanes folded into one partial)
    and of the blocks' partial lists. tests/cpp/groups_stats_driver.cpp states the same for the host definition."""
    groups, chunks, rowinfo, blk = groups.reshape(-1, 8), chunks.reshape(-1, 2), rowinfo.reshape(-1, 2), blk.reshape(-1, 4)
    rows = len(rowinfo) // len(groups)
    runs = {}
    for g, (lm0, nlm, row0, nrows, chunk0, nchunks, n_entries, n_segments) in enumerate(groups):
        for c in range(chunk0, chunk0 + nchunks):
            ent0, n4 = chunks[c]
            E = ent[256 * ent0:256 * (ent0 + n4)].reshape(n4, 64, 4).transpose(1, 0, 2).reshape(64, 4 * n4)
            length = ((E & 0xffff) != rows).sum(axis=1)
            used = np.nonzero(length)[0]
            c1 = rowinfo[g * rows + (E[used, 0] & 0xffff), 0].astype(np.int64)
            c2 = rowinfo[g * rows + (E[used, 0] >> 16), 0].astype(np.int64)
            for key, n in zip(c1 * (n_cams + 1) + c2, length[used]):
                runs[(g, int(key))] = runs.get((g, int(key)), 0) + int(n)
    run = np.array(list(runs.values()))
    seg = (laneinfo[(laneinfo & 0x0fffffff) != 0] >> 28) + 1
    assert run.sum() == groups[:, 6].sum() and len(seg) == groups[:, 7].sum() == blk[:, 3].sum()
    assert (len(longblk) > 0) == bool((blk[:, 3] > GRP_LONG).any())
    return {"rows": rows, "groups": len(groups), "short_runs": int((run <= 4).sum()), "long_runs": int((run > GRP_SLICE).sum()),
            "max_run": int(run.max()), "short_segments": int((seg < GRP_SEG).sum()), "full_segments": int((seg == GRP_SEG).sum()),
            "long_blocks": int(len(longblk)), "max_partials": int(blk[:, 3].max())}


def group_stats_of(pb, n_cams):
    """stats_from_structure of a prepared problem (a context that builds the landmark groups)."""
    names = ("g_groups", "g_chunks", "g_ent", "g_laneinfo", "g_rowinfo", "g_blk", "g_longblk")
    return stats_from_structure(*[pb.structure(n) for n in names], n_cams)


def build_stats_driver(path):
    exe = os.path.join(str(path), "groups_stats_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "groups_stats_driver.cpp")],
                   check=True, capture_output=True)
    return exe


def host_group_stats(exe, A, rows=0):
    """The same figures from ba_groups.hpp's host statement (build_groups), for `rows` rows per group (0: the size the problem
    selects)."""
    order = np.argsort(A.obs_point, kind="stable")
    lm_ptr = np.concatenate([[0], np.cumsum(degree(A))])
    text = " ".join(map(str, [len(A.cam_T_wc), len(A.points), len(order), rows, *lm_ptr, *A.obs_cam[order]]))
    r = subprocess.run([exe], input=text + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    return json.loads(r.stdout)
