"""GPU: the C++ adapters of the track building (include/eacham/TracksHip.hpp) through tests/cpp/tracks_driver.cpp — BuildTracks and
ResidentMatchGraph::Tracks against tests/tracks_reference.py field for field, and GatherTrackPixels' output fed unchanged to
eacham_triangulate_tracks on a noise-free synthetic scene with ground-truth matches: every clean track is the observations of ONE
landmark and every landmark's observations lie in one track; the triangulation returns EACHAM_OK with a status for every track
(the points themselves are tests/test_tri_gpu.py's business: no tolerance here)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import tracks_cases as TC
import tracks_reference as TR
from eacham_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
DTYPES = {"track_ptr": np.int64, "obs_frame": np.uint32, "obs_kp": np.uint32, "flags": np.uint8, "node_track": np.int32}


def build_driver(exe):
    lib = os.path.join(ROOT, "eacham_amd", "lib")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + CPP,
           os.path.join(CPP, "tracks_driver.cpp"), "-L" + lib, "-leacham_hip", "-Wl,-rpath," + lib, "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def write_input(path, case, keep, min_len, policy, geometry=None):
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(case["kp"])))
        f.write(np.asarray(case["kp"], dtype=np.int64).tobytes())
        f.write(struct.pack("i", len(case["counts"])))
        f.write(case["pairs"].astype(np.int32).tobytes() + case["counts"].astype(np.int32).tobytes())
        f.write(np.r_[case["offsets"], case["q"].size].astype(np.int64).tobytes())
        f.write(struct.pack("q", case["q"].size) + case["q"].tobytes() + case["t"].tobytes())
        f.write(struct.pack("i", keep is not None) + (b"" if keep is None else keep.tobytes()))
        f.write(struct.pack("iii", min_len, policy, geometry is not None))
        if geometry is not None:
            f.write(np.asarray(geometry["K"], dtype=np.float64).tobytes() + np.asarray(geometry["T"], dtype=np.float64).tobytes())
            for xy in geometry["keypoints"]:
                f.write(np.asarray(xy, dtype=np.float64).tobytes())
            f.write(struct.pack("ff", 4.0, np.deg2rad(1.0)))


def read_arrays(path, dtypes):
    out = []
    with open(path, "rb") as f:
        for dt in dtypes:
            n, size = struct.unpack("qq", f.read(16))
            assert size == np.dtype(dt).itemsize
            out.append(np.frombuffer(f.read(n * size), dtype=dt))
        assert f.read() == b""
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("tracks") / "tracks_driver"))


def run(driver, tmp_path, case, keep, min_len, policy, geometry=None, extra=()):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_input(fin, case, keep, min_len, policy, geometry)
    r = subprocess.run([driver, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    arrays = read_arrays(fout, list(DTYPES.values()) * 2 + list(extra))
    built, res = dict(zip(DTYPES, arrays[:5])), dict(zip(DTYPES, arrays[5:10]))
    return built, res, arrays[10:]


@pytest.mark.gpu
@pytest.mark.parametrize("which,policy", [("scene", 0), ("scene", 1), ("b_conflict", 1), ("e_empty_pairs_empty_frame", 0)])
def test_adapters_equal_the_reference(driver, tmp_path, which, policy):
    if which == "scene":
        case, keep, min_len = TC.scene(), TC.scene()["keep"], 2
        want = TC.scene_reference(True, 2, policy)
    else:
        case = TC.hand_written()[which][0]
        keep, min_len = case["keep"], case["min_len"]
        want = TR.reference_tracks(case, keep, min_len, policy)
    built, res, _ = run(driver, tmp_path, case, keep, min_len, policy)
    for f in TR.FIELDS:
        assert built[f].tobytes() == want[f].tobytes(), f"BuildTracks: {f}"
        assert res[f].tobytes() == want[f].tobytes(), f"ResidentMatchGraph::Tracks: {f}"


def ground_truth_scene():
    """8 cameras, 300 landmarks seen by 4 cameras each, no pixel noise; a frame's keypoints are its observations in a seeded
    shuffle; every pair of frames lists the landmarks both see."""
    sc = synth.make_scene(8, 300, 4, seed=11, pixel_noise=0.0)
    rng = np.random.default_rng(11)
    F = 8
    lm_of, xy, kp_of = [], [], []
    for f in range(F):
        idx = np.nonzero(sc["obs_cam"] == f)[0]
        idx = idx[rng.permutation(idx.size)]
        lm_of.append(sc["obs_lm"][idx].astype(np.int64))
        xy.append(sc["obs_uv"][idx])
        kp_of.append({int(l): k for k, l in enumerate(lm_of[-1])})
    pm = []
    for f1 in range(F):
        for f2 in range(f1 + 1, F):
            common = sorted(set(kp_of[f1]) & set(kp_of[f2]))
            pm.append(((f1, f2), [(kp_of[f1][l], kp_of[f2][l]) for l in common]))
    case = TC.make([len(l) for l in lm_of], pm)
    return case, lm_of, {"K": sc["K"], "T": sc["T_true"].reshape(F, 16), "keypoints": xy}


@pytest.mark.gpu
def test_tracks_feed_the_triangulation_unchanged(driver, tmp_path):
    case, lm_of, geo = ground_truth_scene()
    built, res, (uv, rc, status, points) = run(driver, tmp_path, case, None, 2, 0, geo, extra=(np.float64, np.int32, np.int32, np.float64))
    want = TR.reference_tracks(case)
    for f in TR.FIELDS:
        assert built[f].tobytes() == want[f].tobytes() == res[f].tobytes(), f
    n_tracks = built["flags"].size
    assert n_tracks > 200 and not built["flags"].any()
    obs_lm = np.array([lm_of[f][k] for f, k in zip(built["obs_frame"], built["obs_kp"])])
    obs_track = np.repeat(np.arange(n_tracks), np.diff(built["track_ptr"]))
    both = np.unique(np.stack([obs_track, obs_lm], axis=1), axis=0)
    assert len(both) == n_tracks == len(np.unique(both[:, 1]))                # one landmark per track, one track per landmark
    seen_twice = [l for l in range(300) if sum((lm_of[f] == l).any() for f in range(8)) >= 2]
    assert sorted(both[:, 1].tolist()) == seen_twice and (np.diff(built["track_ptr"]) == 4).all()
    # GatherTrackPixels: the pixel of every observation, in the observations' order
    want_uv = np.array([geo["keypoints"][f][k] for f, k in zip(built["obs_frame"], built["obs_kp"])])
    assert uv.tobytes() == want_uv.tobytes()
    assert rc.tolist() == [0] and status.size == n_tracks and ((status >= 0) & (status <= 3)).all()
    assert points.size == 3 * n_tracks
