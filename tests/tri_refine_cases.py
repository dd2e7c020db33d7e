"""Seeded inputs of the track refinement tests (tests/test_tri_refine_reference.py, tests/test_tri_refine_gpu.py,
tests/test_tri_refine_cpp_gpu.py, tests/golden/make_tri_refine_golden.py). A track is a point 4..9 deep in front of m cameras whose
centres lie in a box of half-width `baseline` (0.05..1) about the origin, each turned by up to 0.1 rad; K of 960 px; pixel noise of
0 or 1 px. A noisy track starts from the DLT point of its first two views (what eacham_triangulate_tracks hands over, but for the
choice of the pair); an exact one starts 1..5 % of its depth away from the truth. numpy only: nothing here needs the device or mpmath."""
import os

import numpy as np

K = np.array([960.0, 960.0, 640.0, 480.0])
THR = 4.0                      # max_repr_error of the recount, pixels
MAX_TRIES = 20
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tri_refine_golden.npz")
LENGTHS = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 64, 65, 130)   # on either side of the 8-lane trip of the kernel
WAVE_AT = 32                   # gpu_list: the tracks WAVE_AT .. WAVE_AT + 7 share a wave (8 tracks each, aligned)


def unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def camera(rng, baseline):
    """A row-major 4 x 4 world->camera matrix [16]: centre in the box, turned by up to 0.1 rad about a random axis."""
    a, ang = unit(rng), rng.uniform(-0.1, 0.1)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    c = baseline * rng.uniform(-1, 1, 3) * np.array([1.0, 1.0, 0.3])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, -R @ c
    return T.reshape(16)


def project(T, X):
    p = T.reshape(4, 4)[:3, :3] @ X + T.reshape(4, 4)[:3, 3]
    return np.array([K[0] * p[0] / p[2] + K[2], K[1] * p[1] / p[2] + K[3]])


def dlt(T1, uv1, T2, uv2):
    """The two-view DLT point (the null vector of the 4 x 4 of the reference's TriangulatePoint)."""
    A = []
    for T, uv in ((T1, uv1), (T2, uv2)):
        T = T.reshape(4, 4)
        x, y = (uv[0] - K[2]) / K[0], (uv[1] - K[3]) / K[1]
        A += [y * T[2] - T[1], x * T[2] - T[0]]
    v = np.linalg.svd(np.array(A))[2][-1]
    return v[:3] / v[3]


def track(m, seed, noise=1.0, baseline=0.5, off=None):
    """dict T [m, 16], uv [m, 2], X0 [3] (the start), X [3] (the truth). off None: the start is the DLT point of the first two views
    (the truth for m < 2); else the truth moved by `off` times its depth in a random direction."""
    rng = np.random.default_rng(seed)
    X = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4, 9)])
    T = np.array([camera(rng, baseline) for _ in range(m)]).reshape(m, 16)
    uv = np.array([project(t, X) for t in T]).reshape(m, 2) + noise * rng.standard_normal((m, 2))
    step = unit(rng)
    X0 = X + off * X[2] * step if off is not None else (dlt(T[0], uv[0], T[1], uv[1]) if m >= 2 else X.copy())
    return dict(T=T, uv=uv, X0=X0, X=X, m=m, noise=noise, baseline=baseline)


def pack(tracks, masks=None, has=None, seed=5):
    """The wire form of a list of tracks: dict transforms [F, 16], track_ptr int64, obs_frame uint32, obs_uv, points, has_point,
    use_mask (None: masks is None). Every observation has a row of its own in the table; the rows are shuffled, so obs_frame is no
    identity."""
    n_obs = sum(t["m"] for t in tracks)
    perm = np.random.default_rng(seed).permutation(n_obs).astype(np.uint32)
    rows = np.concatenate([t["T"].reshape(-1, 16) for t in tracks] + [np.zeros((0, 16))])
    transforms = np.zeros((n_obs, 16))
    transforms[perm] = rows
    ptr = np.zeros(len(tracks) + 1, np.int64)
    np.cumsum([t["m"] for t in tracks], out=ptr[1:])
    uv = np.concatenate([t["uv"].reshape(-1, 2) for t in tracks] + [np.zeros((0, 2))])
    return dict(transforms=transforms, track_ptr=ptr, obs_frame=perm, obs_uv=uv, points=np.array([t["X0"] for t in tracks]).reshape(-1, 3),
                has_point=np.ones(len(tracks), np.uint8) if has is None else np.asarray(has, np.uint8),
                use_mask=None if masks is None else np.concatenate([np.asarray(m, np.uint8) for m in masks] + [np.zeros(0, np.uint8)]))


def sublist(c, rows):
    """The tracks `rows` of a packed list, in that order, over the same transform table."""
    ptr = c["track_ptr"]
    idx = np.concatenate([np.arange(ptr[t], ptr[t + 1]) for t in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    out = dict(c)
    out["track_ptr"] = np.concatenate([[0], np.cumsum([ptr[t + 1] - ptr[t] for t in rows])]).astype(np.int64)
    out["obs_frame"], out["obs_uv"] = c["obs_frame"][idx], c["obs_uv"][idx]
    out["points"], out["has_point"] = c["points"][list(rows)], c["has_point"][list(rows)]
    out["use_mask"] = None if c["use_mask"] is None else c["use_mask"][idx]
    return out


def args(c, with_mask=True):
    """The positional arguments of refine_tracks (the library's and the restatement's) up to the mask."""
    return (c["transforms"], c["track_ptr"], c["obs_frame"], c["obs_uv"], K, c["points"], c["has_point"], c["use_mask"] if with_mask else None)


def seeded(count=210, seed0=9000):
    """The classes the loop was prototyped on: 2..17 views, baselines 0.05 / 0.2 / 1, 0 or 1 px of noise; a noisy track starts at its
    first pair's DLT point, an exact one 1 / 3 / 5 % of its depth away from the truth. A list of track() dicts."""
    sizes = (2, 3, 4, 5, 7, 8, 9, 12, 16, 17)
    out = []
    for k in range(count):
        noise = float((k // 2) % 2)
        out.append(track(sizes[k % len(sizes)], seed0 + k, noise, (0.05, 0.2, 1.0)[k % 3], None if noise > 0 else (0.01, 0.03, 0.05)[k % 3]))
    return out


def mask_with(n, pattern):
    """A use mask over n observations: 'ones', 'alternating' (every other one from the first), 'two' (the first and the last),
    'one' (the last)."""
    m = np.zeros(n, np.uint8)
    if pattern == "ones":
        m[:] = 1
    elif pattern == "alternating":
        m[::2] = 1
    elif pattern == "two":
        m[0] = m[n - 1] = 1
    else:
        m[n - 1] = 1
    return m


def gpu_list():
    """The list of the byte-identity test: (packed list, notes). 70 tracks:
       0..12   the LENGTHS with every observation used;  13..22 the lengths from 3 on with alternating masks;
       23..28  lengths 9, 17 and 65 with exactly two and exactly one observation used;
       29..31  not refined, in the middle: no point, a used view with the point behind it, a NaN pixel in a used observation;
       32..39  ONE WAVE: exact tracks that start at the truth (converged after one try) around two far starts whose tries are
               rejected (the start 30 and 60 depths beyond the truth);
       40      a NaN pixel in an UNUSED observation (refined as if it were not there);  41 a pair with next to no parallax;
       42..69  fillers of 2..12 views under random masks of at least two used observations."""
    rng = np.random.default_rng(77)
    tracks, masks, has, notes = [], [], [], []

    def add(t, mask, note, point=True):
        tracks.append(t), masks.append(mask), has.append(1 if point else 0), notes.append(note)

    for k, m in enumerate(LENGTHS):
        add(track(m, 100 + k, 1.0, 0.5), mask_with(m, "ones"), f"all {m}")
    for k, m in enumerate(LENGTHS[3:]):
        add(track(m, 120 + k, 1.0, 0.3), mask_with(m, "alternating"), f"alternating {m}")
    for k, m in enumerate((9, 17, 65)):
        add(track(m, 140 + k, 1.0, 0.5), mask_with(m, "two"), f"two of {m}")
        add(track(m, 150 + k, 1.0, 0.5), mask_with(m, "one"), f"one of {m}")
    add(track(6, 160, 1.0, 0.5), mask_with(6, "ones"), "no point", point=False)
    t = track(10, 161, 1.0, 0.5)
    Tb = t["T"][4].reshape(4, 4).copy()
    Tb[:3] = np.diag([1.0, -1.0, -1.0]) @ Tb[:3]                 # view 4 looks the other way: the point is behind it
    t["T"][4] = Tb.reshape(16)
    add(t, mask_with(10, "ones"), "behind")
    t = track(11, 162, 1.0, 0.5)
    t["uv"][9, 1] = np.nan
    add(t, mask_with(11, "ones"), "nan used")
    assert len(tracks) == WAVE_AT
    for j in range(8):
        if j in (3, 6):
            t = track(5 if j == 3 else 12, 170 + j, 1.0, 0.5)
            t["X0"] = t["X"] + (30.0 if j == 3 else 60.0) * t["X"][2] * np.array([0.0, 0.0, 1.0])
            add(t, mask_with(t["m"], "ones"), "far start")
        else:
            t = track(3 + j, 170 + j, 0.0, 0.5, off=0.0)
            add(t, mask_with(t["m"], "ones"), "one try")
    t = track(11, 180, 1.0, 0.5)
    t["uv"][9, 1] = np.nan
    m = mask_with(11, "ones")
    m[9] = 0
    add(t, m, "nan unused")
    add(track(2, 181, 1.0, 1e-6, off=0.05), mask_with(2, "ones"), "no parallax")   # (its DLT point would lie behind the cameras)
    while len(tracks) < 70:
        k = len(tracks)
        n = int(rng.integers(2, 13))
        m = np.zeros(n, np.uint8)
        m[rng.choice(n, int(rng.integers(2, n + 1)), replace=False)] = 1
        add(track(n, 200 + k, 1.0, float(rng.choice([0.05, 0.2, 1.0]))), m, f"filler {n}")
    return pack(tracks, masks, has), notes


def cpp_case():
    """For the C++ adapter, which triangulates itself: 40 tracks of 2..9 views with 1 px of noise over shared frames' worth of
    cameras, every fifth with one observation moved by 40 px (so that track is not added and not refined), a track of one view.
    dict with the packed list (int64 track_ptr; the driver narrows it for eacham_triangulate_tracks), max_repr_error, min_tri_angle."""
    tracks = []
    for k in range(40):
        t = track(1 if k == 17 else 2 + k % 8, 300 + k, 1.0, (0.2, 0.5, 1.0)[k % 3])
        if k % 5 == 4 and t["m"] >= 3:
            t["uv"][1] += 40.0
        tracks.append(t)
    return dict(list=pack(tracks), max_repr_error=4.0, min_tri_angle=0.002)
