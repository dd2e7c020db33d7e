"""Hard geometry for the triangulation kernels (eacham_amd/csrc/triangulate.hip): the inputs that synth.make_scene never
produces. Numpy only, seeded through synth's counter RNG, no file access. tests/tri_mp_reference.py states what they must give
at 60 digits; tests/golden/make_tri_hard_golden.py freezes both into tests/golden/tri_hard_golden.npz.

groups() returns {name: group}. A group is a dict with "kind" and "ladder" (True: built on a threshold ladder, so a few of
its decisions may sit closer to the threshold than double precision resolves) and, by kind,
  "tracks":  T [nf, 16], ptr, frame, uv, K [4], max_err, min_angle   (eacham_triangulate_tracks)
  "reproj":  T [nf, 16], frame, X [n, 3], uv [n, 2], K [4]           (eacham_reprojection_errors)
  "twoview": problems = [(uv1 [n, 2], uv2 [n, 2], Ts [nt, 16])], K, max_err, min_angle, dist, min_solution_matches
             (every problem through eacham_two_view_points under both values of strict, and the list through
             eacham_two_view_batch under both rules)
"""
import numpy as np

from eacham_amd import synth

SEED = 20261
K0 = np.array([960.0, 960.0, 400.0, 400.0])
K_SKEWED = np.array([1100.0, 870.0, 313.7, 455.2])          # fx != fy, principal point off the centre
MAX_ERR = np.float32(4.0)
MIN_ANGLE = np.float32(3.0 * 3.141592 / 180.0)              # SfmConfig.json:18-19 through SfmConfig.h:52-53
TV_MIN_ANGLE = np.float32(np.deg2rad(1.0))
DIST, MIN_SOLUTION = 50.0, 20
LADDER = (1e-1, 1e-3, 1e-6, 1e-9, 1e-12)
TRI_BLOCK = 256


def _u(stream, shape):
    return synth.rng_uniform(SEED, stream, shape)


def rigid(stream, spread=3.0):
    """A seeded world->world rigid motion G (4 x 4)."""
    w = (_u(stream, 6) * 2 - 1)
    G = np.eye(4)
    G[:3, :3] = synth.so3_exp(w[:3] * 1.5)
    G[:3, 3] = w[3:] * spread
    return G


def cam(center, R=None):
    """World->camera transform of a camera at `center` whose rows of R are its axes in world coordinates."""
    R = np.eye(3) if R is None else R
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ np.asarray(center, float)
    return T


def moved(T, G):
    """The camera T after the world moved by G (X -> G X)."""
    return T @ np.linalg.inv(G)


def project(T, X, K=K0):
    p = T[:3, :3] @ X + T[:3, 3]
    return np.array([K[0] * p[0] / p[2] + K[2], K[1] * p[1] / p[2] + K[3]])


def obs(T, X, K=K0, off=(0.0, 0.0)):
    return (T, project(T, X, K) + np.asarray(off, float))


def tracks_group(tracks, K=K0, max_err=MAX_ERR, min_angle=MIN_ANGLE, ladder=False):
    """tracks: a list of lists of (T 4 x 4, uv) or (T, uv, "own"). Equal transforms share one frame of the table, except an
    observation marked "own", which gets a frame slot of its own whatever the table already holds."""
    frames, index, ptr, frame, uv = [], {}, [0], [], []
    for tr in tracks:
        for T, p, *own in tr:
            key = np.ascontiguousarray(T, np.float64).tobytes()
            if own:
                key = (key, len(frames))
            if key not in index:
                index[key] = len(frames)
                frames.append(np.asarray(T, np.float64).reshape(16))
            frame.append(index[key])
            uv.append(p)
        ptr.append(len(frame))
    return {"kind": "tracks", "ladder": ladder, "T": np.array(frames).reshape(-1, 16), "ptr": np.array(ptr, np.int32),
            "frame": np.array(frame, np.uint32), "uv": np.array(uv, np.float64).reshape(-1, 2), "K": np.asarray(K, np.float64),
            "max_err": np.float32(max_err), "min_angle": np.float32(min_angle)}


def stereo(angle, G=None, lateral=(0.0, 0.0), b=1.0, K=K0, off2=(0.0, 0.0)):
    """Two parallel cameras a baseline b apart and a point seen under the triangulation angle `angle` (lateral = 0), after the
    rigid motion G of the whole scene."""
    Z = b / (2.0 * np.tan(angle / 2.0))
    X = np.array([lateral[0], lateral[1], Z])
    T1, T2 = cam([-b / 2, 0, 0]), cam([b / 2, 0, 0])
    a, c = obs(T1, X, K), obs(T2, X, K, off2)
    if G is not None:
        a, c = (moved(T1, G), a[1]), (moved(T2, G), c[1])
    return [a, c]


def good_pair(i, K=K0, stream=900):
    """An ordinary well-posed pair: 10-25 degrees of parallax, a pixel of noise."""
    w = _u(stream + i, 6)
    tr = stereo(np.deg2rad(10 + 15 * w[0]), rigid(stream + 100 + i % 3), lateral=(w[1] - 0.5, w[2] - 0.5), K=K, off2=(w[3] - 0.5, w[4] - 0.5))
    return tr


# ---- pairs ----------------------------------------------------------------------------------------------------------------

def parallax_ladder():
    a0 = float(MIN_ANGLE)
    tracks = []
    for g in range(3):                                   # three placements of the rig; the finest rung once
        for d in LADDER[:4] if g else LADDER:
            for s in (1.0, -1.0):
                tracks.append(stereo(a0 * (1 + s * d), rigid(10 + g) if g else None))
    for k, deg in enumerate((1.0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 2.999, 3.001, 30.0)):
        tracks.append(stereo(np.deg2rad(deg), rigid(20 + k % 3)))
    return tracks_group(tracks, ladder=True)


def depth_over_baseline():
    tracks = []
    for e in range(1, 9):
        for j in range(3):
            w = _u(30 + 8 * j + e, 4)
            Z = 10.0 ** e
            X = np.array([(w[0] - 0.5) * 0.4 * Z, (w[1] - 0.5) * 0.4 * Z, Z])
            T1, T2, G = cam([-0.5, 0, 0]), cam([0.5, 0.1 * j, 0]), rigid(60 + j)
            noise = 0.3 if j else 0.0                                           # (j = 0: exact pixels, kappa grows with the depth)
            a, c = obs(T1, X), obs(T2, X, off=(noise * (w[2] - 0.5), noise * (w[3] - 0.5)))
            tracks.append([(moved(T1, G), a[1]), (moved(T2, G), c[1])] if j else [a, c])
    return tracks_group(tracks)


def zero_baseline():
    """Undefined pairs (the same frame twice with the same pixel; two frames with equal transforms) between ordinary ones, and the
    same frame twice with two different pixels (defined: the null vector is the camera centre, both rays have no length)."""
    tracks = []
    for i in range(8):
        T = moved(cam([0.3 * i, 0.1, -0.2]), rigid(100 + i))
        p = K0[2:] + (_u(110 + i, 2) - 0.5) * 600
        tracks.append(good_pair(i))
        if i % 3 == 0:
            tracks.append([(T, p), (T.copy(), p.copy(), "own")])               # two frame slots, equal transforms
        elif i % 3 == 1:
            tracks.append([(T, p), (T, p)])                                    # one frame twice
        else:
            tracks.append([(T, p), (T, p + np.array([7.0, -3.0]))])            # one frame, two pixels
    tracks.append(good_pair(8))
    eye = np.eye(4)
    tracks.insert(0, [(eye, K0[2:].copy()), (eye, K0[2:].copy())])             # the first item of the call
    return tracks_group(tracks)


def on_baseline():
    """A point on the line through both centres: beyond both cameras (angle 0) and between two cameras that face each other
    (angle pi). With both pixels at the principal point the rays are one line and the point is undefined; a pixel off it is
    defined and badly conditioned."""
    tracks = []
    flip = np.diag([-1.0, 1.0, -1.0])                                            # looks down -z
    for i in range(6):
        G = rigid(130 + i) if i else None
        for T1, T2, X in ((cam([0, 0, 0]), cam([0, 0, 1.0]), np.array([0, 0, 5.0 + i])),
                          (cam([0, 0, 0]), cam([0, 0, 2.0 + i], flip), np.array([0, 0, 1.0]))):
            for off in ((0.0, 0.0), (0.5, 0.25)):
                a, c = obs(T1, X), obs(T2, X, off=off)
                if off == (0.0, 0.0):
                    a, c = (T1, K0[2:].copy()), (T2, K0[2:].copy())
                tracks.append([(moved(T1, G), a[1]), (moved(T2, G), c[1])] if G is not None else [a, c])
    return tracks_group(tracks)


def principal_point():
    """Observation 1 exactly at the principal point under the identity, camera 2 a pure translation: rows of the DLT matrix
    are unit vectors and most of the first sweep's column products are exactly zero."""
    tracks = []
    for i in range(12):
        w = _u(150 + i, 3)
        t = np.array([1.0 + i % 3, (i % 2) * 0.5, 0.0 if i < 8 else 0.25])
        X = np.array([0.0, 0.0, 2.0 + 3 * i])
        T1, T2 = np.eye(4), cam(t)
        tracks.append([(T1, K0[2:].copy()), obs(T2, X, off=(0.0, 0.0) if i % 4 else (w[0], w[1]))])
    return tracks_group(tracks)


def behind():
    """A point behind both cameras (its image through the pinhole is still a pixel) and behind one of two."""
    tracks = []
    flip = np.diag([-1.0, 1.0, -1.0])
    for i in range(12):
        w = _u(170 + i, 3) - 0.5
        G = rigid(180 + i % 3)
        if i % 2 == 0:
            T1, T2, X = cam([-0.7, 0, 0]), cam([0.7, 0, 0]), np.array([w[0], w[1], -4.0 - i])
        else:
            T1, T2 = cam([-0.7, 0, 0]), cam([0.7, 0, 9.0 + i], flip)                 # camera 2 looks down -z from z = 9 + i
            X = np.array([w[0], w[1], 14.0 + i])                                     # in front of camera 1, behind camera 2
        tracks.append([(moved(T1, G), project(T1, X)), (moved(T2, G), project(T2, X))])
    return tracks_group(tracks)


def world_z_nonpositive():
    """In front of both cameras with world z <= 0: TriangulatePointRansac answers false (`point3d.z() > 0`), every
    observation an inlier: status 2."""
    tracks = []
    down = np.diag([1.0, -1.0, -1.0])                                           # looks down -z of the world
    for i in range(12):
        w = _u(200 + i, 3) - 0.5
        X = np.array([w[0], w[1], -(10.0 ** (-(i % 4))) * (1 + i // 4)])
        T1, T2 = cam([-0.6, 0, 6.0], down), cam([0.6, 0.1, 6.0], down)
        tracks.append([obs(T1, X), obs(T2, X, off=(w[2], 0.0))])
    return tracks_group(tracks)


def shift_scale():
    """The scene scaled by 1e-3 and 1e3, and shifted away from the origin. kappa grows with the square of the shift (the
    homogeneous coordinate shrinks while the matrix grows): from 1e4 on the rule's own bound on the point is pixels wide or exceeds
    the scene, so this group is a ladder of shifts and its last rungs are undecided by construction."""
    def placed(base, shift, scale):
        S = np.eye(4)
        S[:3, 3] = shift * np.array([1.0, -0.5, 0.25])
        tr = []
        for T, p in base:
            T = moved(T, S).copy()
            T[:3, 3] *= scale                                                   # the world scaled: centres and points scale along
            tr.append((T, p))
        return tr

    tracks = []
    for i in range(10):
        tracks += [placed(good_pair(i, stream=230), 0.0, 1e-3), placed(good_pair(i, stream=230), 0.0, 1e3)]
    for i in range(13):
        tracks += [placed(good_pair(i, stream=240), s, 1.0) for s in (1e2, 1e3)]
    tracks += [placed(good_pair(i, stream=240), s, 1.0) for i, s in enumerate((1e4, 1e5, 1e6, 1e6, 1e6))]
    return tracks_group(tracks, ladder=True)


def skewed_intrinsics():
    return tracks_group([good_pair(i, K=K_SKEWED, stream=260) for i in range(12)], K=K_SKEWED)


def _dlt(T1, T2, p1, p2, K):
    x1, y1, x2, y2 = (p1[0] - K[2]) / K[0], (p1[1] - K[3]) / K[1], (p2[0] - K[2]) / K[0], (p2[1] - K[3]) / K[1]
    A = np.stack([y1 * T1[2] - T1[1], x1 * T1[2] - T1[0], y2 * T2[2] - T2[1], x2 * T2[2] - T2[0]])
    v = np.linalg.svd(A)[2][3]
    return v[:3] / v[3]


def error_ladder():
    """Observation 2 pushed off its ray until the pair's own point reprojects into camera 2 at max_err * (1 +- d): the push is
    found by a secant iteration on a double-precision DLT, the reference then says where each item really landed."""
    tracks = []
    for g in range(3):
        base = stereo(np.deg2rad(12.0 + 5 * g), rigid(300 + g), lateral=(0.3, -0.2))
        (T1, p1), (T2, p2) = base
        direction = np.array([np.cos(0.7 + g), np.sin(0.7 + g)])

        def err2(s):
            X = _dlt(T1, T2, p1, p2 + s * direction, K0)
            return np.linalg.norm(project(T2, X) - (p2 + s * direction))

        for d in LADDER[:3] if g else LADDER:             # (max_err is a float: rungs under its ulp are undecided, kept once)
            for sgn in (1.0, -1.0):
                target = float(MAX_ERR) * (1 + sgn * d)
                s0, s1 = 2 * target, 2.2 * target
                f0, f1 = err2(s0) - target, err2(s1) - target
                for _ in range(12):
                    if f1 == f0:
                        break
                    s0, s1, f0 = s1, s1 - f1 * (s1 - s0) / (f1 - f0), f1
                    f1 = err2(s1) - target
                tracks.append([(T1, p1), (T2, p2 + s1 * direction)])
    tracks += [good_pair(i, stream=330) for i in range(20)]
    return tracks_group(tracks, ladder=True)


PAIR_GROUPS = {"parallax_ladder": parallax_ladder, "depth_over_baseline": depth_over_baseline, "zero_baseline": zero_baseline,
               "on_baseline": on_baseline, "principal_point": principal_point, "behind": behind,
               "world_z_nonpositive": world_z_nonpositive, "shift_scale": shift_scale, "skewed_intrinsics": skewed_intrinsics,
               "error_ladder": error_ladder}


# ---- tracks ---------------------------------------------------------------------------------------------------------------

def ring(m, X, stream, radius=4.0, noise=0.3, K=K0):
    """m cameras on an arc looking at X, a fraction of a pixel of noise."""
    out = []
    for i in range(m):
        a = -0.6 + 1.2 * i / max(m - 1, 1)
        c = X + radius * np.array([np.sin(a), 0.15 * np.cos(3 * a), -np.cos(a)])
        T = synth.look_at_world_to_cam(c, X + np.array([0.05, 0.02, 0.0]))
        w = _u(stream + i, 2) - 0.5
        out.append(obs(T, X, K, off=noise * w))
    return out


def selection():
    tracks = []
    X, Y = np.array([0.2, -0.1, 6.0]), np.array([0.9, 0.4, 5.0])
    for i in range(6):                                                           # m = 3, all inliers / two of three
        tr = ring(3, X + 0.1 * i, 400 + 3 * i)
        if i % 2:
            tr[2] = (tr[2][0], tr[2][1] + np.array([60.0, -45.0]))
        tracks.append(tr)
    for i in range(4):                                                           # two pairs tie, different masks: the first stays
        a, b = ring(6, X, 430 + 6 * i), ring(6, Y + 0.2 * i, 460 + 6 * i)
        tracks.append(a[:3] + b[3:])                                             # 3 + 3: a tie at three inliers
        tracks.append(a[:2] + b[4:])                                             # 2 + 2: a tie at two, `best > 2` fails
    for i in range(4):                                                           # every pair under the angle gate, m = 3 and 4:
        far = X + np.array([0, 0, 200.0 + 50 * i])                               # cameras 0.4 apart near the origin, the point far away
        tracks.append([obs(cam([0.4 * j, 0.1 * (j % 2), 0.0]), far, off=0.2 * (_u(500 + 4 * i + j, 2) - 0.5)) for j in range(3 + i % 2)])
    for i in range(4):                                                           # the last pair has no baseline, an earlier pair wins
        tr = ring(3, X - 0.1 * i, 520 + 3 * i)
        tracks.append(tr + [(tr[2][0], tr[2][1].copy())])
    for i in range(4):                                                           # a frame twice (two pixels) inside a good track
        tr = ring(4, X + 0.3 * i, 540 + 4 * i)
        tr.insert(2, (tr[1][0], tr[1][1] + np.array([1.5, -1.0])))
        tracks.append(tr)
    return tracks_group(tracks)


def launch_straddle():
    """A track of 23 observations (253 pairs) and then tracks of 4 (6 pairs each): the second track's pairs are 253..258 of
    the flat launch, across the 256-thread workgroup."""
    X = np.array([-0.3, 0.2, 7.0])
    tracks = [ring(23, X, 600, noise=0.5)]
    tracks[0][7] = (tracks[0][7][0], tracks[0][7][1] + np.array([30.0, 30.0]))   # one outlier among the 23
    for i in range(3):
        tracks.append(ring(4, X + 0.5 * (i + 1), 640 + 4 * i))
    return tracks_group(tracks)


LAUNCH_SIZES = (TRI_BLOCK - 1, TRI_BLOCK, TRI_BLOCK + 1)


def launch_pool():
    """Two dozen pairs of every kind above. The tests draw 255 / 256 / 257 tracks from it in turn (tri_hard_rules.tiled) for
    calls that end just before, at and just after a workgroup of the selection kernel."""
    pool = []
    for i in range(8):
        pool += [good_pair(i, stream=700), stereo(np.deg2rad(0.5 + i), rigid(720 + i % 3)),
                 [(np.eye(4), K0[2:] + i), (np.eye(4), K0[2:] + i, "own")] if i % 4 == 0 else good_pair(i, stream=740)]
    return tracks_group(pool)


TRACK_GROUPS = {"selection": selection, "launch_straddle": launch_straddle, "launch_pool": launch_pool}


# ---- reprojection ---------------------------------------------------------------------------------------------------------

def reprojection():
    T, frame, X, uv = [np.eye(4).reshape(16)], [], [], []

    def add(Tm, Xp, p):
        T.append(np.asarray(Tm).reshape(16))
        frame.append(len(T) - 1)
        X.append(Xp)
        uv.append(p)

    for pz in (0.0, -1.0, -1e-3, 1e-300, -1e-300):                               # camera z of the point: zero, negative, denormal-near
        for xy in ((1.0, 2.0), (-0.5, 0.25)):
            add(np.eye(4), np.array([xy[0], xy[1], pz]), np.array([410.0, 395.0]))
    for i in range(24):
        G = rigid(800 + i)
        Tm = moved(cam([0.1 * i, 0, 0]), G)
        w = _u(830 + i, 3) - 0.5
        Xc = np.array([w[0], w[1], 3.0 + i])
        Xw = (G @ np.append(Xc + np.array([0.1 * i, 0, 0]), 1.0))[:3]
        size = (1e-7, 1e-3, 1.0, 4.0, 1e3, 1e7)[i % 6]                             # the error asked for, in pixels
        add(Tm, Xw, project(Tm, Xw) + size * np.array([0.6, -0.8]))
    return {"kind": "reproj", "ladder": False, "T": np.array(T), "frame": np.array(frame, np.uint32), "X": np.array(X),
            "uv": np.array(uv), "K": K0.copy()}


# ---- two views ------------------------------------------------------------------------------------------------------------

def relative_pose(i):
    w = _u(1000 + i, 6) - 0.5
    T = np.eye(4)
    T[:3, :3] = synth.so3_exp(0.3 * w[:3])
    t = np.array([1.0, 0.3 * w[3], 0.3 * w[4]])
    T[:3, 3] = t / np.linalg.norm(t)
    return T


def candidates(T):
    """The pose, its mirror, t scaled by 1e-8, pure rotation."""
    out = []
    for s in (1.0, -1.0, 1e-8, 0.0):
        M = T.copy()
        M[:3, 3] = s * T[:3, 3]
        out.append(M.reshape(16))
    return np.array(out)


def matches(T, n, stream, hard=False):
    """n matches of camera 1 = identity and camera 2 = T: points 2-8 units deep, half a pixel of noise, every ninth a wrong match;
    hard: depths of 10 .. 1e8 baselines and points behind camera 1 instead."""
    w = _u(stream, (n, 6))
    uv1, uv2 = np.zeros((n, 2)), np.zeros((n, 2))
    for i in range(n):
        Z = 2.0 + 6.0 * w[i, 0]
        if hard:
            Z = -3.0 - i if i % 3 == 2 else 10.0 ** (1 + (i % 8))
        X = np.array([(w[i, 1] - 0.5) * 0.5 * Z, (w[i, 2] - 0.5) * 0.5 * Z, Z])
        uv1[i], uv2[i] = project(np.eye(4), X), project(T, X) + (w[i, 3:5] - 0.5) * (0.0 if hard and i % 2 == 0 else 1.0)
        if i % 9 == 8 and not hard:
            uv2[i] += np.array([40.0, -25.0])
    return uv1, uv2


def _twoview(problems, ladder=False, min_solution=MIN_SOLUTION):
    return {"kind": "twoview", "ladder": ladder, "problems": problems, "K": K0.copy(), "max_err": MAX_ERR, "min_angle": TV_MIN_ANGLE,
            "dist": DIST, "min_solution_matches": min_solution}


def two_view_pairs():
    T0, T1 = relative_pose(0), relative_pose(1)
    still = K0[2:] + (_u(1102, (16, 2)) - 0.5) * 500                       # the same pixel in both images: under the identity
    return _twoview([(*matches(T0, 32, 1100), candidates(T0)), (*matches(T1, 24, 1101, hard=True), candidates(T1)),   # candidate, undefined
                     (still, still.copy(), np.array([np.eye(4).reshape(16), T0.reshape(16), np.eye(4).reshape(16)]))])


def two_view_shapes():
    """Problems of 1, 63, 64, 65 and 257 matches drawn in turn from one pool of 32, an empty problem between two ordinary ones,
    and a problem whose two candidates are the same pose (a tie on the vote: the first stays)."""
    T = relative_pose(2)
    u1, u2 = matches(T, 32, 1200)
    C = candidates(T)
    take = lambda n, o: (u1[(np.arange(n) + o) % 32], u2[(np.arange(n) + o) % 32])   # noqa: E731
    problems = [(*take(n, 3 * k), C if k % 2 else np.roll(C, 1, axis=0)) for k, n in enumerate((1, 63, 64, 65, 257))]
    problems.append((np.zeros((0, 2)), np.zeros((0, 2)), C))
    problems.append((*take(40, 5), C[[0, 0]]))
    problems.append((*take(30, 9), C[[1, 0, 0]]))
    return _twoview(problems)


def shifted(c):
    """Camera 2 = the identity rotation at centre c, as a camera-1 -> camera-2 transform."""
    return cam(c)


def with_mirror(T):
    M = T.copy()
    M[:3, 3] = -T[:3, 3]
    return np.array([T.reshape(16), M.reshape(16)])


def exact_matches(T, points, filler, stream):
    """Exact pixels of `points` under cameras I and T, then `filler` ordinary noisy matches."""
    u1 = [project(np.eye(4), X) for X in points]
    u2 = [project(T, X) for X in points]
    f1, f2 = matches(T, filler, stream)
    return np.array(u1 + list(f1)), np.array(u2 + list(f2))


def two_view_ladders():
    """The pair ladders with camera 1 the identity, one problem per gate of the two-view kernels, candidates the pose and its
    mirror, six ordinary matches behind the rungs: the angle around the two-view min_angle, the float reprojection error
    in camera 1 around max_err, z in camera 1 and z in camera 2 around the distance threshold of the cheirality vote."""
    rungs = [(s, d) for d in LADDER for s in (1.0, -1.0)]
    problems = []
    T = shifted([1.0, 0.0, 0.0])                                                # angle: the point on the bisector of the baseline
    a0 = float(TV_MIN_ANGLE)
    pts = [np.array([0.5, 0.0, 0.5 / np.tan(a0 * (1 + s * d) / 2)]) for s, d in rungs]
    problems.append((*exact_matches(T, pts, 6, 1300), with_mirror(T)))
    T = relative_pose(3)                                                        # error: pixel 1 pushed until the DLT point reprojects at the rung
    X = np.array([0.4, -0.3, 5.0])
    p1, p2 = project(np.eye(4), X), project(T, X)
    direction = np.array([np.cos(0.4), np.sin(0.4)])

    def err1(s):
        return np.linalg.norm(project(np.eye(4), _dlt(np.eye(4), T, p1 + s * direction, p2, K0)) - (p1 + s * direction))

    u1, u2 = [], []
    for sgn, d in rungs:
        target = float(MAX_ERR) * (1 + sgn * d)
        s0, s1 = 2 * target, 2.2 * target
        f0, f1 = err1(s0) - target, err1(s1) - target
        for _ in range(12):
            if f1 == f0:
                break
            s0, s1, f0 = s1, s1 - f1 * (s1 - s0) / (f1 - f0), f1
            f1 = err1(s1) - target
        u1.append(p1 + s1 * direction)
        u2.append(p2)
    f1, f2 = matches(T, 6, 1301)
    problems.append((np.array(u1 + list(f1)), np.array(u2 + list(f2)), with_mirror(T)))
    T = shifted([1.0, 0.0, 10.0])                                               # z in camera 1 around dist, z in camera 2 ten units less
    problems.append((*exact_matches(T, [np.array([2.0, -1.0, DIST * (1 + s * d)]) for s, d in rungs], 6, 1302), with_mirror(T)))
    T = shifted([1.0, 0.0, -10.0])                                              # z in camera 2 around dist, z in camera 1 ten units less
    problems.append((*exact_matches(T, [np.array([2.0, -1.0, DIST * (1 + s * d) - 10.0]) for s, d in rungs], 6, 1303), with_mirror(T)))
    return _twoview(problems, ladder=True, min_solution=5)                        # (16 matches each: a solution above 5 wins)


def two_view_degenerate():
    """The degenerate pairs with camera 1 the identity: a point on the baseline (camera 2 straight ahead: both pixels at the
    principal point, undefined; a pixel off it, defined and badly conditioned), pixel 1 exactly at the principal point, and the
    scene scaled by 1e-3 and 1e3 (the candidate's translation scaled: the same pixels)."""
    problems = []
    T = shifted([0.0, 0.0, 1.0])
    n = 12
    pp = np.tile(K0[2:], (n, 1))
    off = np.array([[0.0, 0.0] if i % 2 == 0 else [0.5 + i, 0.25 * i] for i in range(n)])
    problems.append((pp + 0.3 * off[:, ::-1], pp + off, with_mirror(T)))          # (both pixels off it: rays that do not meet in a centre)
    T = shifted([1.0, 0.5, 0.0])
    pts = [np.array([0.0, 0.0, 2.0 + 1.5 * i]) for i in range(n)]
    problems.append((*exact_matches(T, pts, 0, 1400), with_mirror(T)))
    T = relative_pose(4)
    scaled = []
    for s in (1e-3, 1e3):
        M = T.copy()
        M[:3, 3] *= s
        scaled.append(M.reshape(16))
    problems.append((*matches(T, 16, 1401), np.array(scaled)))
    return _twoview(problems)


TWOVIEW_GROUPS = {"two_view_pairs": two_view_pairs, "two_view_shapes": two_view_shapes, "two_view_ladders": two_view_ladders,
                  "two_view_degenerate": two_view_degenerate}


def groups():
    out = {}
    for table in (PAIR_GROUPS, TRACK_GROUPS, {"reprojection": reprojection}, TWOVIEW_GROUPS):
        for name, make in table.items():
            out[name] = make()
    return out
