"""Two-view motion and structure of a list of pairs: the per-pair loop beside one eacham_two_view_batch call.

    python tools/two_view_batch_rate.py [--pairs 1,16,256,4096] [--reps 5] [--out profiles/two_view_batch_rate.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/two_view_batch_rate.py --batch-only 256
    python tools/kernel_stats.py <dir> 1

Workload: P pairs of 300 matches (a quarter gross outliers), the four poses of the pair's essential matrix as candidates — the
essential branch of RecoverPoseTwoView, the one with two device turns per pair. Both sides run on the same library in the same
process, on the same points and candidates, and their results are compared before anything is timed.
  loop   what RecoverPose and then TwoViewPoints (include/eacham/TwoViewHip.hpp, TriangulatorHip.hpp) do per pair, through the
         C-ABI: eacham_two_view_points for the four candidates, the cheirality vote on the host, eacham_two_view_points for the
         winner, the kept matches — two blocking calls per pair. The host steps are numpy on preallocated arrays; their cost is
         part of the loop here as the C++ host steps are part of it in the header.
  batch  one eacham_two_view_batch call (the POSES rule): one blocking call whatever P.
Times are medians of --reps repetitions after one untimed, with [min .. max]; the spread is max - min.
Condition: at P = 1 the batch is not slower than the loop by more than the loop's own spread."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eacham_amd import HipContext, capi, synth, twoview  # noqa: E402

N, NT = 300, 4
MAX_ERR, MIN_ANGLE, DIST = 4.0, float(np.deg2rad(1.0)), 50.0
FLT_MAX = float(np.finfo(np.float32).max)
vp = C.c_void_p


def scene(seed):
    """300 matches of two synth cameras (float32-valued pixels as cv::Point2f, 25 % gross outliers), K, and the four candidate
    poses [R1|t], [R2|t], [R1|-t], [R2|-t] of the true essential matrix."""
    sc = synth.make_scene(2, N, 2, seed=seed, pixel_noise=0.7)
    K, X = sc["K"], sc["points_true"]
    rng = np.random.default_rng(seed)
    uv = []
    for T in sc["T_true"][:2]:
        pc = X @ T[:3, :3].T + T[:3, 3]
        uv.append(np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], 1) + 0.5 * rng.normal(size=(N, 2)))
    bad = rng.random(N) < 0.25
    uv[1][bad] += rng.normal(0, 60, size=(int(bad.sum()), 2))
    T21 = sc["T_true"][1] @ np.linalg.inv(sc["T_true"][0])
    t = T21[:3, 3] / np.linalg.norm(T21[:3, 3])
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ T21[:3, :3]
    U, _, Vt = np.linalg.svd(E)
    U, Vt = (U if np.linalg.det(U) > 0 else -U), (Vt if np.linalg.det(Vt) > 0 else -Vt)
    W = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1.0]])
    cands = np.zeros((NT, 4, 4))
    for k, (R, tt) in enumerate(((U @ W @ Vt, U[:, 2]), (U @ W.T @ Vt, U[:, 2]), (U @ W @ Vt, -U[:, 2]), (U @ W.T @ Vt, -U[:, 2]))):
        cands[k] = np.eye(4)
        cands[k, :3, :3], cands[k, :3, 3] = R, tt
    return [u.astype(np.float32).astype(np.float64) for u in uv], np.asarray(K, np.float64), np.ascontiguousarray(cands.reshape(NT, 16))


def workload(P):
    base = [scene(100 + k) for k in range(min(P, 16))]                             # 16 distinct scenes
    uv1 = [base[p % len(base)][0][0] for p in range(P)]
    uv2 = [base[p % len(base)][0][1] for p in range(P)]
    T = [base[p % len(base)][2] for p in range(P)]
    rng = np.random.default_rng(P)
    masks = [(rng.random(N) < 0.8).astype(np.uint8) for _ in range(P)]            # stands for the E mask RecoverPoseTwoView passes on
    return uv1, uv2, T, masks, base[0][1]


def loop(ctx, uv1, uv2, T, masks, K):
    """Pair by pair: RecoverPose's call and vote, TwoViewPoints' call for the winner. Returns the batch's outputs."""
    L = capi.lib()
    P = len(uv1)
    pts4 = np.zeros((NT, N, 3)); keep4 = np.zeros((NT, N), np.uint8); cnt4 = np.zeros(NT, np.int32)
    pts1 = np.zeros((N, 3)); keep1 = np.zeros(N, np.uint8); cnt1 = np.zeros(1, np.int32)
    winner = np.zeros(P, np.int32); good = np.zeros(P, np.int32); kept = np.zeros(P, np.int32); counts = np.zeros((P, NT), np.int32)
    points = np.zeros((P, N, 3)); keep = np.zeros((P, N), np.uint8); pose_mask = np.zeros((P, N), np.uint8)
    pK = vp(K.ctypes.data)
    for p in range(P):
        a, b, Tp = uv1[p], uv2[p], T[p]
        ctx._check(L.eacham_two_view_points(ctx.handle, N, vp(a.ctypes.data), vp(b.ctypes.data), pK, NT, vp(Tp.ctypes.data), C.c_float(FLT_MAX),
                                            C.c_float(0.0), 0, vp(pts4.ctypes.data), vp(keep4.ctypes.data), vp(cnt4.ctypes.data)))
        allowed = masks[p].astype(bool)
        best, best_mask = 0, None
        for k in range(NT):
            X, M = pts4[k], Tp[k]
            with np.errstate(invalid="ignore", over="ignore"):
                z1 = X[:, 2]
                z2 = ((M[8] * X[:, 0] + M[9] * X[:, 1]) + M[10] * X[:, 2]) + M[11]
                ch = allowed & (z1 > 0) & (z1 < DIST) & (z2 > 0) & (z2 < DIST)
            counts[p, k] = int(ch.sum())
            if k == 0 or counts[p, k] > counts[p, best]:
                best, best_mask = k, ch
        Tw = np.ascontiguousarray(Tp[best])
        ctx._check(L.eacham_two_view_points(ctx.handle, N, vp(a.ctypes.data), vp(b.ctypes.data), pK, 1, vp(Tw.ctypes.data), C.c_float(MAX_ERR),
                                            C.c_float(MIN_ANGLE), 0, vp(pts1.ctypes.data), vp(keep1.ctypes.data), vp(cnt1.ctypes.data)))
        winner[p], good[p], kept[p] = best, counts[p, best], cnt1[0]
        points[p], keep[p], pose_mask[p] = pts1, keep1, best_mask
    return winner, good, kept, counts, points, keep, pose_mask


def batch(ctx, packed, K, rule):
    point_ptr, a, b, transform_ptr, T, M = packed
    return twoview.two_view_batch_raw(ctx, point_ptr, a, b, K, rule, transform_ptr, T, M, MAX_ERR, MIN_ANGLE, DIST, 20)


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,16,256,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch-only", type=int, default=0, help="one warm-up and one batch call at this P (the profiler's run)")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    with HipContext(0) as ctx:
        if args.batch_only:
            uv1, uv2, T, masks, K = workload(args.batch_only)
            packed = twoview.pack(uv1, uv2, T, masks)
            for _ in range(2):
                batch(ctx, packed, K, np.zeros(args.batch_only, np.int32))
            return 0
        say(f"Two-view motion and structure over P pairs x {N} matches, {NT} candidate poses per pair (the essential branch); one MI355X")
        say(f"ms per P pairs, median of {args.reps} after one untimed [min .. max]; loop = 2 blocking calls per pair, batch = 1 call in all")
        ok = True
        for P in [int(x) for x in args.pairs.split(",")]:
            uv1, uv2, T, masks, K = workload(P)
            packed = twoview.pack(uv1, uv2, T, masks)
            rule = np.zeros(P, np.int32)
            g = batch(ctx, packed, K, rule)                                        # the two sides agree, byte for byte, before they are timed
            w = loop(ctx, uv1, uv2, T, masks, K)
            same = (np.array_equal(g.winner, w[0]) and np.array_equal(g.good, w[1]) and np.array_equal(g.kept, w[2])
                    and all(np.array_equal(g.cand_counts[p], w[3][p]) and g.points[p].tobytes() == w[4][p].tobytes()
                            and np.array_equal(g.keep[p], w[5][p]) and np.array_equal(g.pose_mask[p], w[6][p]) for p in range(P)))
            if not same:
                say(f"P = {P}: the batch DIFFERS from the loop")
                ok = False
            tl = timed(lambda: loop(ctx, uv1, uv2, T, masks, K), args.reps)
            tb = timed(lambda: batch(ctx, packed, K, rule), args.reps)
            spread = tl[2] - tl[1]
            verdict = ""
            if P == 1:
                fine = tb[0] <= tl[0] + spread
                ok = ok and fine
                verdict = f"   -> batch {'not slower' if fine else 'SLOWER'} than loop + its spread ({tl[0] + spread:.3f} ms)"
            say(f"  P = {P:5d}   loop {tl[0]:10.3f} [{tl[1]:.3f} .. {tl[2]:.3f}] spread {spread:.3f}   batch {tb[0]:9.3f} [{tb[1]:.3f} .. {tb[2]:.3f}]"
                f"   loop / batch {tl[0] / tb[0]:7.1f}   batch {tb[0] * 1e3 / P:9.1f} us per pair{verdict}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
