"""The fundamental-matrix kind beside the essential one: the seven-point solver's rate, and eacham_graph_verify for F against E.

    python tools/fundamental_rate.py [--reps 5] [--out profiles/fundamental_rate.txt]

  solver    eacham_solve_minimal, 1000 minimal samples of a 300-match pair per launch, for FUNDAMENTAL7 (7 points, up to 3 models),
            ESSENTIAL5 (5 points, up to 10) and HOMOGRAPHY4 (4 points, 1): end to end and the device time of the launch.
  verify    eacham_graph_verify on ONE resident graph of 8 pairs x 300 matches (4 frames x 400 keypoints, integer pixels, a fifth of
            every pair's matches wrong), counter-based samples, retain = 1, no mask download: the fundamental kind at its own
            iteration count (300: cv::findFundamentalMat's 1000 / 0.99 with 7-point samples) and at the essential kind's 89, beside
            the essential kind with K at 89.
One build, one process, one context. One untimed call, then --reps timed: median [min .. max] in ms; dev = between the library's HIP
events around the kernels (eacham_profile_enable; the end-to-end figures are taken with profiling off). Nothing is gated on a time."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eacham_amd import HipContext, ResidentGraph, capi, score  # noqa: E402

K4 = np.array([500.0, 500.0, 320.0, 240.0])
N, FRAMES, KP = 300, 4, 400
vp = C.c_void_p


def project(X, f):
    a = 0.05 * f
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Xc = X @ R.T + np.array([-0.3 * f, 0.02 * f, 0.0])
    return np.rint(np.stack([K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2], K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3]], axis=1))


def graph():
    rng = np.random.default_rng(23)
    X = np.stack([rng.uniform(-2.5, 2.5, KP), rng.uniform(-2, 2, KP), rng.uniform(4, 9, KP)], axis=1)
    perm = [rng.permutation(KP) for _ in range(FRAMES)]
    xy = np.zeros((FRAMES, KP, 2))
    for f in range(FRAMES):
        xy[f][perm[f]] = project(X, f)
    pairs = np.array([(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (2, 0), (3, 1)], dtype=np.int32)
    P = len(pairs)
    q, t = np.zeros((P, N), np.uint32), np.zeros((P, N), np.uint32)
    for p, (f1, f2) in enumerate(pairs):
        pts = rng.choice(KP, N, replace=False)
        other = pts.copy()
        other[rng.choice(N, N // 5, replace=False)] = rng.permutation(np.setdiff1d(np.arange(KP), pts))[:N // 5]
        q[p], t[p] = perm[f1][pts], perm[f2][other]
    return dict(pairs=pairs, counts=np.full(P, N, np.int32), offsets=np.arange(P, dtype=np.int64) * N, q=q.ravel(), t=t.ravel(),
                xy=np.ascontiguousarray(xy.reshape(-1, 2)), seeds=np.arange(P, dtype=np.uint64) + 100, perm=perm)


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), min(t), max(t)


def device_ms(ctx, fn, reps):
    ctx.profile_enable(True)
    fn()
    t = []
    for _ in range(reps):
        ctx.profile_reset()
        fn()
        t.append(ctx.profile_get(capi.KERNEL_SCORE)[1])
    ctx.profile_enable(False)
    return float(np.median(t)), min(t), max(t)


def fmt(t):
    return f"{t[0]:8.3f} [{t[1]:.3f} .. {t[2]:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    g = graph()
    with HipContext(0) as ctx:
        say(f"ms per call, median of {args.reps} after one untimed [min .. max]; dev = between HIP events around the kernels; one MI355X")
        # ---- the solvers: 1000 samples of pair 0 per launch
        s0 = slice(0, N)
        uv1 = g["xy"][0 * KP + g["q"][s0].astype(np.int64)]
        uv2 = g["xy"][1 * KP + g["t"][s0].astype(np.int64)]
        rng = np.random.default_rng(1)
        say(f"eacham_solve_minimal, 1000 samples of a {N}-match pair per launch")
        for kind, m in (("fundamental7", 7), ("essential5", 5), ("homography4", 4)):
            idx = np.array([rng.choice(N, m, replace=False) for _ in range(1000)], dtype=np.int32)
            K = K4 if kind == "essential5" else None
            call = lambda: score.solve_minimal(ctx, kind, uv1, uv2, idx, K)   # noqa: E731
            _, counts = call()
            e, d = timed(call, args.reps), device_ms(ctx, call, args.reps)
            say(f"  {kind:13s} end to end {fmt(e)}   dev {fmt(d)}   {d[0] * 1e3 / 1000:7.3f} us per sample on the device, {counts.sum()} models")
        # ---- eacham_graph_verify, F against E on one resident graph
        P = len(g["counts"])
        rg = ResidentGraph(ctx, FRAMES, g["pairs"], g["counts"], g["offsets"], g["q"], g["t"], [KP] * FRAMES)
        rg.set_keypoints(g["xy"])
        out = (np.zeros((P, 9)), np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.int32), np.zeros((P, 3), np.int32),
               np.zeros(P, np.int32), np.zeros(P, np.int32))

        def verify(code, K, its):
            models, med, thr, inl, win, nc, ns = out
            ctx._check(capi.lib().eacham_graph_verify(rg._h, code, None if K is None else vp(K.ctypes.data), capi.SAMPLING_COUNTER, its,
                                                      vp(g["seeds"].ctypes.data), 1, vp(models.ctypes.data), vp(med.ctypes.data), vp(thr.ctypes.data),
                                                      vp(inl.ctypes.data), None, vp(win.ctypes.data), vp(nc.ctypes.data), vp(ns.ctypes.data), None))

        say(f"eacham_graph_verify, {P} pairs x {N} matches, counter-based samples, retain = 1, no mask download")
        for name, code, K, its in (("fundamental", capi.SOLVE_FUNDAMENTAL7, None, 300), ("fundamental", capi.SOLVE_FUNDAMENTAL7, None, 89),
                                   ("essential", capi.SOLVE_ESSENTIAL5, K4, 89)):
            call = lambda: verify(code, K, its)   # noqa: E731
            e, d = timed(call, args.reps), device_ms(ctx, call, args.reps)
            say(f"  {name:12s} {its:4d} samples per pair   end to end {fmt(e)}   dev {fmt(d)}   inliers {out[3].tolist()} candidates {int(out[5].sum())}")
        rg.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
