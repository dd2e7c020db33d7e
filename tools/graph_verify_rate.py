"""Geometric verification of a whole match graph: the host composition beside one eacham_graph_verify call on the resident graph.

    python tools/graph_verify_rate.py [--pairs 1,256,4096] [--reps 5] [--out profiles/graph_verify_rate.txt]

Workload: P pairs x 300 matches over 16 frames of 400 keypoints (a scene in integer pixels, a fifth of every pair's matches wrong),
essential kind with K, 89 five-point samples per pair, under both sample streams. Both forms run on one build, in one process, on
one context, and their outputs are compared as bytes before anything is timed.
  host      what a caller of eacham_lmeds_batch does: the C++ walk over the matches, gather and twoview_detail::lmeds_samples per pair
            (tools/graph_verify_host.cpp, compiled here with g++ -O2), then eacham_lmeds_batch — 32 bytes per match and the sample lists
            go up, the results and a mask byte per match come back. Its kernels are the lb_* kernels.
  resident  eacham_graph_verify with retain = 1 and no mask download: the gather, the draws and the same lb_* kernels on the device,
            only the per-pair results come back.
Per form: end to end, and the device time between HIP events around its kernels (eacham_profile_enable; the events add nothing to
the end-to-end figures, which are taken with profiling off). One untimed call, then --reps timed: median [min .. max].
Condition: at P = 256 the resident call is not slower end to end than the host composition by more than that composition's own
min .. max spread. P = 1 and P = 4096 are recorded as they fall."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eacham_amd import HipContext, ResidentGraph, capi, lmeds  # noqa: E402

N, FRAMES, KP, ITERATIONS, M = 300, 16, 400, 89, 5
K4 = np.array([500.0, 500.0, 320.0, 240.0])
vp = C.c_void_p


def graph(P):
    rng = np.random.default_rng(1000 + P)
    X = np.stack([rng.uniform(-2.5, 2.5, KP), rng.uniform(-2, 2, KP), rng.uniform(4, 9, KP)], axis=1)
    perm = [rng.permutation(KP) for _ in range(FRAMES)]
    xy = np.zeros((FRAMES, KP, 2))
    for f in range(FRAMES):
        a = 0.02 * f
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Xc = X @ R.T + np.array([-0.1 * f, 0.01 * f, 0.0])
        xy[f][perm[f]] = np.rint(np.stack([K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2], K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3]], axis=1))
    combos = [(i, j) for i in range(FRAMES) for j in range(i + 1, FRAMES)]
    pairs = np.array([combos[p % len(combos)] for p in range(P)], dtype=np.int32)
    q, t = np.zeros((P, N), np.uint32), np.zeros((P, N), np.uint32)
    for p, (f1, f2) in enumerate(pairs):
        pts = rng.choice(KP, N, replace=False)
        other = pts.copy()
        other[rng.choice(N, N // 5, replace=False)] = rng.permutation(np.setdiff1d(np.arange(KP), pts))[:N // 5]
        q[p], t[p] = perm[f1][pts], perm[f2][other]
    kpo = np.arange(FRAMES + 1, dtype=np.int64) * KP
    return dict(pairs=pairs, counts=np.full(P, N, np.int32), offsets=np.arange(P, dtype=np.int64) * N, q=q.ravel(), t=t.ravel(), kpo=kpo,
                xy=np.ascontiguousarray(xy.reshape(-1, 2)), seeds=np.arange(P, dtype=np.uint64) + 100)


def host_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="gv_rate_"), "libgv_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "graph_verify_host.cpp"),
                    "-o", out], check=True)
    L = C.CDLL(out)
    L.gv_host_pack.restype = C.c_longlong
    L.gv_host_pack.argtypes = [C.c_int] + [vp] * 7 + [C.c_int] * 4 + [vp] * 6
    return L


def host(ctx, H, g, sampling):
    """gather + draw + pack in C++, then eacham_lmeds_batch: returns its LmedsBatch."""
    P = len(g["counts"])
    total = int(g["counts"].sum())
    pp, sp = np.zeros(P + 1, np.int64), np.zeros(P + 1, np.int64)
    a, b = np.empty((total, 2)), np.empty((total, 2))
    idx = np.empty((P * ITERATIONS, M), np.int32)
    ns = H.gv_host_pack(P, vp(g["pairs"].ctypes.data), vp(g["counts"].ctypes.data), vp(g["offsets"].ctypes.data), vp(g["q"].ctypes.data),
                        vp(g["t"].ctypes.data), vp(g["kpo"].ctypes.data), vp(g["xy"].ctypes.data), M, 0, sampling, ITERATIONS,
                        vp(g["seeds"].ctypes.data), vp(pp.ctypes.data), vp(a.ctypes.data), vp(b.ctypes.data), vp(sp.ctypes.data), vp(idx.ctypes.data))
    return lmeds.lmeds_batch_raw(ctx, "essential", pp, a, b, sp, idx[:ns], K4)


def resident_call(rg, g, sampling, out):
    """eacham_graph_verify, retain = 1, the per-pair results only (no mask, no samples)."""
    models, med, thr, inl, win, nc, ns = out
    rg.ctx._check(capi.lib().eacham_graph_verify(rg._h, capi.SOLVE_ESSENTIAL5, vp(K4.ctypes.data), sampling, ITERATIONS, vp(g["seeds"].ctypes.data), 1,
                                                 vp(models.ctypes.data), vp(med.ctypes.data), vp(thr.ctypes.data), vp(inl.ctypes.data), None,
                                                 vp(win.ctypes.data), vp(nc.ctypes.data), vp(ns.ctypes.data), None))


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), min(t), max(t)


def device_ms(ctx, fn, reps):
    """Median device time of fn's kernels between the library's HIP events (the scorer's stage holds every kernel of both forms)."""
    ctx.profile_enable(True)
    fn()
    t = []
    for _ in range(reps):
        ctx.profile_reset()
        fn()
        t.append(ctx.profile_get(capi.KERNEL_SCORE)[1])
    ctx.profile_enable(False)
    return float(np.median(t)), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,256,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    H = host_lib()
    ok = True
    with HipContext(0) as ctx:
        say(f"verifying P pairs x {N} matches ({FRAMES} frames x {KP} keypoints), essential kind with K, {ITERATIONS} samples per pair; one MI355X")
        say(f"ms per call, median of {args.reps} after one untimed [min .. max]; host = C++ gather + draws + eacham_lmeds_batch (mask downloaded), "
            "resident = eacham_graph_verify (retain = 1, no mask download); dev = between HIP events around the kernels")
        for P in [int(x) for x in args.pairs.split(",")]:
            g = graph(P)
            rg = ResidentGraph(ctx, FRAMES, g["pairs"], g["counts"], g["offsets"], g["q"], g["t"], [KP] * FRAMES)
            rg.set_keypoints(g["xy"])
            out = (np.zeros((P, 9)), np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.int32), np.zeros((P, 3), np.int32),
                   np.zeros(P, np.int32), np.zeros(P, np.int32))
            for name, sampling in (("opencv", capi.SAMPLING_OPENCV), ("counter", capi.SAMPLING_COUNTER)):
                w = host(ctx, H, g, sampling)                                       # the two forms agree, byte for byte, before they are timed
                r = rg.verify("essential", K4, name, ITERATIONS, g["seeds"], retain=True)
                same = (r.models.tobytes() == w.models.tobytes() and r.medians.tobytes() == w.medians.tobytes() and r.thresholds.tobytes() == w.thresholds.tobytes()
                        and np.array_equal(r.inliers, w.inliers) and np.array_equal(r.winner, w.winner) and np.array_equal(r.n_candidates, w.n_candidates)
                        and r.masks.tobytes() == np.concatenate(w.masks).tobytes())
                if not same:
                    say(f"P = {P} {name}: the resident call DIFFERS from the host composition")
                    ok = False
                th = timed(lambda: host(ctx, H, g, sampling), args.reps)
                tr = timed(lambda: resident_call(rg, g, sampling, out), args.reps)
                dh = device_ms(ctx, lambda: host(ctx, H, g, sampling), args.reps)
                dr = device_ms(ctx, lambda: resident_call(rg, g, sampling, out), args.reps)
                spread = th[2] - th[1]
                verdict = ""
                if P == 256:
                    fine = tr[0] <= th[0] + spread
                    ok = ok and fine
                    verdict = f"   -> resident {'not slower' if fine else 'SLOWER'} than host + its spread ({th[0] + spread:.3f} ms)"
                say(f"  P = {P:5d} {name:8s} host {th[0]:9.3f} [{th[1]:.3f} .. {th[2]:.3f}] dev {dh[0]:8.3f} [{dh[1]:.3f} .. {dh[2]:.3f}]   "
                    f"resident {tr[0]:9.3f} [{tr[1]:.3f} .. {tr[2]:.3f}] dev {dr[0]:8.3f} [{dr[1]:.3f} .. {dr[2]:.3f}]   host / resident {th[0] / tr[0]:5.2f}{verdict}")
            rg.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
