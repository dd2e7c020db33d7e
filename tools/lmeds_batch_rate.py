"""LMedS two-view estimation of a list of pairs: the per-pair loop beside one eacham_lmeds_batch call.

    python tools/lmeds_batch_rate.py [--pairs 1,16,256,4096] [--reps 5] [--out profiles/lmeds_batch_rate.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/lmeds_batch_rate.py --batch-only 256
    python tools/kernel_stats.py <dir> 1

Workload: P pairs of 300 matches (a quarter gross outliers), 89 five-point samples (essential matrix, with K) and 72 four-point
samples (homography) per pair — the iteration counts LMedS runs in the reference's two calls. Both sides run on the same
library in the same process, on the same points and samples, and their results are compared before anything is timed.
  loop   what twoview_detail::lmeds does per pair and per model, through the C-ABI: eacham_solve_minimal, host compaction,
         eacham_score_hypotheses (medians), first smallest, sigma, eacham_score_hypotheses (the winner's errors) — six
         blocking calls per pair. The host steps between them are numpy on preallocated arrays; their cost is part of the
         loop here as the C++ host steps are part of it in the header.
  batch  one eacham_lmeds_batch call per model: two blocking calls whatever P.
Times are medians of --reps repetitions after one untimed, with [min .. max]; the spread is max - min.
Condition: at P = 1 the batch is not slower than the loop by more than the loop's own spread."""
import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eacham_amd import HipContext, capi, lmeds, synth  # noqa: E402

N, SAMPLES = 300, {"essential": 89, "homography": 72}
M = {"essential": 5, "homography": 4}
SOLVE = {"essential": (capi.SOLVE_ESSENTIAL5, capi.SCORE_ESSENTIAL, 10), "homography": (capi.SOLVE_HOMOGRAPHY4, capi.SCORE_HOMOGRAPHY, 1)}
vp = C.c_void_p


def scene(seed, planar):
    """300 matches of two synth cameras, float32-valued pixels as cv::Point2f, 25 % gross outliers."""
    sc = synth.make_scene(2, N, 2, seed=seed, pixel_noise=0.7)
    K, X = sc["K"], sc["points_true"].copy()
    if planar:
        X[:, 0] = 0.05 * X[:, 1] - 0.03 * X[:, 2]
    rng = np.random.default_rng(seed)
    uv = []
    for T in sc["T_true"][:2]:
        pc = X @ T[:3, :3].T + T[:3, 3]
        uv.append(np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], 1) + 0.5 * rng.normal(size=(N, 2)))
    bad = rng.random(N) < 0.25
    uv[1][bad] += rng.normal(0, 60, size=(int(bad.sum()), 2))
    return [u.astype(np.float32).astype(np.float64) for u in uv], np.asarray(K, np.float64)


def workload(P, kind):
    base = [scene(100 + k, kind == "homography") for k in range(min(P, 16))]       # 16 distinct scenes, every pair its own samples
    rng = np.random.default_rng(P)
    uv1 = [base[p % len(base)][0][0] for p in range(P)]
    uv2 = [base[p % len(base)][0][1] for p in range(P)]
    # (m distinct indices per sample: the m smallest of N random numbers)
    samples = [np.ascontiguousarray(rng.random((SAMPLES[kind], N)).argpartition(M[kind], axis=1)[:, :M[kind]], dtype=np.int32) for _ in range(P)]
    return uv1, uv2, samples, base[0][1]


def loop(ctx, kind, uv1, uv2, samples, K):
    """Pair by pair: the three blocking calls of twoview_detail::lmeds and its host steps. Returns the batch's outputs."""
    L = capi.lib()
    solve_kind, score_kind, maxm = SOLVE[kind]
    m, S = M[kind], SAMPLES[kind]
    K4 = K if kind == "essential" else None
    pK = vp(K4.ctypes.data) if K4 is not None else None
    models = np.zeros((S, maxm, 9)); counts = np.zeros(S, np.int32)
    med = np.zeros(S * maxm, np.float32); inl = np.zeros(S * maxm, np.int32)
    err = np.zeros(N, np.float32); cnt = np.zeros(1, np.int32); m1 = np.zeros(1, np.float32)
    P = len(uv1)
    out_model = np.zeros((P, 9)); out_med = np.full(P, np.nan, np.float32); out_thr = np.zeros(P, np.float32)
    out_inl = np.zeros(P, np.int32); out_mask = np.zeros((P, N), np.uint8)
    for p in range(P):
        a, b, idx = uv1[p], uv2[p], samples[p]
        ctx._check(L.eacham_solve_minimal(ctx.handle, solve_kind, N, vp(a.ctypes.data), vp(b.ctypes.data), pK, S, vp(idx.ctypes.data),
                                          vp(models.ctypes.data), vp(counts.ctypes.data)))
        keep = (np.arange(maxm)[None, :] < counts[:, None]).ravel()
        cand = np.ascontiguousarray(models.reshape(-1, 9)[keep])
        nm = len(cand)
        if nm == 0:
            continue
        ctx._check(L.eacham_score_hypotheses(ctx.handle, score_kind, N, vp(a.ctypes.data), vp(b.ctypes.data), nm, vp(cand.ctypes.data), pK,
                                             C.c_float(0.0), None, vp(inl.ctypes.data), vp(med.ctypes.data)))
        mm = med[:nm]
        if np.isnan(mm).all():
            continue
        best = int(np.nanargmin(mm))                                              # the first of the smallest
        sigma = max(2.5 * 1.4826 * (1.0 + 5.0 / max(N - m, 1)) * math.sqrt(float(mm[best])), 0.001)
        thr = np.float32(sigma * sigma)
        win = np.ascontiguousarray(cand[best])
        ctx._check(L.eacham_score_hypotheses(ctx.handle, score_kind, N, vp(a.ctypes.data), vp(b.ctypes.data), 1, vp(win.ctypes.data), pK,
                                             C.c_float(float(thr)), vp(err.ctypes.data), vp(cnt.ctypes.data), vp(m1.ctypes.data)))
        out_model[p], out_med[p], out_thr[p], out_inl[p] = win, mm[best], thr, cnt[0]
        out_mask[p] = err <= thr
    return out_model, out_med, out_thr, out_inl, out_mask


def batch(ctx, kind, packed, K):
    return lmeds.lmeds_batch_raw(ctx, kind, *packed, K if kind == "essential" else None)


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
    ap.add_argument("--batch-only", type=int, default=0, help="one warm-up and one batch call per model at this P (the profiler's run)")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    with HipContext(0) as ctx:
        if args.batch_only:
            for kind in ("essential", "homography"):
                uv1, uv2, samples, K = workload(args.batch_only, kind)
                packed = lmeds.pack(kind, uv1, uv2, samples)
                for _ in range(2):
                    batch(ctx, kind, packed, K)
            return 0
        say(f"LMedS over P pairs x {N} matches, {SAMPLES['essential']} five-point (E, with K) + {SAMPLES['homography']} four-point (H) samples per pair; one MI355X")
        say(f"ms per P pairs, median of {args.reps} after one untimed [min .. max]; loop = 6 blocking calls per pair, batch = 2 calls in all")
        ok = True
        for P in [int(x) for x in args.pairs.split(",")]:
            work = {kind: workload(P, kind) for kind in ("essential", "homography")}
            packed = {kind: lmeds.pack(kind, *work[kind][:3]) for kind in work}
            for kind, (uv1, uv2, samples, K) in work.items():                     # the two sides agree, bit for bit, before they are timed
                g = batch(ctx, kind, packed[kind], K)
                w = loop(ctx, kind, uv1, uv2, samples, K)
                same = (np.array_equal(g.models.view(np.uint64), w[0].view(np.uint64)) and np.array_equal(g.medians.view(np.uint32), w[1].view(np.uint32))
                        and np.array_equal(g.thresholds.view(np.uint32), w[2].view(np.uint32)) and np.array_equal(g.inliers, w[3])
                        and all(np.array_equal(g.masks[p], w[4][p]) for p in range(P)))
                if not same:
                    say(f"P = {P} {kind}: the batch DIFFERS from the loop")
                    ok = False
            tl = timed(lambda: [loop(ctx, kind, *work[kind]) for kind in work], args.reps)
            tb = timed(lambda: [batch(ctx, kind, packed[kind], work[kind][3]) for kind in work], args.reps)
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
