"""PnP RANSAC registration of a list of frames: the per-problem loop beside the batched rounds.

    python tools/pnp_batch_rate.py [--problems 1,16,256] [--reps 5] [--out profiles/pnp_batch_rate.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/pnp_batch_rate.py --batch-only 256
    python tools/kernel_stats.py <dir> 1

Workload: P problems of 600 correspondences with ~30 % gross outliers, up to 10 000 iterations at 4 px and confidence 0.999 —
what RecoverPosePnP asks of cv::solvePnPRansac. Every problem has its own seeded sample stream; both sides run on the same
library in the same process, on the same points and streams, and their results are compared before anything is timed.
  loop   what SolvePnPRansac does per problem through the C-ABI: per chunk of 256 samples eacham_solve_pnp and
         eacham_score_hypotheses, the sequential rule, then eacham_score_hypotheses (the winner's errors), the host compaction and
         eacham_solve_pnp on the inliers — at least four blocking calls per problem. The host steps are numpy / Python here as
         they are C++ in the header.
  batch  eacham_amd.pnp.pnp_ransac_batch: one eacham_pnp_hypotheses_batch call per round and one eacham_pnp_refit_batch call,
         rounds + 1 blocking calls whatever P. "calls" is the share of the batch's time spent inside the two wrappers (the
         list concatenated into the wire form, staging, copies, kernels, synchronisation); the rest is the replay of the rule.
Times are medians of --reps repetitions after one untimed, with [min .. max]; the spread is max - min.
Condition: at P = 1 the batch is not slower than the loop by more than the loop's own spread."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eacham_amd import HipContext, capi, pnp, synth  # noqa: E402

N, M, ITERS, ERR, CONF = 600, 5, 10000, 4.0, 0.999
STREAM = 4 * pnp.CHUNK     # rows drawn per problem: the budget after the first good sample is a few dozen at 30 % outliers
vp = C.c_void_p


def scene(seed):
    sc = synth.make_scene(3, N, 3, seed=seed)
    K, T, X = sc["K"], sc["T_true"][1], sc["points_true"]
    rng = np.random.default_rng(seed)
    pc = X @ T[:3, :3].T + T[:3, 3]
    uv = np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], 1) + 0.8 * rng.normal(size=(N, 2))
    bad = rng.random(N) < 0.3
    uv[bad] += rng.normal(0, 80, size=(int(bad.sum()), 2))
    return np.ascontiguousarray(X), uv.astype(np.float32).astype(np.float64), np.asarray(K, np.float64)


def workload(P):
    base = [scene(200 + k) for k in range(min(P, 16))]          # 16 distinct scenes, every problem its own stream
    rng = np.random.default_rng(P)
    X = [base[p % len(base)][0] for p in range(P)]
    uv = [base[p % len(base)][1] for p in range(P)]
    samples = [np.ascontiguousarray(rng.random((STREAM, N)).argpartition(M, axis=1)[:, :M], dtype=np.int32) for _ in range(P)]
    return X, uv, samples, base[0][2]


def loop(ctx, X, uv, samples, K):
    L = capi.lib()
    thr = float(np.float32(ERR) * np.float32(ERR))
    models = np.zeros((pnp.CHUNK, 12)); okv = np.zeros(pnp.CHUNK, np.int32); inl = np.zeros(pnp.CHUNK, np.int32)
    err = np.zeros(N, np.float32); cnt = np.zeros(1, np.int32); refit = np.zeros(12); rok = np.zeros(1, np.int32)
    out = []
    for x, u, rows in zip(X, uv, samples):
        budget, best, first, done, model = ITERS, -1, 0, 0, np.zeros(12)
        while first < budget:
            idx = rows[first:first + pnp.CHUNK]
            c = len(idx)
            ctx._check(L.eacham_solve_pnp(ctx.handle, N, vp(x.ctypes.data), vp(u.ctypes.data), vp(K.ctypes.data), M, c, vp(idx.ctypes.data),
                                          vp(models.ctypes.data), vp(okv.ctypes.data)))
            ctx._check(L.eacham_score_hypotheses(ctx.handle, capi.SCORE_PNP, N, vp(x.ctypes.data), vp(u.ctypes.data), c, vp(models.ctypes.data),
                                                 vp(K.ctypes.data), C.c_float(thr), None, vp(inl.ctypes.data), None))
            for k in range(c):
                if first + k >= budget:
                    break
                done = first + k + 1
                if okv[k] and inl[k] > max(best, M - 1):
                    best, model = int(inl[k]), models[k].copy()
                    budget = pnp.ransac_update_num_iters(CONF, (N - best) / N, M, budget)
            first += pnp.CHUNK
        rec = {"ok": False, "iterations": done}
        if best >= M:
            ctx._check(L.eacham_score_hypotheses(ctx.handle, capi.SCORE_PNP, N, vp(x.ctypes.data), vp(u.ctypes.data), 1, vp(model.ctypes.data),
                                                 vp(K.ctypes.data), C.c_float(thr), vp(err.ctypes.data), vp(cnt.ctypes.data), None))
            inliers = np.nonzero(err <= np.float32(thr))[0].astype(np.int32)
            ctx._check(L.eacham_solve_pnp(ctx.handle, N, vp(x.ctypes.data), vp(u.ctypes.data), vp(K.ctypes.data), len(inliers), 1,
                                          vp(inliers.ctypes.data), vp(refit.ctypes.data), vp(rok.ctypes.data)))
            rec.update(ok=True, inliers=inliers, pose=refit.copy() if rok[0] else model)
        out.append(rec)
    return out


def batch(ctx, X, uv, samples, K, clock=None):
    hyp, ref = None, None
    if clock is not None:
        def hyp(*a):
            t0 = time.perf_counter()
            r = pnp.pnp_hypotheses_batch(ctx, *a)
            clock[0] += time.perf_counter() - t0
            return r

        def ref(*a):
            t0 = time.perf_counter()
            r = pnp.pnp_refit_batch(ctx, *a)
            clock[0] += time.perf_counter() - t0
            return r
    return pnp.pnp_ransac_batch(ctx, X, uv, K, samples, ITERS, ERR, CONF, hypotheses=hyp, refit=ref)


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
    ap.add_argument("--problems", default="1,16,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch-only", type=int, default=0, help="one warm-up and one batched run at this P (the profiler's run)")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    with HipContext(0) as ctx:
        if args.batch_only:
            w = workload(args.batch_only)
            for _ in range(2):
                batch(ctx, *w)
            return 0
        say(f"PnP RANSAC over P problems x {N} correspondences, ~30 % outliers, {ITERS} iterations asked, 4 px, confidence {CONF}; one MI355X")
        say(f"ms per P problems, median of {args.reps} after one untimed [min .. max]; loop = 2 blocking calls per chunk + 2 per problem, batch = rounds + 1 in all")
        ok = True
        for P in [int(x) for x in args.problems.split(",")]:
            X, uv, samples, K = workload(P)
            got, turns = batch(ctx, X, uv, samples, K)
            want = loop(ctx, X, uv, samples, K)
            for p in range(P):                                                     # the two sides agree, bit for bit, before they are timed
                g, w = got[p], want[p]
                same = g["ok"] == w["ok"] and g["iterations"] == w["iterations"] and (not w["ok"] or (
                    np.array_equal(g["inliers"], w["inliers"]) and np.array_equal(g["pose"].view(np.uint64), w["pose"].view(np.uint64))))
                if not same:
                    say(f"P = {P} problem {p}: the batch DIFFERS from the loop")
                    ok = False
                    break
            tl = timed(lambda: loop(ctx, X, uv, samples, K), args.reps)
            tb = timed(lambda: batch(ctx, X, uv, samples, K), args.reps)
            clock = [0.0]
            batch(ctx, X, uv, samples, K, clock)
            spread = tl[2] - tl[1]
            verdict = ""
            if P == 1:
                fine = tb[0] <= tl[0] + spread
                ok = ok and fine
                verdict = f"   -> batch {'not slower' if fine else 'SLOWER'} than loop + its spread ({tl[0] + spread:.3f} ms)"
            say(f"  P = {P:4d}   loop {tl[0]:9.3f} [{tl[1]:.3f} .. {tl[2]:.3f}] spread {spread:.3f}   batch {tb[0]:8.3f} [{tb[1]:.3f} .. {tb[2]:.3f}]"
                f"   of which calls {clock[0] * 1e3:8.3f} ({turns} turns)   loop / batch {tl[0] / tb[0]:6.1f}   batch {tb[0] * 1e3 / P:8.1f} us per problem{verdict}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
