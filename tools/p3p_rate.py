"""PnP RANSAC on four-point samples (P3P) beside the five-point EPnP form: one round, and the whole loop.

    python tools/p3p_rate.py [--problems 1,16,256] [--reps 5] [--out profiles/p3p_rate.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/p3p_rate.py --round-only p3p  --at 256
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/p3p_rate.py --round-only epnp --at 256
    python tools/kernel_stats.py <dir> 1

Protocol: one MI355X, one build, one process; the P3P outputs are checked (the round against eacham_solve_p3p + the scorer, on the
first problems) before anything is timed; times are medians of --reps repetitions after one untimed call, with [min .. max].
Workload: the inputs of tools/pnp_batch_rate.py — P problems x 600 correspondences, ~30 % gross outliers, 0.8 px noise.
  round   ONE RANSAC round of 256 samples per problem on arrays already in the wire form: eacham_pnp_hypotheses_batch_p3p (m = 4, one
          launch) against eacham_pnp_hypotheses_batch (m = 5: front, back x 3, count — the parent's kernels, so it is the baseline).
          "device" is the time of the call's launches by the library's own events (eacham_profile_get).
  loop    pnp_ransac_batch(solver="p3p") against pnp_ransac_batch(solver="epnp"), 10 000 iterations asked, 4 px, confidence 0.999:
          rounds (device turns - 1), samples consumed, inliers, and the refitted pose's max-abs distance from the true pose.
Expectation: at P = 256 a P3P round is not slower than the EPnP round plus the EPnP round's own min .. max spread."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pnp_batch_rate as B  # noqa: E402
from eacham_amd import HipContext, capi, pnp, score, synth  # noqa: E402

N, ITERS, ERR, CONF = B.N, B.ITERS, B.ERR, B.CONF
THR = float(np.float32(ERR) * np.float32(ERR))


def workload(P, m):
    """B.workload's points with m-point streams, in lists and in the wire form of one round; T = the true poses."""
    X, uv, _, K = B.workload(P)
    nb = min(P, 16)
    truth = [synth.make_scene(3, N, 3, seed=200 + k)["T_true"][1] for k in range(nb)]
    T = [np.concatenate([truth[p % nb][:3, :3].reshape(-1), truth[p % nb][:3, 3]]) for p in range(P)]
    rng = np.random.default_rng(1000 + P)
    samples = [np.ascontiguousarray(rng.random((B.STREAM, N)).argpartition(m, axis=1)[:, :m], dtype=np.int32) for _ in range(P)]
    pp, A, Bv = pnp.pack_points(X, uv)
    rows = [s[:pnp.CHUNK] for s in samples]
    wire = dict(point_ptr=pp, X=A, uv=Bv, sample_ptr=pnp._ptr([len(r) for r in rows]), sample_idx=np.ascontiguousarray(np.concatenate(rows)))
    return dict(X=X, uv=uv, K=K, T=T, samples=samples, wire=wire)


def round_p3p(ctx, w):
    q = w["wire"]
    return pnp.pnp_hypotheses_batch_p3p_raw(ctx, q["point_ptr"], q["X"], q["uv"], w["K"], q["sample_ptr"], q["sample_idx"], THR)


def round_epnp(ctx, w):
    q = w["wire"]
    return pnp.pnp_hypotheses_batch_raw(ctx, q["point_ptr"], q["X"], q["uv"], w["K"], q["sample_ptr"], 5, q["sample_idx"], THR)


def check_round(ctx, w, upto=4):
    """The round's outputs against eacham_solve_p3p + eacham_score_hypotheses on the first problems, as bytes."""
    got = round_p3p(ctx, w)
    for p in range(min(upto, len(w["X"]))):
        rows = w["samples"][p][:pnp.CHUNK]
        models, ok = pnp.solve_p3p(ctx, w["X"][p], w["uv"][p], w["K"], rows, want_candidates=False)
        cnt = score.score_hypotheses(ctx, "pnp", w["X"][p], w["uv"][p], models, w["K"], THR)[1]
        if not (np.array_equal(got.models[p].view(np.uint64), models.view(np.uint64)) and np.array_equal(got.n_models[p], ok)
                and np.array_equal(got.inlier_counts[p], np.where(ok != 0, cnt, 0))):
            return False
    return True


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), min(t), max(t)


def device_ms(ctx, fn):
    ctx.profile_enable(True)
    ctx.profile_reset()
    fn()
    _, ms = ctx.profile_get(capi.KERNEL_SCORE)
    ctx.profile_enable(False)
    return ms


def summary(res, T):
    ok = [r for r in res if r["ok"]]
    err = [float(np.abs(r["pose"] - t).max()) for r, t in zip(res, T) if r["ok"]]
    return (f"ok {len(ok)}/{len(res)}, samples consumed {sum(r['iterations'] for r in res)}, inliers mean {np.mean([len(r['inliers']) for r in ok]):.1f}, "
            f"pose error median {np.median(err):.2e} max {np.max(err):.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="1,16,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--round-only", choices=["p3p", "epnp"], default=None, help="one warm-up and one round of this form (the profiler's run)")
    ap.add_argument("--at", type=int, default=256)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    with HipContext(0) as ctx:
        if args.round_only:
            w = workload(args.at, 4 if args.round_only == "p3p" else 5)
            for _ in range(2):
                (round_p3p if args.round_only == "p3p" else round_epnp)(ctx, w)
            return 0
        say(f"PnP RANSAC, P problems x {N} correspondences, ~30 % outliers; P3P (4-point samples) beside EPnP (5-point samples); one MI355X, one process")
        say(f"ms, median of {args.reps} after one untimed [min .. max]; round = {pnp.CHUNK} samples per problem, arrays in the wire form")
        fine = True
        for P in [int(x) for x in args.problems.split(",")]:
            w4, w5 = workload(P, 4), workload(P, 5)
            if not check_round(ctx, w4):
                say(f"P = {P}: the P3P round DIFFERS from eacham_solve_p3p + the scorer; nothing timed")
                return 1
            t5 = timed(lambda: round_epnp(ctx, w5), args.reps)
            t4 = timed(lambda: round_p3p(ctx, w4), args.reps)
            d5, d4 = device_ms(ctx, lambda: round_epnp(ctx, w5)), device_ms(ctx, lambda: round_p3p(ctx, w4))
            spread = t5[2] - t5[1]
            verdict = ""
            if P == 256:
                good = t4[0] <= t5[0] + spread
                fine = fine and good
                verdict = f"   -> P3P round {'not slower' if good else 'SLOWER'} than the EPnP round + its spread ({t5[0] + spread:.3f} ms)"
            say(f"  round P = {P:4d}   epnp {t5[0]:8.3f} [{t5[1]:.3f} .. {t5[2]:.3f}] spread {spread:.3f} device {d5:7.3f}   "
                f"p3p {t4[0]:8.3f} [{t4[1]:.3f} .. {t4[2]:.3f}] device {d4:7.3f}   epnp / p3p {t5[0] / t4[0]:5.2f} (device {d5 / max(d4, 1e-9):5.2f}){verdict}")
            r5, turns5 = pnp.pnp_ransac_batch(ctx, w5["X"], w5["uv"], w5["K"], w5["samples"], ITERS, ERR, CONF)
            r4, turns4 = pnp.pnp_ransac_batch(ctx, w4["X"], w4["uv"], w4["K"], w4["samples"], ITERS, ERR, CONF, solver="p3p")
            e5 = timed(lambda: pnp.pnp_ransac_batch(ctx, w5["X"], w5["uv"], w5["K"], w5["samples"], ITERS, ERR, CONF), args.reps)
            e4 = timed(lambda: pnp.pnp_ransac_batch(ctx, w4["X"], w4["uv"], w4["K"], w4["samples"], ITERS, ERR, CONF, solver="p3p"), args.reps)
            say(f"  loop  P = {P:4d}   epnp {e5[0]:8.3f} [{e5[1]:.3f} .. {e5[2]:.3f}] rounds {turns5 - 1}: {summary(r5, w5['T'])}")
            say(f"                    p3p  {e4[0]:8.3f} [{e4[1]:.3f} .. {e4[2]:.3f}] rounds {turns4 - 1}: {summary(r4, w4['T'])}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if fine else 1


if __name__ == "__main__":
    sys.exit(main())
