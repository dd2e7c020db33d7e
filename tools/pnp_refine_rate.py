"""The PnP polish (eacham_pnp_refine_batch: Levenberg-Marquardt on the inliers, the whole loop in one launch) on two lists of frames.

    python tools/pnp_refine_rate.py [--reps 10] [--out profiles/pnp_refine_rate.txt]

Protocol: one MI355X, one build, one process; every output of the call is checked as bytes against the CPU restatement
(tests/cpp/pnp_refine_reference.c) before anything is timed; times are medians of --reps calls after one untimed call, with
[min .. max]. "end to end" is the host's wall time of the call on arrays already in the wire form (staging, launch, copy back);
"device" is the time of the call's launch by the library's own events (eacham_profile_get).
Jobs:   large   100 frames with 300 .. 2000 inliers each
        small   10 000 frames with 5 .. 64 inliers each
        a frame has its inliers (1 px of noise) and 30 % more rows that are not used (gross outliers, mask byte 0); the start pose
        is the truth turned by 0.02 rad and moved by 0.02; cap of 20 tries, recount asked for.
Context: eacham_pnp_refit_batch (EPnP on the inliers of the same start pose, a workgroup per frame) on the same lists, and the C
restatement of the polish on one host thread. There is no bar: nothing comparable exists before this call."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnp_refine_cases as RC  # noqa: E402
import pnp_refine_reference as R  # noqa: E402
from eacham_amd import HipContext, capi, pnp  # noqa: E402

JOBS = (("large", 100, 300, 2000), ("small", 10000, 5, 64))


def workload(frames, lo, hi, seed):
    rng = np.random.default_rng(seed)
    X, uv, T0, use = [], [], [], []
    for k in range(frames):
        m = int(rng.integers(lo, hi + 1))
        extra = (3 * m + 9) // 10
        x, u, t0, _ = RC.problem(m + extra, seed * 100003 + k, 0.02, noise=1.0)
        mask = np.zeros(m + extra, np.uint8)
        mask[rng.permutation(m + extra)[:m]] = 1
        u[mask == 0] = rng.uniform(0, 800, (extra, 2))
        X.append(x), uv.append(u), T0.append(t0), use.append(mask)
    pp, A, B = pnp.pack_points(X, uv)
    return dict(X=X, uv=uv, use=use, pp=pp, A=A, B=B, T0=np.array(T0), has=np.ones(frames, np.uint8), mask=np.concatenate(use))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    fine = True
    with HipContext(0) as ctx:
        say("PnP polish: eacham_pnp_refine_batch (LM on the inliers, a wave per frame, one launch) beside eacham_pnp_refit_batch (EPnP on the")
        say(f"inliers, a workgroup per frame) and the C restatement on one host thread; one MI355X, one process; ms, median of {args.reps} after one untimed [min .. max]")
        for name, frames, lo, hi in JOBS:
            w = workload(frames, lo, hi, 7 if name == "large" else 8)
            refine = lambda: pnp.pnp_refine_batch_raw(ctx, w["pp"], w["A"], w["B"], RC.K, w["T0"], w["has"], w["mask"], RC.MAX_TRIES, RC.THR)   # noqa: E731
            refit = lambda: pnp.pnp_refit_batch_raw(ctx, w["pp"], w["A"], w["B"], RC.K, w["T0"], w["has"], RC.THR)   # noqa: E731
            t0 = time.perf_counter()
            want = R.refine_batch(w["X"], w["uv"], RC.K, w["T0"], w["has"], w["use"], RC.MAX_TRIES, RC.THR)
            host = (time.perf_counter() - t0) * 1e3
            got = refine()
            same = all(np.array_equal(np.ascontiguousarray(getattr(got, f)).view(np.uint8), np.ascontiguousarray(getattr(want, f)).view(np.uint8))
                       for f in ("refined", "cost", "tries", "status", "n_inliers")) and all(np.array_equal(a, b) for a, b in zip(got.masks, want.masks))
            if not same:
                say(f"{name}: the call DIFFERS from the restatement; nothing timed")
                fine = False
                continue
            e = timed(refine, args.reps)
            f = timed(refit, args.reps)
            de, df = device_ms(ctx, refine), device_ms(ctx, refit)
            used = int(w["mask"].sum())
            say(f"  {name}: {frames} frames, {lo} .. {hi} inliers ({used} used rows of {len(w['mask'])}); tries mean {got.tries.mean():.2f} most {int(got.tries.max())}, "
                f"status counts {np.bincount(got.status, minlength=3).tolist()}, cost {got.cost[:, 0].sum():.4g} -> {got.cost[:, 1].sum():.4g}")
            say(f"      refine  end to end {e[0]:9.3f} [{e[1]:.3f} .. {e[2]:.3f}]   device {de:9.3f}   ({1e3 * de / frames:.2f} us a frame)")
            say(f"      refit   end to end {f[0]:9.3f} [{f[1]:.3f} .. {f[2]:.3f}]   device {df:9.3f}")
            say(f"      restatement on the host {host:9.3f}   ({host / max(de, 1e-9):.1f} x the device time)")
    if args.out:
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")
    return 0 if fine else 1


if __name__ == "__main__":
    sys.exit(main())
