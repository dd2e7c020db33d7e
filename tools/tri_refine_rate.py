"""The track polish (eacham_triangulate_refine_tracks: Levenberg-Marquardt on a track's point over its inlier views, 8 lanes per track,
the whole loop in one launch) on the tracks of the S200 synthetic BA scene.

    python tools/tri_refine_rate.py [--reps 10] [--tracks 50000] [--out profiles/tri_refine_rate.txt]

Protocol: one MI355X, one build, one process; every output of the call is checked as bytes against the CPU restatement
(tests/cpp/tri_refine_reference.c) before anything is timed; times are medians of --reps calls after one untimed call, with
[min .. max]. "end to end" is the host's wall time of the call on arrays already in the wire form (staging, launch, copy back);
"device" is the time of the call's launch by the library's own events (eacham_profile_get).
Input:  the S200 scene (eacham_amd/synth.py: 200 cameras, 50 000 landmarks seen by 10 cameras each, 500 000 observations, 1 px of
        noise, the true cameras); the start points, has_point (status == 3) and the masks are eacham_triangulate_tracks' own outputs
        on the same tracks; cap of 20 tries, recount asked for.
Context: eacham_triangulate_tracks on the same tracks, and the C restatement of the polish on 16 host threads (the list cut into 16
runs of tracks). There is no bar: nothing comparable exists before this call. Also reported: the sum of the costs and the mean
distance to the true points before and after — what the polish is for."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tri_refine_reference as R  # noqa: E402
from eacham_amd import HipContext, capi, synth, triangulate as tri  # noqa: E402

MAX_TRIES, MAX_ERR, MIN_ANGLE, THREADS = 20, 4.0, 0.002, 16


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
    _, ms = ctx.profile_get(capi.KERNEL_TRIANGULATE)
    ctx.profile_enable(False)
    return ms


def restatement(T, tp, of, uv, K, points, has, masks, threads):
    """The C restatement over `threads` runs of tracks at once (ctypes releases the interpreter lock during the call)."""
    n = len(tp) - 1
    cuts = [n * k // threads for k in range(threads + 1)]

    def run(k):
        a, b = cuts[k], cuts[k + 1]
        lo, hi = int(tp[a]), int(tp[b])
        return R.refine_tracks(T, tp[a:b + 1] - tp[a], of[lo:hi], uv[lo:hi], K, points[a:b], has[a:b], masks[lo:hi], MAX_TRIES, MAX_ERR)

    R.lib()
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(run, range(threads)))
    ms = (time.perf_counter() - t0) * 1e3
    cat = lambda f: np.concatenate([getattr(p, f) for p in parts])   # noqa: E731
    return tri.TrackRefine(cat("refined"), cat("cost"), cat("tries"), cat("status"), cat("masks"), cat("n_inliers")), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tracks", type=int, default=50_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    scene = synth.make_scene(n_landmarks=args.tracks)
    g = synth.make_tracks(scene, min_obs=10, max_obs=10, outlier_frac=0.0)
    T, K, of, uv = g["transforms"], g["K"], g["obs_frame"], g["obs_uv"]
    tp32, tp = g["track_ptr"], g["track_ptr"].astype(np.int64)
    truth = scene["points_true"][g["landmark"]]
    n = len(tp) - 1
    fine = True
    with HipContext(0) as ctx:
        say("Track polish: eacham_triangulate_refine_tracks (LM on a track's point over its inlier views, 8 lanes per track, one launch) beside")
        say(f"eacham_triangulate_tracks and the C restatement on {THREADS} host threads; one MI355X, one process; ms, median of {args.reps} after one untimed [min .. max]")
        triangulate = lambda: tri.triangulate_tracks(ctx, T, tp32, of, uv, K, MAX_ERR, MIN_ANGLE)   # noqa: E731
        points, status, masks = triangulate()
        has = (status == tri.STATUS_ADD).astype(np.uint8)
        refine = lambda: tri.refine_tracks_raw(ctx, T, len(T), n, tp, of, uv, K, points, has, masks, MAX_TRIES, MAX_ERR)   # noqa: E731
        want, host = restatement(T, tp, of, uv, K, points, has, masks, THREADS)
        got = refine()
        same = all(np.array_equal(np.ascontiguousarray(getattr(got, f)).view(np.uint8), np.ascontiguousarray(getattr(want, f)).view(np.uint8))
                   for f in ("refined", "cost", "tries", "status", "n_inliers", "masks"))
        if not same:
            say("the call DIFFERS from the restatement; nothing timed")
            fine = False
        else:
            e, f = timed(refine, args.reps), timed(triangulate, args.reps)
            de, df = device_ms(ctx, refine), device_ms(ctx, triangulate)
            live = got.status != tri.REFINE_NOT_REFINED
            d0 = np.linalg.norm(points[live] - truth[live], axis=1).mean()
            d1 = np.linalg.norm(got.refined[live] - truth[live], axis=1).mean()
            say(f"  S200: {n} tracks, {len(of)} observations; {int(has.sum())} tracks added by the triangulation and handed over, {int(masks[np.repeat(has, np.diff(tp)) != 0].sum())} used observations")
            say(f"      status counts {np.bincount(got.status, minlength=3).tolist()} (converged, cap, not refined); tries mean {got.tries[live].mean():.2f} most {int(got.tries.max())}")
            say(f"      sum of costs {got.cost[live, 0].sum():.6g} -> {got.cost[live, 1].sum():.6g} px^2; mean distance to the true point {d0:.5f} -> {d1:.5f}; "
                f"inliers at the point {int(masks[np.repeat(live, np.diff(tp))].sum())} -> {int(got.n_inliers[live].sum())}")
            say(f"      refine       end to end {e[0]:9.3f} [{e[1]:.3f} .. {e[2]:.3f}]   device {de:9.3f}   ({1e3 * n / max(e[0], 1e-9):.4g} tracks/s end to end, {1e3 * n / max(de, 1e-9):.4g} on the device)")
            say(f"      triangulate  end to end {f[0]:9.3f} [{f[1]:.3f} .. {f[2]:.3f}]   device {df:9.3f}")
            say(f"      restatement on {THREADS} host threads {host:9.3f}   ({host / max(de, 1e-9):.1f} x the device time, {host / max(e[0], 1e-9):.1f} x end to end)")
    if args.out:
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")
    return 0 if fine else 1


if __name__ == "__main__":
    sys.exit(main())
