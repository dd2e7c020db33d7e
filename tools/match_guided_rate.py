"""Rate of guided matching (eacham_match_guided, eacham_amd/csrc/match_guided.hip) beside the blind matcher on the same pairs.

  python tools/match_guided_rate.py [--pairs 200] [--rows 2000] [--reps 20] [--out profiles/match_guided_rate.txt]

The job: `pairs` pairs (the first of all pairs of 21 frames) of `rows` x `rows` keypoints, random integer descriptors at 128-D and
256-D, random integer pixels in 640 x 480; every pair under the same model — the F of cameras 0 and 3 of tests/guided_cases.py, or
the H of the plane 0.1 x + z = 6 between them — with max_error 4 (squared pixels) and +inf (no gate: every element is admitted and
goes through the top-2), cross-check on. The F kind at max_error 4 runs twice: with the division-free screen in front of the exact
gate (the default) and with EACHAM_GUIDED_SCREEN=0 on a second context; the two must return the same bytes. Per configuration one untimed call, then `reps` timed ones:
  kernel   the device time of the sweep, tail, scan and compaction (HIP events of the C-ABI's EACHAM_KERNEL_MATCH_GUIDED slot)
  wall     the host-pointer call end to end (it ends in a synchronise)
as pairs/s, median [min .. max]. The yardstick is eacham_match_all_pairs (stats form, thresholds off) on the same pairs in the same
process, its kernel time the EACHAM_KERNEL_MATCH_TILE + _FINALIZE slots; the ratio guided / blind is by kernel time and by wall.
The share of elements admitted is counted on the CPU for pair 0 with the reference's gate (tests/guided_reference.py).
No rate is a pass condition. Prints one JSON line; --out also writes the text report."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=200)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import guided_cases as GCS
    import guided_reference as GR
    from eacham_amd import HipContext, capi, synth
    from eacham_amd import guided as G

    n_frames = 21
    pairs = np.ascontiguousarray(synth.all_pairs(n_frames)[:a.pairs], dtype=np.int32)
    P = len(pairs)
    rng = np.random.default_rng(1)
    xys = [GCS.random_pixels(rng, a.rows) for _ in range(n_frames)]
    kpo, xy = G.pack_keypoints(xys)
    models = {"fundamental": GCS.true_F(0, 3), "homography": GCS.plane_H(0, 3, np.array([0.1, 0.0, 1.0]), 6.0)}
    share = {k: float(GR.admissible(k, xys[pairs[0][0]], xys[pairs[0][1]], m, None, 4).mean()) for k, m in models.items()}
    ms = lambda xs: f"{1e3 * float(np.median(xs)):9.3f} [{1e3 * min(xs):.3f} .. {1e3 * max(xs):.3f}] ms"          # noqa: E731
    rate = lambda xs: f"{P / float(np.median(xs)):9.0f} [{P / max(xs):.0f} .. {P / min(xs):.0f}] pairs/s"          # noqa: E731
    lines = [f"{P} pairs of {a.rows} x {a.rows} keypoints; one untimed call, then {a.reps} timed; median [min .. max]",
             f"share of elements admitted at max_error 4 (pair 0, CPU reference): F {share['fundamental']:.4%}, H {share['homography']:.4%}"]
    out = {"pairs": P, "rows": a.rows, "share_admitted": share}
    # the division-free screen in front of the exact gate (F and E kinds) on, then off: EACHAM_GUIDED_SCREEN is read at eacham_ctx_create
    ctxs = {}
    for screen in ("on", "off"):
        os.environ["EACHAM_GUIDED_SCREEN"] = "1" if screen == "on" else "0"
        ctxs[screen] = HipContext(0)
    os.environ.pop("EACHAM_GUIDED_SCREEN")
    ctx = ctxs["on"]
    try:
        for dim in (128, 256):
            descs = [GCS.random_desc(rng, a.rows, dim) for _ in range(n_frames)]
            for c in ctxs.values():
                c.clear_descriptors()
                for f in range(n_frames):
                    c.upload_descriptors(f, descs[f])
                c.sync()
                c.profile_enable(True)

            def timed(call, slots, on):
                call()
                wall, dev = [], []
                for _ in range(a.reps):
                    on.profile_reset()
                    t0 = time.perf_counter()
                    res = call()
                    wall.append(time.perf_counter() - t0)
                    dev.append(sum(on.profile_get(s)[1] for s in slots) * 1e-3)
                return wall, dev, res

            bw, bd, _ = timed(lambda: ctx.match_all_pairs(pairs, 0.8, 0, -1, cap=P * a.rows, stats=True), (capi.KERNEL_MATCH_TILE, capi.KERNEL_MATCH_FINALIZE), ctx)
            lines += [f"{dim}-D", f"  blind eacham_match_all_pairs (stats form)  kernel {ms(bd)} {rate(bd)}", f"  {'':42s} wall   {ms(bw)} {rate(bw)}"]
            out[f"blind_{dim}"] = {"kernel_pairs_per_s": P / float(np.median(bd)), "wall_pairs_per_s": P / float(np.median(bw))}
            for kind, M in models.items():
                mm = np.tile(M, (P, 1))
                digest_on = None
                for max_error, screen in ((4.0, "on"), (4.0, "off"), (float("inf"), "on")):
                    if screen == "off" and kind == "homography":
                        continue   # (the homography's error has no division: no screen)
                    cx = ctxs[screen]
                    call = lambda: G.guided_raw(cx, G.KINDS[kind], mm, None, max_error, 0.8, 0, 1, P, P * a.rows, pairs=pairs, kpo=kpo, xy=xy)   # noqa: E731
                    w, d, res = timed(call, (capi.KERNEL_MATCH_GUIDED,), cx)
                    if res[0] != capi.OK:
                        sys.exit(f"eacham_match_guided failed: {res[0]}")
                    digest = b"".join(x.tobytes() for x in res[2])
                    if screen == "on" and max_error == 4.0:
                        digest_on = digest
                    elif screen == "off" and digest != digest_on:
                        sys.exit("the screen changed the result")
                    label = f"guided {kind[0].upper()} max_error {max_error:g}" + (" screen off" if screen == "off" else "")
                    lines += [f"  {label:42s} kernel {ms(d)} {rate(d)}   x{float(np.median(bd)) / float(np.median(d)):.3f} the blind rate",
                              f"  {'':42s} wall   {ms(w)} {rate(w)}   x{float(np.median(bw)) / float(np.median(w)):.3f} the blind rate; {res[1]} matches"]
                    out[f"{kind}_{dim}_{max_error:g}" + ("_noscreen" if screen == "off" else "")] = {
                        "kernel_pairs_per_s": P / float(np.median(d)), "wall_pairs_per_s": P / float(np.median(w)),
                        "kernel_vs_blind": float(np.median(bd)) / float(np.median(d)), "wall_vs_blind": float(np.median(bw)) / float(np.median(w)),
                        "matches": res[1]}
    finally:
        for c in ctxs.values():
            c.close()
    print("\n".join(lines), file=sys.stderr)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
