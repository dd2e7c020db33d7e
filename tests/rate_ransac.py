"""Threshold RANSAC over a match-graph-sized list of pairs (eacham_ransac_batch), one JSON line.

The job: 4950 pairs (all pairs of 100 frames), 31 .. 600 matches per pair, nominal outlier shares 0.2 .. 0.7 (64 base scenes, every pair
a random subset of one), essential kind, 1000 five-point samples per pair, confidence 0.999, 1 px. Every figure is the MEDIAN of
`--reps` (default 10) timed calls after a warm-up call:
  (a) eacham_lmeds_batch on the same pairs with its own 89 samples — what the library could do before, for context;
  (b) RANSAC in a single pass (stage1 >= S);
  (c) RANSAC at stage1 in {16, 32, 64, 128}, each alternated with (b) call by call in the same loop.
end_to_end_ms: the host clock around the synchronising call, profiler off. kernels_ms: the EACHAM_KERNEL_SCORE slot, profiler on, in
a loop of its own, reset before every call. samples_solved and table_ms (host milliseconds spent building the budget rows) are the
library's own figures (eacham_ransac_debug_last); samples_consumed is the sum of n_used. bytes_equal_single: every output of (c)
against (b). The script times the library as built: a second rb_count mapping is a second build selected with EACHAM_HIP_LIB.
Run on the GPU box:  python tests/rate_ransac.py [--pairs 4950] [--reps 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from eacham_amd import HipContext, capi, lmeds, ransac  # noqa: E402
import score_cases as SC  # noqa: E402

STAGES = (16, 32, 64, 128)
SAMPLES, LMEDS_SAMPLES, CONFIDENCE, BASES = 1000, 89, 0.999, 64


def draw(rng, n, m, count):
    """count rows of m distinct indices out of n: uniform draws, rows with a repeat drawn again."""
    idx = rng.integers(0, n, (count, m), dtype=np.int32)
    while True:
        s = np.sort(idx, axis=1)
        bad = np.flatnonzero((s[:, 1:] == s[:, :-1]).any(axis=1))
        if bad.size == 0:
            return idx
        idx[bad] = rng.integers(0, n, (bad.size, m), dtype=np.int32)


def make_job(pairs, seed=1):
    rng = np.random.default_rng(seed)
    bases = [SC.two_view_case(n=600, n_models=1, seed=100 + k, outliers=0.2 + 0.5 * k / (BASES - 1), facing=True) for k in range(BASES)]
    uv1, uv2, samples, share = [], [], [], []
    for p in range(pairs):
        c = bases[p % BASES]
        n = int(rng.integers(31, 601))
        keep = rng.permutation(600)[:n]
        uv1.append(c["uv1"][keep]), uv2.append(c["uv2"][keep]), share.append(float(c["bad"][keep].mean()))
        samples.append(draw(rng, n, 5, SAMPLES))
    K = np.asarray(bases[0]["K"], dtype=np.float64)
    return uv1, uv2, samples, K, share


def timed_pair(fa, fb, reps):
    """fa and fb alternated call by call after a warm-up call of each: two lists of seconds."""
    fa(), fb()
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); fa(); ta.append(time.perf_counter() - t0)   # noqa: E702
        t0 = time.perf_counter(); fb(); tb.append(time.perf_counter() - t0)   # noqa: E702
    return ta, tb


def device_ms(ctx, fn, reps):
    """Median over `reps` calls of the device time one call leaves in the EACHAM_KERNEL_SCORE slot, after a warm-up call."""
    fn()
    ctx.profile_enable(True)
    ms = []
    for _ in range(reps):
        ctx.profile_reset()
        fn()
        ms.append(ctx.profile_get(capi.KERNEL_SCORE)[1])
    ctx.profile_enable(False)
    return float(np.median(ms))


def med_ms(ts):
    return round(float(np.median(ts)) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4950)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    uv1, uv2, samples, K, share = make_job(a.pairs)
    thr = float(np.float32((1.0 / ((K[0] + K[1]) / 2)) ** 2))
    pp, A, B, sp, idx = lmeds.pack("essential", uv1, uv2, samples)
    lpp, lA, lB, lsp, lidx = lmeds.pack("essential", uv1, uv2, [s[:LMEDS_SAMPLES] for s in samples])
    out = {"pairs": a.pairs, "matches": int(pp[-1]), "samples": int(sp[-1]), "reps": a.reps,
           "outlier_share_min_max": [round(min(share), 3), round(max(share), 3)]}
    with HipContext(0) as ctx:
        run = lambda stage1: ransac.ransac_batch_raw(ctx, "essential", pp, A, B, sp, idx, thr, CONFIDENCE, stage1, K)   # noqa: E731
        single = lambda: run(1 << 20)                                                                                    # noqa: E731
        lm = lambda: lmeds.lmeds_batch_raw(ctx, "essential", lpp, lA, lB, lsp, lidx, K)                                   # noqa: E731
        ref = single()
        out["samples_consumed"] = int(ref.n_used.astype(np.int64).sum())
        out["pairs_with_a_model"] = int((ref.winner[:, 0] >= 0).sum())
        solved_single, _ = ransac.debug_last(ctx)
        ta, tb = timed_pair(lm, lm, (a.reps + 1) // 2)
        out["lmeds_89"] = {"end_to_end_ms": med_ms(ta + tb), "timed_calls": len(ta + tb), "kernels_ms": round(device_ms(ctx, lm, a.reps), 3),
                           "samples_solved": int(lsp[-1])}
        out["single"] = {"kernels_ms": round(device_ms(ctx, single, a.reps), 3), "samples_solved": solved_single}
        singles, tables = [], []
        for stage1 in STAGES:
            got = run(stage1)
            solved, table_ms = ransac.debug_last(ctx)
            tables.append(table_ms)
            same = all(np.array_equal(getattr(got, f), getattr(ref, f)) for f in ("inliers", "winner", "n_candidates", "n_used")) and \
                np.array_equal(got.models.view(np.uint64), ref.models.view(np.uint64)) and all(np.array_equal(x, y) for x, y in zip(got.masks, ref.masks))
            tb, tc = timed_pair(single, lambda: run(stage1), a.reps)
            singles += tb
            out[f"stage1_{stage1}"] = {"end_to_end_ms": med_ms(tc), "end_to_end_min_max_ms": [round(min(tc) * 1e3, 3), round(max(tc) * 1e3, 3)],
                                       "single_alternated_ms": med_ms(tb), "kernels_ms": round(device_ms(ctx, lambda: run(stage1), a.reps), 3),
                                       "samples_solved": solved, "bytes_equal_single": bool(same)}
        out["single"].update(end_to_end_ms=med_ms(singles), timed_calls=len(singles),
                             end_to_end_min_max_ms=[round(min(singles) * 1e3, 3), round(max(singles) * 1e3, 3)],
                             end_to_end_spread_ms=round(float(np.percentile(singles, 75) - np.percentile(singles, 25)) * 1e3, 3))
        for _ in range(a.reps):
            run(0)
            tables.append(ransac.debug_last(ctx)[1])
        out["table_ms"] = round(float(np.median(tables)), 3)   # host time of ransac_build_table inside a call, median over the calls read
        out["default_stage1_solved"] = ransac.debug_last(ctx)[0]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
