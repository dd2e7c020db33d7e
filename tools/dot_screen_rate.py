"""Rate of the screened dot-product matcher (eacham_match_all_pairs_dot_screened) beside eacham_match_all_pairs_dot of the same build.

  python tools/dot_screen_rate.py [--cases s200_ms0.5,s200_noms,worst24,d128] [--reps 5] [--out FILE]

Inputs: `s200_*` are the inputs of bench.py's s200_d256_f32 line (200 frames x 2000 x 256-D unit-norm floats, 19 900 pairs) at
min_score 0.5 and at -inf; `worst24` is 24 frames of 2000 near-identical rows (every row and column is open: the exact pass does
all the work, after a sweep that decided nothing); `d128` is the s200 scene at 128-D. Each (case, form) runs in a child process of
its own, one after the other on the same device: one untimed call, then `reps` timed ones, median [min .. max]. Figures: the
host-pointer call end to end, and the device time of its kernels from the C-ABI's HIP-event slots (tile slot = sweep + classify +
exact pass, or the fp32 tile kernel; finalize slot = finalize + scan + compaction). Results are not checked here
(tests/test_match_dot_screen_gpu.py does that); no figure is a pass condition. Prints one JSON line; --out also writes the text report."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {   # name -> (frames, rows, dim, min_score)
    "s200_ms0.5": (200, 2000, 256, 0.5),
    "s200_noms": (200, 2000, 256, float("-inf")),
    "worst24": (24, 2000, 256, float("-inf")),
    "d128": (200, 2000, 128, 0.5),
}


def descriptors(case, f):
    import numpy as np
    from eacham_amd import synth
    frames, rows, dim, _ = CASES[case]
    if case == "worst24":
        one = synth.unit_float_descriptors(1, dim, 1, 99)
        return np.ascontiguousarray(one + 1e-6 * synth.rng_normal(1, f, (rows, dim)), np.float32)
    base = synth.unit_float_descriptors(rows, dim, 1, 99)
    return synth.unit_float_descriptors(rows, dim, 1, f, shared=base[:rows // 2])


def child(case, form, reps):
    import numpy as np
    from eacham_amd import HipContext, capi, synth
    frames, rows, dim, ms = CASES[case]
    pairs = synth.all_pairs(frames)
    with HipContext(0) as ctx:
        for f in range(frames):
            ctx.upload_descriptors_f32(f, descriptors(case, f))
        cap = len(pairs) * rows
        call = lambda: ctx.match_all_pairs_dot(pairs, ms, 30, 30, cap=cap, stats=False, screened=form == "screened")   # noqa: E731
        res = call()                                              # untimed: workspace growth, code load, the fp16 images
        ctx.profile_enable(True)
        wall, dev = [], []
        for _ in range(reps):
            ctx.profile_reset()
            t0 = time.perf_counter()
            res = call()
            wall.append(time.perf_counter() - t0)
            dev.append((ctx.profile_get(capi.KERNEL_MATCH_TILE)[1] + ctx.profile_get(capi.KERNEL_MATCH_FINALIZE)[1]) * 1e-3)
        tile = ctx.profile_get(capi.KERNEL_MATCH_TILE)[1]
        tally = ctx.match_dot_screen() if form == "screened" else None
    n = len(pairs)
    rate = lambda ts: {"median": n / float(np.median(ts)), "min": n / max(ts), "max": n / min(ts)}   # noqa: E731
    print(json.dumps({"case": case, "form": form, "pairs": n, "edges": int((res[0] > 0).sum()), "matches": int(res[0].sum()),
                      "end_to_end_pairs_per_s": rate(wall), "device_pairs_per_s": rate(dev), "tile_slot_ms_last": tile, "screen": tally}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, metavar=("CASE", "FORM"))
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.reps)
    out, lines = {}, []
    for case in a.cases.split(","):
        frames, rows, dim, ms = CASES[case]
        res = {}
        for form in ("exact", "screened"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, form, "--reps", str(a.reps)], capture_output=True, text=True)
            if r.returncode != 0:      # (nothing more is started on the device after a failed child)
                sys.exit(f"{case} {form} run failed ({r.returncode}):\n{r.stdout}{r.stderr}")
            res[form] = json.loads(r.stdout.strip().splitlines()[-1])
        out[case] = res
        lines.append(f"{case}: {frames} frames x {rows} x {dim}-D, min_score {ms}, {res['exact']['pairs']} pairs, {a.reps} timed after one untimed, median [min .. max] pairs/s")
        for key, label in (("device_pairs_per_s", "kernels (HIP events)"), ("end_to_end_pairs_per_s", "host-pointer call end to end")):
            e, s = res["exact"][key], res["screened"][key]
            lines.append(f"  {label}:")
            lines.append(f"    eacham_match_all_pairs_dot          {e['median']:10.0f} [{e['min']:.0f} .. {e['max']:.0f}]")
            lines.append(f"    eacham_match_all_pairs_dot_screened {s['median']:10.0f} [{s['min']:.0f} .. {s['max']:.0f}]  x{s['median'] / e['median']:.2f}"
                         + ("  SLOWER than the fp32 call" if s["median"] < e["median"] else ""))
        t = res["screened"]["screen"]
        lines.append(f"  screen: rows dead/settled/open {t['rows']}, columns {t['cols']}, fallback pairs {t['fallback_pairs']}; "
                     f"matches exact {res['exact']['matches']} screened {res['screened']['matches']}")
    print("\n".join(lines), file=sys.stderr)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
