"""Rate of the dot-product form of the float matcher beside the L2 form: all 19 900 pairs of 200 frames x 2000 x 256-D unit-norm
float descriptors (the inputs of bench.py's s200_d256_f32 line, built from eacham_amd/synth.py directly).

  python tools/dot_rate.py [--l2-lib PATH] [--frames 200] [--kpts 2000] [--reps 5] [--out FILE]

Each form runs in a child process of its own, one after the other in the same session on the same device: one untimed call,
then `reps` timed ones, median taken. --l2-lib names the library the L2 form is measured on (the parent commit's build for a
before/after comparison; default: the library in the tree). Figures per form: the call end to end through the host-pointer
entry point (what a caller sees: it includes the copy of ~2 x 10^7 matches to the host) and the device time of its tile and
finalize kernels from the C-ABI's HIP-event slots. Acceptance (printed): the dot-form median in pairs/s is at least the L2
median minus the L2 run's own min-to-max spread. Prints one JSON line; --out also writes the text report."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(form, frames, kpts, reps):
    import numpy as np
    from eacham_amd import HipContext, capi, synth
    base = synth.unit_float_descriptors(kpts, 256, 1, 99)
    pairs = synth.all_pairs(frames)
    with HipContext(0) as ctx:
        for f in range(frames):
            ctx.upload_descriptors_f32(f, synth.unit_float_descriptors(kpts, 256, 1, f, shared=base[:kpts // 2]))
        cap = len(pairs) * kpts
        if form == "l2":
            call = lambda: ctx.match_all_pairs(pairs, cap=cap, stats=False)          # noqa: E731
        else:
            call = lambda: ctx.match_all_pairs_dot(pairs, 0.5, 30, 30, cap=cap, stats=False)   # noqa: E731
        res = call()                                                                 # untimed: workspace growth, code load
        ctx.profile_enable(True)
        wall, dev = [], []
        for _ in range(reps):
            ctx.profile_reset()
            t0 = time.perf_counter()
            res = call()
            wall.append(time.perf_counter() - t0)
            dev.append((ctx.profile_get(capi.KERNEL_MATCH_TILE)[1] + ctx.profile_get(capi.KERNEL_MATCH_FINALIZE)[1]) * 1e-3)
        tile = ctx.profile_get(capi.KERNEL_MATCH_TILE)[1]
    n = len(pairs)
    rate = lambda ts: {"median": n / float(np.median(ts)), "min": n / max(ts), "max": n / min(ts)}   # noqa: E731
    print(json.dumps({"form": form, "pairs": n, "edges": int((res[0] > 0).sum()), "matches": int(res[0].sum()),
                      "end_to_end_pairs_per_s": rate(wall), "device_pairs_per_s": rate(dev), "tile_kernel_ms_last": tile,
                      "lib": os.path.relpath(capi.LIB_PATH, ROOT)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--l2-lib", default=None)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--kpts", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.frames, a.kpts, a.reps)
    out = {}
    for form in ("l2", "dot"):
        env = dict(os.environ)
        if form == "l2" and a.l2_lib:
            env["EACHAM_HIP_LIB"] = os.path.abspath(a.l2_lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", form, "--frames", str(a.frames), "--kpts", str(a.kpts),
                            "--reps", str(a.reps)], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"{form} run failed ({r.returncode}):\n{r.stdout}{r.stderr}")
        out[form] = json.loads(r.stdout.strip().splitlines()[-1])
    lines = [f"{a.frames} frames x {a.kpts} x 256-D float, {out['l2']['pairs']} pairs, {a.reps} timed repetitions after one untimed, median [min .. max] pairs/s"]
    for key, label in (("device_pairs_per_s", "tile + finalize kernels (HIP events)"), ("end_to_end_pairs_per_s", "host-pointer call end to end")):
        l2, dot = out["l2"][key], out["dot"][key]
        spread = l2["max"] - l2["min"]
        ok = dot["median"] >= l2["median"] - spread
        out[key + "_accepted"] = bool(ok)
        lines.append(f"  {label}:")
        lines.append(f"    L2  {l2['median']:10.0f} [{l2['min']:.0f} .. {l2['max']:.0f}]  spread {spread:.0f}   ({out['l2']['lib']})")
        lines.append(f"    dot {dot['median']:10.0f} [{dot['min']:.0f} .. {dot['max']:.0f}]  -> {'not slower' if ok else 'SLOWER'} (needs >= {l2['median'] - spread:.0f})")
    lines.append(f"  L2: {out['l2']['edges']} edges / {out['l2']['matches']} matches; dot: {out['dot']['edges']} edges / {out['dot']['matches']} matches")
    print("\n".join(lines), file=sys.stderr)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
