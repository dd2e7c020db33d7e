"""Rate of the wide Hamming path (FP4 sweep, eacham_amd/csrc/matcher_ham_wide.hip) beside the narrow kind on the same rows.

  python tools/match_hamming_wide_rate.py [--frames 100] [--rows 2000] [--rounds 6] [--reps 3] [--out profiles/match_hamming_wide_rate.txt]

The job is that of tools/match_hamming_rate.py: all pairs of `frames` frames x `rows` rows from tests/ham_cases.py (landmark rows with
each bit flipped with p = 0.08 per observation, distractors, shuffled), eacham_match_all_pairs_hamming, lean mutual form with the
literal thresholds 30 / 30. Three forms:
  narrow32   32-byte rows uploaded with eacham_upload_descriptors_bits       (0 / 255 in the int8 kernels: FP6 screen + exact pass)
  wide32     the same rows uploaded with eacham_upload_descriptors_bits_wide (+-1 on the FP4 matrix cores, KS 4)
  wide64     64-byte rows, wide                                              (KS 8: the matrix work of a 256-D int8 row)
The forms alternate, `rounds` times, each run in a child process of its own on the same device: one untimed call, then `reps`
timed ones. Per call: wall time end to end (host-pointer entry point) and the device time of the sweep and tail kernels (the C-ABI's
HIP-event slots); pairs/s from both, median [min .. max] over all timed calls. narrow32 and wide32 must return the same bytes
(checked on counts, q, t and distances: a difference ends the tool with a non-zero exit status). No rate is a pass condition.
Prints one JSON line; --out also writes the text report."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FORMS = {"narrow32": (32, False), "wide32": (32, True), "wide64": (64, True)}


def child(form, frames, rows, reps):
    from eacham_amd import HipContext, capi, synth
    import ham_cases as HC
    nbytes, wide = FORMS[form]
    descs = HC.binary_frames(nbytes, [rows] * frames, (3 * rows) // 5, 7, inject=False)
    pairs = synth.all_pairs(frames)
    with HipContext(0) as ctx:
        t0 = time.perf_counter()
        for f, d in enumerate(descs):
            (ctx.upload_descriptors_bits_wide if wide else ctx.upload_descriptors_bits)(f, d)
        ctx.sync()
        upload_s = time.perf_counter() - t0
        cap = len(pairs) * rows
        call = lambda: ctx.match_all_pairs_hamming(pairs, cap=cap, stats=False)        # noqa: E731
        res = call()
        ctx.profile_enable(True)
        wall, dev = [], []
        for _ in range(reps):
            ctx.profile_reset()
            t0 = time.perf_counter()
            res = call()
            wall.append(time.perf_counter() - t0)
            dev.append((ctx.profile_get(capi.KERNEL_MATCH_TILE)[1] + ctx.profile_get(capi.KERNEL_MATCH_FINALIZE)[1]) * 1e-3)
        extra = {"wide_debug": ctx.match_debug_hamming_wide()} if wide else {}
    digest = hashlib.sha256(b"".join(a.tobytes() for a in res[:5])).hexdigest()
    print(json.dumps({"form": form, "pairs": len(pairs), "edges": int((res[0] > 0).sum()), "matches": int(res[0].sum()), "digest": digest,
                      "upload_s": upload_s, "wall_s": wall, "device_s": dev, **extra}))


def run_child(form, a):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", form, "--frames", str(a.frames), "--rows", str(a.rows),
                        "--reps", str(a.reps)], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"{form} run failed ({r.returncode}):\n{r.stdout}{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.frames, a.rows, a.reps)
    import numpy as np
    runs = {f: [] for f in FORMS}
    for _ in range(a.rounds):
        for f in FORMS:
            runs[f].append(run_child(f, a))
    npairs = runs["wide64"][0]["pairs"]
    flat = lambda form, key: [x for r in runs[form] for x in r[key]]                                      # noqa: E731
    ms = lambda xs: f"{1e3 * float(np.median(xs)):9.3f} [{1e3 * min(xs):.3f} .. {1e3 * max(xs):.3f}] ms"  # noqa: E731
    rate = lambda xs: f"{npairs / float(np.median(xs)):11.0f} [{npairs / max(xs):.0f} .. {npairs / min(xs):.0f}] pairs/s"   # noqa: E731
    lines = [f"{a.frames} frames x {a.rows} rows, {npairs} pairs, eacham_match_all_pairs_hamming, lean mutual form 30 / 30; {a.rounds} alternating rounds, "
             f"{a.reps} timed calls each after one untimed; median [min .. max] over all timed calls"]
    out = {}
    for f in FORMS:
        d, w = flat(f, "device_s"), flat(f, "wall_s")
        r0 = runs[f][0]
        lines += [f"  {f:9s} sweep + tail kernels (HIP events): {ms(d)}  {rate(d)}",
                  f"  {'':9s} call end to end:                    {ms(w)}  {rate(w)}",
                  f"  {'':9s} {r0['edges']} edges / {r0['matches']} matches" + (f"; {r0['wide_debug']}" if "wide_debug" in r0 else "")]
        out[f] = {"device_pairs_per_s": npairs / float(np.median(d)), "wall_pairs_per_s": npairs / float(np.median(w))}
    same = len({r["digest"] for f in ("narrow32", "wide32") for r in runs[f]}) == 1
    out["wide32_equals_narrow32"] = same
    med = lambda f: float(np.median(flat(f, "device_s")))                                                 # noqa: E731
    lines += [f"  wide32 against narrow32 (device time, medians): x{med('narrow32') / med('wide32'):.3f} the rate; the same bytes: {same}",
              f"  wide64 against narrow32 (the int8 256-D sweep on the same scene shape): x{med('narrow32') / med('wide64'):.3f} the rate"]
    print("\n".join(lines), file=sys.stderr)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(out))
    if not same:
        sys.exit("wide32 and narrow32 returned different bytes")


if __name__ == "__main__":
    main()
