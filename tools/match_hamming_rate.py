"""Rate of Hamming matching of binary descriptors beside the only route the parent commit has for them: the same rows expanded
to {0, 255} floats, uploaded with eacham_upload_descriptors and matched with eacham_match_all_pairs (L2).

  python tools/match_hamming_rate.py --base-lib <libeacham_hip.so of the parent commit> [--frames 100] [--rows 2000] [--bytes 32]
                                     [--rounds 6] [--reps 3] [--out profiles/match_hamming_rate.txt]

The job: all pairs of `frames` frames x `rows` rows x `bytes` bytes from tests/ham_cases.py (landmark rows with each bit flipped
with p = 0.08 per observation, distractors, shuffled), lean mutual form with the literal thresholds 30 / 30. The two libraries
alternate, `rounds` times, each run in a child process of its own on the same device (EACHAM_HIP_LIB selects the library):
one untimed call, then `reps` timed ones. Per run: the upload of all frames (wall, bytes sent), the matching call end to end
(host-pointer entry point) and the device time of its sweep and tail kernels (the C-ABI's HIP-event slots). The matching
kernels are the same code, so the acceptance (printed) is: the Hamming median of the device time lies inside the baseline's own
min-to-max spread over all its timed calls; a median above it ends the tool with a non-zero exit status. The end-to-end time is
reported beside it without a criterion. The L2 baseline's MATCHES differ (sqrt in its ratio test): only times compare.
The Hamming runs also report the screen's open fraction and the settled / verified counts of the column pruning, and the job
is repeated at 16 bytes (the bound form of the sweep) under EACHAM_MATCH_SWEEP_FORM=bound (the default there) and =exact.
Prints one JSON line; --out also writes the text report."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def child(form, frames, rows, nbytes, reps):
    import numpy as np
    from eacham_amd import HipContext, capi, synth
    import ham_cases as HC
    import ham_reference as R
    descs = HC.binary_frames(nbytes, [rows] * frames, (3 * rows) // 5, 7, inject=False)
    pairs = synth.all_pairs(frames)
    if form == "l2":   # the parent's route: 32 x the bytes, expanded on the host
        descs = [R.embed(d) for d in descs]
    sent = sum(d.nbytes for d in descs)
    with HipContext(0) as ctx:
        t0 = time.perf_counter()
        for f, d in enumerate(descs):
            (ctx.upload_descriptors if form == "l2" else ctx.upload_descriptors_bits)(f, d)
        ctx.sync()
        upload_s = time.perf_counter() - t0
        cap = len(pairs) * rows
        if form == "l2":
            call = lambda: ctx.match_all_pairs(pairs, cap=cap, stats=False)                # noqa: E731
        else:
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
        extra = {}
        if form != "l2":
            extra = {"screen_rows_open": ctx.match_screen(), "colprune_settled_verified": ctx.match_colprune()}
    print(json.dumps({"form": form, "pairs": len(pairs), "edges": int((res[0] > 0).sum()), "matches": int(res[0].sum()),
                      "upload_s": upload_s, "upload_bytes": sent, "wall_s": wall, "device_s": dev, **extra,
                      "lib": os.path.relpath(capi.LIB_PATH, ROOT)}))


def run_child(form, a, nbytes, lib=None, sweep_form=None):
    env = dict(os.environ)
    if lib:
        env["EACHAM_HIP_LIB"] = os.path.abspath(lib)
    if sweep_form:
        env["EACHAM_MATCH_SWEEP_FORM"] = sweep_form
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", form, "--frames", str(a.frames), "--rows", str(a.rows),
                        "--bytes", str(nbytes), "--reps", str(a.reps)], env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"{form} run failed ({r.returncode}):\n{r.stdout}{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", default=None, help="the parent commit's library (default: the library in the tree, for a dry run)")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--bytes", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.frames, a.rows, a.bytes, a.reps)
    import numpy as np
    runs = {"l2": [], "ham": []}
    for _ in range(a.rounds):
        runs["l2"].append(run_child("l2", a, a.bytes, lib=a.base_lib))
        runs["ham"].append(run_child("ham", a, a.bytes))
    ms = lambda xs: f"{1e3 * float(np.median(xs)):9.3f} [{1e3 * min(xs):.3f} .. {1e3 * max(xs):.3f}]"   # noqa: E731
    flat = lambda form, key: [x for r in runs[form] for x in r[key]]                                      # noqa: E731
    l2, ham = runs["l2"][0], runs["ham"][0]
    lines = [f"{a.frames} frames x {a.rows} rows x {a.bytes} bytes, {l2['pairs']} pairs, lean mutual form 30 / 30; {a.rounds} alternating rounds, "
             f"{a.reps} timed calls each after one untimed; ms, median [min .. max] over all timed calls",
             f"  baseline = rows expanded to 0 / 255 floats + eacham_upload_descriptors + eacham_match_all_pairs on {l2['lib']}",
             f"  new      = eacham_upload_descriptors_bits + eacham_match_all_pairs_hamming on {ham['lib']}"]
    out = {"runs": runs}
    b, h = flat("l2", "device_s"), flat("ham", "device_s")
    med = float(np.median(h))
    verdict = "inside" if min(b) <= med <= max(b) else "BELOW (faster than)" if med < min(b) else "ABOVE (slower than)"
    accepted = med <= max(b)          # the acceptance: the same kernels may not be slower than the baseline's own spread allows
    out["device_s_verdict"], out["accepted"] = verdict, bool(accepted)
    lines += ["  sweep + tail kernels (HIP events) — the acceptance figure:", f"    baseline {ms(b)}",
              f"    new      {ms(h)}  -> median {verdict} the baseline's spread: {'accepted' if accepted else 'NOT ACCEPTED'}"]
    b, h = flat("l2", "wall_s"), flat("ham", "wall_s")
    lines += ["  matching call end to end (reported, no criterion: the Hamming call also brings the distances back):", f"    baseline {ms(b)}",
              f"    new      {ms(h)}  median {1e3 * (float(np.median(h)) - float(np.median(b))):+.3f} ms against the baseline's"]
    up_b, up_h = [r["upload_s"] for r in runs["l2"]], [r["upload_s"] for r in runs["ham"]]
    lines += [f"  upload of {a.frames} frames (wall, first call of the process included):",
              f"    baseline {ms(up_b)}  {l2['upload_bytes']} bytes sent", f"    new      {ms(up_h)}  {ham['upload_bytes']} bytes sent"]
    sr, so = ham["screen_rows_open"]
    cs, cv = ham["colprune_settled_verified"]
    lines += [f"  baseline (L2 ratio test): {l2['edges']} edges / {l2['matches']} matches; new (Hamming ratio test): {ham['edges']} edges / {ham['matches']} matches",
              f"  screen sweep: {so} of {sr} query rows left open for the exact pass ({100.0 * so / max(sr, 1):.2f} %)",
              f"  column pruning: {cs} candidate columns settled from the row minima, {cv} verified by the column pass ({100.0 * cs / max(cs + cv, 1):.2f} % settled)"]
    # the bound form of the sweep (<= 128 bits): no counter of its open rows is exposed; its effect shows as device time against the exact form
    b16 = {sf: run_child("ham", a, 16, sweep_form=sf) for sf in ("bound", "exact")}
    out["bytes16"] = b16
    lines.append(f"  16-byte rows, same job, sweep + tail kernels: bound form (default) {ms(b16['bound']['device_s'])}   exact form {ms(b16['exact']['device_s'])}")
    lines.append(f"    ({b16['bound']['matches']} / {b16['exact']['matches']} matches; column pruning settled / verified {b16['bound']['colprune_settled_verified']})")
    print("\n".join(lines), file=sys.stderr)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    out.pop("runs")
    print(json.dumps(out))
    if not accepted:
        sys.exit("NOT ACCEPTED: the device-time median of the Hamming path lies above the baseline's min-to-max spread")


if __name__ == "__main__":
    main()
