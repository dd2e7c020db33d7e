"""The case the screen sweep is expected to lose: a pair list of adjacent frames only at 256-D, every row a noisy copy of the same
base row, so the bound leaves most rows open and the exact pass recomputes them on top of the FP6 sweep. Times the job with
EACHAM_MATCH_SWEEP_FORM=screen and =exact and prints the share of rows left open (bound_sweep_heavy_candidates.py is the 128-D
model of this run).  python tools/experiments/screen_sweep_heavy_candidates.py [noise]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
from eacham_amd import HipContext, synth  # noqa: E402
import oracle_api as O  # noqa: E402

noise = float(sys.argv[1]) if len(sys.argv) > 1 else 3.0
dim, n, F = 256, 2000, 48
base = synth.random_u8_descriptors(n, dim, 7, 0)
descs = [np.clip(base + np.rint(noise * synth.rng_normal(7, 10 + k, (n, dim))), 0, 255).astype(np.float32) for k in range(F)]
pairs = np.array([[a, a + 1] for a in range(F - 1)] + [[a + 1, a] for a in range(F - 1)], dtype=np.int32)   # adjacent frames only
res = {}
for form in ("exact", "screen"):
    os.environ["EACHAM_MATCH_SWEEP_FORM"] = form
    ctx = HipContext(0)
    for f, d in enumerate(descs):
        ctx.upload_descriptors(f, d)
    got = ctx.match_all_pairs(pairs, stats=False)
    ctx.sync()
    times = []
    for _ in range(7):
        t0 = time.perf_counter()
        got = ctx.match_all_pairs(pairs, stats=False)
        ctx.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    rows, left_open = ctx.match_screen()
    res[form] = got
    print(form, "ms per job: median", round(float(np.median(times)), 3), "min", round(min(times), 3), "max", round(max(times), 3),
          "matches per pair", round(float(got[0].mean()), 1), "open rows", left_open, "of", rows)
    ctx.close()
print("same bytes:", all(a.tobytes() == b.tobytes() for a, b in zip(res["exact"][:4], res["screen"][:4])))
want = O.match_all_pairs(descs, pairs[:6])
print("bit exact on 6 pairs:", all(np.array_equal(a[:len(b)] if a.ndim == 1 and len(a) > len(b) else a, b) for a, b in zip(
    [res["screen"][0][:6], res["screen"][1][:7], res["screen"][2][:res["screen"][1][6]], res["screen"][3][:res["screen"][1][6]]], want[:4])))
