#!/usr/bin/env python3
"""Rate of the track building (eacham_tracks_build / eacham_graph_tracks) on two match graphs:

  S200    the graph `bench.py --gpus 1 --steps 1 --warmup 1 --dump-outputs DIR` writes (200 frames x 2000 keypoints):
          --s200 DIR (skipped when the directory is not there)
  30x600  the seeded scene of tests/tracks_cases.py

Per graph and entry point: end-to-end wall time of the call and the device time between its first and last kernel by HIP events
(eacham_profile_enable + eacham_tracks_debug_last), median of 5 with min .. max after one warm-up call, and the rounds used.
For reference only, a single-threaded C++ union-find over the same arrays (tests/cpp/tracks_driver.cpp ... uf): it is no parent
and no pass condition. Writes the lines to stdout; profiles/tracks_rate.txt keeps a copy of a run.
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from eacham_amd import HipContext, ResidentGraph  # noqa: E402
from eacham_amd import tracks as T  # noqa: E402


def load_s200(dirname, kpts):
    pairs = np.load(os.path.join(dirname, "pairs.npy")).astype(np.int32).reshape(-1, 2)
    counts = np.load(os.path.join(dirname, "counts.npy")).astype(np.int32)
    offsets = np.load(os.path.join(dirname, "offsets.npy")).astype(np.int64)[:len(counts)]
    edges = np.load(os.path.join(dirname, "edges.npy")).astype(np.uint32).reshape(-1, 2)
    n_frames = int(pairs.max()) + 1
    return {"kp": [kpts] * n_frames, "pairs": pairs, "counts": counts, "offsets": offsets,
            "q": np.ascontiguousarray(edges[:, 0]), "t": np.ascontiguousarray(edges[:, 1]), "keep": None}


def fmt(xs):
    return f"{statistics.median(xs):9.3f} ms  ({min(xs):.3f} .. {max(xs):.3f})"


def measure(ctx, name, case, reps):
    n_frames = len(case["kp"])
    args = (n_frames, case["pairs"], case["counts"], case["offsets"], case["q"], case["t"], case["kp"])
    g = ResidentGraph(ctx, *args)
    try:
        for what, call in (("eacham_tracks_build", lambda: T.build_tracks(ctx, *args, case["keep"])),
                           ("eacham_graph_tracks", lambda: g.tracks(case["keep"]))):
            call()
            wall, dev, info, tr = [], [], None, None
            for _ in range(reps):
                t0 = time.perf_counter()
                tr = call()
                wall.append((time.perf_counter() - t0) * 1e3)
                info = T.last_call_info(ctx)
                dev.append(info["kernel_ms"])
            print(f"{name:7s} {what:20s} end to end {fmt(wall)}   kernels {fmt(dev)}   rounds {info['rounds']} of {info['round_cap']}, "
                  f"{info['readbacks']} read-backs; {tr.n_tracks} tracks, {tr.obs_frame.size} observations, "
                  f"{int(tr.flags.sum())} conflicting, from {int(case['counts'].sum())} matches over {int(sum(case['kp']))} keypoints")
    finally:
        g.close()


def host_union_find(name, case):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_tracks_cpp_gpu as D
    with tempfile.TemporaryDirectory() as tmp:
        exe = D.build_driver(os.path.join(tmp, "tracks_driver"))
        fin = os.path.join(tmp, "in.bin")
        D.write_input(fin, case, case["keep"], 2, 0)
        r = subprocess.run([exe, fin, os.path.join(tmp, "out.bin"), "uf"], capture_output=True, text=True)
        if r.returncode != 0:
            print(f"{name:7s} host union-find: driver failed: {r.stderr.strip()}")
            return
        ms = [float(l.split()[1]) for l in r.stdout.splitlines() if l.startswith("union_find_ms")]
        print(f"{name:7s} {'host union-find (1 thread)':20s} {fmt(ms)}   [reference only]")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--s200", metavar="DIR", default=os.path.join("results", "outputs"))
    ap.add_argument("--kpts", type=int, default=2000, help="keypoints per frame of the dumped graph")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import tracks_cases as TC
    graphs = []
    if os.path.exists(os.path.join(a.s200, "edges.npy")):
        graphs.append(("S200", load_s200(a.s200, a.kpts)))
    else:
        print(f"S200    skipped: no match graph under {a.s200} (bench.py --dump-outputs writes it)")
    graphs.append(("30x600", TC.scene()))
    with HipContext(0) as ctx:
        ctx._check(ctx._L.eacham_profile_enable(ctx.handle, 1))
        for name, case in graphs:
            measure(ctx, name, case, a.reps)
    for name, case in graphs:
        host_union_find(name, case)


if __name__ == "__main__":
    main()
