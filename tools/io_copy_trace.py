"""Each of the staged entry points once after a warm-up pass, a host-to-device copy of SEP bytes between two calls, for a
memory-copy trace of its own:

    rocprofv3 --memory-copy-trace --output-format csv -d <dir> -- python tools/io_copy_trace.py
    python tools/io_copy_trace.py --table <dir> [<dir of another build>]

--table splits the trace at the separators and prints, per entry point, the copies of the call and their bytes in order."""
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEP = 7777
NAMES = ["solve_minimal", "solve_pnp", "score_hypotheses", "triangulate_tracks", "reprojection_errors", "two_view_points",
         "two_view_batch", "lmeds_batch", "graph_set_frames", "match_all_pairs", "match_all_pairs_nostats", "match_pair",
         "graph_best_pair", "(second context: float frames, warm-up)", "match_all_pairs_dot"]


def calls():
    import torch
    from eacham_amd import HipContext, score, synth, triangulate as tri
    from eacham_amd import graph as G
    import lmeds_batch_cases as LC
    import score_cases as SC
    import two_view_batch_cases as TC
    from test_graph_oracle import scenario
    from test_tri_oracle import _two_view_case

    lc, tc = LC.mixed("homography"), TC.mixed()
    pn = SC.pnp_case(n=800, n_models=64, seed=17)
    samples = np.array([np.random.default_rng(s).choice(800, size=5, replace=False) for s in range(300)], np.int32)
    tr = synth.make_tracks(synth.make_scene(12, 600, 6, seed=7), seed=7, min_obs=2, outlier_frac=0.3)
    first = np.asarray(tr["track_ptr"][:-1])[np.diff(tr["track_ptr"]) > 0]
    uv1, uv2, K, Ts = _two_view_case(seed=5, n=2000)
    pairs, counts, offsets, q, t, valid, has3d, _ = scenario(40, 3)
    import dot_cases as DC
    u8, _ = synth.make_frame_descriptors(synth.make_scene(4, 1200, 4, seed=9), 300, 128, seed=9)
    f32, ordered = DC.scene("d64"), DC.ordered_pairs(4)
    sep_src = torch.zeros(SEP, dtype=torch.uint8)
    with HipContext(0) as ctx:
        rg = G.ResidentGraph(ctx, 40, pairs, counts, offsets, q, t, [len(a) for a in has3d])
        pts = tri.triangulate_tracks(ctx, tr["transforms"], tr["track_ptr"], tr["obs_frame"], tr["obs_uv"], tr["K"], 4.0, 0.0175)[0]
        fns = [lambda: score.solve_minimal(ctx, "homography4", lc["uv1"][3], lc["uv2"][3], lc["samples"][3]),
               lambda: score.solve_pnp(ctx, pn["X"], pn["uv"], pn["K"], samples),
               lambda: score.score_hypotheses(ctx, "pnp", pn["X"], pn["uv"], pn["models"], pn["K"], 16.0),
               lambda: tri.triangulate_tracks(ctx, tr["transforms"], tr["track_ptr"], tr["obs_frame"], tr["obs_uv"], tr["K"], 4.0, 0.0175),
               lambda: tri.reprojection_errors(ctx, tr["transforms"], np.asarray(tr["obs_frame"])[first], pts[:len(first)],
                                               np.asarray(tr["obs_uv"]).reshape(-1, 2)[first], tr["K"]),
               lambda: tri.two_view_points(ctx, uv1, uv2, K, Ts, 4.0, 0.0175, True),
               lambda: ctx.two_view_batch(tc["uv1"], tc["uv2"], tc["K"], tc["rules"], tc["transforms"], tc["max_err"], tc["min_angle"]),
               lambda: ctx.lmeds_batch("homography", lc["uv1"], lc["uv2"], lc["samples"], lc["K"]),
               lambda: rg.set_frames(list(range(7)), [valid[f] for f in range(7)], [has3d[f] for f in range(7)]),
               lambda: ctx.match_all_pairs(ordered, 0.8, 1, 0),
               lambda: ctx.match_all_pairs(ordered, 0.8, 1, 0, stats=False),
               lambda: ctx.match_pair(0, 1),
               lambda: G.best_pair_for_valid(ctx, 40, pairs, counts, offsets, q, t, valid, has3d)]
        for f, d in enumerate(u8):
            ctx.upload_descriptors(f, d)
        for f in fns:
            f()
        for f in fns:
            sep_src.cuda()
            torch.cuda.synchronize()
            f()
        sep_src.cuda()
        torch.cuda.synchronize()
        rg.close()
    with HipContext(0) as ctx:           # float frames cannot be resident beside int8 ones: a context of its own
        for f, d in enumerate(f32):
            ctx.upload_descriptors_f32(f, d)
        for _ in range(2):               # the warm-up call closes the segment of the context change, the second call is the one counted
            ctx.match_all_pairs_dot(ordered, 0.5, 0, -1)
            sep_src.cuda()
            torch.cuda.synchronize()


def table(d):
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    key = lambda r: int(r.get("Start_Timestamp") or r.get("Start"))                     # noqa: E731
    size = lambda r: int(r.get("Size") or r.get("Bytes") or 0)                           # noqa: E731
    rows.sort(key=key)
    segs, cur = [], None
    for r in rows:
        if size(r) == SEP:
            if cur is not None:
                segs.append(cur)
            cur = []
        elif cur is not None:
            cur.append((r.get("Direction", "?").replace("MEMORY_COPY_", ""), size(r)))
    return segs


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--table":
        for d in sys.argv[2:]:
            segs = table(d)
            print(f"{d}: {len(segs)} calls")
            for name, seg in zip(NAMES, segs):
                print(f"  {name:22s} {len(seg)} copies: " + ", ".join(f"{a} {b}" for a, b in seg))
    else:
        calls()
