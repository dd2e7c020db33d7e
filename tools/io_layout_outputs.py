"""Every output of the host-pointer entry points that stage through IoStage, as raw bytes, for a before/after run of two
builds of the library (EACHAM_HIP_LIB selects the build; each build needs a process of its own):

    EACHAM_HIP_LIB=<parent build> python tools/io_layout_outputs.py --dump /tmp/parent.npz
    python tools/io_layout_outputs.py --dump /tmp/new.npz
    python tools/io_layout_outputs.py --compare /tmp/parent.npz /tmp/new.npz [--out profiles/io_layout_parent_vs_new.txt]

Inputs: the cases of tests/two_view_batch_cases.py (eacham_two_view_batch, and eacham_two_view_points problem by problem), the
cases of tests/lmeds_batch_cases.py in their three variants (eacham_lmeds_batch, and eacham_solve_minimal +
eacham_score_hypotheses problem by problem), tests/test_tri_oracle.py's two-view case (seed 5, 2000 matches, both angle rules), one
synth.make_tracks scene (eacham_triangulate_tracks, eacham_reprojection_errors), one PnP batch (eacham_solve_pnp,
eacham_score_hypotheses), the resident graph after eacham_graph_set_frames (its query's answer), eacham_graph_best_pair on the
same scenario (with and without an excluded mask), eacham_pnp_hypotheses_batch on the HYP_CASES of tests/pnp_batch_cases.py and
eacham_pnp_refit_batch on its refit_case(), eacham_graph_verify on the graphs of tests/graph_verify_cases.py (both kinds, both sample
streams) and the matching calls: eacham_match_pair / _match_all_pairs (with and
without stats) / _match_pairs_directed on int8 frames and on float frames, the four dot-product calls on the float frames, each on
a 12-pair list and on a list long enough for the direct copies (33 000 pairs); the Hamming calls — pair, directed, all pairs with
and without stats, and the device-pointer form with distances — on binary frames of 32 bytes per row and on wide ones of 64.
--matching with --dump leaves out everything but the matching calls, --staged the matching calls."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def dump(path, only_matching=False, only_staged=False):
    import torch
    torch.cuda.init()   # (before the library touches the device: the device-pointer calls below hand it torch tensors)
    out = {}

    def put(name, *arrays):
        for k, a in enumerate(arrays):
            a = np.ascontiguousarray(a)
            out[f"{name}/{k}"] = np.frombuffer(a.tobytes(), np.uint8)

    if not only_matching:
        staged(put)
    if not only_staged:
        matching(put)
    np.savez(path, **out)
    print(f"{len(out)} arrays, {sum(a.size for a in out.values())} bytes -> {path}")


def staged(put):
    from eacham_amd import HipContext, score, synth, triangulate as tri
    from eacham_amd import capi, graph as G
    import graph_verify_cases as GC
    import lmeds_batch_cases as LC
    import pnp_batch_cases as PC
    import score_cases as SC
    import two_view_batch_cases as TC
    from test_graph_oracle import scenario
    from test_tri_oracle import _two_view_case

    with HipContext(0) as ctx:
        for name, make in TC.CASES.items():
            c = make()
            g = ctx.two_view_batch(c["uv1"], c["uv2"], c["K"], c["rules"], c["transforms"], c["max_err"], c["min_angle"], c["in_mask"], c["dist"],
                                   c["min_solution_matches"])
            put(f"two_view_batch/{name}", g.winner, g.good, g.kept, *g.cand_counts, *g.points, *g.keep, *g.pose_mask)
            for p in range(len(c["uv1"])):
                if len(c["transforms"][p]):
                    for strict in (False, True):
                        put(f"two_view_points/{name}/{p}/{int(strict)}",
                            *tri.two_view_points(ctx, c["uv1"][p], c["uv2"][p], c["K"], c["transforms"][p], c["max_err"], c["min_angle"], strict))
        for name, make in LC.CASES.items():
            for variant in ("homography", "essential", "essential_noK"):
                c = make(variant.split("_")[0])
                if variant.endswith("noK"):
                    c = LC.normalised(c)
                g = ctx.lmeds_batch(c["kind"], c["uv1"], c["uv2"], c["samples"], c["K"])
                put(f"lmeds_batch/{name}/{variant}", g.models, g.medians, g.thresholds, g.inliers, *g.masks, g.winner, g.n_candidates)
                solver = "homography4" if c["kind"] == "homography" else "essential5"
                for p in range(len(c["uv1"])):
                    if len(c["samples"][p]) == 0:
                        continue
                    models, nm = score.solve_minimal(ctx, solver, c["uv1"][p], c["uv2"][p], c["samples"][p], c["K"])
                    put(f"solve_minimal/{name}/{variant}/{p}", models, nm)
                    cand = np.concatenate([models[s, :nm[s]] for s in range(len(nm))]).reshape(-1, 9)
                    if len(cand):
                        put(f"score/{name}/{variant}/{p}", *score.score_hypotheses(ctx, c["kind"], c["uv1"][p], c["uv2"][p], cand, c["K"], 1e-4))
                        put(f"score_medians_only/{name}/{variant}/{p}",
                            *score.score_hypotheses(ctx, c["kind"], c["uv1"][p], c["uv2"][p], cand, c["K"], 0.0, want_errors=False)[1:])
        uv1, uv2, K, Ts = _two_view_case(seed=5, n=2000)
        for strict in (True, False):
            put(f"two_view_points/seed5/{int(strict)}", *tri.two_view_points(ctx, uv1, uv2, K, Ts, 4.0, float(np.deg2rad(1.0)), strict))
        sc = synth.make_scene(12, 600, 6, seed=7)
        tr = synth.make_tracks(sc, seed=7, min_obs=2, outlier_frac=0.3)
        pts, status, masks = tri.triangulate_tracks(ctx, tr["transforms"], tr["track_ptr"], tr["obs_frame"], tr["obs_uv"], tr["K"], 4.0,
                                                    float(np.deg2rad(1.0)))
        put("triangulate_tracks", pts, status, masks)
        first = np.asarray(tr["track_ptr"][:-1])
        keep = np.diff(tr["track_ptr"]) > 0
        put("reprojection_errors", tri.reprojection_errors(ctx, tr["transforms"], np.asarray(tr["obs_frame"])[first[keep]], pts[keep],
                                                           np.asarray(tr["obs_uv"]).reshape(-1, 2)[first[keep]], tr["K"]))
        c = SC.pnp_case(n=800, n_models=64, seed=17)
        rng = np.random.default_rng(17)
        for size in (5, 6, 100):                                          # the loop's sample sizes, and the all-inlier refit's form
            samples = np.array([rng.choice(800, size=size, replace=False) for _ in range(300)], np.int32)
            models, ok = score.solve_pnp(ctx, c["X"], c["uv"], c["K"], samples)
            put(f"solve_pnp/{size}", models, ok)
            put(f"score_pnp/{size}", *score.score_hypotheses(ctx, "pnp", c["X"], c["uv"], models, c["K"], 16.0))
        pairs, counts, offsets, q, t, valid, has3d, excluded = scenario(40, 3)
        rg = G.ResidentGraph(ctx, 40, pairs, counts, offsets, q, t, [len(a) for a in has3d])
        try:
            for lo in range(0, 40, 7):
                fr = list(range(lo, min(lo + 7, 40)))
                rg.set_frames(fr, [valid[f] for f in fr], [has3d[f] for f in fr])
                put(f"graph_set_frames/{lo}", np.array(rg.query(), np.int64), np.array(rg.query(np.nonzero(excluded)[0]), np.int64))
        finally:
            rg.close()
        for ex in (None, excluded):
            best, ec = G.best_pair_for_valid(ctx, 40, pairs, counts, offsets, q, t, valid, has3d, ex, want_edge_counts=True)
            put(f"graph_best_pair/{int(ex is not None)}", np.array(best, np.int64), ec)
        for name, make in PC.HYP_CASES.items():
            c = make()
            g = ctx.pnp_hypotheses_batch(c["X"], c["uv"], c["K"], c["samples"], PC.THR)
            put(f"pnp_hypotheses_batch/{name}", *g.models, *g.n_models, *g.inlier_counts)
        c = PC.refit_case()
        g = ctx.pnp_refit_batch(c["X"], c["uv"], c["K"], c["models"], c["has_model"], PC.THR)
        put("pnp_refit_batch", *g.masks, g.n_inliers, g.refit, g.refit_ok)
        for name, its in (("small", 72), ("small", 89), ("large", 3), ("eight", 89)):
            gr = getattr(GC, name)()
            rg = G.ResidentGraph(ctx, gr["n_frames"], gr["pairs"], gr["counts"], gr["offsets"], gr["q"], gr["t"], gr["n_kp"])
            try:
                rg.set_keypoints(gr["xy"])
                for kind, m in (("homography", 4), ("essential", 5)):
                    for sampling in (capi.SAMPLING_OPENCV, capi.SAMPLING_COUNTER):
                        got = rg._verify_raw(capi.SOLVE_HOMOGRAPHY4 if m == 4 else capi.SOLVE_ESSENTIAL5, m, GC.K4 if m == 5 else None, sampling, its,
                                             gr["seeds"], False, True, preset=0x55)
                        put(f"graph_verify/{name}/{its}/{kind}/{sampling}", got.models, got.medians, got.thresholds, got.inliers, got.masks,
                            got.winner, got.n_candidates, got.n_samples, got.samples)
            finally:
                rg.close()


def matching(put):
    """The matching calls (eacham_amd/csrc/matcher.hip), each build in a context of its own per descriptor kind."""
    import ctypes as C
    from eacham_amd import HipContext, synth
    import dot_cases as DC
    ordered = DC.ordered_pairs(4)
    long = ordered[np.arange(33000) % 12]

    def directed(ctx, pr):
        counts, offsets = np.zeros(len(pr), np.int32), np.zeros(len(pr) + 1, np.int64)
        cap = 300 * len(pr)
        q, t, total = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), C.c_int64(0)
        pr = np.ascontiguousarray(pr, np.int32)
        ctx._check(ctx._L.eacham_match_pairs_directed(ctx.handle, pr.ctypes.data, len(pr), 0.8, counts.ctypes.data, offsets.ctypes.data,
                                                      q.ctypes.data, t.ctypes.data, cap, C.byref(total)))
        return counts, offsets, q[:total.value], t[:total.value]

    sc = synth.make_scene(4, 1200, 4, seed=9)
    u8, _ = synth.make_frame_descriptors(sc, 300, 128, seed=9)
    f32 = DC.float_frames(64, [300, 237, 150, 97], 80, 101)
    for kind, descs in (("i8", u8), ("f32", f32)):
        with HipContext(0) as ctx:
            for f, d in enumerate(descs):
                (ctx.upload_descriptors if kind == "i8" else ctx.upload_descriptors_f32)(f, d)
            for a, b in ordered:
                put(f"match_pair/{kind}/{a}_{b}", *ctx.match_pair(int(a), int(b)))
            for tag, pr in (("12", ordered), ("33000", long if kind == "i8" else long[:6000])):
                for md, mm in ((30, 30), (1, 0)):
                    put(f"match_all_pairs/{kind}/{tag}/{md}_{mm}", *ctx.match_all_pairs(pr, 0.8, md, mm))
                    put(f"match_all_pairs_nostats/{kind}/{tag}/{md}_{mm}", *ctx.match_all_pairs(pr, 0.8, md, mm, stats=False)[:4])
                put(f"match_pairs_directed/{kind}/{tag}", *directed(ctx, pr))
            if kind == "f32":
                for a, b in ordered:
                    put(f"match_pair_dot/{a}_{b}", *ctx.match_pair_dot(int(a), int(b), 0.5))
                for tag, pr in (("12", ordered), ("6000", long[:6000])):
                    put(f"match_pairs_directed_dot/{tag}", *ctx.match_pairs_directed_dot(pr, 0.5))
                    for screened in (False, True):
                        name = "match_all_pairs_dot_screened" if screened else "match_all_pairs_dot"
                        put(f"{name}/{tag}", *ctx.match_all_pairs_dot(pr, 0.5, 0, -1, screened=screened))
                        put(f"{name}_nostats/{tag}", *ctx.match_all_pairs_dot(pr, 0.5, 5, 5, stats=False, screened=screened)[:5])
    import torch
    import ham_cases as HC
    dev = torch.device("cuda", 0)
    for kind, nbytes in (("bits", 32), ("wide", 64)):
        descs = HC.binary_frames(nbytes, [300, 237, 150, 97], 120, 13)
        with HipContext(0) as ctx:
            for f, d in enumerate(descs):
                (ctx.upload_descriptors_bits if kind == "bits" else ctx.upload_descriptors_bits_wide)(f, d)
            for a, b in ordered:
                put(f"match_pair_hamming/{kind}/{a}_{b}", *ctx.match_pair_hamming(int(a), int(b), 0.8))
            for tag, pr in (("12", ordered), ("6000", long[:6000])):
                put(f"match_pairs_directed_hamming/{kind}/{tag}", *ctx.match_pairs_directed_hamming(pr, 0.8))
                for md, mm in ((30, 30), (1, 0)):
                    put(f"match_all_pairs_hamming/{kind}/{tag}/{md}_{mm}", *ctx.match_all_pairs_hamming(pr, 0.8, md, mm))
                    put(f"match_all_pairs_hamming_nostats/{kind}/{tag}/{md}_{mm}", *ctx.match_all_pairs_hamming(pr, 0.8, md, mm, stats=False)[:5])
            cap = 300 * len(ordered)
            with torch.cuda.stream(torch.cuda.ExternalStream(ctx.stream, device=dev)):
                for with_stats in (True, False):
                    pd = torch.from_numpy(np.ascontiguousarray(ordered)).to(dev)
                    counts = torch.full((len(ordered),), -1, dtype=torch.int32, device=dev)
                    offsets = torch.zeros(len(ordered) + 1, dtype=torch.int64, device=dev)
                    total = torch.zeros(1, dtype=torch.int64, device=dev)
                    edges = torch.zeros(2 * cap, dtype=torch.int32, device=dev)
                    dist = torch.full((cap,), -7, dtype=torch.int32, device=dev)
                    st = torch.zeros(4 * len(ordered), dtype=torch.int32, device=dev)
                    ctx.sync()
                    ctx.match_all_pairs_hamming_dev(pd.data_ptr(), len(ordered), counts.data_ptr(), offsets.data_ptr(), edges.data_ptr(), cap,
                                                    total.data_ptr(), st.data_ptr() if with_stats else 0, dist.data_ptr(), ratio=0.8, min_dir=1, min_mutual=0)
                    ctx.sync()
                    put(f"match_all_pairs_hamming_dev/{kind}/{int(with_stats)}", *(x.cpu().numpy() for x in (counts, offsets, total, edges, dist, st)))


def compare(a_path, b_path, out_path):
    a, b = np.load(a_path), np.load(b_path)
    lines = [f"Outputs of the staged entry points, parent build against this one, as raw bytes ({os.path.basename(a_path)} vs {os.path.basename(b_path)})"]
    groups = {}
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        g = groups.setdefault(k.split("/")[0], [0, 0, 0])
        x, y = a[k], b[k]
        g[0] += 1
        g[1] += x.size
        g[2] += int((x != y).sum()) if x.size == y.size else max(x.size, y.size)
    for name, (n, size, diff) in groups.items():
        lines.append(f"  {name:22s} {n:5d} arrays {size:10d} bytes   differing bytes: {diff}")
    total = sum(g[2] for g in groups.values())
    lines.append(f"  arrays in one file only: {len(bad)}   differing bytes in all: {total}")
    print("\n".join(lines))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if total == 0 and not bad else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--out")
    ap.add_argument("--matching", action="store_true", help="with --dump: the matching calls only")
    ap.add_argument("--staged", action="store_true", help="with --dump: everything but the matching calls")
    args = ap.parse_args()
    if args.dump:
        dump(args.dump, args.matching, args.staged)
        sys.exit(0)
    sys.exit(compare(args.compare[0], args.compare[1], args.out))
