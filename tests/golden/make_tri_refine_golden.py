"""Writes tests/golden/tri_refine_golden.npz: track refinement problems with the minimiser of their reprojection error at 60 digits
(tests/tri_refine_mp_reference.py, mpmath). Run from the repository root: python tests/golden/make_tri_refine_golden.py

  the first COUNT tracks of tri_refine_cases.seeded(): 2..17 views, baselines 0.05 / 0.2 / 1 against depths 4..9, 0 and 1 px of noise,
  starts at the first pair's DLT point (noisy) or 1 / 3 / 5 % of the depth off (exact)
  track_ptr [n + 1], T [sum, 16] (the transform of each observation), uv [sum, 2], X0 [n, 3] (the start), X [n, 3] (the truth)
  minimiser [n, 3]: the 60-digit minimiser (Newton on the gradient from X until max |F| < 1e-50), rounded to double; min_cost [n]
  deviation: the restatement's largest distance from the minimiser, max |X - X*| / (1 + max |X*|), over its converged tracks (all of
  them here); bound = 8 deviation (the rule of the PnP refinement's golden file), what tests/test_tri_refine_reference.py holds
  every converged track to."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import tri_refine_cases as RC          # noqa: E402
import tri_refine_mp_reference as MP   # noqa: E402
import tri_refine_reference as R       # noqa: E402

COUNT = 80


def distance(X, Xmin):
    return np.abs(X - Xmin).max(1) / (1 + np.abs(Xmin).max(1))


def build():
    cases = RC.seeded()[:COUNT]
    mins, costs = [], []
    for k, c in enumerate(cases):
        X, cost, it, size = MP.minimise(c["T"], c["uv"], RC.K, c["X"])
        print(f"track {k}: {c['m']} views, noise {c['noise']}, {it} Newton steps, max |F| {size:.1e}, cost {cost:.6g}", flush=True)
        mins.append(X), costs.append(cost)
    mins = np.array(mins)
    out = R.refine_tracks(*RC.args(RC.pack(cases), with_mask=False))
    assert (out.status == R.CONVERGED).all(), np.bincount(out.status)
    dev = float(distance(out.refined, mins).max())
    assert 8 * dev <= 1e-6, dev
    ptr = np.zeros(len(cases) + 1, np.int64)
    np.cumsum([c["m"] for c in cases], out=ptr[1:])
    return dict(track_ptr=ptr, T=np.concatenate([c["T"] for c in cases]), uv=np.concatenate([c["uv"] for c in cases]),
                X0=np.array([c["X0"] for c in cases]), X=np.array([c["X"] for c in cases]), K=RC.K, minimiser=mins, min_cost=np.array(costs),
                deviation=np.float64(dev), bound=np.float64(8 * dev))


if __name__ == "__main__":
    g = build()
    np.savez_compressed(RC.GOLDEN, **g)
    print(f"{RC.GOLDEN}: {os.path.getsize(RC.GOLDEN)} bytes, {len(g['X'])} tracks, deviation {float(g['deviation']):.3e}, bound {float(g['bound']):.3e}")
