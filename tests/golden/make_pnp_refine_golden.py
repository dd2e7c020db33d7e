"""Writes tests/golden/pnp_refine_golden.npz: PnP refinement problems with the minimiser of their reprojection error at 60 digits
(tests/pnp_refine_mp_reference.py, mpmath). Run from the repository root: python tests/golden/make_pnp_refine_golden.py

  the first COUNT problems of pnp_refine_cases.seeded(): 3..300 points, planar scenes, 0 and 1 px of noise, starts 0.01 / 0.05 / 0.2 off
  point_ptr [P + 1], X [sum, 3], uv [sum, 2], T0 [P, 12] (the start), T [P, 12] (the true pose)
  minimiser [P, 12]: the 60-digit minimiser (Newton on the gradient from T until max |F| < 1e-50), rounded to double; min_cost [P]
  deviation: the restatement's largest max-abs distance from the minimiser over its converged problems (all of them here);
  bound = 8 deviation (the rule of the P3P golden file), what tests/test_pnp_refine_reference.py holds every converged problem to."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import pnp_refine_cases as RC          # noqa: E402
import pnp_refine_mp_reference as MP   # noqa: E402
import pnp_refine_reference as R       # noqa: E402
from eacham_amd import pnp             # noqa: E402

COUNT = 52


def build():
    cases = RC.seeded()[:COUNT]
    X, uv, T0, has = RC.lists(cases)
    T = np.array([c["T"] for c in cases])
    mins, costs = [], []
    for k, c in enumerate(cases):
        M, cost, it, size = MP.minimise(c["X"], c["uv"], RC.K, c["T"])
        print(f"case {k}: {c['n']} points, noise {c['noise']}, {it} Newton steps, max |F| {size:.1e}, cost {cost:.6g}", flush=True)
        mins.append(M), costs.append(cost)
    mins = np.array(mins)
    out = R.refine_batch(X, uv, RC.K, T0, has)
    assert (out.status == R.CONVERGED).all(), np.bincount(out.status)
    dev = float(np.abs(out.refined - mins).max())
    assert 8 * dev <= 1e-5, dev
    point_ptr, A, B = pnp.pack_points(X, uv)
    return dict(point_ptr=point_ptr, X=A, uv=B, T0=T0, T=T, K=RC.K, minimiser=mins, min_cost=np.array(costs), deviation=np.float64(dev),
                bound=np.float64(8 * dev))


if __name__ == "__main__":
    g = build()
    np.savez_compressed(RC.GOLDEN, **g)
    print(f"{RC.GOLDEN}: {os.path.getsize(RC.GOLDEN)} bytes, {len(g['T'])} problems, deviation {float(g['deviation']):.3e}, bound {float(g['bound']):.3e}")
