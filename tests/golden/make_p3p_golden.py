"""Writes tests/golden/p3p_golden.npz: the P3P samples the CPU restatement and the kernels are held on, with their solution set at
60 digits (tests/p3p_mp_reference.py, mpmath). Run from the repository root: python tests/golden/make_p3p_golden.py

  256 samples of the scene generator of tests/p3p_cases.py (exact pixels), 32 of planar scenes, 32 with 1 px of noise  (kind 0, 1, 2)
  X, uv [4 S, .], samples [S, 4], T [S, 12] (the true pose; of the noisy samples: the pose before the noise)
  mp_count [S], mp_ptr [S + 1], mp_candidates [sum, 12]: the 60-digit positive-depth poses rounded to double, in ascending v
  decided [S]: the 60-digit solution set is clear of every threshold of the definition (p3p_mp_reference.solve says which)
  deviation: the restatement's largest max-abs distance from its 60-digit counterpart over the decided samples;
  bound = 8 deviation (the convention of tests/tri_hard_rules.py), what tests/test_p3p_reference.py holds every candidate to."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import p3p_cases as PC          # noqa: E402
import p3p_mp_reference as MP   # noqa: E402
import p3p_reference as R       # noqa: E402

SETS = ((256, 101, False, 0.0), (32, 102, True, 0.0), (32, 103, False, 1.0))   # count, seed, planar, noise px


def build():
    parts = [PC.scenes(*s) for s in SETS]
    X, uv, T = (np.concatenate([p[k] for p in parts]) for k in (0, 1, 3))
    S = len(T)
    samples = np.arange(4 * S, dtype=np.int32).reshape(S, 4)
    kind = np.concatenate([np.full(s[0], k, np.int32) for k, s in enumerate(SETS)])
    cands, decided = zip(*(MP.solve(X[4 * s:4 * s + 4], uv[4 * s:4 * s + 4], PC.K) for s in range(S)))
    decided = np.array(decided, dtype=np.uint8)
    count = np.array([len(c) for c in cands], dtype=np.int32)
    ptr = np.zeros(S + 1, np.int64)
    np.cumsum(count, out=ptr[1:])
    _, _, rc, rn = R.solve_p3p(X, uv, PC.K, samples)
    dev = 0.0
    for s in np.nonzero(decided)[0]:
        assert rn[s] == count[s], f"sample {s}: the restatement has {rn[s]} candidates, the 60-digit set {count[s]}"
        if count[s]:
            dev = max(dev, float(np.abs(rc[s, :count[s]] - cands[s]).max()))
    undecided = S - int(decided.sum())
    assert undecided <= 0.02 * S, f"{undecided} of {S} samples undecided"
    assert 8 * dev <= 1e-8, dev
    return dict(X=X, uv=uv, samples=samples, T=T, kind=kind, K=PC.K, mp_count=count, mp_ptr=ptr, mp_candidates=np.concatenate(cands),
                decided=decided, deviation=np.float64(dev), bound=np.float64(8 * dev))


if __name__ == "__main__":
    g = build()
    np.savez_compressed(PC.GOLDEN, **g)
    print(f"{PC.GOLDEN}: {os.path.getsize(PC.GOLDEN)} bytes, {len(g['T'])} samples, {len(g['T']) - int(g['decided'].sum())} undecided, "
          f"deviation {float(g['deviation']):.3e}, bound {float(g['bound']):.3e}, counts {np.bincount(g['mp_count']).tolist()}")
