"""Writes tests/golden/essential5_golden.npz: the five-point samples the CPU restatement (oracle/solve_oracle.c) and the kernels are held
on, with their solution set at 60 digits (tests/essential5_mp_reference.py, mpmath). Run from the repository root:
python tests/golden/make_essential5_golden.py   (about five CPU-minutes, spread over the cores)

  the 8 scenes of tests/essential5_cases.py, 64 samples each
  uv1, uv2 [8 N, 2], samples [512, 5], scene [512], K, E_true [8, 9] (of the noisy scenes: the motion before the noise)
  mp_count [512], mp_ptr [513], mp_models [sum, 9]: the 60-digit solutions rounded to double (unit norm, largest entry positive)
  decided [512]: the 60-digit solution set is clear of every threshold of the definition (essential5_mp_reference.py says which)
  deviation: the restatement's largest max-abs distance, up to sign, from its 60-digit counterpart over the decided samples;
  bound = 8 deviation (the convention of tests/tri_hard_rules.py and the P3P fixture), what the tests hold every model to
  dropped_before [8]: per scene the decided samples on which the restatement returned FEWER models than mp_count under its
      former root rules — degree drop, start circle, stop test against the root bound; the same source compiled with
      -DSOLVE_ORACLE_ROOTS_BEFORE — : the fixture sees that defect."""
import multiprocessing
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import essential5_cases as EC          # noqa: E402
import essential5_mp_reference as MP   # noqa: E402
import oracle_api as O                 # noqa: E402


def _mp(args):
    return MP.solve(*args)


def restatement_before(uv1, uv2, samples):
    """Model counts of oracle_essential5 with the root finder's former rules."""
    import ctypes as C
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "libsolve_before.so")
        subprocess.run([os.environ.get("CC", "gcc"), "-O3", "-march=native", "-fopenmp", "-fPIC", "-std=c11", "-fno-fast-math", "-DSOLVE_ORACLE_ROOTS_BEFORE",
                        "-shared", "-o", so, os.path.join(ROOT, "oracle", "solve_oracle.c"), "-lm"], check=True)
        L = C.CDLL(so)
        models, counts = np.zeros((len(samples), 10, 9)), np.zeros(len(samples), np.int32)
        vp = C.c_void_p
        L.oracle_solve_minimal.restype = None
        L.oracle_solve_minimal(C.c_int(1), vp(uv1.ctypes.data), vp(uv2.ctypes.data), vp(EC.K.ctypes.data), C.c_int(len(samples)), vp(samples.ctypes.data),
                               vp(models.ctypes.data), vp(counts.ctypes.data))
    return counts


def build():
    uv1, uv2, samples, scene, E_true = EC.all_scenes()
    n = len(samples)
    with multiprocessing.Pool(min(os.cpu_count() or 1, 16)) as pool:
        sols, decided = zip(*pool.map(_mp, [(uv1[s], uv2[s], EC.K) for s in samples], chunksize=4))
    decided = np.array(decided, dtype=np.uint8)
    count = np.array([len(e) for e in sols], dtype=np.int32)
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(count, out=ptr[1:])
    assert (count % 2 == 0).all(), "the real roots of a real degree-10 polynomial come in pairs"
    undecided = n - int(decided.sum())
    assert undecided <= 0.05 * n, f"{undecided} of {n} samples undecided"
    models, rn = O.solve_minimal("essential5", uv1, uv2, samples, EC.K)
    before = restatement_before(uv1, uv2, samples)
    dev, mismatch = 0.0, 0
    for s in np.nonzero(decided)[0]:
        worst, pairs = EC.match_sets(models[s, :rn[s]], sols[s])
        if rn[s] != count[s] or pairs != count[s]:
            mismatch += 1
            print(f"sample {s} ({EC.NAMES[scene[s]]}): the restatement has {rn[s]} models, the 60-digit set {count[s]}")
            continue
        dev = max(dev, worst)
    dropped = np.array([int(((before < count) & (decided != 0) & (scene == k)).sum()) for k in range(len(EC.SCENES))], dtype=np.int32)
    print("decided samples on which the former root rules lost solutions:", dict(zip(EC.NAMES, dropped.tolist())),
          f"— {int(dropped[list(EC.HARD)].sum())} on the near-planar and short-baseline scenes")
    print(f"decided samples with a count mismatch now: {mismatch}")
    assert dropped[list(EC.HARD)].sum() >= 5
    assert mismatch == 0
    return dict(uv1=uv1, uv2=uv2, samples=samples, scene=scene, K=EC.K, E_true=E_true, mp_count=count, mp_ptr=ptr, mp_models=np.concatenate(sols),
                decided=decided, deviation=np.float64(dev), bound=np.float64(8 * dev), dropped_before=dropped)


if __name__ == "__main__":
    g = build()
    np.savez_compressed(EC.GOLDEN, **g)
    print(f"{EC.GOLDEN}: {os.path.getsize(EC.GOLDEN)} bytes, {len(g['samples'])} samples, {len(g['samples']) - int(g['decided'].sum())} undecided, "
          f"deviation {float(g['deviation']):.3e}, bound {float(g['bound']):.3e}, counts {np.bincount(g['mp_count']).tolist()}")
