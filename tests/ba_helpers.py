"""What the bundle-adjustment test files share: the error measures, the context factory and the oracle's Schur-against-dense
check. Test infrastructure (tests/test_ba_gpu.py, tests/test_ba_oracle.py, tests/test_ba_ragged_*.py)."""
import os

import numpy as np


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def backward_error(S, g, x):
    """Normwise backward error of x as a solution of S x = g, ||S x - g|| / (||S|| ||x|| + ||g||) in infinity norms, evaluated
    in extended precision: it judges a step by the system alone, whatever algorithm produced it."""
    S, g, x = (np.asarray(v, dtype=np.longdouble) for v in (S, g, x))
    r = S @ x - g
    return float(np.abs(r).max() / (np.abs(S).sum(axis=1).max() * np.abs(x).max() + np.abs(g).max()))


def ctx_with(**env):
    """A context of its own created under the given environment switches (they are read once, at eacham_ctx_create)."""
    from eacham_amd import HipContext
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        return HipContext(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def schur_step_equals_dense_step(A, lam):
    """The oracle's step through the Schur complement against its dense solve of ALL variables (cameras, K, landmarks) of the
    same damped system. Returns the Schur form's (S, g, dc, dl, error, lin_change, ok)."""
    import oracle_api as O
    S, g, dc, dl, err, lin, ok = O.ba_step(A, lam, 0)
    S2, g2, dc2, dl2, err2, lin2, ok2 = O.ba_step(A, lam, 1)
    assert ok and ok2
    scale = max(np.abs(dc2).max(), 1e-12)
    assert np.abs(dc - dc2).max() < 1e-9 * scale and np.abs(dl - dl2).max() < 1e-9 * max(np.abs(dl2).max(), 1e-12)
    assert np.isclose(lin, lin2, rtol=1e-9) and lin > 0 and np.isclose(err, err2, rtol=1e-12)  # OpenMP sum order
    assert np.allclose(S, S.T, rtol=0, atol=1e-9 * np.abs(S).max())
    # the reduced system reproduces the camera part of the step
    assert np.allclose(np.linalg.solve(S, g), dc, rtol=1e-7, atol=1e-10)
    return S, g, dc, dl, err, lin, ok
