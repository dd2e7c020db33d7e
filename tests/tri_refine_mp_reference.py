"""The MINIMISER of the reprojection error of a track's point at 60 digits (mpmath), and the derivative of one residual: what the
restatement (tests/cpp/tri_refine_reference.c) and through it the kernel are held to. Test infrastructure; needed only where the
golden file is made or re-derived (tests/golden/make_tri_refine_golden.py; tests/test_tri_refine_reference.py re-derives two tracks
and the Jacobians) — the other tests read the file.

The inputs are the doubles taken exactly. The minimiser is found by Newton's iteration on the gradient F(X) = sum J'r, started at the
true point: the 3 x 3 derivative of F by forward differences of 1e-25, the step by LU, until max |F| < 1e-50."""
import mpmath as mp
import numpy as np

DIGITS = 60
STOP = mp.mpf("1e-50")
STEP = mp.mpf("1e-25")


def _mpf(a):
    return [mp.mpf(float(x)) for x in np.asarray(a, dtype=np.float64).reshape(-1)]


def _camera(T, X):
    return tuple(T[4 * r] * X[0] + T[4 * r + 1] * X[1] + T[4 * r + 2] * X[2] + T[4 * r + 3] for r in range(3))


def _residual(T, u, X, K):
    x, y, z = _camera(T, X)
    return K[0] * x / z + K[2] - u[0], K[1] * y / z + K[3] - u[1]


def jacobian(T, uv, X, K):
    """d r / d X for one observation, [2, 3] as doubles: numerical differentiation at 60 digits."""
    with mp.workdps(DIGITS):
        Tm, um, Xm, Km = _mpf(T), _mpf(uv), _mpf(X), _mpf(K)
        J = np.zeros((2, 3))
        for k in range(3):
            for c in range(2):
                f = lambda s, k=k, c=c: _residual(Tm, um, [Xm[e] + (s if e == k else 0) for e in range(3)], Km)[c]   # noqa: E731
                J[c, k] = float(mp.diff(f, 0))
        return J


def _gradient(X, Ts, us, K):
    """(F [3] = sum J'r, cost = sum r'r): J by the chain rule, d r / d X_c times d X_c / d X = R."""
    F = [mp.mpf(0)] * 3
    cost = mp.mpf(0)
    for T, u in zip(Ts, us):
        x, y, z = _camera(T, X)
        r0, r1 = K[0] * x / z + K[2] - u[0], K[1] * y / z + K[3] - u[1]
        cost += r0 * r0 + r1 * r1
        e = (K[0] / z * r0, K[1] / z * r1, -(K[0] * x * r0 + K[1] * y * r1) / (z * z))   # (d r / d X_c)' r
        F = [F[j] + (T[j] * e[0] + T[4 + j] * e[1] + T[8 + j] * e[2]) for j in range(3)]   # R' e
    return F, cost


def minimise(T, uv, K, X0, max_iter=40):
    """(point [3] as doubles, cost at it as a double, iterations, max |F| as a float) from the start X0."""
    with mp.workdps(DIGITS):
        Ts = [_mpf(t) for t in np.asarray(T, dtype=np.float64).reshape(-1, 16)]
        us = [_mpf(u) for u in np.asarray(uv, dtype=np.float64).reshape(-1, 2)]
        Km, X = _mpf(K), _mpf(X0)
        for it in range(max_iter):
            F, cost = _gradient(X, Ts, us, Km)
            size = max(abs(f) for f in F)
            if size < STOP:
                return np.array([float(x) for x in X]), float(cost), it, float(size)
            A = mp.matrix(3, 3)
            for k in range(3):
                Fk, _ = _gradient([X[e] + (STEP if e == k else 0) for e in range(3)], Ts, us, Km)
                for r in range(3):
                    A[r, k] = (Fk[r] - F[r]) / STEP
            d = mp.lu_solve(A, mp.matrix([-f for f in F]))
            X = [X[k] + d[k] for k in range(3)]
        raise RuntimeError(f"no minimiser within {max_iter} Newton steps (max |F| = {mp.nstr(size, 5)})")
