"""The MINIMISER of the reprojection error of a PnP problem at 60 digits (mpmath), and the derivative of one residual: what the
restatement (tests/cpp/pnp_refine_reference.c) and through it the kernel are held to. Test infrastructure; needed only where the
golden file is made or re-derived (tests/golden/make_pnp_refine_golden.py; tests/test_pnp_refine_reference.py re-derives two cases
and the Jacobians) — the other tests read the file.

The inputs are the doubles taken exactly. The minimiser is found by Newton's iteration on the gradient F(M) = sum J'r (in the chart
of the definition: X_c' = C(w) X_c + v with the Cayley map C), started at the true pose: the 6 x 6 derivative of F by forward
differences of 1e-25 in that chart, the step by LU, the pose updated by the exact retraction, until max |F| < 1e-50."""
import mpmath as mp
import numpy as np

DIGITS = 60
STOP = mp.mpf("1e-50")
STEP = mp.mpf("1e-25")


def _mpf(a):
    return [mp.mpf(float(x)) for x in np.asarray(a, dtype=np.float64).reshape(-1)]


def retract(M, d):
    """R <- C(w) R, t <- C(w) t + v; C(w) = ((4 - |w|^2) I + 2 w w' + 4 [w]x) / (4 + |w|^2)."""
    x, y, z = d[0], d[1], d[2]
    n2 = x * x + y * y + z * z
    f = 1 / (4 + n2)
    C = [f * (4 + x * x - y * y - z * z), f * 2 * (x * y - 2 * z), f * 2 * (x * z + 2 * y),
         f * 2 * (x * y + 2 * z), f * (4 - x * x + y * y - z * z), f * 2 * (y * z - 2 * x),
         f * 2 * (x * z - 2 * y), f * 2 * (y * z + 2 * x), f * (4 - x * x - y * y + z * z)]
    out = [None] * 12
    for r in range(3):
        for c in range(3):
            out[3 * r + c] = C[3 * r] * M[c] + C[3 * r + 1] * M[3 + c] + C[3 * r + 2] * M[6 + c]
        out[9 + r] = C[3 * r] * M[9] + C[3 * r + 1] * M[10] + C[3 * r + 2] * M[11] + d[3 + r]
    return out


def _camera(M, X):
    return tuple(M[3 * r] * X[0] + M[3 * r + 1] * X[1] + M[3 * r + 2] * X[2] + M[9 + r] for r in range(3))


def _residual(M, X, u, K):
    x, y, z = _camera(M, X)
    return K[0] * x / z + K[2] - u[0], K[1] * y / z + K[3] - u[1]


def jacobian(X, uv, M, K):
    """d r / d [w, v] at 0 of r(retract(M, [w, v])) for one correspondence, [2, 6] as doubles: numerical differentiation at 60 digits."""
    with mp.workdps(DIGITS):
        Xm, um, Mm, Km = _mpf(X), _mpf(uv), _mpf(M), _mpf(K)
        J = np.zeros((2, 6))
        for k in range(6):
            for c in range(2):
                f = lambda s, k=k, c=c: _residual(retract(Mm, [s if e == k else mp.mpf(0) for e in range(6)]), Xm, um, Km)[c]   # noqa: E731
                J[c, k] = float(mp.diff(f, 0))
        return J


def _gradient(M, Xs, us, K):
    """(F [6] = sum J'r, cost = sum r'r): J by the chain rule, d r / d X_c times d X_c / d [w, v] = [-[X_c]x | I]."""
    F = [mp.mpf(0)] * 6
    cost = mp.mpf(0)
    for X, u in zip(Xs, us):
        x, y, z = _camera(M, X)
        r0, r1 = K[0] * x / z + K[2] - u[0], K[1] * y / z + K[3] - u[1]
        cost += r0 * r0 + r1 * r1
        # e = (d r / d X_c)' r
        e = (K[0] / z * r0, K[1] / z * r1, -(K[0] * x * r0 + K[1] * y * r1) / (z * z))
        # (-[X_c]x)' e = X_c x e
        F = [F[0] + (y * e[2] - z * e[1]), F[1] + (z * e[0] - x * e[2]), F[2] + (x * e[1] - y * e[0]), F[3] + e[0], F[4] + e[1], F[5] + e[2]]
    return F, cost


def minimise(X, uv, K, T, max_iter=40):
    """(pose [12] as doubles, cost at it as a double, iterations, max |F| as a float) from the start T."""
    with mp.workdps(DIGITS):
        Xs = [_mpf(x) for x in np.asarray(X, dtype=np.float64).reshape(-1, 3)]
        us = [_mpf(u) for u in np.asarray(uv, dtype=np.float64).reshape(-1, 2)]
        Km, M = _mpf(K), _mpf(T)
        for it in range(max_iter):
            F, cost = _gradient(M, Xs, us, Km)
            size = max(abs(f) for f in F)
            if size < STOP:
                return np.array([float(m) for m in M]), float(cost), it, float(size)
            A = mp.matrix(6, 6)
            for k in range(6):
                Fk, _ = _gradient(retract(M, [STEP if e == k else mp.mpf(0) for e in range(6)]), Xs, us, Km)
                for r in range(6):
                    A[r, k] = (Fk[r] - F[r]) / STEP
            d = mp.lu_solve(A, mp.matrix([-f for f in F]))
            M = retract(M, [d[k] for k in range(6)])
        raise RuntimeError(f"no minimiser within {max_iter} Newton steps (max |F| = {mp.nstr(size, 5)})")
