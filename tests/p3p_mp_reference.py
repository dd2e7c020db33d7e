"""The SOLUTION SET of a P3P sample at 60 digits (mpmath): what the restatement (tests/cpp/p3p_reference.c) and through it the kernels
are held to where that set is decided. Test infrastructure; needed only where the golden file is made or re-derived
(tests/golden/make_p3p_golden.py, tests/test_p3p_reference.py skips its re-derivation without mpmath) — the GPU tests read the file.

It forms Grunert's quartic of include/eacham_hip.h from the double inputs taken exactly, takes its roots with polyroots, and forms
depths and poses in closed form: no Newton polish, no tolerance inside the solver."""
import mpmath as mp
import numpy as np

DIGITS = 60
REAL_BELOW, COMPLEX_ABOVE = mp.mpf("1e-30"), mp.mpf("1e-4")
APART, MARGIN = mp.mpf("1e-4"), mp.mpf("1e-6")


def _frame(P0, P1, P2):
    a = P1 - P0
    e1 = a / mp.norm(a)
    g = _cross(e1, P2 - P0)
    e3 = g / mp.norm(g)
    return e1, _cross(e3, e1), e3


def _cross(a, b):
    return mp.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def solve(X, uv, K):
    """X [4, 3], uv [4, 2] (the fourth row is not used), K = fx fy cx cy, doubles. Returns (candidates [k, 12] as doubles in
    ascending v, decided): every positive-depth pose of the three correspondences."""
    with mp.workdps(DIGITS):
        P = [mp.matrix([mp.mpf(float(c)) for c in X[k]]) for k in range(3)]
        fx, fy, cx, cy = (mp.mpf(float(k)) for k in K)
        f = []
        for k in range(3):
            y = mp.matrix([(mp.mpf(float(uv[k][0])) - cx) / fx, (mp.mpf(float(uv[k][1])) - cy) / fy, 1])
            f.append(y / mp.norm(y))
        sq = lambda a: a[0] * a[0] + a[1] * a[1] + a[2] * a[2]   # noqa: E731
        dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]   # noqa: E731
        A, B, C = sq(P[1] - P[2]), sq(P[0] - P[2]), sq(P[0] - P[1])
        ca, cb, cg = dot(f[1], f[2]), dot(f[0], f[2]), dot(f[0], f[1])
        p, q, rA, rC = (A - C) / B, (A + C) / B, A / B, C / B
        A4 = (p - 1) ** 2 - 4 * rC * ca ** 2
        A3 = 4 * (p * (1 - p) * cb - (1 - q) * ca * cg + 2 * rC * ca ** 2 * cb)
        A2 = 2 * (p ** 2 - 1 + 2 * p ** 2 * cb ** 2 + 2 * (1 - rC) * ca ** 2 - 4 * q * ca * cb * cg + 2 * (1 - rA) * cg ** 2)
        A1 = 4 * (-p * (1 + p) * cb + 2 * rA * cg ** 2 * cb - (1 - q) * ca * cg)
        A0 = (1 + p) ** 2 - 4 * rA * cg ** 2
        z = mp.polyroots([A4, A3, A2, A1, A0], maxsteps=2000, extraprec=4 * DIGITS)
        decided = True
        real = []
        for r in z:
            rel = abs(mp.im(r)) / (1 + abs(mp.re(r)))
            if rel < REAL_BELOW:
                real.append(mp.re(r))
            elif not rel > COMPLEX_ABOVE:
                decided = False
        for i in range(len(z)):
            for j in range(i):
                if not abs(z[i] - z[j]) > APART * (1 + abs(z[i])):
                    decided = False
        EX = _frame(P[0], P[1], P[2])
        out = []
        for v in sorted(real):
            den = 2 * (cg - v * ca)
            d = 1 + v * v - 2 * v * cb
            if not abs(den) > MARGIN or not d > MARGIN:
                decided = False
            if den == 0 or not d > 0:
                continue
            u = ((p - 1) * v * v - 2 * p * cb * v + 1 + p) / den
            s0 = mp.sqrt(B / d)
            s = [s0, u * s0, v * s0]
            if not (all(x > MARGIN for x in s) or any(x < -MARGIN for x in s)):
                decided = False
            if not all(x > 0 for x in s):
                continue
            Q = [s[k] * f[k] for k in range(3)]
            EQ = _frame(Q[0], Q[1], Q[2])
            R = [[sum(EQ[k][r] * EX[k][c] for k in range(3)) for c in range(3)] for r in range(3)]
            t = [Q[0][r] - sum(R[r][c] * P[0][c] for c in range(3)) for r in range(3)]
            out.append([float(R[r][c]) for r in range(3) for c in range(3)] + [float(x) for x in t])
        return np.array(out, dtype=np.float64).reshape(-1, 12), decided
