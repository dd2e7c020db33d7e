"""The SOLUTION SET of a five-point sample at 60 digits (mpmath): what the restatement (oracle/solve_oracle.c, oracle_essential5) and
through it the kernels are held to where that set is decided. Test infrastructure; needed only where the golden file is made or
re-derived (tests/golden/make_essential5_golden.py; tests/test_essential5_reference.py skips its re-derivation without mpmath) —
the GPU tests read the file.

Written from the definition, not from the kernel. The double inputs are taken exactly. E = x X + y Y + z Z + W over a basis of
the null space of the five epipolar constraints (SVD; the solution set does not depend on the basis); the ten cubic constraints
det E = 0 and 2 E E^T E - tr(E E^T) E = 0 are expanded as polynomials in (x, y, z) term by term; z is hidden: the constraints are
C(z) m = 0 with m = (x^3, x^2 y, x y^2, y^3, x^2, x y, y^2, x, y, 1) and C(z) 10 x 10 of degrees 0 0 0 0 1 1 1 2 2 3 per column;
det C(z), of degree 10, is interpolated from its values at the 11th roots of unity; its roots come from polyroots; per real root
the null vector of C(z) (SVD) gives x = m[7] / m[9], y = m[8] / m[9]. No Newton polish, no tolerance inside the solver; every
solution is checked against the ten constraints before it is returned (residual below 1e-40 of the terms' size).

A sample is DECIDED when
  the five constraints are independent (the fifth singular value of the 5 x 9 system is above 1e-8 of the first),
  every non-real root is at least 1e-5 (1 + |Re z|) from the real axis (and every real one within 1e-30 of it),
  every pair of real roots is at least 1e-5 (1 + |z|) apart,
  det C has its full degree (the leading coefficient is above 1e-20 of the largest: no solution at infinity in this basis),
  the back-substitution is unambiguous: at every real root the second smallest singular value of the column-scaled C(z) is
      above 1e-8 of the largest (the smallest is zero to working precision; 1e-8 = the square root of double precision,
      below which a double-precision solver could not tell rank 9 from rank 8), and m[9] is not zero,
  and no two solutions are closer than 1e-4 as unit-norm matrices up to sign (the tests match models to solutions one to one
      within a bound of 1e-10: the matching must not depend on its order).
Anything else is left to the solvers' own tolerances and is not compared. On the 512 samples of the fixture every sample is decided.

WHICH SIDE IS OFF where a forward-motion sample has equal counts on both sides and a 60-digit solution with no double-precision
model near it (seen on noise-free forward motion: 1 sample of 64 at a distance of 0.17, found by scanning six such scenes that
are NOT in the fixture; the fixture's own forward scenes have no such sample): the restatement, and neither of the two suspects.
  Not the back-substitution here: every solution returned satisfies the ten constraints to 1e-40, C(z) has rank 9 at all of
      them (second smallest singular value 2.7e-5 .. 4e-3 of the largest on that sample), so the singular-value criterion does
      not flag it at any margin one could argue for from the number formats.
  Not the polish merging two roots: the four polished models are distinct; three are solutions, the fourth is nothing.
  The cause is the degree-10 polynomial IN DOUBLE: on that sample it has a real root and a complex pair 0.02 from the axis within
      0.08 of each other (and two more real roots within 0.002), its coefficients carry the rounding of a 10 x 10 elimination,
      and in that cluster its real root is not where a solution is. x and y from B(z) at such a z start the three
      Gauss-Newton steps outside their basin: they drift (z 1.314 -> 1.372, -> 1.409 after twelve steps) without arriving.
      No reading of the root finder changes that (numpy.roots on the same coefficients returns the same root); it would
      take another elimination or a polish that does not start from the polynomial's root, and is left as the next step for the
      restatement and the kernel together (docs/HISTORY.md). Such a sample is decided by every criterion above: if one ever
      enters the fixture the tests fail on it, which is the right outcome."""
import mpmath as mp
import numpy as np

DIGITS = 60
REAL_BELOW, COMPLEX_ABOVE, APART = mp.mpf("1e-30"), mp.mpf("1e-5"), mp.mpf("1e-5")
FULL_DEGREE, RANK_MARGIN, MODEL_APART = mp.mpf("1e-20"), mp.mpf("1e-8"), 1e-4
RESIDUAL = mp.mpf("1e-40")

MONO = ((3, 0), (2, 1), (1, 2), (0, 3), (2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))   # (ex, ey) of m's entries


def _pmul(p, q):
    out = {}
    for a, u in p.items():
        for b, v in q.items():
            k = (a[0] + b[0], a[1] + b[1], a[2] + b[2])
            out[k] = out.get(k, 0) + u * v
    return out


def _padd(p, q, s=1):
    out = dict(p)
    for k, v in q.items():
        out[k] = out.get(k, 0) + s * v
    return out


def _constraints(basis):
    """The ten cubics as dicts (ex, ey, ez) -> coefficient, from the four null vectors X, Y, Z, W (each 9 entries)."""
    unit = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0))
    E = [[{unit[b]: basis[b][3 * r + c] for b in range(4)} for c in range(3)] for r in range(3)]
    det = {}
    for (i, j, k), s in (((0, 1, 2), 1), ((1, 2, 0), 1), ((2, 0, 1), 1), ((0, 2, 1), -1), ((1, 0, 2), -1), ((2, 1, 0), -1)):
        det = _padd(det, _pmul(_pmul(E[0][i], E[1][j]), E[2][k]), s)
    EEt = [[{} for _ in range(3)] for _ in range(3)]
    for r in range(3):
        for c in range(3):
            for k in range(3):
                EEt[r][c] = _padd(EEt[r][c], _pmul(E[r][k], E[c][k]))
    tr = _padd(_padd(EEt[0][0], EEt[1][1]), EEt[2][2])
    out = [det]
    for r in range(3):
        for c in range(3):
            p = {}
            for k in range(3):
                p = _padd(p, _pmul(EEt[r][k], E[k][c]), 2)
            out.append(_padd(p, _pmul(tr, E[r][c]), -1))
    return out


def _C(cons, z):
    """C(z): row = constraint, column = monomial of MONO, entry = sum over ez of the coefficient times z^ez."""
    zp = [1, z, z * z, z * z * z]
    return mp.matrix([[sum((p.get((ex, ey, ez), 0) * zp[ez] for ez in range(4 - ex - ey)), mp.mpf(0)) for ex, ey in MONO] for p in cons])


def solve(p1, p2, K=None):
    """p1, p2 [5, 2] (pixels of view 1 / view 2, or normalised coordinates with K = None), K = fx fy cx cy, doubles. Returns
    (E [k, 9] as doubles: unit norm, the entry of largest magnitude positive, in ascending z of this reference's own basis; decided)."""
    with mp.workdps(DIGITS):
        rows = []
        for (u1, v1), (u2, v2) in zip(np.asarray(p1, dtype=np.float64), np.asarray(p2, dtype=np.float64)):
            x1, y1, x2, y2 = (mp.mpf(float(v)) for v in (u1, v1, u2, v2))
            if K is not None:
                fx, fy, cx, cy = (mp.mpf(float(k)) for k in K)
                x1, y1, x2, y2 = (x1 - cx) / fx, (y1 - cy) / fy, (x2 - cx) / fx, (y2 - cy) / fy
            rows.append([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, mp.mpf(1)])
        _, sv, V = mp.svd_r(mp.matrix(rows), full_matrices=True)
        decided = bool(sv[4] > RANK_MARGIN * sv[0])                      # five independent constraints: a four-dimensional null space
        basis = [[V[5 + b, e] for e in range(9)] for b in range(4)]
        cons = _constraints(basis)
        # det C(z) from its values on the unit circle (an inverse DFT of length 11)
        w = [mp.expjpi(mp.mpf(2 * k) / 11) for k in range(11)]
        dets = [mp.det(_C(cons, wk)) for wk in w]
        coef = [mp.re(sum(dets[k] * w[(-j * k) % 11] for k in range(11)) / 11) for j in range(11)]
        cmax = max(abs(c) for c in coef)
        if not cmax > 0 or not abs(coef[10]) > FULL_DEGREE * cmax:
            return np.zeros((0, 9)), False
        roots = mp.polyroots(coef[::-1], maxsteps=2000, extraprec=4 * DIGITS)
        real = []
        for r in roots:
            rel = abs(mp.im(r)) / (1 + abs(mp.re(r)))
            if rel < REAL_BELOW:
                real.append(mp.re(r))
            elif not rel > COMPLEX_ABOVE:
                decided = False
        real.sort()
        for a, b in zip(real, real[1:]):
            if not b - a > APART * (1 + abs(a)):
                decided = False
        out = []
        for z in real:
            C = _C(cons, z)
            scale = [max(abs(C[r, c]) for r in range(10)) for c in range(10)]          # columns carry x^3 .. 1: scaled to unit size
            if min(scale) == 0:
                decided = False
                continue
            Cs = mp.matrix([[C[r, c] / scale[c] for c in range(10)] for r in range(10)])
            _, s, Vt = mp.svd_r(Cs)
            m = [Vt[9, c] / scale[c] for c in range(10)]
            if not s[8] > RANK_MARGIN * s[0]:
                decided = False
            if m[9] == 0:
                decided = False
                continue
            x, y = m[7] / m[9], m[8] / m[9]
            # the ten constraints themselves, at (x, y, z): the elimination above is held to the definition
            for p in cons:
                terms = [c * x ** k[0] * y ** k[1] * z ** k[2] for k, c in p.items()]
                if not abs(sum(terms)) <= RESIDUAL * max(abs(t) for t in terms):
                    raise ArithmeticError("a 60-digit solution misses a constraint: the reference is wrong")
            E = [basis[0][e] * x + basis[1][e] * y + basis[2][e] * z + basis[3][e] for e in range(9)]
            n = mp.sqrt(sum(e * e for e in E))
            lead = max(E, key=abs)
            out.append([float(e / n * mp.sign(lead)) for e in E])
        out = np.array(out, dtype=np.float64).reshape(-1, 9)
        for i in range(len(out)):
            for j in range(i):
                if min(np.abs(out[i] - out[j]).max(), np.abs(out[i] + out[j]).max()) < MODEL_APART:
                    decided = False
        return out, decided
