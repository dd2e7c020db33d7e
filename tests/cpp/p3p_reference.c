/* p3p_reference.c — CPU restatement of the P3P solver of eacham_solve_p3p / eacham_pnp_hypotheses_batch_p3p (include/eacham_hip.h
 * states the definition; eacham_amd/csrc/p3p_dev.hpp is the device form). Test infrastructure only: tests/p3p_reference.py compiles
 * it with -ffp-contract=off and no fast-math, so every product, sum, quotient and square root is rounded on its own and the sums run
 * in the order written — the same operations in the same order as the kernels, which are held to it as bytes.
 * Only + - * / sqrt, fabs, fmax, fmin (all correctly rounded or exact). */
#include <math.h>
#include <stdint.h>

static int finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }

/* Durand-Kerner on c0 + c1 z + .. + c4 z^4: real_roots3 (eacham_amd/csrc/solve_dev.hpp, tests/cpp/fundamental_reference.c)
 * carried to degree <= 4, nothing else changed. */
static int real_roots4(double c0, double c1, double c2, double c3, double c4, double* roots /* 4 */) {
    double cmax = 0.0;
    cmax = fmax(cmax, fabs(c0));
    cmax = fmax(cmax, fabs(c1));
    cmax = fmax(cmax, fabs(c2));
    cmax = fmax(cmax, fabs(c3));
    cmax = fmax(cmax, fabs(c4));
    if (!(cmax > 0.0)) return 0;
    int deg = 4;
    double lead = c4;
    if (fabs(c4) <= 1e-14 * cmax) {
        deg = 3, lead = c3;
        if (fabs(c3) <= 1e-14 * cmax) {
            deg = 2, lead = c2;
            if (fabs(c2) <= 1e-14 * cmax) {
                deg = 1, lead = c1;
                if (fabs(c1) <= 1e-14 * cmax) deg = 0;
            }
        }
    }
    if (deg == 0) return 0;
    const double c[4] = {c0, c1, c2, c3};
    double m[4];
    for (int k = 0; k < 4; ++k) m[k] = k < deg ? c[k] / lead : 0.0;
    double bound = 0.0;
    for (int k = 0; k < 4; ++k)
        if (k < deg) bound = fmax(bound, fabs(m[k]));
    bound += 1.0;
    double zr[4] = {0, 0, 0, 0}, zi[4] = {0, 0, 0, 0};
    {
        double r0 = 1.0;
        const double a0 = fabs(m[0]);
        if (a0 > 0.0) {
            double y = a0 > 1.0 ? a0 : 1.0;
            for (int it = 0; it < 80; ++it) {
                double yp = 1.0;
                for (int j = 0; j < deg - 1; ++j) yp *= y;
                y = ((deg - 1) * y + a0 / yp) / deg;
            }
            r0 = y;
        }
        r0 = fmin(fmax(r0, 0.5), bound);
        double cr = 1.0, ci = 0.0;
        for (int k = 0; k < 4; ++k) {
            if (k < deg) zr[k] = r0 * cr, zi[k] = r0 * ci;
            const double tr = cr * 0.4 - ci * 0.9, ti = cr * 0.9 + ci * 0.4;
            cr = tr, ci = ti;
        }
    }
    for (int it = 0; it < 200; ++it) {
        double change = 0.0, nzr[4], nzi[4];
        for (int k = 0; k < 4; ++k) {
            nzr[k] = zr[k], nzi[k] = zi[k];
            double pr = 1.0, pi = 0.0; /* Horner on the monic polynomial */
            for (int j = 3; j >= 0; --j)
                if (j < deg) {
                    const double tr = pr * zr[k] - pi * zi[k] + m[j], ti = pr * zi[k] + pi * zr[k];
                    pr = tr, pi = ti;
                }
            double dr = 1.0, di = 0.0;
            for (int j = 0; j < 4; ++j)
                if (j < deg && j != k) {
                    const double ar = zr[k] - zr[j], ai = zi[k] - zi[j];
                    const double tr = dr * ar - di * ai, ti = dr * ai + di * ar;
                    dr = tr, di = ti;
                }
            const double den = dr * dr + di * di;
            if (k < deg && den > 0.0) {
                const double qr = (pr * dr + pi * di) / den, qi = (pi * dr - pr * di) / den;
                nzr[k] = zr[k] - qr;
                nzi[k] = zi[k] - qi;
                change = fmax(change, fabs(qr) + fabs(qi));
            }
        }
        for (int k = 0; k < 4; ++k) zr[k] = nzr[k], zi[k] = nzi[k];
        if (change <= 1e-11 * bound) break;
    }
    double z[4] = {0, 0, 0, 0};
    int real[4];
    for (int k = 0; k < 4; ++k) {
        real[k] = k < deg && !(fabs(zi[k]) > 1e-7 * (1.0 + fabs(zr[k])));
        double v = zr[k];
        int going = real[k];
        for (int it = 0; it < 4; ++it) { /* Newton polish on the real polynomial: stops for good at a zero derivative */
            double p = lead, d = 0.0;
            for (int j = 3; j >= 0; --j)
                if (j < deg) {
                    d = d * v + p;
                    p = p * v + c[j];
                }
            going = going && fabs(d) > 0.0;
            if (going) v -= p / d;
        }
        z[k] = real[k] ? v : 0.0;
    }
    /* ascending, equals in iterate order: root k goes to the slot of its rank */
    int n = 0;
    for (int k = 0; k < 4; ++k) n += real[k];
    for (int s = 0; s < 4; ++s) roots[s] = 0.0;
    for (int k = 0; k < 4; ++k) {
        int rank = 0;
        for (int j = 0; j < 4; ++j)
            if (j != k && real[j] && (z[j] < z[k] || (z[j] == z[k] && j < k))) ++rank;
        for (int s = 0; s < 4; ++s)
            if (real[k] && rank == s) roots[s] = z[k];
    }
    return n;
}

static double det3(double a00, double a01, double a02, double a10, double a11, double a12, double a20, double a21, double a22) {
    return a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20);
}

/* the orthonormal frame of a triangle, e1 e2 e3 in E[0..2] E[3..5] E[6..8] */
static void tri_frame(const double* P0, const double* P1, const double* P2, double* E) {
    const double a0 = P1[0] - P0[0], a1 = P1[1] - P0[1], a2 = P1[2] - P0[2];
    const double n1 = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
    E[0] = a0 / n1, E[1] = a1 / n1, E[2] = a2 / n1;
    const double b0 = P2[0] - P0[0], b1 = P2[1] - P0[1], b2 = P2[2] - P0[2];
    const double g0 = E[1] * b2 - E[2] * b1, g1 = E[2] * b0 - E[0] * b2, g2 = E[0] * b1 - E[1] * b0;
    const double n3 = sqrt(g0 * g0 + g1 * g1 + g2 * g2);
    E[6] = g0 / n3, E[7] = g1 / n3, E[8] = g2 / n3;
    E[3] = E[7] * E[2] - E[8] * E[1], E[4] = E[8] * E[0] - E[6] * E[2], E[5] = E[6] * E[1] - E[7] * E[0];
}

/* PnPRansacCallback::computeError as the device scorer states it (score_dev.hpp, kind PNP): projection in double, difference in float */
static float pnp_error(const double* a, const double* b, const double* M, const double* K) {
    const double X = M[0] * a[0] + M[1] * a[1] + M[2] * a[2] + M[9];
    const double Y = M[3] * a[0] + M[4] * a[1] + M[5] * a[2] + M[10];
    double Z = M[6] * a[0] + M[7] * a[1] + M[8] * a[2] + M[11];
    Z = Z != 0.0 ? 1.0 / Z : 1.0;
    const float u = (float)(X * Z * K[0] + K[2]), v = (float)(Y * Z * K[1] + K[3]);
    const float dx = (float)b[0] - u, dy = (float)b[1] - v;
    return dx * dx + dy * dy;
}

/* Steps 1-7 on one sample. X: 4 x 3, x: 4 x 2, K = fx fy cx cy. M: 12 (zero without a model), cand: 4 x 12 in root order (slots
 * behind *n_cand zero), quartic: A0..A4 and roots: 4 (diagnostics, may be NULL). Returns n_models (1 or 0). */
static int p3p_sample(const double* X, const double* x, const double* K, double* M, double* cand, int* n_cand, double* quartic, double* roots_out,
                      int* n_roots_out) {
    for (int k = 0; k < 12; ++k) M[k] = 0.0;
    for (int k = 0; k < 48; ++k) cand[k] = 0.0;
    *n_cand = 0;
    if (quartic)
        for (int k = 0; k < 5; ++k) quartic[k] = 0.0;
    if (roots_out)
        for (int k = 0; k < 4; ++k) roots_out[k] = 0.0;
    if (n_roots_out) *n_roots_out = 0;
    /* 1. bearings */
    double f[9];
    for (int k = 0; k < 3; ++k) {
        const double y0 = (x[2 * k] - K[2]) / K[0], y1 = (x[2 * k + 1] - K[3]) / K[1];
        const double nrm = sqrt(y0 * y0 + y1 * y1 + 1.0);
        f[3 * k] = y0 / nrm, f[3 * k + 1] = y1 / nrm, f[3 * k + 2] = 1.0 / nrm;
    }
    /* 2. triangle */
    const double *X0 = X, *X1 = X + 3, *X2 = X + 6;
    const double a0 = X1[0] - X0[0], a1 = X1[1] - X0[1], a2 = X1[2] - X0[2];
    const double b0 = X2[0] - X0[0], b1 = X2[1] - X0[1], b2 = X2[2] - X0[2];
    const double e0 = X1[0] - X2[0], e1 = X1[1] - X2[1], e2 = X1[2] - X2[2];
    const double A = e0 * e0 + e1 * e1 + e2 * e2, B = b0 * b0 + b1 * b1 + b2 * b2, C = a0 * a0 + a1 * a1 + a2 * a2;
    if (!finite_d(A) || !finite_d(B) || !finite_d(C) || A == 0.0 || B == 0.0 || C == 0.0) return 0;
    for (int k = 0; k < 9; ++k)
        if (!finite_d(f[k])) return 0;
    const double g0 = a1 * b2 - a2 * b1, g1 = a2 * b0 - a0 * b2, g2 = a0 * b1 - a1 * b0;
    if (g0 * g0 + g1 * g1 + g2 * g2 <= 1e-20 * B * C) return 0;
    const double ca = f[3] * f[6] + f[4] * f[7] + f[5] * f[8];
    const double cb = f[0] * f[6] + f[1] * f[7] + f[2] * f[8];
    const double cg = f[0] * f[3] + f[1] * f[4] + f[2] * f[5];
    /* 3. Grunert's quartic in v = s2 / s0 */
    const double p = (A - C) / B, q = (A + C) / B, rA = A / B, rC = C / B;
    const double ca2 = ca * ca, cb2 = cb * cb, cg2 = cg * cg;
    const double A4 = (p - 1.0) * (p - 1.0) - 4.0 * rC * ca2;
    const double A3 = 4.0 * (p * (1.0 - p) * cb - (1.0 - q) * ca * cg + 2.0 * rC * ca2 * cb);
    const double A2 = 2.0 * (p * p - 1.0 + 2.0 * (p * p) * cb2 + 2.0 * (1.0 - rC) * ca2 - 4.0 * q * ca * cb * cg + 2.0 * (1.0 - rA) * cg2);
    const double A1 = 4.0 * (-p * (1.0 + p) * cb + 2.0 * rA * cg2 * cb - (1.0 - q) * ca * cg);
    const double A0 = (1.0 + p) * (1.0 + p) - 4.0 * rA * cg2;
    /* 4. roots */
    double roots[4];
    const int nr = real_roots4(A0, A1, A2, A3, A4, roots);
    if (quartic) quartic[0] = A0, quartic[1] = A1, quartic[2] = A2, quartic[3] = A3, quartic[4] = A4;
    if (roots_out)
        for (int k = 0; k < 4; ++k) roots_out[k] = roots[k];
    if (n_roots_out) *n_roots_out = nr;
    double EX[9];
    tri_frame(X0, X1, X2, EX);
    int nc = 0, best = -1;
    float best_err = 0.f;
    for (int k = 0; k < 4; ++k) {
        if (k >= nr) continue;
        /* 5. depths */
        const double v = roots[k], v2 = v * v;
        const double den = 2.0 * (cg - v * ca);
        if (den == 0.0) continue;
        const double u = ((p - 1.0) * v2 - 2.0 * p * cb * v + 1.0 + p) / den;
        const double d = 1.0 + v2 - 2.0 * v * cb;
        if (!(d > 0.0)) continue;
        double s0 = sqrt(B / d), s1 = u * s0, s2 = v * s0;
        int ok = 1;
        for (int it = 0; it < 2; ++it) { /* Newton on the three law-of-cosines equations, Cramer's rule */
            const double F0 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * ca - A;
            const double F1 = s0 * s0 + s2 * s2 - 2.0 * s0 * s2 * cb - B;
            const double F2 = s0 * s0 + s1 * s1 - 2.0 * s0 * s1 * cg - C;
            const double j01 = 2.0 * s1 - 2.0 * s2 * ca, j02 = 2.0 * s2 - 2.0 * s1 * ca;
            const double j10 = 2.0 * s0 - 2.0 * s2 * cb, j12 = 2.0 * s2 - 2.0 * s0 * cb;
            const double j20 = 2.0 * s0 - 2.0 * s1 * cg, j21 = 2.0 * s1 - 2.0 * s0 * cg;
            const double det = det3(0.0, j01, j02, j10, 0.0, j12, j20, j21, 0.0);
            if (det == 0.0) ok = 0;
            if (ok) {
                s0 -= det3(F0, j01, j02, F1, 0.0, j12, F2, j21, 0.0) / det;
                s1 -= det3(0.0, F0, j02, j10, F1, j12, j20, F2, 0.0) / det;
                s2 -= det3(0.0, j01, F0, j10, 0.0, F1, j20, j21, F2) / det;
                if (!finite_d(s0) || !finite_d(s1) || !finite_d(s2)) ok = 0;
            }
        }
        if (!ok) continue;
        if (!(s0 > 0.0 && s1 > 0.0 && s2 > 0.0)) continue;
        /* 6. pose */
        const double Q[9] = {s0 * f[0], s0 * f[1], s0 * f[2], s1 * f[3], s1 * f[4], s1 * f[5], s2 * f[6], s2 * f[7], s2 * f[8]};
        double EQ[9], T[12];
        tri_frame(Q, Q + 3, Q + 6, EQ);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) T[3 * r + c] = EQ[r] * EX[c] + EQ[3 + r] * EX[3 + c] + EQ[6 + r] * EX[6 + c];
        for (int r = 0; r < 3; ++r) T[9 + r] = Q[r] - (T[3 * r] * X0[0] + T[3 * r + 1] * X0[1] + T[3 * r + 2] * X0[2]);
        for (int e = 0; e < 12; ++e) cand[12 * nc + e] = T[e];
        /* 7. the fourth point chooses: the first strictly smallest error, a NaN never wins */
        const float err = pnp_error(X + 9, x + 6, T, K);
        if (err == err && (best < 0 || err < best_err)) {
            best = nc, best_err = err;
            for (int e = 0; e < 12; ++e) M[e] = T[e];
        }
        ++nc;
    }
    *n_cand = nc;
    return best >= 0 ? 1 : 0;
}

/* eacham_solve_p3p: obj n x 3, img n x 2, idx n_samples x 4 (checked by the caller). quartic n_samples x 5, roots n_samples x 4,
 * n_roots n_samples: optional diagnostics. */
void p3pref_solve(const double* obj, const double* img, const double* K, int n_samples, const int32_t* idx, double* models, int32_t* n_models,
                  double* candidates, int32_t* n_candidates, double* quartic, double* roots, int32_t* n_roots) {
    for (int s = 0; s < n_samples; ++s) {
        double X[12], x[8];
        for (int k = 0; k < 4; ++k) {
            const int i = idx[4 * s + k];
            for (int e = 0; e < 3; ++e) X[3 * k + e] = obj[3 * (long long)i + e];
            for (int e = 0; e < 2; ++e) x[2 * k + e] = img[2 * (long long)i + e];
        }
        int nc = 0, nr = 0;
        n_models[s] = p3p_sample(X, x, K, models + 12 * (long long)s, candidates + 48 * (long long)s, &nc, quartic ? quartic + 5 * (long long)s : 0,
                                 roots ? roots + 4 * (long long)s : 0, &nr);
        n_candidates[s] = nc;
        if (n_roots) n_roots[s] = nr;
    }
}

/* eacham_score_hypotheses(kind PNP): errors nm x n (optional), counts nm */
void p3pref_score(int n, const double* obj, const double* img, const double* K, int nm, const double* models, float threshold, float* errors,
                  int32_t* counts) {
    for (int mdl = 0; mdl < nm; ++mdl) {
        int c = 0;
        for (int i = 0; i < n; ++i) {
            const float e = pnp_error(obj + 3 * (long long)i, img + 2 * (long long)i, models + 12 * (long long)mdl, K);
            if (errors) errors[(long long)mdl * n + i] = e;
            c += e <= threshold;
        }
        counts[mdl] = c;
    }
}
