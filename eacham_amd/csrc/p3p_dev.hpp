// p3p_dev.hpp — the P3P hypothesis of the PnP RANSAC: three correspondences give up to four poses, a fourth picks one. ONE device
// function (p3p_sample) runs the whole definition — include/eacham_hip.h states it with eacham_solve_p3p — on values that depend on
// neither the lane nor the launch shape, and both kernels of p3p.hip call it, so a sample gives the same bits through either entry
// point. The only includer is p3p.hip, compiled with -ffp-contract=off (csrc/Makefile): only + - * / sqrt, fabs, fmax, fmin, every
// operation rounded on its own, every sum in the order written. tests/cpp/p3p_reference.c is the CPU restatement, held as bytes.
//
// Relation to OpenCV: cv::solvePnPRansac(SOLVEPNP_P3P) runs p3p.cpp, which follows Gao et al. (2003) and solves its quartic in closed
// form. Here the same three law-of-cosines equations are eliminated as Grunert did (a quartic in v = s2 / s0, Haralick et al. 1994
// eq. 8-9), its roots come from the project's Durand-Kerner recipe, and every root's depths get two Newton steps on the three
// equations: the same solution set, not the same bits.
#pragma once

#include "score_dev.hpp"

namespace eacham {
namespace {

__device__ __forceinline__ bool p3p_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// real_roots3 (solve_dev.hpp) carried to degree <= 4, nothing else changed: degree drop at 1e-14 cmax, monic, the start values
// r0 (0.4 + 0.9 i)^k with r0 = |m0|^(1/deg) by 80 Newton steps clamped to [0.5, bound], at most 200 simultaneous sweeps stopped at a
// largest correction of 1e-11 bound, a root is real iff |zi| <= 1e-7 (1 + |zr|), four Newton steps on the real polynomial, real roots
// ascending (equals in iterate order).
__device__ __forceinline__ int real_roots4(double c0, double c1, double c2, double c3, double c4 /* c0 + c1 z + .. + c4 z^4 */, double* roots /* 4 */) {
    // (the coefficients by value and the leading one picked in the branches: as an array indexed by the degree they went to scratch)
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
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = k < deg ? c[k] / lead : 0.0;
    double bound = 0.0;
#pragma unroll
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
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < deg) zr[k] = r0 * cr, zi[k] = r0 * ci;
            const double tr = cr * 0.4 - ci * 0.9, ti = cr * 0.9 + ci * 0.4;
            cr = tr, ci = ti;
        }
    }
    for (int it = 0; it < 200; ++it) {
        double change = 0.0, nzr[4], nzi[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            nzr[k] = zr[k], nzi[k] = zi[k];
            double pr = 1.0, pi = 0.0;  /* Horner on the monic polynomial */
#pragma unroll
            for (int j = 3; j >= 0; --j)
                if (j < deg) {
                    const double tr = pr * zr[k] - pi * zi[k] + m[j], ti = pr * zi[k] + pi * zr[k];
                    pr = tr, pi = ti;
                }
            double dr = 1.0, di = 0.0;
#pragma unroll
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
#pragma unroll
        for (int k = 0; k < 4; ++k) zr[k] = nzr[k], zi[k] = nzi[k];
        if (change <= 1e-11 * bound) break;
    }
    double z[4] = {0, 0, 0, 0};
    bool real[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        real[k] = k < deg && !(fabs(zi[k]) > 1e-7 * (1.0 + fabs(zr[k])));
        double v = zr[k];
        bool going = real[k];
#pragma unroll
        for (int it = 0; it < 4; ++it) {  /* Newton polish on the real polynomial: stops for good at a zero derivative */
            double p = lead, d = 0.0;
#pragma unroll
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
#pragma unroll
    for (int k = 0; k < 4; ++k) n += real[k];
#pragma unroll
    for (int s = 0; s < 4; ++s) roots[s] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j != k && real[j] && (z[j] < z[k] || (z[j] == z[k] && j < k))) ++rank;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (real[k] && rank == s) roots[s] = z[k];
    }
    return n;
}

__device__ __forceinline__ double p3p_det3(double a00, double a01, double a02, double a10, double a11, double a12, double a20, double a21, double a22) {
    return a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20);
}

// the orthonormal frame of a triangle: e1 = (P1 - P0) / |P1 - P0|, e3 = e1 x (P2 - P0) normalised, e2 = e3 x e1, in E[0..2] E[3..5] E[6..8]
__device__ __forceinline__ void p3p_frame(const double* P0, const double* P1, const double* P2, double* E) {
    const double a0 = P1[0] - P0[0], a1 = P1[1] - P0[1], a2 = P1[2] - P0[2];
    const double n1 = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
    E[0] = a0 / n1, E[1] = a1 / n1, E[2] = a2 / n1;
    const double b0 = P2[0] - P0[0], b1 = P2[1] - P0[1], b2 = P2[2] - P0[2];
    const double g0 = E[1] * b2 - E[2] * b1, g1 = E[2] * b0 - E[0] * b2, g2 = E[0] * b1 - E[1] * b0;
    const double n3 = sqrt(g0 * g0 + g1 * g1 + g2 * g2);
    E[6] = g0 / n3, E[7] = g1 / n3, E[8] = g2 / n3;
    E[3] = E[7] * E[2] - E[8] * E[1], E[4] = E[8] * E[0] - E[6] * E[2], E[5] = E[6] * E[1] - E[7] * E[0];
}

// One sample: X = its four object points (4 x 3), x = its four pixels (4 x 2), K = fx fy cx cy. M (12, registers) = the chosen
// pose, zero without one; returns n_models (1 or 0). cand: null, or where the up-to-four candidates go in root order (4 x 12 doubles
// of GLOBAL memory, every slot written: the ones behind *n_cand zero) — candidate k is stored as it is made, so no array is indexed
// by a run-time slot and nothing goes to scratch.
__device__ __forceinline__ int p3p_sample(const double* X, const double* x, const double* K, double* M, double* __restrict__ cand, int* n_cand) {
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = 0.0;
    int nc = 0, nr = 0;
    bool have = false;
    // 1. bearings
    double f[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double y0 = (x[2 * k] - K[2]) / K[0], y1 = (x[2 * k + 1] - K[3]) / K[1];
        const double nrm = sqrt(y0 * y0 + y1 * y1 + 1.0);
        f[3 * k] = y0 / nrm, f[3 * k + 1] = y1 / nrm, f[3 * k + 2] = 1.0 / nrm;
    }
    // 2. triangle
    const double *X0 = X, *X1 = X + 3, *X2 = X + 6;
    const double a0 = X1[0] - X0[0], a1 = X1[1] - X0[1], a2 = X1[2] - X0[2];
    const double b0 = X2[0] - X0[0], b1 = X2[1] - X0[1], b2 = X2[2] - X0[2];
    const double e0 = X1[0] - X2[0], e1 = X1[1] - X2[1], e2 = X1[2] - X2[2];
    const double A = e0 * e0 + e1 * e1 + e2 * e2, B = b0 * b0 + b1 * b1 + b2 * b2, C = a0 * a0 + a1 * a1 + a2 * a2;
    bool good = p3p_finite(A) && p3p_finite(B) && p3p_finite(C) && A != 0.0 && B != 0.0 && C != 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) good = good && p3p_finite(f[k]);
    const double g0 = a1 * b2 - a2 * b1, g1 = a2 * b0 - a0 * b2, g2 = a0 * b1 - a1 * b0;
    good = good && !(g0 * g0 + g1 * g1 + g2 * g2 <= 1e-20 * B * C);
    const double ca = f[3] * f[6] + f[4] * f[7] + f[5] * f[8];
    const double cb = f[0] * f[6] + f[1] * f[7] + f[2] * f[8];
    const double cg = f[0] * f[3] + f[1] * f[4] + f[2] * f[5];
    // 3. Grunert's quartic in v = s2 / s0
    const double p = (A - C) / B, q = (A + C) / B, rA = A / B, rC = C / B;
    double roots[4] = {0, 0, 0, 0};
    if (good) {
        const double ca2 = ca * ca, cb2 = cb * cb, cg2 = cg * cg;
        const double A4 = (p - 1.0) * (p - 1.0) - 4.0 * rC * ca2;
        const double A3 = 4.0 * (p * (1.0 - p) * cb - (1.0 - q) * ca * cg + 2.0 * rC * ca2 * cb);
        const double A2 = 2.0 * (p * p - 1.0 + 2.0 * (p * p) * cb2 + 2.0 * (1.0 - rC) * ca2 - 4.0 * q * ca * cb * cg + 2.0 * (1.0 - rA) * cg2);
        const double A1 = 4.0 * (-p * (1.0 + p) * cb + 2.0 * rA * cg2 * cb - (1.0 - q) * ca * cg);
        const double A0 = (1.0 + p) * (1.0 + p) - 4.0 * rA * cg2;
        // 4. roots
        nr = real_roots4(A0, A1, A2, A3, A4, roots);
    }
    double EX[9];
    p3p_frame(X0, X1, X2, EX);
    float best_err = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // 5. depths
        const double v = roots[k], v2 = v * v;
        const double den = 2.0 * (cg - v * ca);
        const double u = ((p - 1.0) * v2 - 2.0 * p * cb * v + 1.0 + p) / den;
        const double d = 1.0 + v2 - 2.0 * v * cb;
        bool ok = k < nr && den != 0.0 && d > 0.0;
        double s0 = sqrt(B / d), s1 = u * s0, s2 = v * s0;
#pragma unroll
        for (int it = 0; it < 2; ++it) {   // Newton on the three law-of-cosines equations, Cramer's rule
            const double F0 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * ca - A;
            const double F1 = s0 * s0 + s2 * s2 - 2.0 * s0 * s2 * cb - B;
            const double F2 = s0 * s0 + s1 * s1 - 2.0 * s0 * s1 * cg - C;
            const double j01 = 2.0 * s1 - 2.0 * s2 * ca, j02 = 2.0 * s2 - 2.0 * s1 * ca;
            const double j10 = 2.0 * s0 - 2.0 * s2 * cb, j12 = 2.0 * s2 - 2.0 * s0 * cb;
            const double j20 = 2.0 * s0 - 2.0 * s1 * cg, j21 = 2.0 * s1 - 2.0 * s0 * cg;
            const double det = p3p_det3(0.0, j01, j02, j10, 0.0, j12, j20, j21, 0.0);
            if (det == 0.0) ok = false;
            if (ok) {
                s0 -= p3p_det3(F0, j01, j02, F1, 0.0, j12, F2, j21, 0.0) / det;
                s1 -= p3p_det3(0.0, F0, j02, j10, F1, j12, j20, F2, 0.0) / det;
                s2 -= p3p_det3(0.0, j01, F0, j10, 0.0, F1, j20, j21, F2) / det;
                if (!p3p_finite(s0) || !p3p_finite(s1) || !p3p_finite(s2)) ok = false;
            }
        }
        ok = ok && s0 > 0.0 && s1 > 0.0 && s2 > 0.0;
        if (ok) {
            // 6. pose
            const double Q[9] = {s0 * f[0], s0 * f[1], s0 * f[2], s1 * f[3], s1 * f[4], s1 * f[5], s2 * f[6], s2 * f[7], s2 * f[8]};
            double EQ[9], T[12];
            p3p_frame(Q, Q + 3, Q + 6, EQ);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) T[3 * r + c] = EQ[r] * EX[c] + EQ[3 + r] * EX[3 + c] + EQ[6 + r] * EX[6 + c];
#pragma unroll
            for (int r = 0; r < 3; ++r) T[9 + r] = Q[r] - (T[3 * r] * X0[0] + T[3 * r + 1] * X0[1] + T[3 * r + 2] * X0[2]);
            if (cand) {
#pragma unroll
                for (int e = 0; e < 12; ++e) cand[12 * nc + e] = T[e];
            }
            // 7. the fourth point chooses: the first strictly smallest error, a NaN never wins
            const float err = score_one<2>(X + 9, x + 6, T, K, false);
            if (err == err && (!have || err < best_err)) {
                have = true, best_err = err;
#pragma unroll
                for (int e = 0; e < 12; ++e) M[e] = T[e];
            }
            ++nc;
        }
    }
    if (cand)
        for (int k = nc; k < 4; ++k)
#pragma unroll
            for (int e = 0; e < 12; ++e) cand[12 * k + e] = 0.0;
    *n_cand = nc;
    return have ? 1 : 0;
}

}  // namespace
}  // namespace eacham
