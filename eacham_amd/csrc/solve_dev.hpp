// solve_dev.hpp — the device functions of the minimal solvers that more than one translation unit runs: the homography
// (4 points), five-point (essential matrix) and seven-point (fundamental matrix) solvers by one wave per sample, EPnP's two halves, and the small dense algebra
// under them. solve.hip holds the solver kernels of every entry point (one template per stage, a one-problem and a list
// instantiation: solve_launch.hpp); pnp_batch.hip includes this file for the refit body (pnp_refit_body) and the rule among
// EPnP's three starts (pnp_first_smallest). Every includer is compiled with -ffp-contract=off (csrc/Makefile).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace eacham {
namespace {

constexpr int SOLVE_WAVES = 4;   // samples (waves) per workgroup of the minimal-sample kernels

__device__ __forceinline__ void wave_sync_lds() {  // a wave's own LDS traffic: order its writes before its reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* cyclic Jacobi on a symmetric N x N matrix (N <= 12): A is destroyed, V's COLUMNS are the eigenvectors, w the eigenvalues.
 * Small N (3, 4) unrolls completely and stays in registers. */
template <int N, class MA, class MV>
__device__ __forceinline__ void jacobi_eig(MA A, MV V, double* w) {
    constexpr int n = N;
#pragma unroll
    for (int i = 0; i < n; ++i)
#pragma unroll
        for (int j = 0; j < n; ++j) V[i * n + j] = i == j ? 1.0 : 0.0;
    auto rotate = [&](int p, int q) {
        const double apq = A[p * n + q];
        if (apq == 0.0) return;
        const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < n; ++k) {  /* columns p, q */
            const double akp = A[k * n + p], akq = A[k * n + q];
            A[k * n + p] = c * akp - s * akq;
            A[k * n + q] = s * akp + c * akq;
        }
#pragma unroll
        for (int k = 0; k < n; ++k) {  /* rows p, q */
            const double apk = A[p * n + k], aqk = A[q * n + k];
            A[p * n + k] = c * apk - s * aqk;
            A[q * n + k] = s * apk + c * aqk;
        }
#pragma unroll
        for (int k = 0; k < n; ++k) {
            const double vkp = V[k * n + p], vkq = V[k * n + q];
            V[k * n + p] = c * vkp - s * vkq;
            V[k * n + q] = s * vkp + c * vkq;
        }
    };
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int p = 0; p < n; ++p) {
            diag += A[p * n + p] * A[p * n + p];
#pragma unroll
            for (int q = p + 1; q < n; ++q) off += A[p * n + q] * A[p * n + q];
        }
        if (off <= 1e-60 || off <= 1e-32 * diag) break;
        if constexpr (N <= 4) {
#pragma unroll
            for (int p = 0; p < n - 1; ++p)
#pragma unroll
                for (int q = p + 1; q < n; ++q) rotate(p, q);
        } else {
            for (int p = 0; p < n - 1; ++p)
                for (int q = p + 1; q < n; ++q) rotate(p, q);
        }
    }
#pragma unroll
    for (int i = 0; i < n; ++i) w[i] = A[i * n + i];
}

/* ---- five-point ---------------------------------------------------------------------------------------------- */
/* column of the monomial x^ex y^ey z^ez (total degree <= 3) in Nister's elimination order */
__device__ static int mono_col(int ex, int ey, int ez) {
    constexpr int8_t order[20][3] = {{3, 0, 0}, {0, 3, 0}, {2, 1, 0}, {1, 2, 0}, {2, 0, 1}, {2, 0, 0}, {0, 2, 1}, {0, 2, 0}, {1, 1, 1}, {1, 1, 0},
                                        {1, 0, 2}, {1, 0, 1}, {1, 0, 0}, {0, 1, 2}, {0, 1, 1}, {0, 1, 0}, {0, 0, 3}, {0, 0, 2}, {0, 0, 1}, {0, 0, 0}};
    for (int k = 0; k < 20; ++k)
        if (order[k][0] == ex && order[k][1] == ey && order[k][2] == ez) return k;
    return -1;
}

/* ---- five-point, one WAVE per sample ---------------------------------------------------------------------------------------
 * The arithmetic of essential5 / oracle_essential5 entry by entry, spread over the lanes wherever entries are independent:
 *   null space      the Householder reflections of the 9 x 5 system: a lane per column of Q, a lane per row of P
 *   constraints     the 10 x 20 matrix: an entry per lane (four rounds), each adding ITS monomial's terms in the order of the
 *                   sequential triple loop (a table lists, per monomial, the (a, b, c) factor choices that produce it)
 *   Gauss-Jordan    on one shared copy in LDS: pivot search by every lane (same values), row swap / scale by 20 lanes, the
 *                   180 eliminated entries of a step over the wave
 *   det B(z)        every lane, in registers (a few hundred operations on identical values)
 *   roots           Durand-Kerner in its simultaneous form: root k on lane k, the other iterates by lane shuffles
 *   x, y, polish    a real root per lane: the 3 Gauss-Newton steps read the assembled constraints from LDS
 * Nothing is indexed at run time outside LDS: no scratch. A wave's LDS operations execute in program order; the fences only
 * pin the compiler. */
struct E5Lds {
    double A[200], A0[200];  // the constraints as eliminated / as assembled
    double Q[45], P[81];     // Q^T (9 x 5) and the orthogonal factor
    double lin[36];          // entry e of E as a linear form in (x, y, z, 1)
    double poly[11], mon[11];
    double B[45];            // B(z): [row][column][power of z]
    unsigned char mcol[64];     // column of the monomial x^ex y^ey z^ez at [16 ex + 4 ey + ez]
    unsigned char term[20][8];  // per monomial: the (a, b, c) choices of mul3acc that produce it, packed a | b << 2 | c << 4, in loop order
    unsigned char nterm[20];
};

__device__ __forceinline__ double readlane_f64(double v, int lane_uniform) {  // the value of lane `lane_uniform` (a wave-uniform index)
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, lane_uniform), hi = __builtin_amdgcn_readlane((int)(b >> 32), lane_uniform);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double wave_max_lanes(double v) {  // max over the wave (order-independent)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

__device__ static int essential5_wave(const double* p1, const double* p2, bool has_K, double fx, double fy, double cx, double cy,
                                      double* __restrict__ Eout /* global: 10 x 9 */, E5Lds& S) {
    const int lane = threadIdx.x & 63;
    // ---- the monomial table (lane 0..19: its own monomial) ----
    if (lane < 20) {
        int n = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int ex = (a == 0) + (b == 0) + (c == 0), ey = (a == 1) + (b == 1) + (c == 1), ez = (a == 2) + (b == 2) + (c == 2);
                    if (mono_col(ex, ey, ez) == lane) S.term[lane][n++] = (unsigned char)(a | (b << 2) | (c << 4));
                }
        S.nterm[lane] = (unsigned char)n;
    }
    {
        const int ex = lane >> 4, ey = (lane >> 2) & 3, ez = lane & 3;
        S.mcol[lane] = ex + ey + ez <= 3 ? (unsigned char)mono_col(ex, ey, ez) : (unsigned char)0;
    }
    // ---- Q^T ----
    if (lane < 5) {
        const int i = lane;
        double x1 = p1[2 * i], y1 = p1[2 * i + 1], x2 = p2[2 * i], y2 = p2[2 * i + 1];
        if (has_K) {
            x1 = (x1 - cx) / fx; y1 = (y1 - cy) / fy;
            x2 = (x2 - cx) / fx; y2 = (y2 - cy) / fy;
        }
        const double row[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0};
#pragma unroll
        for (int k = 0; k < 9; ++k) S.Q[k * 5 + i] = row[k];
    }
    for (int e = lane; e < 81; e += 64) S.P[e] = (e / 9 == e % 9) ? 1.0 : 0.0;
    wave_sync_lds();
    // ---- Householder QR of Q^T: lanes 0..4 own a column of Q, lanes 16..24 a row of P ----
    for (int k = 0; k < 5; ++k) {
        double norm = 0.0;
        for (int r = k; r < 9; ++r) norm += S.Q[r * 5 + k] * S.Q[r * 5 + k];
        norm = sqrt(norm);
        if (!(norm > 0.0)) return 0;  // (wave-uniform)
        double v[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) v[r] = r < k ? 0.0 : S.Q[r * 5 + k];
        {
            const double add = S.Q[k * 5 + k] >= 0.0 ? norm : -norm;
#pragma unroll
            for (int r = 0; r < 9; ++r)
                if (r == k) v[r] += add;
        }
        double vv = 0.0;
#pragma unroll
        for (int r = 0; r < 9; ++r)
            if (r >= k) vv += v[r] * v[r];
        if (!(vv > 0.0)) return 0;
        wave_sync_lds();  // every lane has read column k before anybody rewrites it
        if (lane < 5 && lane >= k) {  /* Q <- (I - 2 v v^T / vv) Q, column `lane` */
            const int c = lane;
            double d = 0.0;
#pragma unroll
            for (int r = 0; r < 9; ++r)
                if (r >= k) d += v[r] * S.Q[r * 5 + c];
            d = 2.0 * d / vv;
#pragma unroll
            for (int r = 0; r < 9; ++r)
                if (r >= k) S.Q[r * 5 + c] -= d * v[r];
        }
        if (lane >= 16 && lane < 25) {  /* P <- P (I - 2 v v^T / vv), row `lane - 16` */
            const int r = lane - 16;
            double d = 0.0;
#pragma unroll
            for (int c = 0; c < 9; ++c)
                if (c >= k) d += S.P[r * 9 + c] * v[c];
            d = 2.0 * d / vv;
#pragma unroll
            for (int c = 0; c < 9; ++c)
                if (c >= k) S.P[r * 9 + c] -= d * v[c];
        }
        wave_sync_lds();
    }
    if (lane < 36) S.lin[lane] = S.P[(lane >> 2) * 9 + 5 + (lane & 3)];
    wave_sync_lds();
    // ---- the ten cubic constraints: entry (row, col) of the 10 x 20 matrix per lane ----
    for (int e = lane; e < 200; e += 64) {
        const int row = e / 20, col = e % 20;
        const int nt = S.nterm[col];
        double acc = 0.0;
        auto mul3 = [&](int e1, int e2, int e3, double sgn) {  // acc += the terms of sgn * l(e1) l(e2) l(e3) that fall on monomial `col`
            for (int t = 0; t < nt; ++t) {
                const int tc = S.term[col][t];
                acc += sgn * (S.lin[4 * e1 + (tc & 3)] * S.lin[4 * e2 + ((tc >> 2) & 3)]) * S.lin[4 * e3 + (tc >> 4)];
            }
        };
        if (row == 0) {  /* det E */
            const int perm[6][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {1, 0, 2}, {2, 1, 0}};
#pragma unroll
            for (int p = 0; p < 6; ++p) mul3(perm[p][0], 3 + perm[p][1], 6 + perm[p][2], p < 3 ? 1.0 : -1.0);
        } else {         /* 2 E E^T E - tr(E E^T) E */
            const int i = (row - 1) / 3, j = (row - 1) % 3;
            for (int k = 0; k < 3; ++k)
                for (int l = 0; l < 3; ++l) {
                    mul3(3 * i + l, 3 * k + l, 3 * k + j, 2.0);
                    mul3(3 * k + l, 3 * k + l, 3 * i + j, -1.0);
                }
        }
        S.A[e] = acc;
        S.A0[e] = acc;
    }
    wave_sync_lds();
    // ---- Gauss-Jordan, partial pivoting ----
    for (int col = 0; col < 10; ++col) {
        int piv = col;
        for (int r = col + 1; r < 10; ++r)
            if (fabs(S.A[r * 20 + col]) > fabs(S.A[piv * 20 + col])) piv = r;
        if (!(fabs(S.A[piv * 20 + col]) > 1e-300)) return 0;  // (wave-uniform)
        wave_sync_lds();
        if (piv != col && lane < 20) {
            const double t = S.A[piv * 20 + lane];
            S.A[piv * 20 + lane] = S.A[col * 20 + lane];
            S.A[col * 20 + lane] = t;
        }
        wave_sync_lds();
        const double inv = 1.0 / S.A[col * 20 + col];
        wave_sync_lds();
        if (lane < 20) S.A[col * 20 + lane] *= inv;
        wave_sync_lds();
        double f[3];
        int at[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {  // the 9 x 20 entries of the other rows, three per lane: factors first, then the update
            const int e = lane + 64 * t;
            int r = e / 20;
            if (r >= col) ++r;
            at[t] = e < 180 ? r * 20 + e % 20 : -1;
            f[t] = e < 180 ? S.A[r * 20 + col] : 0.0;
        }
        wave_sync_lds();
#pragma unroll
        for (int t = 0; t < 3; ++t)
            if (at[t] >= 0 && f[t] != 0.0) S.A[at[t]] -= f[t] * S.A[col * 20 + at[t] % 20];
        wave_sync_lds();
    }
    /* B(z): rows k = e - z f, l = g - z h, m = i - z j; entries = polynomials in z (ascending), degrees 3, 3, 4. An entry per lane:
     * column j of row r reads e[top_j - k] and f[top_j - k + 1] with top = 2, 5, 9 and 3, 3, 4 coefficients of e */
    if (lane < 45) {
        const int r = lane / 15, j = (lane % 15) / 5, k = lane % 5;
        const double* e = S.A + (4 + 2 * r) * 20 + 10;
        const double* f = S.A + (5 + 2 * r) * 20 + 10;
        const int top = j == 0 ? 2 : (j == 1 ? 5 : 9), ne = j == 2 ? 4 : 3;
        double v;
        if (k == 0) v = e[top];
        else if (k < ne) v = e[top - k] - f[top - k + 1];
        else if (k == ne) v = -f[top - k + 1];
        else v = 0.0;
        S.B[lane] = v;
    }
    wave_sync_lds();
    /* det B(z) by cofactor expansion along row 0, coefficient k on lane k: for every coefficient the products enter in the order the
     * sequential polynomial multiplications add them (first factor's power ascending) */
    if (lane <= 10) {
        const int k = lane;
        double pk = 0.0;
        for (int c0 = 0; c0 < 3; ++c0) {
            const int c1 = c0 == 0 ? 1 : (c0 == 1 ? 2 : 0), c2 = c0 == 0 ? 2 : (c0 == 1 ? 0 : 1);
            const int d1 = c1 == 2 ? 4 : 3, d2 = c2 == 2 ? 4 : 3, d0 = c0 == 2 ? 4 : 3;
            if (k > d0 + d1 + d2) continue;
            double tk = 0.0;  /* term[k] = sum_i B[0][c0][i] * minor[k - i] */
            for (int i = 0; i <= d0; ++i) {
                const int j = k - i;
                if (j < 0 || j > d1 + d2) continue;
                double m1 = 0.0, m2 = 0.0;  /* minor[j] = (B[1][c1] B[2][c2] - B[1][c2] B[2][c1])[j] */
                for (int a = 0; a <= d1; ++a) {
                    const int b = j - a;
                    if (b >= 0 && b <= d2) m1 += S.B[15 + 5 * c1 + a] * S.B[30 + 5 * c2 + b];
                }
                for (int a = 0; a <= d2; ++a) {
                    const int b = j - a;
                    if (b >= 0 && b <= d1) m2 += S.B[15 + 5 * c2 + a] * S.B[30 + 5 * c1 + b];
                }
                tk += S.B[5 * c0 + i] * (m1 - m2);
            }
            pk += tk;
        }
        S.poly[k] = pk;
    }
    wave_sync_lds();
    // ---- the real roots of poly: Durand-Kerner, root k on lane k ----
    double cmax = 0.0;
    for (int k = 0; k <= 10; ++k) cmax = fmax(cmax, fabs(S.poly[k]));
    if (!(cmax > 0.0)) return 0;
    int deg = 10;
    for (; deg > 0; --deg) {  // a leading coefficient that puts a root beyond 1e14 counts as zero (solve_oracle.c, real_roots10)
        double t = fabs(S.poly[deg]);
        bool beyond = false;
        for (int k = deg - 1; k >= 0; --k) {
            t *= 1e14;
            if (fabs(S.poly[k]) > t) beyond = true;
        }
        if (!beyond) break;
    }
    if (deg == 0) return 0;
    const double lead = S.poly[deg];
    if (lane <= deg) S.mon[lane] = S.poly[lane] / lead;  /* monic */
    wave_sync_lds();
    double bound = 0.0;
    for (int k = 0; k < deg; ++k) bound = fmax(bound, fabs(S.mon[k]));
    bound += 1.0;
    double zr = 0.0, zi = 0.0;
    {
        double r0 = 1.0;
        const double a0 = fabs(S.mon[0]);
        if (a0 > 0.0) {
            double y = 1.0;  // the first power of two whose deg-th power reaches a0 (why not a0 itself: solve_oracle.c, real_roots10)
            for (;;) {
                double yp = 1.0;
                for (int j = 0; j < deg; ++j) yp *= y;
                if (!(yp < a0)) break;
                y *= 2.0;
            }
            for (int it = 0; it < 24; ++it) {
                double yp = 1.0;
                for (int j = 0; j < deg - 1; ++j) yp *= y;
                y = ((deg - 1) * y + a0 / yp) / deg;
            }
            r0 = y;
        }
        r0 = fmin(fmax(r0, 0.5), bound);
        double cr = 1.0, ci = 0.0;
        for (int k = 0; k < deg; ++k) {
            if (k == lane) zr = r0 * cr, zi = r0 * ci;
            const double tr = cr * 0.4 - ci * 0.9, ti = cr * 0.9 + ci * 0.4;
            cr = tr, ci = ti;
        }
    }
    const bool mine = lane < deg;
#ifndef E5_EXP_DK_SWEEPS
#define E5_EXP_DK_SWEEPS 200
#endif
    // one sweep: this lane's correction from the iterates the sweep starts with. The sweeps end when no lane's correction exceeds
    // 1e-11 (1 + |zr| + |zi|) of the iterate it was computed from: every lane tests its own root (a NaN correction asks for no
    // further sweep, there and here); why per root and not against the root bound, and the sweep limit: see the CPU
    // restatement (solve_oracle.c, real_roots10)
    auto correct = [&](double pr, double pi, double dr, double di) {
        const double den = dr * dr + di * di;
        bool more = false;
        if (mine && den > 0.0) {
            const double qr = (pr * dr + pi * di) / den, qi = (pi * dr - pr * di) / den;
            more = fabs(qr) + fabs(qi) > 1e-11 * (1.0 + fabs(zr) + fabs(zi));
            zr -= qr;
            zi -= qi;
        }
        return __ballot(more) == 0ull;
    };
    if (deg == 10) {  // the usual case: coefficients in registers, the other iterates by v_readlane with constant lanes
        double mm[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) mm[j] = S.mon[j];
        for (int it = 0; it < E5_EXP_DK_SWEEPS; ++it) {
            double pr = 1.0, pi = 0.0;  /* Horner on the monic polynomial */
#pragma unroll
            for (int j = 9; j >= 0; --j) {
                const double tr = pr * zr - pi * zi + mm[j], ti = pr * zi + pi * zr;
                pr = tr, pi = ti;
            }
            double dr = 1.0, di = 0.0;
#pragma unroll
            for (int j = 0; j < 10; ++j) {
                const double zrj = readlane_f64(zr, j), zij = readlane_f64(zi, j);
                if (j != lane) {
                    const double ar = zr - zrj, ai = zi - zij;
                    const double tr = dr * ar - di * ai, ti = dr * ai + di * ar;
                    dr = tr, di = ti;
                }
            }
            if (correct(pr, pi, dr, di)) break;
        }
    } else {
        for (int it = 0; it < E5_EXP_DK_SWEEPS; ++it) {
            double pr = 1.0, pi = 0.0;
            for (int j = deg - 1; j >= 0; --j) {
                const double mj = S.mon[j];
                const double tr = pr * zr - pi * zi + mj, ti = pr * zi + pi * zr;
                pr = tr, pi = ti;
            }
            double dr = 1.0, di = 0.0;
            for (int j = 0; j < deg; ++j) {
                const double zrj = readlane_f64(zr, j), zij = readlane_f64(zi, j);  // (j is wave-uniform: two v_readlane, no LDS permute)
                if (j != lane) {
                    const double ar = zr - zrj, ai = zi - zij;
                    const double tr = dr * ar - di * ai, ti = dr * ai + di * ar;
                    dr = tr, di = ti;
                }
            }
            if (correct(pr, pi, dr, di)) break;
        }
    }
    bool real = mine && !(fabs(zi) > 1e-7 * (1.0 + fabs(zr)));
    double z = zr;
    if (real)
        for (int it = 0; it < 4; ++it) {  /* Newton polish on the real polynomial */
            double p = S.poly[deg], d = 0.0;
            for (int j = deg - 1; j >= 0; --j) {
                d = d * z + p;
                p = p * z + S.poly[j];
            }
            if (!(fabs(d) > 0.0)) break;
            z -= p / d;
        }
    // position of this root in the ascending list (the sequential insertion sort is stable)
    int rank = 0;
    for (int j = 0; j < deg; ++j) {
        const double zj = __shfl(z, j);
        const int rj = __shfl((int)real, j);
        if (rj && (zj < z || (zj == z && j < lane))) ++rank;
    }
    // ---- x, y and the polish, a real root per lane ----
    bool ok = false;
    double Ev[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) Ev[e] = 0.0;
    if (real) {
        double b[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double v = S.B[15 * i + 5 * j + 4];
#pragma unroll
                for (int k = 3; k >= 0; --k) v = v * z + S.B[15 * i + 5 * j + k];
                b[i][j] = v;
            }
        /* [x y 1]^T spans the null space of b: two of its rows, the pair with the largest 2 x 2 determinant */
        const double d01 = b[0][0] * b[1][1] - b[0][1] * b[1][0], d02 = b[0][0] * b[2][1] - b[0][1] * b[2][0], d12 = b[1][0] * b[2][1] - b[1][1] * b[2][0];
        int bp = 0;
        double bd = 0.0;
        if (fabs(d01) > fabs(bd)) bd = d01, bp = 0;
        if (fabs(d02) > fabs(bd)) bd = d02, bp = 1;
        if (fabs(d12) > fabs(bd)) bd = d12, bp = 2;
        if (fabs(bd) > 0.0) {
            double u0[3], u1[3];  // the two rows chosen
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                u0[c] = bp == 2 ? b[1][c] : b[0][c];
                u1[c] = bp == 0 ? b[1][c] : b[2][c];
            }
            double x = (u0[1] * u1[2] - u0[2] * u1[1]) / bd;
            double y = (u0[2] * u1[0] - u0[0] * u1[2]) / bd;
            double zz = z;
#ifndef E5_EXP_POLISH
#define E5_EXP_POLISH 3
#endif
            for (int it = 0; it < E5_EXP_POLISH; ++it) {  /* three Gauss-Newton steps on the ten constraints themselves, in (x, y, z) */
                // (rolled loops and powers by selection: unrolled, the 20 monomials and their derivatives are ~100 live registers
                // per lane and the kernel spills; the monomial's column comes from a 64-byte table)
                const double x2 = x * x, x3 = x * x * x, y2 = y * y, y3 = y * y * y, z2 = zz * zz, z3 = zz * zz * zz;
                auto pw = [](double v1, double v2, double v3, int e) { return e == 0 ? 1.0 : (e == 1 ? v1 : (e == 2 ? v2 : v3)); };
                double JtJ[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, Jtr[3] = {0, 0, 0};
#pragma clang loop unroll(disable)
                for (int row = 0; row < 10; ++row) {
                    double rv = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
#pragma clang loop unroll(disable)
                    for (int ex = 0; ex <= 3; ++ex)
#pragma clang loop unroll(disable)
                        for (int ey = 0; ex + ey <= 3; ++ey)
#pragma clang loop unroll(disable)
                            for (int ez = 0; ex + ey + ez <= 3; ++ez) {
                                const double cf = S.A0[row * 20 + S.mcol[16 * ex + 4 * ey + ez]];
                                const double pxe = pw(x, x2, x3, ex), pye = pw(y, y2, y3, ey), pze = pw(zz, z2, z3, ez);
                                rv += cf * (pxe * pye) * pze;
                                if (ex) g0 += cf * (ex * pw(x, x2, x3, ex - 1) * pye) * pze;
                                if (ey) g1 += cf * (pxe * (ey * pw(y, y2, y3, ey - 1))) * pze;
                                if (ez) g2 += cf * (pxe * pye) * (ez * pw(zz, z2, z3, ez - 1));
                            }
                    const double g[3] = {g0, g1, g2};
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        Jtr[u] += g[u] * rv;
#pragma unroll
                        for (int v = 0; v < 3; ++v) JtJ[u][v] += g[u] * g[v];
                    }
                }
                /* 3 x 3 solve by cofactors */
                const double c00 = JtJ[1][1] * JtJ[2][2] - JtJ[1][2] * JtJ[2][1], c01 = JtJ[1][2] * JtJ[2][0] - JtJ[1][0] * JtJ[2][2],
                             c02 = JtJ[1][0] * JtJ[2][1] - JtJ[1][1] * JtJ[2][0];
                const double dt = JtJ[0][0] * c00 + JtJ[0][1] * c01 + JtJ[0][2] * c02;
                if (!(fabs(dt) > 0.0)) break;
                const double c10 = JtJ[0][2] * JtJ[2][1] - JtJ[0][1] * JtJ[2][2], c11 = JtJ[0][0] * JtJ[2][2] - JtJ[0][2] * JtJ[2][0],
                             c12 = JtJ[0][1] * JtJ[2][0] - JtJ[0][0] * JtJ[2][1];
                const double c20 = JtJ[0][1] * JtJ[1][2] - JtJ[0][2] * JtJ[1][1], c21 = JtJ[0][2] * JtJ[1][0] - JtJ[0][0] * JtJ[1][2],
                             c22 = JtJ[0][0] * JtJ[1][1] - JtJ[0][1] * JtJ[1][0];
                const double dx = (c00 * Jtr[0] + c10 * Jtr[1] + c20 * Jtr[2]) / dt;
                const double dy = (c01 * Jtr[0] + c11 * Jtr[1] + c21 * Jtr[2]) / dt;
                const double dz = (c02 * Jtr[0] + c12 * Jtr[1] + c22 * Jtr[2]) / dt;
                if (!(fabs(dx) + fabs(dy) + fabs(dz) < 1e300)) break;
                x -= dx, y -= dy, zz -= dz;
            }
            double nrm = 0.0;
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                Ev[e] = S.lin[4 * e] * x + S.lin[4 * e + 1] * y + S.lin[4 * e + 2] * zz + S.lin[4 * e + 3];
                nrm += Ev[e] * Ev[e];
            }
            nrm = sqrt(nrm);
            if (nrm > 0.0 && nrm < 1e300) {
                ok = true;
#pragma unroll
                for (int e = 0; e < 9; ++e) Ev[e] = Ev[e] / nrm;
            }
        }
    }
    // the models leave in ascending root order, the failed ones squeezed out
    int slot = 0, n = 0;
    for (int j = 0; j < deg; ++j) {
        const int okj = __shfl((int)ok, j), rkj = __shfl(rank, j);
        n += okj;
        if (okj && rkj < rank) ++slot;
    }
    if (ok)
#pragma unroll
        for (int e = 0; e < 9; ++e) Eout[9 * slot + e] = Ev[e];
    return n;
}

/* least squares min |A x - b| for an R x C system (C <= R <= 6, C <= 5), Householder QR on a copy, every loop unrolled: the working array and the
 * callers' matrices stay in registers (as run-time-indexed arrays they are scratch memory). Returns 0 if a column collapses. Same
 * operations in the same order as lsq_small(R, C, ...) of the CPU restatement (solve_oracle.c). */
template <int R, int C>
__device__ __forceinline__ int lsq_rc(const double* A, const double* b, double* x) {
    constexpr int r = R, c = C;
    static_assert(C <= R && R <= 6, "an over-determined or square system of at most six rows");
    double Q[R][C + 1];
#pragma unroll
    for (int i = 0; i < r; ++i) {
#pragma unroll
        for (int j = 0; j < c; ++j) Q[i][j] = A[i * c + j];
        Q[i][c] = b[i];
    }
#pragma unroll
    for (int j = 0; j < c; ++j) {
        double nrm = 0.0;
#pragma unroll
        for (int i = j; i < r; ++i) nrm += Q[i][j] * Q[i][j];
        nrm = sqrt(nrm);
        if (!(nrm > 0.0)) return 0;
        const double alpha = Q[j][j] > 0.0 ? -nrm : nrm;
        double v[6];
#pragma unroll
        for (int i = j; i < r; ++i) v[i] = Q[i][j];
        v[j] -= alpha;
        double vv = 0.0;
#pragma unroll
        for (int i = j; i < r; ++i) vv += v[i] * v[i];
        if (!(vv > 0.0)) return 0;
#pragma unroll
        for (int k = j; k <= c; ++k) {
            double d = 0.0;
#pragma unroll
            for (int i = j; i < r; ++i) d += v[i] * Q[i][k];
            d = 2.0 * d / vv;
#pragma unroll
            for (int i = j; i < r; ++i) Q[i][k] -= d * v[i];
        }
        Q[j][j] = alpha;
    }
#pragma unroll
    for (int j = c - 1; j >= 0; --j) {
        double s = Q[j][c];
#pragma unroll
        for (int k = j + 1; k < c; ++k) s -= Q[j][k] * x[k];
        x[j] = s / Q[j][j];
    }
#pragma unroll
    for (int j = 0; j < c; ++j)
        if (!(fabs(x[j]) < 1e300)) return 0;
    return 1;
}
template <int C>
__device__ __forceinline__ int lsq6(const double* A, const double* b, double* x) { return lsq_rc<6, C>(A, b, x); }

// The N x N eigenproblem (N = 9, 12) by ONE WAVE on one shared copy of A and V, in the ROUND-ROBIN ordering of
// the CPU restatement (solve_oracle.c)'s jacobi_eig_rr: a sweep is N' - 1 rounds of N' / 2 disjoint rotations (N' = N rounded up to even; position 0
// holds index 0, position j >= 1 holds 1 + ((j - 1 - round) mod (N' - 1)), pair i = positions i and N' - 1 - i, index N is a bye).
// The unit of work is an ITEM (pair i, k): a lane owns item `lane` and, for N = 12, item 64 + lane (72 items). The lane forms the rotation of
// its items' pairs ITSELF from the matrix the round starts with (the same operations on the same values in every lane that
// needs them: the same bits, and no trip through LDS and no barrier to hand six rotations round), then the two stages —
// columns p, q of row k; rows p, q at column k together with the eigenvector columns — run with every read of a stage issued before
// its first write: no element is written twice inside a stage and none is read by another item after it was written, and element by
// element the arithmetic is the restatement's, so the result is the same bits. A wave's LDS operations execute in program order:
// the barriers only pin the compiler. (Until round 5 lanes 0..5 formed the rotations and handed them over through LDS, and a
// stage made two dependent passes over its 72 items: ~3.7 k cycles per round, 133 us for the front half of a five-point EPnP sample.)
struct JacRound {   // (kept for the callers' LDS layouts; the rotations no longer pass through it)
    double c[8], s[8];
    int p[8], q[8], on[8];
};
template <int N>
__device__ __forceinline__ void jacobi_wave(double* A, double* V, double* w, JacRound& R) {
    (void)R;
    constexpr int n = N, np = N + (N & 1), half = np / 2;
    constexpr int ITEMS = half * n, PASSES = (ITEMS + 63) / 64;
    const int lane = threadIdx.x & 63;
    for (int e = lane; e < n * n; e += 64) V[e] = (e / n == e % n) ? 1.0 : 0.0;
    wave_sync_lds();
#ifndef JAC_EXP_SWEEPS
#define JAC_EXP_SWEEPS 60
#endif
    for (int sweep = 0; sweep < JAC_EXP_SWEEPS; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < n; ++p) {
            diag += A[p * n + p] * A[p * n + p];
            for (int q = p + 1; q < n; ++q) off += A[p * n + q] * A[p * n + q];
        }
        if (off <= 1e-60 || off <= 1e-32 * diag) break;
        for (int round = 0; round < np - 1; ++round) {
            int ip[PASSES], iq[PASSES], ik[PASSES];
            bool on[PASSES];
            double rc[PASSES], rs[PASSES];
#pragma unroll
            for (int ps = 0; ps < PASSES; ++ps) {
                const int e = lane + 64 * ps, i = e / n, j1 = i, j2 = np - 1 - i;
                ik[ps] = e % n;
                const int a = j1 == 0 ? 0 : 1 + ((j1 - 1 - round) % (np - 1) + (np - 1)) % (np - 1);
                const int b = 1 + ((j2 - 1 - round) % (np - 1) + (np - 1)) % (np - 1);
                const int p = a < b ? a : b, q = a < b ? b : a;
                ip[ps] = p, iq[ps] = q;
                on[ps] = false, rc[ps] = 1.0, rs[ps] = 0.0;
                if (e < ITEMS && q < n) {
                    const double apq = A[p * n + q];
                    if (apq != 0.0) {
                        const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        rc[ps] = 1.0 / sqrt(t * t + 1.0), rs[ps] = t * rc[ps];
                        on[ps] = true;
                    }
                }
            }
            {   /* columns p, q of every pair: row k of the item */
                double akp[PASSES], akq[PASSES];
#pragma unroll
                for (int ps = 0; ps < PASSES; ++ps)
                    if (on[ps]) akp[ps] = A[ik[ps] * n + ip[ps]], akq[ps] = A[ik[ps] * n + iq[ps]];
                wave_sync_lds();   // (every lane's reads of the round's start, the pivots above included, before the first write)
#pragma unroll
                for (int ps = 0; ps < PASSES; ++ps)
                    if (on[ps]) {
                        A[ik[ps] * n + ip[ps]] = rc[ps] * akp[ps] - rs[ps] * akq[ps];
                        A[ik[ps] * n + iq[ps]] = rs[ps] * akp[ps] + rc[ps] * akq[ps];
                    }
            }
            wave_sync_lds();
            {   /* rows p, q of every pair at column k; the eigenvector columns */
                double apk[PASSES], aqk[PASSES], vkp[PASSES], vkq[PASSES];
#pragma unroll
                for (int ps = 0; ps < PASSES; ++ps)
                    if (on[ps]) {
                        apk[ps] = A[ip[ps] * n + ik[ps]], aqk[ps] = A[iq[ps] * n + ik[ps]];
                        vkp[ps] = V[ik[ps] * n + ip[ps]], vkq[ps] = V[ik[ps] * n + iq[ps]];
                    }
                wave_sync_lds();
#pragma unroll
                for (int ps = 0; ps < PASSES; ++ps)
                    if (on[ps]) {
                        A[ip[ps] * n + ik[ps]] = rc[ps] * apk[ps] - rs[ps] * aqk[ps];
                        A[iq[ps] * n + ik[ps]] = rs[ps] * apk[ps] + rc[ps] * aqk[ps];
                        V[ik[ps] * n + ip[ps]] = rc[ps] * vkp[ps] - rs[ps] * vkq[ps];
                        V[ik[ps] * n + iq[ps]] = rs[ps] * vkp[ps] + rc[ps] * vkq[ps];
                    }
            }
            wave_sync_lds();
        }
    }
    for (int i = 0; i < n; ++i) w[i] = A[i * n + i];
}

/* homography4 by one wave: L^T L (shared, an upper-triangle entry per lane, the four points added in order), the 9 x 9 eigenproblem by
 * jacobi_wave, the rest on identical values in every lane. a, b: this sample's 4 x 2 points. Returns 1 / 0; H (9) valid in every lane. */
__device__ static int homography4_wave(const double* a, const double* b, double* H, double* LtL /* 81 */, double* V /* 81 */, JacRound& R) {
    const int lane = threadIdx.x & 63;
    const int count = 4;
    double cM[2] = {0, 0}, cm[2] = {0, 0}, sM[2] = {0, 0}, sm[2] = {0, 0};
#pragma unroll
    for (int i = 0; i < count; ++i) {
        cM[0] += a[2 * i]; cM[1] += a[2 * i + 1];
        cm[0] += b[2 * i]; cm[1] += b[2 * i + 1];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) cM[k] /= count, cm[k] /= count;
#pragma unroll
    for (int i = 0; i < count; ++i)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            sM[k] += fabs(a[2 * i + k] - cM[k]);
            sm[k] += fabs(b[2 * i + k] - cm[k]);
        }
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (fabs(sM[k]) < 2.220446049250313e-16 || fabs(sm[k]) < 2.220446049250313e-16) return 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) sM[k] = count / sM[k], sm[k] = count / sm[k];
    for (int e = lane; e < 81; e += 64) {
        const int j = e / 9, k = e % 9;
        if (k < j) continue;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < count; ++i) {
            const double x = (b[2 * i] - cm[0]) * sm[0], y = (b[2 * i + 1] - cm[1]) * sm[1];
            const double X = (a[2 * i] - cM[0]) * sM[0], Y = (a[2 * i + 1] - cM[1]) * sM[1];
            const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x};
            const double Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
            double lxj = 0, lxk = 0, lyj = 0, lyk = 0;
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                if (q == j) lxj = Lx[q], lyj = Ly[q];
                if (q == k) lxk = Lx[q], lyk = Ly[q];
            }
            acc += lxj * lxk + lyj * lyk;
        }
        LtL[j * 9 + k] = acc;
        LtL[k * 9 + j] = acc;
    }
    wave_sync_lds();
    double w[9];
    jacobi_wave<9>(LtL, V, w, R);
    int best = 0;
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        double wb = 0;
#pragma unroll
        for (int q = 0; q < 9; ++q)
            if (q == best) wb = w[q];
        if (w[i] < wb) best = i;
    }
    double H0[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) H0[k] = V[k * 9 + best];
    const double inv[9] = {1.0 / sm[0], 0, cm[0], 0, 1.0 / sm[1], cm[1], 0, 0, 1};
    const double n2[9] = {sM[0], 0, -cM[0] * sM[0], 0, sM[1], -cM[1] * sM[1], 0, 0, 1};
    double T[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) T[3 * r + c] = inv[3 * r] * H0[c] + inv[3 * r + 1] * H0[3 + c] + inv[3 * r + 2] * H0[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) H[3 * r + c] = T[3 * r] * n2[c] + T[3 * r + 1] * n2[3 + c] + T[3 * r + 2] * n2[6 + c];
    if (!(fabs(H[8]) > 0.0)) return 0;
    const double s = 1.0 / H[8];
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] *= s;
    return 1;
}

/* ---- seven-point (fundamental matrix), one WAVE per sample ------------------------------------------------------------------
 * OpenCV 4.5.5's run7Point (fundam.cpp) restated, with two deliberate deviations:
 *   1. HARTLEY NORMALISATION. Each image's seven points are translated to their centroid (p0 + (sum of (pi - p0)) / 7) and scaled so
 *      that their mean distance from it is sqrt(2) (sums in index order, every operation rounded on its own), the models are denormalised as
 *      T2^T F^ T1. OpenCV solves on raw pixels with a one-sided Jacobi SVD of the 7 x 9 system; here the null space comes from
 *      the 9 x 9 eigen-solver on A^T A (jacobi_wave<9>, what homography4_wave uses), which squares the condition number: on raw
 *      pixels that form is useless (held-out epipolar errors above 1e4 px^2 on exact data), normalised it is better than
 *      OpenCV's own (1e-11 against 8e-5 px^2).
 *   2. SCALING. A model leaves with unit Frobenius norm, as ESSENTIAL5 emits its models, not with F[8] = 1 (which OpenCV gives
 *      up on when F[8] ~ 0).
 * Steps: the normalisations; A^T A shared (an upper-triangle entry per lane, the seven points added in order; row of a
 * correspondence = x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1); jacobi_wave<9>; f2 = the eigenvector of the smallest eigenvalue,
 * f1 = that of the second smallest (first of equals by strict <), minus f2; the cubic det(z f1 + f2) by run7Point's four c[]
 * expressions in the order written below; its real roots by real_roots3; per root F^ = f1 z + f2, denormalised, / its norm.
 * Everything after the eigen-solver runs on identical values in every lane.
 * A DEGENERATE sample is no error: 0 models when a normalisation scale is not finite (all points of an image coincide, or a
 * coordinate is not finite), when the cubic is all zero, or when no real root is left; a root whose model has no finite positive
 * norm is squeezed out.
 *
 * real_roots3: the Durand-Kerner recipe essential5_wave / real_roots10 (solve_oracle.c) had when this kind was added, for degree <= 3,
 * run sequentially (the five-point solver has since changed its degree drop, start and stop test; this copy keeps the recipe below):
 * degree drop at 1e-14 cmax, monic, the start values r0 (0.4 + 0.9 i)^k with r0 = |m0|^(1/deg) by 80 Newton steps clamped to
 * [0.5, bound], at most 200 simultaneous sweeps stopped at a largest correction of 1e-11 bound, a root is real iff
 * |zi| <= 1e-7 (1 + |zr|), four Newton steps on the real polynomial, real roots ascending (equals in iterate order).
 * Only + - * / sqrt, fabs, fmax, fmin: the CPU restatement (tests/cpp/fundamental_reference.c) gives the same bits. */
__device__ __forceinline__ int real_roots3(double c0, double c1, double c2, double c3 /* c0 + c1 z + c2 z^2 + c3 z^3 */, double* roots /* 3 */) {
    // (the coefficients by value and the leading one picked in the branches: as an array indexed by the degree they went to scratch)
    double cmax = 0.0;
    cmax = fmax(cmax, fabs(c0));
    cmax = fmax(cmax, fabs(c1));
    cmax = fmax(cmax, fabs(c2));
    cmax = fmax(cmax, fabs(c3));
    if (!(cmax > 0.0)) return 0;
    int deg = 3;
    double lead = c3;
    if (fabs(c3) <= 1e-14 * cmax) {
        deg = 2, lead = c2;
        if (fabs(c2) <= 1e-14 * cmax) {
            deg = 1, lead = c1;
            if (fabs(c1) <= 1e-14 * cmax) deg = 0;
        }
    }
    if (deg == 0) return 0;
    const double c[3] = {c0, c1, c2};
    double m[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] = k < deg ? c[k] / lead : 0.0;
    double bound = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < deg) bound = fmax(bound, fabs(m[k]));
    bound += 1.0;
    double zr[3] = {0, 0, 0}, zi[3] = {0, 0, 0};
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
        for (int k = 0; k < 3; ++k) {
            if (k < deg) zr[k] = r0 * cr, zi[k] = r0 * ci;
            const double tr = cr * 0.4 - ci * 0.9, ti = cr * 0.9 + ci * 0.4;
            cr = tr, ci = ti;
        }
    }
    for (int it = 0; it < 200; ++it) {
        double change = 0.0, nzr[3], nzi[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            nzr[k] = zr[k], nzi[k] = zi[k];
            double pr = 1.0, pi = 0.0;  /* Horner on the monic polynomial */
#pragma unroll
            for (int j = 2; j >= 0; --j)
                if (j < deg) {
                    const double tr = pr * zr[k] - pi * zi[k] + m[j], ti = pr * zi[k] + pi * zr[k];
                    pr = tr, pi = ti;
                }
            double dr = 1.0, di = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j)
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
        for (int k = 0; k < 3; ++k) zr[k] = nzr[k], zi[k] = nzi[k];
        if (change <= 1e-11 * bound) break;
    }
    double z[3] = {0, 0, 0};
    bool real[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        real[k] = k < deg && !(fabs(zi[k]) > 1e-7 * (1.0 + fabs(zr[k])));
        double v = zr[k];
        bool going = real[k];
#pragma unroll
        for (int it = 0; it < 4; ++it) {  /* Newton polish on the real polynomial: stops for good at a zero derivative */
            double p = lead, d = 0.0;
#pragma unroll
            for (int j = 2; j >= 0; --j)
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
    for (int k = 0; k < 3; ++k) n += real[k];
#pragma unroll
    for (int s = 0; s < 3; ++s) roots[s] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j != k && real[j] && (z[j] < z[k] || (z[j] == z[k] && j < k))) ++rank;
#pragma unroll
        for (int s = 0; s < 3; ++s)
            if (real[k] && rank == s) roots[s] = z[k];
    }
    return n;
}

// centroid and scale of a sample's seven points in one image; false: the scale is not finite
__device__ __forceinline__ bool f7_normalisation(const double* p, double& cx, double& cy, double& s) {
    // the centroid as p0 + (sum of (pi - p0)) / 7: seven coincident points give differences, distances and a mean distance of exactly 0
    // (as (sum of pi) / 7 the centroid of seven equal points can miss them by an ulp, and the scale comes out finite and huge)
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int i = 0; i < 7; ++i) sx += p[2 * i] - p[0], sy += p[2 * i + 1] - p[1];
    cx = p[0] + sx / 7.0, cy = p[1] + sy / 7.0;
    double d = 0.0;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const double dx = p[2 * i] - cx, dy = p[2 * i + 1] - cy;
        d += sqrt(dx * dx + dy * dy);
    }
    d = d / 7.0;
    s = 1.4142135623730951 / d;
    return s <= 1.7976931348623157e308;   // (false for a NaN as well)
}

/* a, b: this sample's 7 x 2 points of image 1 / image 2. Returns the number of models (0..3); F (27, the slots behind the count
 * zero) valid in every lane. */
__device__ static int fundamental7_wave(const double* a, const double* b, double* F, double* AtA /* 81 */, double* V /* 81 */, JacRound& R) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 27; ++k) F[k] = 0.0;
    double c1x, c1y, s1, c2x, c2y, s2;
    const bool ok1 = f7_normalisation(a, c1x, c1y, s1), ok2 = f7_normalisation(b, c2x, c2y, s2);
    if (!ok1 || !ok2) return 0;   // (wave-uniform)
    for (int e = lane; e < 81; e += 64) {
        const int j = e / 9, k = e % 9;
        if (k < j) continue;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const double x1 = (a[2 * i] - c1x) * s1, y1 = (a[2 * i + 1] - c1y) * s1;
            const double x2 = (b[2 * i] - c2x) * s2, y2 = (b[2 * i + 1] - c2y) * s2;
            const double row[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0};
            double rj = 0, rk = 0;
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                if (q == j) rj = row[q];
                if (q == k) rk = row[q];
            }
            acc += rj * rk;
        }
        AtA[j * 9 + k] = acc;
        AtA[k * 9 + j] = acc;
    }
    wave_sync_lds();
    double w[9];
    jacobi_wave<9>(AtA, V, w, R);
    int lo = 0, lo2 = -1;
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        double wb = 0;
#pragma unroll
        for (int q = 0; q < 9; ++q)
            if (q == lo) wb = w[q];
        if (w[i] < wb) lo = i;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        if (i == lo) continue;
        double wb = 0;
#pragma unroll
        for (int q = 0; q < 9; ++q)
            if (q == lo2) wb = w[q];
        if (lo2 < 0 || w[i] < wb) lo2 = i;
    }
    double f1[9], f2[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        f2[k] = V[k * 9 + lo];
        f1[k] = V[k * 9 + lo2] - f2[k];
    }
    /* det(z f1 + f2) = c[0] z^3 + c[1] z^2 + c[2] z + c[3], run7Point's expressions */
    double c[4], t0, t1, t2;
    t0 = f2[4] * f2[8] - f2[5] * f2[7];
    t1 = f2[3] * f2[8] - f2[5] * f2[6];
    t2 = f2[3] * f2[7] - f2[4] * f2[6];
    c[3] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2;
    c[2] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2 - f1[3] * (f2[1] * f2[8] - f2[2] * f2[7]) + f1[4] * (f2[0] * f2[8] - f2[2] * f2[6]) -
           f1[5] * (f2[0] * f2[7] - f2[1] * f2[6]) + f1[6] * (f2[1] * f2[5] - f2[2] * f2[4]) - f1[7] * (f2[0] * f2[5] - f2[2] * f2[3]) +
           f1[8] * (f2[0] * f2[4] - f2[1] * f2[3]);
    t0 = f1[4] * f1[8] - f1[5] * f1[7];
    t1 = f1[3] * f1[8] - f1[5] * f1[6];
    t2 = f1[3] * f1[7] - f1[4] * f1[6];
    c[1] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2 - f2[3] * (f1[1] * f1[8] - f1[2] * f1[7]) + f2[4] * (f1[0] * f1[8] - f1[2] * f1[6]) -
           f2[5] * (f1[0] * f1[7] - f1[1] * f1[6]) + f2[6] * (f1[1] * f1[5] - f1[2] * f1[4]) - f2[7] * (f1[0] * f1[5] - f1[2] * f1[3]) +
           f2[8] * (f1[0] * f1[4] - f1[1] * f1[3]);
    c[0] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2;
    double roots[3];
    const int nr = real_roots3(c[3], c[2], c[1], c[0], roots);
    /* T2^T = [s2 0 0; 0 s2 0; -c2x s2, -c2y s2, 1], T1 = [s1 0 -c1x s1; 0 s1 -c1y s1; 0 0 1] */
    const double t2t[9] = {s2, 0, 0, 0, s2, 0, -c2x * s2, -c2y * s2, 1};
    const double t1m[9] = {s1, 0, -c1x * s1, 0, s1, -c1y * s1, 0, 0, 1};
    int n = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double Fh[9], T[9], G[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Fh[k] = f1[k] * roots[r] + f2[k];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) T[3 * i + j] = t2t[3 * i] * Fh[j] + t2t[3 * i + 1] * Fh[3 + j] + t2t[3 * i + 2] * Fh[6 + j];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) G[3 * i + j] = T[3 * i] * t1m[j] + T[3 * i + 1] * t1m[3 + j] + T[3 * i + 2] * t1m[6 + j];
        double nrm = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) nrm += G[k] * G[k];
        nrm = sqrt(nrm);
        const bool emit = r < nr && nrm > 0.0 && nrm < 1e300;
#pragma unroll
        for (int k = 0; k < 9; ++k) {   // slot n (0 <= n <= r) by selection: no run-time index into F
#pragma unroll
            for (int s = 0; s < 3; ++s)
                if (s <= r && emit && s == n) F[9 * s + k] = G[k] / nrm;
        }
        n += emit;
    }
    return n;
}

/* ---- EPnP ------------------------------------------------------------------------------------------------------ */
// EPnP by one wave. Lane l accumulates the points l, l + 64, ... of every pass over the points; the partial sums are added in
// lane order — for at most 64 points that is the sequential sum over the points, bit for bit, and the CPU restatement defines the
// sums of more than 64 points the same way (64 strided partials) — and the small dense algebra then runs on identical values in
// every lane, with everything that is indexed at run time (M^T M, its eigenvectors, the 6 x 10 distance system) in one SHARED
// copy in LDS. BIG = false: samples of at most 64 points (the RANSAC loop's 5-point samples: a point per lane, its two rows
// of the projection system parked in LDS, an entry of M^T M per lane) — 16 KB of LDS per wave, ten waves per CU; BIG = true: the
// all-inlier refit, any number of points, a private partial M^T M per lane (40 KB).
struct PnpLds {
    double red[64];
    double A[144], V[144];   // M^T M and its eigenvectors
    double ev[48], L[60];    // the four null vectors, the distance system
    JacRound R;
};

// sum of one value per lane in LANE ORDER over the first `terms` lanes, ((v0 + v1) + v2) + ..., returned to every lane
__device__ __forceinline__ double ordered_wave_sum(double v, double* red, int terms) {
    red[threadIdx.x & 63] = v;
    wave_sync_lds();
    double t = red[0];
    for (int l = 1; l < terms; ++l) t += red[l];
    wave_sync_lds();
    return t;
}

// What the front half leaves in registers (identical in every lane) for the back half: the control-point frame and the six squared
// control-point distances; the four null vectors (S.ev) and the distance system (S.L) stay in LDS.
struct PnpFrame {
    double c0[3], ax[3][3], sc[3], rho[6];
    bool planar;  // a coplanar point set: three control points (sc[2] == 0 marks it in the stored frame), see epnp_front
};

// Front half, ONE WAVE per sample: control points, M^T M (shared), its eigenvectors by jacobi_wave, the distance system.
template <bool BIG>
__device__ static int epnp_front(int m, const int* idx, const double* obj, const double* img, const double* K, PnpFrame& F, PnpLds& S,
                                 double* rows /* !BIG: 64 x 24 */, double* part /* BIG: 78 x 64 */) {
    if (m < 4 || (!BIG && m > 64)) return 0;
    const int lane = threadIdx.x & 63;
    const int terms = m < 64 ? m : 64;  // lanes that hold a partial sum
    auto total = [&](double v) { return ordered_wave_sum(v, S.red, terms); };
    const double fu = K[0], uc = K[2], fv = K[1], vc = K[3];
    double (&c0)[3] = F.c0;
    double (&ax)[3][3] = F.ax;
    double (&sc)[3] = F.sc;
    double (&rho)[6] = F.rho;
    /* control points: centroid + principal axes scaled by the spread along them */
    c0[0] = c0[1] = c0[2] = 0.0;
    for (int k = lane; k < m; k += 64)
#pragma unroll
        for (int e = 0; e < 3; ++e) c0[e] += obj[3 * (size_t)idx[k] + e];
#pragma unroll
    for (int e = 0; e < 3; ++e) c0[e] = total(c0[e]) / (double)m;
    double C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, V3[9], w3[3];
    for (int k = lane; k < m; k += 64) {
        double d[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) d[e] = obj[3 * (size_t)idx[k] + e] - c0[e];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) C[3 * i + j] += d[i] * d[j];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) C[i] = total(C[i]);
    jacobi_eig<3>(C, V3, w3);
    double wmax = w3[0] > w3[1] ? w3[0] : w3[1];
    wmax = wmax > w3[2] ? wmax : w3[2];
    /* ax[k] = unit axis k, sc[k] = its length: control point k+1 = c0 + sc[k] ax[k] */
    if (!(wmax > 0.0)) return 0;
    const int kmin = w3[1] < w3[0] ? (w3[2] < w3[1] ? 2 : 1) : (w3[2] < w3[0] ? 2 : 0);  // the axis of the smallest spread (ties: the lower index)
    if ((kmin != 0 && !(w3[0] > 1e-12 * wmax)) || (kmin != 1 && !(w3[1] > 1e-12 * wmax)) || (kmin != 2 && !(w3[2] > 1e-12 * wmax))) return 0;  // collinear / coincident
    const double wflat = kmin == 0 ? w3[0] : (kmin == 1 ? w3[1] : w3[2]);
    const bool planar = !(wflat > 1e-12 * wmax);
    F.planar = planar;
    /* A COPLANAR set takes the paper's three-control-point form inside the same arrays (solve_oracle.c's header): the flat axis goes
     * last with length 0 — control point 3 coincides with the centroid and carries barycentric coordinate 0 — and its three
     * diagonal entries of M^T M are set above every eigenvalue of the 9 x 9 part below. A set with volume keeps the axes as the
     * eigenproblem leaves them. */
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int src = !planar ? k : (k == 0 ? (kmin == 0 ? 1 : 0) : (k == 1 ? (kmin == 2 ? 1 : 2) : kmin));
        const double wk = src == 0 ? w3[0] : (src == 1 ? w3[1] : w3[2]);
        sc[k] = (planar && k == 2) ? 0.0 : sqrt(wk / (double)m);
#pragma unroll
        for (int e = 0; e < 3; ++e) ax[k][e] = src == 0 ? V3[3 * e] : (src == 1 ? V3[3 * e + 1] : V3[3 * e + 2]);
    }
#define EPNP_ALPHAS(i, al)                                                                        \
    {                                                                                             \
        double d_[3];                                                                             \
        _Pragma("unroll") for (int e_ = 0; e_ < 3; ++e_) d_[e_] = obj[3 * (size_t)(i) + e_] - c0[e_];               \
        _Pragma("unroll") for (int k_ = 0; k_ < 3; ++k_)                                           \
            (al)[k_ + 1] = (planar && k_ == 2) ? 0.0 : (ax[k_][0] * d_[0] + ax[k_][1] * d_[1] + ax[k_][2] * d_[2]) / sc[k_]; \
        (al)[0] = 1.0 - (al)[1] - (al)[2] - (al)[3];                                              \
    }
    /* M^T M of the 2m x 12 projection system  sum_j alpha_j (fu Xc_j + (uc - u) Zc_j) = 0, same with v */
    if constexpr (!BIG) {
        if (lane < m) {  // this lane's point: its two rows
            double al[4];
            EPNP_ALPHAS(idx[lane], al);
            const double du = uc - img[2 * (size_t)idx[lane]], dv = vc - img[2 * (size_t)idx[lane] + 1];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                rows[24 * lane + 3 * j] = al[j] * fu, rows[24 * lane + 3 * j + 1] = 0.0, rows[24 * lane + 3 * j + 2] = al[j] * du;
                rows[24 * lane + 12 + 3 * j] = 0.0, rows[24 * lane + 12 + 3 * j + 1] = al[j] * fv, rows[24 * lane + 12 + 3 * j + 2] = al[j] * dv;
            }
        }
        wave_sync_lds();
        for (int e = lane; e < 144; e += 64) {  // an entry per lane: the points in order, as the sequential loop adds them
            const int i = e / 12, j = e % 12;
            if (j < i) continue;
            double acc = 0.0;
            for (int k = 0; k < m; ++k) acc += rows[24 * k + i] * rows[24 * k + j] + rows[24 * k + 12 + i] * rows[24 * k + 12 + j];
            S.A[12 * i + j] = acc;
            S.A[12 * j + i] = acc;
        }
        wave_sync_lds();
    } else {
        for (int e = 0; e < 78; ++e) part[64 * e + lane] = 0.0;
        for (int k = lane; k < m; k += 64) {
            double al[4], r1[12], r2[12];
            EPNP_ALPHAS(idx[k], al);
            const double du = uc - img[2 * (size_t)idx[k]], dv = vc - img[2 * (size_t)idx[k] + 1];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                r1[3 * j] = al[j] * fu, r1[3 * j + 1] = 0.0, r1[3 * j + 2] = al[j] * du;
                r2[3 * j] = 0.0, r2[3 * j + 1] = al[j] * fv, r2[3 * j + 2] = al[j] * dv;
            }
            int e = 0;
#pragma unroll
            for (int i = 0; i < 12; ++i)
#pragma unroll
                for (int j = i; j < 12; ++j, ++e) part[64 * e + lane] += r1[i] * r1[j] + r2[i] * r2[j];
        }
        wave_sync_lds();
        for (int e = lane; e < 78; e += 64) {  // entry e of the upper triangle: the 64 partials in lane order
            double t = part[64 * e];
            for (int l = 1; l < 64; ++l) t += part[64 * e + l];
            int i = 0, rem = e;
            while (rem >= 12 - i) rem -= 12 - i, ++i;
            const int j = i + rem;
            S.A[12 * i + j] = t;
            S.A[12 * j + i] = t;
        }
        wave_sync_lds();
    }
    if (planar) {  // rows / columns 9..11 are exact zeros: their diagonal goes above every eigenvalue of the 9 x 9 part
        if (lane == 0) {
            double tr = 0.0;
            for (int i = 0; i < 9; ++i) tr += S.A[13 * i];
            for (int i = 9; i < 12; ++i) S.A[13 * i] = 2.0 * tr + 1.0;
        }
        wave_sync_lds();
    }
    double w[12];
    jacobi_wave<12>(S.A, S.V, w, S.R);
    int ord[4];  /* the four smallest eigenvalues, ascending (ties: lower index first) */
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int best = -1;
        double wbest = 0.0;
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            bool used = false;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < k) used |= ord[q] == i;
            if (!used && (best < 0 || w[i] < wbest)) best = i, wbest = w[i];
        }
        ord[k] = best;
    }
    // ev[k][i] = V[12 i + ord[k]]: the shared copy, an element per lane
    if (lane < 48) {
        const int k = lane / 12, i = lane % 12;
        int o = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q == k) o = ord[q];
        S.ev[12 * k + i] = S.V[12 * i + o];
    }
    wave_sync_lds();
    /* the six control-point distance constraints, quadratic in beta: L (6 x 10) over [b00 b01 b11 b02 b12 b22 b03 b13 b23 b33] */
    double cw[4][3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        cw[0][e] = c0[e];
#pragma unroll
        for (int k = 0; k < 3; ++k) cw[k + 1][e] = c0[e] + sc[k] * ax[k][e];
    }
    {
        constexpr int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
        if (lane < 60) {  // entry (p, col) of L per lane
            const int p = lane / 10, col = lane % 10;
            int i = 0, j = 0, cc = 0;
            for (int jj = 0; jj < 4; ++jj)
                for (int ii = 0; ii <= jj; ++ii, ++cc)
                    if (cc == col) i = ii, j = jj;
            int a_ = 0, b_ = 0;
#pragma unroll
            for (int q = 0; q < 6; ++q)
                if (q == p) a_ = pa[q], b_ = pb[q];
            double di[3], dj[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                di[e] = S.ev[12 * i + 3 * a_ + e] - S.ev[12 * i + 3 * b_ + e];
                dj[e] = S.ev[12 * j + 3 * a_ + e] - S.ev[12 * j + 3 * b_ + e];
            }
            const double d = di[0] * dj[0] + di[1] * dj[1] + di[2] * dj[2];
            S.L[10 * p + col] = i == j ? d : 2.0 * d;
        }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            rho[p] = 0.0;
#pragma unroll
            for (int e = 0; e < 3; ++e) rho[p] += (cw[pa[p]][e] - cw[pb[p]][e]) * (cw[pa[p]][e] - cw[pb[p]][e]);
        }
        wave_sync_lds();
    }
    return 1;
}

// One linearised start of the back half (variant 0 / 1 / 2 = the first 1 / 2 / 3 null vectors' leading terms): least squares for
// the start, five Gauss-Newton steps, Horn's absolute orientation, the reprojection error. Returns the error (< 0: no pose) and
// the pose in cand[12].
template <bool LANE, int variant>
__device__ static double epnp_back_variant(int m, const int* idx, const double* obj, const double* img, const double* K, const PnpFrame& F,
                                           const double* ev, const double* L, size_t es, double* red, double* cand) {
    const int lane = LANE ? 0 : (int)(threadIdx.x & 63);
    const int kstep = LANE ? 1 : 64;
    const int terms = m < 64 ? m : 64;
    auto total = [&](double v) { return LANE ? v : ordered_wave_sum(v, red, terms); };
    const double fu = K[0], fv = K[1], uc = K[2], vc = K[3];
    const double (&c0)[3] = F.c0;
    const double (&ax)[3][3] = F.ax;
    const double (&sc)[3] = F.sc;
    const double (&rho)[6] = F.rho;
    const bool planar = F.planar;
    {
        /* linearised start: the products b_i b_j that involve only the first 1 / 2 / 3 null vectors' leading terms */
        constexpr int ncol[3] = {4, 3, 5};
        constexpr int cols[3][5] = {{0, 1, 3, 6, 0}, {0, 1, 2, 0, 0}, {0, 1, 2, 3, 4}};
        double A[30], x[5], beta[4] = {0, 0, 0, 0};
        if (planar) {
            /* three control points: the distance equations of the pairs (0,1), (0,2), (1,2) = rows 0, 1, 3; start 0 takes the first
             * null vector alone (x = b00), start 1 the first two (x = b00 b01 b11, a square system); there is no third start.
             * Gauss-Newton runs on the unknowns of the start (1 or 2 betas against three equations). */
            if constexpr (variant == 2) {
                return -1.0;
            } else {
                constexpr int rows3[3] = {0, 1, 3}, nb = variant + 1, nc3 = variant == 0 ? 1 : 3;
                double l3[3][3], rho3[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    rho3[p] = rho[rows3[p]];
#pragma unroll
                    for (int j = 0; j < 3; ++j) l3[p][j] = L[(size_t)(10 * rows3[p] + j) * es];
#pragma unroll
                    for (int j = 0; j < nc3; ++j) A[p * nc3 + j] = l3[p][j];
                }
                if (!lsq_rc<3, nc3>(A, rho3, x)) return -1.0;
                const double s = x[0] < 0.0 ? -1.0 : 1.0;
                beta[0] = sqrt(s * x[0]);
                if (variant == 1) {
                    beta[1] = s * x[2] > 0.0 ? sqrt(s * x[2]) : 0.0;
                    if (x[1] < 0.0) beta[0] = -beta[0];
                }
                if (!(beta[0] != 0.0)) return -1.0;
                for (int it = 0; it < 5; ++it) {
                    double J[6], r[3], dx[2];
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                        const double* l = l3[p];
                        J[nb * p] = 2.0 * l[0] * beta[0] + l[1] * beta[1];
                        if (nb == 2) J[nb * p + 1] = l[1] * beta[0] + 2.0 * l[2] * beta[1];
                        r[p] = rho3[p] - (l[0] * beta[0] * beta[0] + l[1] * beta[0] * beta[1] + l[2] * beta[1] * beta[1]);
                    }
                    if (!lsq_rc<3, nb>(J, r, dx)) break;
#pragma unroll
                    for (int k = 0; k < nb; ++k) beta[k] += dx[k];
                }
            }
        } else {
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int j = 0; j < 5; ++j)
                    if (j < ncol[variant]) A[p * ncol[variant] + j] = L[(size_t)(10 * p + cols[variant][j]) * es];
            const int solved = variant == 0 ? lsq6<4>(A, rho, x) : (variant == 1 ? lsq6<3>(A, rho, x) : lsq6<5>(A, rho, x));
            if (!solved) return -1.0;
            if (variant == 0) {  /* x = b00 b01 b02 b03 */
                const double s = x[0] < 0.0 ? -1.0 : 1.0;
                beta[0] = sqrt(s * x[0]);
                if (!(beta[0] > 0.0)) return -1.0;
#pragma unroll
                for (int k = 1; k < 4; ++k) beta[k] = s * x[k] / beta[0];
            } else {             /* x = b00 b01 b11 (b02 b12) */
                const double s = x[0] < 0.0 ? -1.0 : 1.0;
                beta[0] = sqrt(s * x[0]);
                beta[1] = s * x[2] > 0.0 ? sqrt(s * x[2]) : 0.0;
                if (x[1] < 0.0) beta[0] = -beta[0];
                if (!(beta[0] != 0.0)) return -1.0;
                if (variant == 2) beta[2] = x[3] / beta[0];
            }
            for (int it = 0; it < 5; ++it) {  /* Gauss-Newton on the six distance equations */
                double J[24], r[6], dx[4];
#pragma unroll
                for (int p = 0; p < 6; ++p) {
                    double l[10];
#pragma unroll
                    for (int q = 0; q < 10; ++q) l[q] = L[(size_t)(10 * p + q) * es];
                    J[4 * p + 0] = 2.0 * l[0] * beta[0] + l[1] * beta[1] + l[3] * beta[2] + l[6] * beta[3];
                    J[4 * p + 1] = l[1] * beta[0] + 2.0 * l[2] * beta[1] + l[4] * beta[2] + l[7] * beta[3];
                    J[4 * p + 2] = l[3] * beta[0] + l[4] * beta[1] + 2.0 * l[5] * beta[2] + l[8] * beta[3];
                    J[4 * p + 3] = l[6] * beta[0] + l[7] * beta[1] + l[8] * beta[2] + 2.0 * l[9] * beta[3];
                    r[p] = rho[p] - (l[0] * beta[0] * beta[0] + l[1] * beta[0] * beta[1] + l[2] * beta[1] * beta[1] + l[3] * beta[0] * beta[2] +
                                     l[4] * beta[1] * beta[2] + l[5] * beta[2] * beta[2] + l[6] * beta[0] * beta[3] + l[7] * beta[1] * beta[3] +
                                     l[8] * beta[2] * beta[3] + l[9] * beta[3] * beta[3]);
                }
                if (!lsq6<4>(J, r, dx)) break;
#pragma unroll
                for (int k = 0; k < 4; ++k) beta[k] += dx[k];
            }
        }
        /* control points in the camera frame, sign from the first point's depth */
        double cc[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 3; ++e)
                cc[j][e] = beta[0] * ev[(size_t)(3 * j + e) * es] + beta[1] * ev[(size_t)(12 + 3 * j + e) * es] + beta[2] * ev[(size_t)(24 + 3 * j + e) * es] + beta[3] * ev[(size_t)(36 + 3 * j + e) * es];
        {
            double al[4];
            EPNP_ALPHAS(idx[0], al);
            const double z0 = al[0] * cc[0][2] + al[1] * cc[1][2] + al[2] * cc[2][2] + al[3] * cc[3][2];
            if (z0 < 0.0)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int e = 0; e < 3; ++e) cc[j][e] = -cc[j][e];
        }
        /* absolute orientation world -> camera (Horn's quaternion form): S = sum pc (pw - c0)^T */
        double Sm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, pcm[3] = {0, 0, 0};
        for (int k = lane; k < m; k += kstep) {
            double al[4], pc[3];
            EPNP_ALPHAS(idx[k], al);
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                pc[e] = al[0] * cc[0][e] + al[1] * cc[1][e] + al[2] * cc[2][e] + al[3] * cc[3][e];
                pcm[e] += pc[e];
            }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) Sm[3 * i + j] += pc[i] * (obj[3 * (size_t)idx[k] + j] - c0[j]);
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) Sm[i] = total(Sm[i]);
#pragma unroll
        for (int e = 0; e < 3; ++e) pcm[e] = total(pcm[e]) / (double)m;
        /* Sm[i][j] = sum camera_i world_j; the rotation maximising tr(R^T S) is the top eigenvector of Horn's 4 x 4 matrix
         * written for the map world -> camera (its "left" set is the world points: Sxy = sum world_x camera_y = S[y][x]) */
        const double Sxx = Sm[0], Sxy = Sm[3], Sxz = Sm[6], Syx = Sm[1], Syy = Sm[4], Syz = Sm[7], Szx = Sm[2], Szy = Sm[5], Szz = Sm[8];
        double N[16] = {Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx,
                        Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz,
                        Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy,
                        Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz};
        double V4[16], w4[4];
        jacobi_eig<4>(N, V4, w4);
        double q0 = V4[0], qx = V4[4], qy = V4[8], qz = V4[12], wtop = w4[0];
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (w4[k] > wtop) wtop = w4[k], q0 = V4[k], qx = V4[4 + k], qy = V4[8 + k], qz = V4[12 + k];
        cand[0] = q0 * q0 + qx * qx - qy * qy - qz * qz, cand[1] = 2.0 * (qx * qy - q0 * qz), cand[2] = 2.0 * (qx * qz + q0 * qy);
        cand[3] = 2.0 * (qy * qx + q0 * qz), cand[4] = q0 * q0 - qx * qx + qy * qy - qz * qz, cand[5] = 2.0 * (qy * qz - q0 * qx);
        cand[6] = 2.0 * (qz * qx - q0 * qy), cand[7] = 2.0 * (qz * qy + q0 * qx), cand[8] = q0 * q0 - qx * qx - qy * qy + qz * qz;
#pragma unroll
        for (int i = 0; i < 3; ++i) cand[9 + i] = pcm[i] - (cand[3 * i] * c0[0] + cand[3 * i + 1] * c0[1] + cand[3 * i + 2] * c0[2]);
        double err = 0.0;
        for (int k = lane; k < m; k += kstep) {
            const double* X = obj + 3 * (size_t)idx[k];
            const double xc = cand[0] * X[0] + cand[1] * X[1] + cand[2] * X[2] + cand[9];
            const double yc = cand[3] * X[0] + cand[4] * X[1] + cand[5] * X[2] + cand[10];
            const double zc = cand[6] * X[0] + cand[7] * X[1] + cand[8] * X[2] + cand[11];
            const double eu = uc + fu * xc / zc - img[2 * (size_t)idx[k]], evv = vc + fv * yc / zc - img[2 * (size_t)idx[k] + 1];
            err += sqrt(eu * eu + evv * evv);
        }
        err = total(err);
        if (!(err < 1e300)) return -1.0;
        return err;
    }
}
#undef EPNP_ALPHAS

// The frame one sample leaves between the front and the back half of the at-most-64-point form — 130 doubles: c0 3, axes 9,
// lengths 3, rho 6, null vectors 48, distance system 60, valid 1 — field-major in the batch (element e of sample s at
// frame[e * n_samples + s]).
constexpr int PNP_FRAME = 130, PNP_F_C0 = 0, PNP_F_AX = 3, PNP_F_SC = 12, PNP_F_RHO = 15, PNP_F_EV = 21, PNP_F_L = 69, PNP_F_VALID = 129;

// The front half's wave leaves its sample's frame at dst = frame + s (ns = n_samples: the stride of one element).
__device__ __forceinline__ void pnp_frame_pack(double* dst, size_t ns, int ok, const PnpFrame& F, const PnpLds& S) {
    const int lane = threadIdx.x & 63;
    if (lane == 0) {
        dst[PNP_F_VALID * ns] = ok ? 1.0 : 0.0;
        if (ok) {
#pragma unroll
            for (int e = 0; e < 3; ++e) dst[(PNP_F_C0 + e) * ns] = F.c0[e], dst[(PNP_F_SC + e) * ns] = F.sc[e];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int e = 0; e < 3; ++e) dst[(PNP_F_AX + 3 * k + e) * ns] = F.ax[k][e];
#pragma unroll
            for (int q = 0; q < 6; ++q) dst[(PNP_F_RHO + q) * ns] = F.rho[q];
        }
    }
    if (ok) {
        if (lane < 48) dst[(PNP_F_EV + lane) * ns] = S.ev[lane];
        if (lane < 60) dst[(PNP_F_L + lane) * ns] = S.L[lane];
    }
}
// Which of EPnP's three linearised starts is the pose: the first strictly smallest non-negative error (the order of the CPU
// restatement's loop over the starts), -1 = none gave a pose.
__device__ __forceinline__ int pnp_first_smallest(double e0, double e1, double e2) {
    const double e[3] = {e0, e1, e2};
    double best = -1.0;
    int which = -1;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const double err = e[v];
        if (err >= 0.0 && (best < 0.0 || err < best)) best = err, which = v;
    }
    return which;
}

// EPnP on ONE row of any number of points (the all-inlier refit) by a workgroup of at least three waves. Wave 0 runs the front half
// (a partial M^T M per lane) and leaves the frame, the null vectors and the distance system in LDS; then each of the waves 0..2 takes
// ONE linearised start of the back half (its sums over the points spread over the wave's lanes, each wave with its own reduction
// scratch) and thread 0 picks the start: its return value (-1..2; other threads: -1), the pose of start v in W.result[v][1..12].
// With at most 64 rows a lane holds one term and the partials are added in lane order: the sequential sum of the at-most-64-point
// form term by term. One wave running the three starts in a row was 234 us per refit of the incremental loop.
struct PnpRefitLds {
    PnpLds lds;
    double part[78 * 64];
    PnpFrame frame;
    int front_ok;
    double red[3][64], result[3][13];
};
__device__ __forceinline__ int pnp_refit_body(int m, const int* rows_idx, const double* obj, const double* img, const double* K4, PnpRefitLds& W) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave == 0) {
        PnpFrame F;
        const int ok = epnp_front<true>(m, rows_idx, obj, img, K4, F, W.lds, nullptr, W.part);
        if (lane == 0) W.frame = F, W.front_ok = ok;
    }
    __syncthreads();
    if (W.front_ok && wave < 3) {   // (front_ok is workgroup-uniform)
        const PnpFrame F = W.frame;
        double cand[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) cand[k] = 0.0;
        double err;
        if (wave == 0) err = epnp_back_variant<false, 0>(m, rows_idx, obj, img, K4, F, W.lds.ev, W.lds.L, 1, W.red[0], cand);
        else if (wave == 1) err = epnp_back_variant<false, 1>(m, rows_idx, obj, img, K4, F, W.lds.ev, W.lds.L, 1, W.red[1], cand);
        else err = epnp_back_variant<false, 2>(m, rows_idx, obj, img, K4, F, W.lds.ev, W.lds.L, 1, W.red[2], cand);
        if (lane == 0) {
            W.result[wave][0] = err;
#pragma unroll
            for (int k = 0; k < 12; ++k) W.result[wave][1 + k] = cand[k];
        }
    }
    __syncthreads();
    return threadIdx.x == 0 && W.front_ok ? pnp_first_smallest(W.result[0][0], W.result[1][0], W.result[2][0]) : -1;
}

// The minimal sample's M point pairs (idx: the sample's own row of indices into a / b) as x y x y ...
template <int M>
__device__ __forceinline__ void gather_sample(const int* __restrict__ idx, const double* __restrict__ a, const double* __restrict__ b, double* pa, double* pb) {
#pragma unroll
    for (int k = 0; k < M; ++k) {
        const size_t i = (size_t)idx[k];
        pa[2 * k] = a[2 * i]; pa[2 * k + 1] = a[2 * i + 1];
        pb[2 * k] = b[2 * i]; pb[2 * k + 1] = b[2 * i + 1];
    }
}

}  // namespace
}  // namespace eacham
