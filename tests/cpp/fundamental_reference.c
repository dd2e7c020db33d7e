/* fundamental_reference.c — CPU reference of the fundamental-matrix kind of the robust two-view estimators: the seven-point
 * solver (EACHAM_SOLVE_FUNDAMENTAL7), the error (EACHAM_SCORE_FUNDAMENTAL) and the LMedS rule for one problem, written step
 * for step as the kernels run them (eacham_amd/csrc/solve_dev.hpp: fundamental7_wave, real_roots3, jacobi_wave<9>;
 * score_dev.hpp: score_one<3>, block_median; lmeds_batch.hip: lb_select_kernel): the same round-robin Jacobi ordering, the same
 * root recipe, the same order of every sum. Compiled by tests/fundamental_reference.py with -ffp-contract=off and no fast-math,
 * so that every product and sum is rounded on its own, as on the device. Only + - * / sqrt, fabs, fmax, fmin. Test
 * infrastructure only. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* ---- 9 x 9 symmetric eigenproblem, round-robin Jacobi: jacobi_wave<9> element by element -------------------------------- */
static void jacobi_eig_rr9(double* A, double* V, double* w) {
    const int n = 9, np = 10, half = 5;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[i * n + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < n; ++p) {
            diag += A[p * n + p] * A[p * n + p];
            for (int q = p + 1; q < n; ++q) off += A[p * n + q] * A[p * n + q];
        }
        if (off <= 1e-60 || off <= 1e-32 * diag) break;
        for (int round = 0; round < np - 1; ++round) {
            int P[5], Q[5], on[5];
            double C[5], S[5];
            for (int i = 0; i < half; ++i) {  /* every rotation of the round from the matrix the round starts with */
                const int j1 = i, j2 = np - 1 - i;
                const int a = j1 == 0 ? 0 : 1 + ((j1 - 1 - round) % (np - 1) + (np - 1)) % (np - 1);
                const int b = 1 + ((j2 - 1 - round) % (np - 1) + (np - 1)) % (np - 1);
                P[i] = a < b ? a : b, Q[i] = a < b ? b : a;
                on[i] = 0, C[i] = 1.0, S[i] = 0.0;
                if (Q[i] >= n) continue;  /* the bye */
                const double apq = A[P[i] * n + Q[i]];
                if (apq == 0.0) continue;
                const double theta = (A[Q[i] * n + Q[i]] - A[P[i] * n + P[i]]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                C[i] = 1.0 / sqrt(t * t + 1.0), S[i] = t * C[i];
                on[i] = 1;
            }
            for (int i = 0; i < half; ++i) {  /* columns p, q of every pair */
                if (!on[i]) continue;
                for (int k = 0; k < n; ++k) {
                    const double akp = A[k * n + P[i]], akq = A[k * n + Q[i]];
                    A[k * n + P[i]] = C[i] * akp - S[i] * akq;
                    A[k * n + Q[i]] = S[i] * akp + C[i] * akq;
                }
            }
            for (int i = 0; i < half; ++i) {  /* rows p, q of every pair */
                if (!on[i]) continue;
                for (int k = 0; k < n; ++k) {
                    const double apk = A[P[i] * n + k], aqk = A[Q[i] * n + k];
                    A[P[i] * n + k] = C[i] * apk - S[i] * aqk;
                    A[Q[i] * n + k] = S[i] * apk + C[i] * aqk;
                }
            }
            for (int i = 0; i < half; ++i) {  /* the eigenvector columns */
                if (!on[i]) continue;
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[k * n + P[i]], vkq = V[k * n + Q[i]];
                    V[k * n + P[i]] = C[i] * vkp - S[i] * vkq;
                    V[k * n + Q[i]] = S[i] * vkp + C[i] * vkq;
                }
            }
        }
    }
    for (int i = 0; i < n; ++i) w[i] = A[i * n + i];
}

/* ---- real roots of c0 + c1 z + c2 z^2 + c3 z^3, ascending: real_roots3 ----------------------------------------------------- */
static int real_roots3(double c0, double c1, double c2, double c3, double* roots) {
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
    for (int k = 0; k < 3; ++k) m[k] = k < deg ? c[k] / lead : 0.0;
    double bound = 0.0;
    for (int k = 0; k < deg; ++k) bound = fmax(bound, fabs(m[k]));
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
        for (int k = 0; k < deg; ++k) {
            zr[k] = r0 * cr, zi[k] = r0 * ci;
            const double tr = cr * 0.4 - ci * 0.9, ti = cr * 0.9 + ci * 0.4;
            cr = tr, ci = ti;
        }
    }
    for (int it = 0; it < 200; ++it) {  /* simultaneous sweeps: every correction from the iterates the sweep starts with */
        double change = 0.0, nzr[3], nzi[3];
        for (int k = 0; k < deg; ++k) {
            double pr = 1.0, pi = 0.0;  /* Horner on the monic polynomial */
            for (int j = deg - 1; j >= 0; --j) {
                const double tr = pr * zr[k] - pi * zi[k] + m[j], ti = pr * zi[k] + pi * zr[k];
                pr = tr, pi = ti;
            }
            double dr = 1.0, di = 0.0;
            for (int j = 0; j < deg; ++j)
                if (j != k) {
                    const double ar = zr[k] - zr[j], ai = zi[k] - zi[j];
                    const double tr = dr * ar - di * ai, ti = dr * ai + di * ar;
                    dr = tr, di = ti;
                }
            const double den = dr * dr + di * di;
            nzr[k] = zr[k], nzi[k] = zi[k];
            if (!(den > 0.0)) continue;
            const double qr = (pr * dr + pi * di) / den, qi = (pi * dr - pr * di) / den;
            nzr[k] = zr[k] - qr;
            nzi[k] = zi[k] - qi;
            change = fmax(change, fabs(qr) + fabs(qi));
        }
        for (int k = 0; k < deg; ++k) zr[k] = nzr[k], zi[k] = nzi[k];
        if (change <= 1e-11 * bound) break;
    }
    double z[3] = {0, 0, 0};
    int real[3] = {0, 0, 0}, n = 0;
    for (int k = 0; k < deg; ++k) {
        real[k] = !(fabs(zi[k]) > 1e-7 * (1.0 + fabs(zr[k])));
        if (!real[k]) continue;
        double v = zr[k];
        for (int it = 0; it < 4; ++it) {  /* Newton polish on the real polynomial */
            double p = lead, d = 0.0;
            for (int j = deg - 1; j >= 0; --j) {
                d = d * v + p;
                p = p * v + c[j];
            }
            if (!(fabs(d) > 0.0)) break;
            v -= p / d;
        }
        z[k] = v;
        ++n;
    }
    for (int s = 0; s < 3; ++s) roots[s] = 0.0;
    for (int k = 0; k < 3; ++k) {  /* ascending, equals in iterate order: root k goes to the slot of its rank */
        int rank = 0;
        for (int j = 0; j < 3; ++j)
            if (j != k && real[j] && (z[j] < z[k] || (z[j] == z[k] && j < k))) ++rank;
        if (real[k]) roots[rank] = z[k];
    }
    return n;
}

static int normalisation7(const double* p, double* cx, double* cy, double* s) {
    double sx = 0.0, sy = 0.0;
    for (int i = 0; i < 7; ++i) sx += p[2 * i] - p[0], sy += p[2 * i + 1] - p[1];   /* relative to p0: coincident points give exactly 0 */
    *cx = p[0] + sx / 7.0, *cy = p[1] + sy / 7.0;
    double d = 0.0;
    for (int i = 0; i < 7; ++i) {
        const double dx = p[2 * i] - *cx, dy = p[2 * i + 1] - *cy;
        d += sqrt(dx * dx + dy * dy);
    }
    d = d / 7.0;
    *s = 1.4142135623730951 / d;
    return *s <= 1.7976931348623157e308;
}

/* a, b: 7 x 2 pixels of image 1 / image 2. F: 3 x 9 (zero behind the count), cubic (optional): c[0] z^3 + .. + c[3] of
 * run7Point, roots (optional, 3). Returns the number of models. */
static int solve7(const double* a, const double* b, double* F, double* cubic, double* roots_out) {
    for (int k = 0; k < 27; ++k) F[k] = 0.0;
    if (cubic) cubic[0] = cubic[1] = cubic[2] = cubic[3] = 0.0;
    if (roots_out) roots_out[0] = roots_out[1] = roots_out[2] = 0.0;
    double c1x, c1y, s1, c2x, c2y, s2;
    const int ok1 = normalisation7(a, &c1x, &c1y, &s1), ok2 = normalisation7(b, &c2x, &c2y, &s2);
    if (!ok1 || !ok2) return 0;
    double AtA[81], V[81], w[9];
    for (int j = 0; j < 9; ++j)
        for (int k = j; k < 9; ++k) {
            double acc = 0.0;
            for (int i = 0; i < 7; ++i) {
                const double x1 = (a[2 * i] - c1x) * s1, y1 = (a[2 * i + 1] - c1y) * s1;
                const double x2 = (b[2 * i] - c2x) * s2, y2 = (b[2 * i + 1] - c2y) * s2;
                const double row[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0};
                acc += row[j] * row[k];
            }
            AtA[j * 9 + k] = acc;
            AtA[k * 9 + j] = acc;
        }
    jacobi_eig_rr9(AtA, V, w);
    int lo = 0, lo2 = -1;
    for (int i = 1; i < 9; ++i)
        if (w[i] < w[lo]) lo = i;
    for (int i = 0; i < 9; ++i) {
        if (i == lo) continue;
        if (lo2 < 0 || w[i] < w[lo2]) lo2 = i;
    }
    double f1[9], f2[9];
    for (int k = 0; k < 9; ++k) {
        f2[k] = V[k * 9 + lo];
        f1[k] = V[k * 9 + lo2] - f2[k];
    }
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
    if (cubic) memcpy(cubic, c, sizeof(c));
    double roots[3];
    const int nr = real_roots3(c[3], c[2], c[1], c[0], roots);
    if (roots_out) memcpy(roots_out, roots, sizeof(roots));
    const double t2t[9] = {s2, 0, 0, 0, s2, 0, -c2x * s2, -c2y * s2, 1};
    const double t1m[9] = {s1, 0, -c1x * s1, 0, s1, -c1y * s1, 0, 0, 1};
    int n = 0;
    for (int r = 0; r < nr; ++r) {
        double Fh[9], T[9], G[9];
        for (int k = 0; k < 9; ++k) Fh[k] = f1[k] * roots[r] + f2[k];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) T[3 * i + j] = t2t[3 * i] * Fh[j] + t2t[3 * i + 1] * Fh[3 + j] + t2t[3 * i + 2] * Fh[6 + j];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) G[3 * i + j] = T[3 * i] * t1m[j] + T[3 * i + 1] * t1m[3 + j] + T[3 * i + 2] * t1m[6 + j];
        double nrm = 0.0;
        for (int k = 0; k < 9; ++k) nrm += G[k] * G[k];
        nrm = sqrt(nrm);
        if (!(nrm > 0.0 && nrm < 1e300)) continue;
        for (int k = 0; k < 9; ++k) F[9 * n + k] = G[k] / nrm;
        ++n;
    }
    return n;
}

/* eacham_solve_minimal(kind FUNDAMENTAL7): models n_samples x 3 x 9, n_models n_samples; cubic / roots optional (n_samples x 4 / 3) */
void fref_solve_minimal(const double* a, const double* b, int n_samples, const int32_t* idx, double* models, int32_t* n_models,
                        double* cubic, double* roots) {
    for (int s = 0; s < n_samples; ++s) {
        double pa[14], pb[14];
        for (int k = 0; k < 7; ++k) {
            const size_t i = (size_t)idx[7 * (size_t)s + k];
            pa[2 * k] = a[2 * i], pa[2 * k + 1] = a[2 * i + 1];
            pb[2 * k] = b[2 * i], pb[2 * k + 1] = b[2 * i + 1];
        }
        n_models[s] = solve7(pa, pb, models + 27 * (size_t)s, cubic ? cubic + 4 * (size_t)s : 0, roots ? roots + 3 * (size_t)s : 0);
    }
}

/* ---- the error: score_one<3> ----------------------------------------------------------------------------------------------- */
static float error1(const double* F, const double* a, const double* b) {
    double l2[3], l1[3];
    for (int r = 0; r < 3; ++r) {
        l2[r] = (F[3 * r] * a[0] + F[3 * r + 1] * a[1]) + F[3 * r + 2];
        l1[r] = (F[r] * b[0] + F[3 + r] * b[1]) + F[6 + r];
    }
    const double d = (b[0] * l2[0] + b[1] * l2[1]) + l2[2];
    const double d2 = d * d;
    const double e1 = d2 / (l1[0] * l1[0] + l1[1] * l1[1]);
    const double e2 = d2 / (l2[0] * l2[0] + l2[1] * l2[1]);
    return (float)(e1 < e2 ? e2 : e1);
}

/* the total order of floats of the device's radix select (fkey): negatives reversed, a NaN with a clear sign bit last */
static uint32_t fkey(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static float fkey_inv(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static int cmp_u32(const void* x, const void* y) {
    const uint32_t a = *(const uint32_t*)x, b = *(const uint32_t*)y;
    return a < b ? -1 : (a > b ? 1 : 0);
}
/* block_median: the upper middle, averaged with the lower one when n is even (float arithmetic); NaN for n = 0 */
static float median_of(const float* e, int n, uint32_t* keys) {
    if (n == 0) return fkey_inv(fkey(NAN));
    for (int i = 0; i < n; ++i) keys[i] = fkey(e[i]);
    qsort(keys, (size_t)n, sizeof(uint32_t), cmp_u32);
    float med = fkey_inv(keys[n / 2]);
    if (n % 2 == 0) med = (fkey_inv(keys[n / 2 - 1]) + med) * 0.5f;
    return med;
}

/* eacham_score_hypotheses(kind FUNDAMENTAL): errors n_models x n, counts (err <= threshold), medians */
void fref_score(int n, const double* a, const double* b, int n_models, const double* models, float threshold, float* errors,
                int32_t* counts, float* medians) {
    uint32_t* keys = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(n > 0 ? n : 1));
    float* row = (float*)malloc(sizeof(float) * (size_t)(n > 0 ? n : 1));
    for (int m = 0; m < n_models; ++m) {
        int c = 0;
        for (int i = 0; i < n; ++i) {
            row[i] = error1(models + 9 * (size_t)m, a + 2 * (size_t)i, b + 2 * (size_t)i);
            c += row[i] <= threshold;
            if (errors) errors[(size_t)m * n + i] = row[i];
        }
        if (counts) counts[m] = c;
        if (medians) medians[m] = median_of(row, n, keys);
    }
    free(keys);
    free(row);
}

/* ---- the LMedS rule for one problem: what eacham_lmeds_batch does for each of its problems ------------------------------- */
/* n points, n_samples samples of 7 local indices. Outputs as eacham_lmeds_batch's per problem: model 9, median, threshold,
 * inliers, mask n bytes, winner 3, n_candidates. */
void fref_lmeds(int n, const double* a, const double* b, int n_samples, const int32_t* idx, double* model, float* median, float* threshold,
                int32_t* inliers, uint8_t* mask, int32_t* winner, int32_t* n_candidates) {
    const int m = 7;
    for (int k = 0; k < 9; ++k) model[k] = 0.0;
    *median = fkey_inv(fkey(NAN)), *threshold = 0.f, *inliers = 0, *n_candidates = 0;
    winner[0] = winner[1] = winner[2] = -1;
    for (int i = 0; i < n; ++i) mask[i] = 0;
    if (n < m) return;   /* its samples are not looked at */
    uint32_t* keys = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)n);
    float* row = (float*)malloc(sizeof(float) * (size_t)n);
    int cand = 0, best = -1, best_s = -1, best_r = -1;
    float best_med = 0.f;
    double best_F[9];
    for (int s = 0; s < n_samples; ++s) {
        double pa[14], pb[14], F[27];
        for (int k = 0; k < 7; ++k) {
            const size_t i = (size_t)idx[7 * (size_t)s + k];
            pa[2 * k] = a[2 * i], pa[2 * k + 1] = a[2 * i + 1];
            pb[2 * k] = b[2 * i], pb[2 * k + 1] = b[2 * i + 1];
        }
        const int nm = solve7(pa, pb, F, 0, 0);
        for (int r = 0; r < nm; ++r, ++cand) {   /* flattened: sample order, then root order */
            for (int i = 0; i < n; ++i) row[i] = error1(F + 9 * r, a + 2 * (size_t)i, b + 2 * (size_t)i);
            const float med = median_of(row, n, keys);
            if (med == med && (best < 0 || med < best_med)) {   /* the first smallest non-NaN median */
                best = cand, best_s = s, best_r = r, best_med = med;
                memcpy(best_F, F + 9 * r, sizeof(best_F));
            }
        }
    }
    *n_candidates = cand;
    if (best >= 0) {
        const int d = n - m > 1 ? n - m : 1;
        const double f = 1.0 + 5.0 / (double)d;
        double sigma = ((2.5 * 1.4826) * f) * sqrt((double)best_med);
        if (sigma < 0.001) sigma = 0.001;
        const float thr = (float)(sigma * sigma);
        memcpy(model, best_F, sizeof(best_F));
        *median = best_med, *threshold = thr;
        winner[0] = best, winner[1] = best_s, winner[2] = best_r;
        int c = 0;
        for (int i = 0; i < n; ++i) {
            mask[i] = error1(best_F, a + 2 * (size_t)i, b + 2 * (size_t)i) <= thr;
            c += mask[i];
        }
        *inliers = c;
    }
    free(keys);
    free(row);
}
