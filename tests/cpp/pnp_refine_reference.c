/* pnp_refine_reference.c — CPU restatement of eacham_pnp_refine_batch (include/eacham_hip.h states the definition;
 * eacham_amd/csrc/pnp_dev.hpp and pnp_refine.hip are the device form). Test infrastructure only: tests/pnp_refine_reference.py
 * compiles it with -ffp-contract=off and no fast-math, so every product, sum and quotient is rounded on its own and the sums run in
 * the order written — the same operations in the same order as the kernel, which is held to it as bytes. Only + - * /.
 *
 * The 64 "lanes" of the definition are the 64 rows of part[][] here: lane l owns the rows i with i % 64 == l and adds the used ones
 * among them in ascending order, starting from zero; the 64 partials are then folded 32, 16, 8, 4, 2, 1 (part[l] += part[l + off]).
 *
 * With -DPNP_REFINE_MAIN the file is a program of its own: pnp_refine_reference <cases.bin> runs the case list the tests write
 * (tests/pnp_refine_reference.py: write_cases) and prints a line per problem; the sanitizer test builds it that way. */
#include <stdint.h>
#include <string.h>

enum { ST_CONVERGED = 0, ST_CAP = 1, ST_NOT_REFINED = 2 };
enum { NS = 28 }; /* 21 entries of H (upper triangle, row by row), 6 of g, the cost */

static int hidx(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); } /* i <= j */

/* The camera-frame point, the residual and the two Jacobian rows of one correspondence under M = R | t. Returns z. */
static double row_terms(const double* X, const double* x, const double* M, const double* K, double* Ju, double* Jv, double* r) {
    const double xc = M[0] * X[0] + M[1] * X[1] + M[2] * X[2] + M[9];
    const double yc = M[3] * X[0] + M[4] * X[1] + M[5] * X[2] + M[10];
    const double zc = M[6] * X[0] + M[7] * X[1] + M[8] * X[2] + M[11];
    const double iz = 1.0 / zc;
    const double xn = xc * iz, yn = yc * iz;
    r[0] = (K[0] * xn + K[2]) - x[0];
    r[1] = (K[1] * yn + K[3]) - x[1];
    const double a = K[0] * iz, b = K[1] * iz;
    Ju[0] = -(K[0] * xn * yn), Ju[1] = K[0] * (1.0 + xn * xn), Ju[2] = -(K[0] * yn), Ju[3] = a, Ju[4] = 0.0, Ju[5] = -(a * xn);
    Jv[0] = -(K[1] * (1.0 + yn * yn)), Jv[1] = K[1] * xn * yn, Jv[2] = K[1] * xn, Jv[3] = 0.0, Jv[4] = b, Jv[5] = -(b * yn);
    return zc;
}

static void add_row(double* S, const double* Ju, const double* Jv, const double* r) {
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) S[hidx(i, j)] = S[hidx(i, j)] + (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
    for (int i = 0; i < 6; ++i) S[21 + i] = S[21 + i] + (Ju[i] * r[0] + Jv[i] * r[1]);
    S[27] = S[27] + (r[0] * r[0] + r[1] * r[1]);
}

/* H, g and the cost of M over the used rows of one problem; *used = their number, returns 1 if a used row has !(z > 0). */
static int sums(int n, const double* obj, const double* img, const uint8_t* use, const double* M, const double* K, double* S, int* used) {
    double part[64][NS];
    memset(part, 0, sizeof(part));
    int bad = 0, m = 0;
    for (int i = 0; i < n; ++i) {
        if (use && !use[i]) continue;
        double Ju[6], Jv[6], r[2];
        const double z = row_terms(obj + 3 * (long long)i, img + 2 * (long long)i, M, K, Ju, Jv, r);
        if (!(z > 0.0)) bad = 1;
        add_row(part[i % 64], Ju, Jv, r);
        ++m;
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l)
            for (int k = 0; k < NS; ++k) part[l][k] = part[l][k] + part[l + off][k];
    for (int k = 0; k < NS; ++k) S[k] = part[0][k];
    *used = m;
    return bad;
}

/* (H + lambda diag H) d = -g by an unpivoted L D L' factorisation; 0 if a pivot is not > 0. */
static int solve6(const double* S, double lambda, double* d) {
    double L[6][6], D[6], y[6];
    for (int j = 0; j < 6; ++j) {
        double v = S[hidx(j, j)] + lambda * S[hidx(j, j)];
        for (int k = 0; k < j; ++k) v = v - L[j][k] * D[k] * L[j][k];
        if (!(v > 0.0)) return 0;
        D[j] = v;
        for (int i = j + 1; i < 6; ++i) {
            double w = S[hidx(j, i)];
            for (int k = 0; k < j; ++k) w = w - L[i][k] * D[k] * L[j][k];
            L[i][j] = w / v;
        }
    }
    for (int i = 0; i < 6; ++i) {
        double v = -S[21 + i];
        for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
        y[i] = v;
    }
    for (int i = 5; i >= 0; --i) {
        double v = y[i] / D[i];
        for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * d[k];
        d[i] = v;
    }
    return 1;
}

/* R <- C(w) R, t <- C(w) t + v with the Cayley map C(w) = ((4 - |w|^2) I + 2 w w' + 4 [w]x) / (4 + |w|^2), d = [w, v]. */
static void retract(const double* M, const double* d, double* Mc) {
    const double x = d[0], y = d[1], z = d[2];
    const double xx = x * x, yy = y * y, zz = z * z;
    const double f = 1.0 / (4.0 + (xx + yy + zz));
    double C[9];
    C[0] = f * (4.0 + xx - yy - zz), C[1] = f * (2.0 * (x * y - 2.0 * z)), C[2] = f * (2.0 * (x * z + 2.0 * y));
    C[3] = f * (2.0 * (x * y + 2.0 * z)), C[4] = f * (4.0 - xx + yy - zz), C[5] = f * (2.0 * (y * z - 2.0 * x));
    C[6] = f * (2.0 * (x * z - 2.0 * y)), C[7] = f * (2.0 * (y * z + 2.0 * x)), C[8] = f * (4.0 - xx - yy + zz);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Mc[3 * r + c] = C[3 * r] * M[c] + C[3 * r + 1] * M[3 + c] + C[3 * r + 2] * M[6 + c];
        Mc[9 + r] = C[3 * r] * M[9] + C[3 * r + 1] * M[10] + C[3 * r + 2] * M[11] + d[3 + r];
    }
}

static float pnp_error(const double* a, const double* b, const double* M, const double* K) { /* eacham_score_hypotheses, kind PNP */
    const double X = M[0] * a[0] + M[1] * a[1] + M[2] * a[2] + M[9];
    const double Y = M[3] * a[0] + M[4] * a[1] + M[5] * a[2] + M[10];
    double Z = M[6] * a[0] + M[7] * a[1] + M[8] * a[2] + M[11];
    Z = Z != 0.0 ? 1.0 / Z : 1.0;
    const float u = (float)(X * Z * K[0] + K[2]), v = (float)(Y * Z * K[1] + K[3]);
    const float dx = (float)b[0] - u, dy = (float)b[1] - v;
    return dx * dx + dy * dy;
}

static double canonical(double c) { /* a NaN cost leaves as ONE bit pattern, whatever produced it */
    if (c == c) return c;
    const uint64_t q = 0x7ff8000000000000ull;
    memcpy(&c, &q, sizeof(c));
    return c;
}

/* One problem. trace (optional): max_tries rows of (candidate cost, accepted, lambda of the try); rows of tries that solved nothing
 * hold (0, -1, lambda). */
static void refine_one(int n, const double* obj, const double* img, const uint8_t* use, const double* K, const double* pose, int has, int max_tries,
                       double* refined, double* cost, int32_t* tries, int32_t* status, double* trace) {
    double M[12], S[NS];
    for (int k = 0; k < 12; ++k) M[k] = has ? pose[k] : 0.0, refined[k] = M[k];
    cost[0] = cost[1] = 0.0, *tries = 0, *status = ST_NOT_REFINED;
    if (!has) return;
    int used = 0;
    const int bad = sums(n, obj, img, use, M, K, S, &used);
    cost[0] = cost[1] = canonical(S[27]);
    if (used < 3 || bad || !(S[27] - S[27] == 0.0)) return;
    double lambda = 1e-3;
    int t = 0, st = ST_CAP;
    while (t < max_tries) {
        double d[6], Mc[12], Sc[NS];
        if (trace) trace[3 * t] = 0.0, trace[3 * t + 1] = -1.0, trace[3 * t + 2] = lambda;
        ++t;
        if (!solve6(S, lambda, d)) {
            lambda = 10.0 * lambda < 1e12 ? 10.0 * lambda : 1e12;
            continue;
        }
        double big = 0.0;
        for (int k = 0; k < 6; ++k) {
            const double a = d[k] < 0.0 ? -d[k] : d[k];
            if (!(a <= big)) big = a; /* (a NaN step is not small) */
        }
        if (big <= 1e-10) {
            st = ST_CONVERGED;
            break;
        }
        retract(M, d, Mc);
        int uc = 0;
        const int badc = sums(n, obj, img, use, Mc, K, Sc, &uc);
        const int accept = !badc && Sc[27] < S[27];
        if (trace) trace[3 * (t - 1)] = Sc[27], trace[3 * (t - 1) + 1] = accept;
        if (accept) {
            const double dec = S[27] - Sc[27];
            for (int k = 0; k < 12; ++k) M[k] = Mc[k];
            for (int k = 0; k < NS; ++k) S[k] = Sc[k];
            lambda = lambda / 10.0 > 1e-12 ? lambda / 10.0 : 1e-12;
            if (dec <= 1e-9 * S[27]) {
                st = ST_CONVERGED;
                break;
            }
        } else {
            lambda = 10.0 * lambda < 1e12 ? 10.0 * lambda : 1e12;
        }
    }
    for (int k = 0; k < 12; ++k) refined[k] = M[k];
    cost[1] = S[27], *tries = t, *status = st;
}

/* eacham_pnp_refine_batch. inlier_mask / n_inliers / trace may be NULL; trace: n_problems x max_tries x 3. */
void pnprefine_batch(int n_problems, const int64_t* point_ptr, const double* obj, const double* img, const double* K, const double* poses,
                     const uint8_t* has_pose, const uint8_t* use_mask, int max_tries, float threshold, double* refined, double* cost, int32_t* tries,
                     int32_t* status, uint8_t* inlier_mask, int32_t* n_inliers, double* trace) {
    for (int p = 0; p < n_problems; ++p) {
        const long long base = point_ptr[p];
        const int n = (int)(point_ptr[p + 1] - base);
        const double* a = obj + 3 * base;
        const double* b = img + 2 * base;
        refine_one(n, a, b, use_mask ? use_mask + base : 0, K, poses + 12 * (long long)p, has_pose[p] != 0, max_tries, refined + 12 * (long long)p,
                   cost + 2 * (long long)p, tries + p, status + p, trace ? trace + 3 * (long long)max_tries * p : 0);
        int c = 0;
        for (int i = 0; i < n; ++i) {
            const int in = has_pose[p] != 0 && pnp_error(a + 3 * (long long)i, b + 2 * (long long)i, refined + 12 * (long long)p, K) <= threshold;
            if (inlier_mask) inlier_mask[base + i] = (uint8_t)in;
            c += in;
        }
        if (n_inliers) n_inliers[p] = c;
    }
}

/* The residual (2) and the Jacobian (2 x 6, row-major: d r / d [w, v]) of one correspondence, as the loop uses them. */
void pnprefine_jacobian(const double* X, const double* x, const double* M, const double* K, double* J, double* r) {
    (void)row_terms(X, x, M, K, J, J + 6, r);
}

#ifdef PNP_REFINE_MAIN
#include <stdio.h>
#include <stdlib.h>
/* cases.bin: int32 P, int32 max_tries, int32 with_mask, float threshold, 4 doubles K, int64 point_ptr[P + 1], obj, img, poses [12 P],
 * has_pose [P], use_mask [NP] when with_mask. */
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t head[3];
    float thr;
    double K[4];
    if (fread(head, sizeof(head), 1, f) != 1 || fread(&thr, sizeof(thr), 1, f) != 1 || fread(K, sizeof(K), 1, f) != 1) return 4;
    const int P = head[0], max_tries = head[1];
    int64_t* pp = malloc(sizeof(int64_t) * ((size_t)P + 1));
    if (fread(pp, sizeof(int64_t), (size_t)P + 1, f) != (size_t)P + 1) return 4;
    const size_t NP = (size_t)pp[P];
    double* obj = malloc(sizeof(double) * 3 * NP + 8);
    double* img = malloc(sizeof(double) * 2 * NP + 8);
    double* poses = malloc(sizeof(double) * 12 * (size_t)P + 8);
    uint8_t* has = malloc((size_t)P + 1);
    uint8_t* use = head[2] ? malloc(NP + 1) : 0;
    if (fread(obj, sizeof(double), 3 * NP, f) != 3 * NP || fread(img, sizeof(double), 2 * NP, f) != 2 * NP ||
        fread(poses, sizeof(double), 12 * (size_t)P, f) != 12 * (size_t)P || fread(has, 1, (size_t)P, f) != (size_t)P ||
        (use && fread(use, 1, NP, f) != NP))
        return 4;
    fclose(f);
    double* refined = malloc(sizeof(double) * 12 * (size_t)P + 8);
    double* cost = malloc(sizeof(double) * 2 * (size_t)P + 8);
    int32_t* tries = malloc(sizeof(int32_t) * (size_t)P + 4);
    int32_t* status = malloc(sizeof(int32_t) * (size_t)P + 4);
    uint8_t* mask = malloc(NP + 1);
    int32_t* ni = malloc(sizeof(int32_t) * (size_t)P + 4);
    double* trace = malloc(sizeof(double) * 3 * (size_t)max_tries * (size_t)P + 8);
    pnprefine_batch(P, pp, obj, img, K, poses, has, use, max_tries, thr, refined, cost, tries, status, mask, ni, trace);
    for (int p = 0; p < P; ++p) printf("%d %d %d %d %.17g %.17g\n", p, status[p], tries[p], ni[p], cost[2 * p], cost[2 * p + 1]);
    free(pp), free(obj), free(img), free(poses), free(has), free(use), free(refined), free(cost), free(tries), free(status), free(mask), free(ni), free(trace);
    return 0;
}
#endif
