/* tri_refine_reference.c — CPU restatement of eacham_triangulate_refine_tracks (include/eacham_hip.h states the definition;
 * eacham_amd/csrc/tri_refine.hip is the device form). Test infrastructure only: tests/tri_refine_reference.py compiles it with
 * -ffp-contract=off and no fast-math, so every product, sum and quotient is rounded on its own and the sums run in the order
 * written — the same operations in the same order as the kernel, which is held to it as bytes. The loop uses only + - * /; the
 * recount restates is_inlier of triangulate.hip (a square root, correctly rounded on both sides).
 *
 * The 8 "lanes" of the definition are the 8 rows of part[][] here: lane l owns the observations i of the track with i % 8 == l and
 * adds the used ones among them in ascending order, starting from zero; the 8 partials are then folded 4, 2, 1
 * (part[l] += part[l + off]).
 *
 * With -DTRI_REFINE_MAIN the file is a program of its own: tri_refine_reference <cases.bin> runs the case list the tests write
 * (tests/tri_refine_reference.py: write_cases) and prints a line per track; the sanitizer test builds it that way. */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { ST_CONVERGED = 0, ST_CAP = 1, ST_NOT_REFINED = 2 };
enum { NS = 10 }; /* 6 entries of H (upper triangle, row by row), 3 of g, the cost */

static int hidx(int i, int j) { return i * 3 - i * (i - 1) / 2 + (j - i); } /* i <= j */

/* The residual and the two Jacobian rows of one observation (T: row-major 4 x 4 world -> camera, (u, v) = x) at X. Returns z. */
static double row_terms(const double* T, const double* x, const double* X, const double* K, double* Ju, double* Jv, double* r) {
    const double xc = ((T[0] * X[0] + T[1] * X[1]) + T[2] * X[2]) + T[3];
    const double yc = ((T[4] * X[0] + T[5] * X[1]) + T[6] * X[2]) + T[7];
    const double zc = ((T[8] * X[0] + T[9] * X[1]) + T[10] * X[2]) + T[11];
    const double iz = 1.0 / zc;
    const double xn = xc * iz, yn = yc * iz;
    r[0] = (K[0] * xn + K[2]) - x[0];
    r[1] = (K[1] * yn + K[3]) - x[1];
    const double a = K[0] * iz, b = K[1] * iz;
    for (int j = 0; j < 3; ++j) {
        Ju[j] = a * (T[j] - xn * T[8 + j]);
        Jv[j] = b * (T[4 + j] - yn * T[8 + j]);
    }
    return zc;
}

static void add_row(double* S, const double* Ju, const double* Jv, const double* r) {
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) S[hidx(i, j)] = S[hidx(i, j)] + (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
    for (int i = 0; i < 3; ++i) S[6 + i] = S[6 + i] + (Ju[i] * r[0] + Jv[i] * r[1]);
    S[9] = S[9] + (r[0] * r[0] + r[1] * r[1]);
}

/* H, g and the cost of X over the used observations of one track; *used = their number, returns 1 if a used one has !(z > 0). */
static int sums(int n, const double* transforms, const uint32_t* frame, const double* uv, const uint8_t* use, const double* X, const double* K,
                double* S, int* used) {
    double part[8][NS];
    memset(part, 0, sizeof(part));
    int bad = 0, m = 0;
    for (int i = 0; i < n; ++i) {
        if (use && !use[i]) continue;
        double Ju[3], Jv[3], r[2];
        const double z = row_terms(transforms + 16 * (size_t)frame[i], uv + 2 * (size_t)i, X, K, Ju, Jv, r);
        if (!(z > 0.0)) bad = 1;
        add_row(part[i % 8], Ju, Jv, r);
        ++m;
    }
    for (int off = 4; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l)
            for (int k = 0; k < NS; ++k) part[l][k] = part[l][k] + part[l + off][k];
    for (int k = 0; k < NS; ++k) S[k] = part[0][k];
    *used = m;
    return bad;
}

/* (H + lambda diag H) d = -g by an unpivoted L D L' factorisation; 0 if a pivot is not > 0. */
static int solve3(const double* S, double lambda, double* d) {
    double L[3][3], D[3], y[3];
    for (int j = 0; j < 3; ++j) {
        double v = S[hidx(j, j)] + lambda * S[hidx(j, j)];
        for (int k = 0; k < j; ++k) v = v - L[j][k] * D[k] * L[j][k];
        if (!(v > 0.0)) return 0;
        D[j] = v;
        for (int i = j + 1; i < 3; ++i) {
            double w = S[hidx(j, i)];
            for (int k = 0; k < j; ++k) w = w - L[i][k] * D[k] * L[j][k];
            L[i][j] = w / v;
        }
    }
    for (int i = 0; i < 3; ++i) {
        double v = -S[6 + i];
        for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
        y[i] = v;
    }
    for (int i = 2; i >= 0; --i) {
        double v = y[i] / D[i];
        for (int k = i + 1; k < 3; ++k) v = v - L[k][i] * d[k];
        d[i] = v;
    }
    return 1;
}

static double max_abs3(const double* v) {
    double big = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double a = v[k] < 0.0 ? -v[k] : v[k];
        if (!(a <= big)) big = a; /* (a NaN is not small) */
    }
    return big;
}

static int is_inlier(const double* T, const double* x, const double* K, const double* X, float max_err) { /* triangulate.hip */
    const double px = T[0] * X[0] + T[1] * X[1] + T[2] * X[2] + T[3];
    const double py = T[4] * X[0] + T[5] * X[1] + T[6] * X[2] + T[7];
    const double pz = T[8] * X[0] + T[9] * X[1] + T[10] * X[2] + T[11];
    const double u = (K[0] * px) / pz + K[2], v = (K[1] * py) / pz + K[3];
    const float err = (float)sqrt((x[0] - u) * (x[0] - u) + (x[1] - v) * (x[1] - v));
    return err < max_err && pz >= 2.220446049250313e-16;
}

static double canonical(double c) { /* a NaN cost leaves as ONE bit pattern, whatever produced it */
    if (c == c) return c;
    const uint64_t q = 0x7ff8000000000000ull;
    memcpy(&c, &q, sizeof(c));
    return c;
}

/* One track. trace (optional): max_tries rows of (candidate cost, accepted, lambda of the try); rows of tries that solved nothing
 * hold (0, -1, lambda). */
static void refine_one(int n, const double* transforms, const uint32_t* frame, const double* uv, const uint8_t* use, const double* K,
                       const double* point, int has, int max_tries, double* refined, double* cost, int32_t* tries, int32_t* status, double* trace) {
    double X[3], S[NS];
    for (int k = 0; k < 3; ++k) X[k] = has ? point[k] : 0.0, refined[k] = X[k];
    cost[0] = cost[1] = 0.0, *tries = 0, *status = ST_NOT_REFINED;
    if (!has) return;
    int used = 0;
    const int bad = sums(n, transforms, frame, uv, use, X, K, S, &used);
    cost[0] = cost[1] = canonical(S[9]);
    if (used < 2 || bad || !(S[9] - S[9] == 0.0)) return;
    double lambda = 1e-3;
    int t = 0, st = ST_CAP;
    while (t < max_tries) {
        double d[3], Xc[3], Sc[NS];
        if (trace) trace[3 * t] = 0.0, trace[3 * t + 1] = -1.0, trace[3 * t + 2] = lambda;
        ++t;
        if (!solve3(S, lambda, d)) {
            lambda = 10.0 * lambda < 1e12 ? 10.0 * lambda : 1e12;
            continue;
        }
        if (max_abs3(d) <= 1e-10 * (1.0 + max_abs3(X))) {
            st = ST_CONVERGED;
            break;
        }
        for (int k = 0; k < 3; ++k) Xc[k] = X[k] + d[k];
        int uc = 0;
        const int badc = sums(n, transforms, frame, uv, use, Xc, K, Sc, &uc);
        const int accept = !badc && Sc[9] < S[9];
        if (trace) trace[3 * (t - 1)] = Sc[9], trace[3 * (t - 1) + 1] = accept;
        if (accept) {
            const double dec = S[9] - Sc[9];
            for (int k = 0; k < 3; ++k) X[k] = Xc[k];
            for (int k = 0; k < NS; ++k) S[k] = Sc[k];
            lambda = lambda / 10.0 > 1e-12 ? lambda / 10.0 : 1e-12;
            if (dec <= 1e-9 * S[9]) {
                st = ST_CONVERGED;
                break;
            }
        } else {
            lambda = 10.0 * lambda < 1e12 ? 10.0 * lambda : 1e12;
        }
    }
    for (int k = 0; k < 3; ++k) refined[k] = X[k];
    cost[1] = S[9], *tries = t, *status = st;
}

/* eacham_triangulate_refine_tracks. use_mask / inlier_mask / n_inliers / trace may be NULL; trace: n_tracks x max_tries x 3. */
void trirefine_tracks(const double* transforms, int n_tracks, const int64_t* track_ptr, const uint32_t* obs_frame, const double* obs_uv,
                      const double* K, const double* points, const uint8_t* has_point, const uint8_t* use_mask, int max_tries, float max_repr_error,
                      double* refined, double* cost, int32_t* tries, int32_t* status, uint8_t* inlier_mask, int32_t* n_inliers, double* trace) {
    for (int t = 0; t < n_tracks; ++t) {
        const long long base = track_ptr[t];
        const int n = (int)(track_ptr[t + 1] - base);
        const uint32_t* fr = obs_frame + base;
        const double* uv = obs_uv + 2 * base;
        refine_one(n, transforms, fr, uv, use_mask ? use_mask + base : 0, K, points + 3 * (long long)t, has_point[t] != 0, max_tries,
                   refined + 3 * (long long)t, cost + 2 * (long long)t, tries + t, status + t, trace ? trace + 3 * (long long)max_tries * t : 0);
        int c = 0;
        for (int i = 0; i < n; ++i) {
            const int in = has_point[t] != 0 && is_inlier(transforms + 16 * (size_t)fr[i], uv + 2 * (size_t)i, K, refined + 3 * (long long)t, max_repr_error);
            if (inlier_mask) inlier_mask[base + i] = (uint8_t)in;
            c += in;
        }
        if (n_inliers) n_inliers[t] = c;
    }
}

/* The residual (2) and the Jacobian (2 x 3, row-major: d r / d X) of one observation, as the loop uses them. */
void trirefine_jacobian(const double* T, const double* x, const double* X, const double* K, double* J, double* r) {
    (void)row_terms(T, x, X, K, J, J + 3, r);
}

#ifdef TRI_REFINE_MAIN
#include <stdio.h>
#include <stdlib.h>
/* cases.bin: int32 n_tracks, int32 n_frames, int32 max_tries, int32 with_mask, float max_repr_error, 4 doubles K,
 * int64 track_ptr[n_tracks + 1], transforms [16 n_frames], obs_frame [NO] uint32, obs_uv [2 NO], points [3 n_tracks],
 * has_point [n_tracks], use_mask [NO] when with_mask. */
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t head[4];
    float thr;
    double K[4];
    if (fread(head, sizeof(head), 1, f) != 1 || fread(&thr, sizeof(thr), 1, f) != 1 || fread(K, sizeof(K), 1, f) != 1) return 4;
    const int P = head[0], F = head[1], max_tries = head[2];
    int64_t* tp = malloc(sizeof(int64_t) * ((size_t)P + 1));
    if (fread(tp, sizeof(int64_t), (size_t)P + 1, f) != (size_t)P + 1) return 4;
    const size_t NO = (size_t)tp[P];
    double* T = malloc(sizeof(double) * 16 * (size_t)F + 8);
    uint32_t* fr = malloc(sizeof(uint32_t) * NO + 4);
    double* uv = malloc(sizeof(double) * 2 * NO + 8);
    double* pts = malloc(sizeof(double) * 3 * (size_t)P + 8);
    uint8_t* has = malloc((size_t)P + 1);
    uint8_t* use = head[3] ? malloc(NO + 1) : 0;
    if (fread(T, sizeof(double), 16 * (size_t)F, f) != 16 * (size_t)F || fread(fr, sizeof(uint32_t), NO, f) != NO ||
        fread(uv, sizeof(double), 2 * NO, f) != 2 * NO || fread(pts, sizeof(double), 3 * (size_t)P, f) != 3 * (size_t)P ||
        fread(has, 1, (size_t)P, f) != (size_t)P || (use && fread(use, 1, NO, f) != NO))
        return 4;
    fclose(f);
    for (size_t i = 0; i < NO; ++i)
        if (fr[i] >= (uint32_t)F) return 5;
    double* refined = malloc(sizeof(double) * 3 * (size_t)P + 8);
    double* cost = malloc(sizeof(double) * 2 * (size_t)P + 8);
    int32_t* tries = malloc(sizeof(int32_t) * (size_t)P + 4);
    int32_t* status = malloc(sizeof(int32_t) * (size_t)P + 4);
    uint8_t* mask = malloc(NO + 1);
    int32_t* ni = malloc(sizeof(int32_t) * (size_t)P + 4);
    double* trace = malloc(sizeof(double) * 3 * (size_t)max_tries * (size_t)P + 8);
    trirefine_tracks(T, P, tp, fr, uv, K, pts, has, use, max_tries, thr, refined, cost, tries, status, mask, ni, trace);
    for (int p = 0; p < P; ++p) printf("%d %d %d %d %.17g %.17g\n", p, status[p], tries[p], ni[p], cost[2 * p], cost[2 * p + 1]);
    free(tp), free(T), free(fr), free(uv), free(pts), free(has), free(use), free(refined), free(cost), free(tries), free(status), free(mask), free(ni),
        free(trace);
    return 0;
}
#endif
