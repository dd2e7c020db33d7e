// pnp_dev.hpp — the inlier test of the PnP RANSAC as its kernels share it (pb_count_kernel and pb_refit_kernel of pnp_batch.hip,
// p3p_count_kernel of p3p.hip): a point within the threshold of a pose, a wave's count of such points, a wave's write-out of the pose.
// Below them: the pieces of the Levenberg-Marquardt polish of a pose (pnp_refine_kernel of pnp_refine.hip).
// It runs score_one: only translation units compiled with -ffp-contract=off (csrc/Makefile) may include it.
#pragma once

#include "score_dev.hpp"

namespace eacham {

// Point i of obj / img (a problem's own rows) lies within the threshold of the pose M = R | t.
__device__ __forceinline__ bool pnp_inlier(const double* obj, const double* img, int i, const double* M, const double* K, float threshold) {
    const double X[3] = {obj[3 * (size_t)i], obj[3 * (size_t)i + 1], obj[3 * (size_t)i + 2]}, x[2] = {img[2 * (size_t)i], img[2 * (size_t)i + 1]};
    return score_one<2>(X, x, M, K, false) <= threshold;
}

// The inliers of M among the n points of obj / img, counted by ONE wave with M in registers (the same in every lane, as is the result).
__device__ __forceinline__ int pnp_count(int lane, const double* obj, const double* img, int n, const double* M, const double* K, float threshold) {
    int c = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {   // (every lane takes every trip: the ballot sees the whole wave)
        const int i = i0 + lane;
        c += __popcll(__ballot(i < n && pnp_inlier(obj, img, i, M, K, threshold)));
    }
    return c;
}

// out[lane] = M[lane] for the 12 entries of a pose that every lane holds in registers (by selection: no register is indexed).
__device__ __forceinline__ void pnp_write_model(int lane, const double* M, double* out) {
    if (lane >= 12) return;
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < 12; ++k)
        if (k == lane) v = M[k];
    out[lane] = v;
}

// ---- Levenberg-Marquardt on the reprojection error (eacham_pnp_refine_batch, pnp_refine.hip; include/eacham_hip.h states the
// definition, tests/cpp/pnp_refine_reference.c restates it on the CPU and the kernel gives its bytes). Only + - * /, every operation
// rounded on its own, every sum in the order written. The lane-local pieces are __host__ __device__ so that they can be stepped
// through on the CPU; nothing in the product calls them there.

constexpr int PNP_REFINE_NS = 28;   // 21 entries of H (upper triangle, row by row), 6 of g, the cost
constexpr int PNP_REFINE_CONVERGED = 0, PNP_REFINE_CAP = 1, PNP_REFINE_NOT_REFINED = 2;   // EACHAM_PNP_REFINE_* of the header

__host__ __device__ constexpr int pnp_hidx(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }   // i <= j

// S += the terms of one correspondence under M = R | t: J'J, J'r and r'r with r = (fx x/z + cx - u, fy y/z + cy - v) and J its
// derivative by [w, v] of X_c' = X_c + w x X_c + v. Returns z.
__host__ __device__ __forceinline__ double pnp_refine_row(const double* X, const double* x, const double* M, const double* K, double* S) {
    const double xc = M[0] * X[0] + M[1] * X[1] + M[2] * X[2] + M[9];
    const double yc = M[3] * X[0] + M[4] * X[1] + M[5] * X[2] + M[10];
    const double zc = M[6] * X[0] + M[7] * X[1] + M[8] * X[2] + M[11];
    const double iz = 1.0 / zc;
    const double xn = xc * iz, yn = yc * iz;
    const double r0 = (K[0] * xn + K[2]) - x[0], r1 = (K[1] * yn + K[3]) - x[1];
    const double a = K[0] * iz, b = K[1] * iz;
    const double Ju[6] = {-(K[0] * xn * yn), K[0] * (1.0 + xn * xn), -(K[0] * yn), a, 0.0, -(a * xn)};
    const double Jv[6] = {-(K[1] * (1.0 + yn * yn)), K[1] * xn * yn, K[1] * xn, 0.0, b, -(b * yn)};
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) S[pnp_hidx(i, j)] = S[pnp_hidx(i, j)] + (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
#pragma unroll
    for (int i = 0; i < 6; ++i) S[21 + i] = S[21 + i] + (Ju[i] * r0 + Jv[i] * r1);
    S[27] = S[27] + (r0 * r0 + r1 * r1);
    return zc;
}

// (H + lambda diag H) d = -g by an unpivoted L D L' factorisation in registers; false if a pivot is not > 0.
__host__ __device__ __forceinline__ bool pnp_refine_solve(const double* S, double lambda, double* d) {
    double L[6][6], D[6], y[6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double v = S[pnp_hidx(j, j)] + lambda * S[pnp_hidx(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) v = v - L[j][k] * D[k] * L[j][k];
        ok = ok && v > 0.0;   // (the rest is computed and thrown away: no divergence, no early exit from an unrolled nest)
        D[j] = v;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double w = S[pnp_hidx(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) w = w - L[i][k] * D[k] * L[j][k];
            L[i][j] = w / v;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = -S[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
        y[i] = v;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = y[i] / D[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * d[k];
        d[i] = v;
    }
    return ok;
}

// R <- C(w) R, t <- C(w) t + v with the Cayley map of the BA's Pose3 chart, C(w) = ((4 - |w|^2) I + 2 w w' + 4 [w]x) / (4 + |w|^2).
__host__ __device__ __forceinline__ void pnp_refine_retract(const double* M, const double* d, double* Mc) {
    const double x = d[0], y = d[1], z = d[2];
    const double xx = x * x, yy = y * y, zz = z * z;
    const double f = 1.0 / (4.0 + (xx + yy + zz));
    const double C[9] = {f * (4.0 + xx - yy - zz), f * (2.0 * (x * y - 2.0 * z)), f * (2.0 * (x * z + 2.0 * y)),
                         f * (2.0 * (x * y + 2.0 * z)), f * (4.0 - xx + yy - zz), f * (2.0 * (y * z - 2.0 * x)),
                         f * (2.0 * (x * z - 2.0 * y)), f * (2.0 * (y * z + 2.0 * x)), f * (4.0 - xx - yy + zz)};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Mc[3 * r + c] = C[3 * r] * M[c] + C[3 * r + 1] * M[3 + c] + C[3 * r + 2] * M[6 + c];
        Mc[9 + r] = C[3 * r] * M[9] + C[3 * r + 1] * M[10] + C[3 * r + 2] * M[11] + d[3 + r];
    }
}

// H, g and the cost of M over the used rows (use null: every row) of a problem's n points, by ONE wave: lane l owns the rows i with
// i % 64 == l and adds the used ones in ascending order from zero; the 64 partials are folded 32, 16, 8, 4, 2, 1 (a butterfly: a + b
// is b + a, so every lane ends with the sum lane 0 of a shuffle-down tree would hold). used = the number of used rows; returns true
// if one of them has !(z > 0). The same in every lane.
__device__ __forceinline__ bool pnp_refine_sums(int lane, const double* __restrict__ obj, const double* __restrict__ img,
                                                const unsigned char* __restrict__ use, int n, const double* M, const double* K, double* S, int& used) {
#pragma unroll
    for (int k = 0; k < PNP_REFINE_NS; ++k) S[k] = 0.0;
    bool bad = false;
    int m = 0;
    for (int i = lane; i < n; i += 64) {
        if (use && !use[i]) continue;
        const double X[3] = {obj[3 * (size_t)i], obj[3 * (size_t)i + 1], obj[3 * (size_t)i + 2]}, x[2] = {img[2 * (size_t)i], img[2 * (size_t)i + 1]};
        const double z = pnp_refine_row(X, x, M, K, S);
        bad = bad || !(z > 0.0);
        ++m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < PNP_REFINE_NS; ++k) S[k] = S[k] + __shfl_xor(S[k], off);
        m += __shfl_xor(m, off);
    }
    used = m;
    return __ballot(bad) != 0ull;
}

}  // namespace eacham
