// pnp_dev.hpp — the inlier test of the PnP RANSAC as its kernels share it (pb_count_kernel and pb_refit_kernel of pnp_batch.hip,
// p3p_count_kernel of p3p.hip): a point within the threshold of a pose, a wave's count of such points, a wave's write-out of the pose.
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

}  // namespace eacham
