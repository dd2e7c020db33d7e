// score.hip — batch scoring of pose hypotheses for the robust estimators of eacham's two-view / PnP stage
// (SURVEY.md §8(f) rank 3), gfx950.
//
//   cv::findEssentialMat(..., cv::LMEDS, 0.99, 4.0, 1000, mask)      /root/reference/modules/sfm/reconstruction/ReconstructionManager.cpp:57-61
//   cv::findHomography(pts1, pts2, cv::LMEDS, 4.0, mask2, 100, 0.999)  :75
//   cv::solvePnPRansac(..., 10000, 4.0f, 0.999f, inliers, SOLVEPNP_EPNP)  :227-228   (10 000 hypotheses x every correspondence)
//
// What runs here is the part of those estimators that is data-parallel over (hypothesis, correspondence): the
// error each model assigns to each point — OpenCV 4.5.5's EMEstimatorCallback / HomographyEstimatorCallback /
// PnPRansacCallback ::computeError (the tests hold a CPU restatement of the same formulas) —, the inlier count under a threshold
// (RANSAC) and the median (LMedS). Drawing minimal samples and solving them stays with the caller.
// Layout: correspondences resident once (n x 2 / n x 3 doubles), models nm x 9 / nm x 12 doubles; one workgroup per
// model sweeps the points (coalesced), keeps its n errors as ordered-uint keys in LDS (n <= 16384) or re-reads them
// from the optional error matrix, counts inliers with a fixed-order block sum and finds the median by a 4-pass
// 8-bit radix select — no sort, no atomics on data, bit-identical with the oracle (no FMA contraction: every
// product and sum is an explicit round-to-nearest intrinsic, as a baseline x86-64 OpenCV build computes them).
// HBM-bound in principle (n x 32 B read per model from L2), latency-bound at the sizes the reference has
// (<= 15 000 matches): one launch scores all 10 000 PnP hypotheses.
#include "context.hpp"
#include "score_dev.hpp"

#include <cmath>
#include <vector>

// HIP's __fmul_rn / __dadd_rn are plain operators to the compiler, and hipcc contracts a * b + c into an FMA by
// default: this file is compiled with -ffp-contract=off (csrc/Makefile); the reference arithmetic has no fused
// operations (the GPU parity tests are bit-exact, so dropping the flag shows at once).

namespace eacham {
namespace {

template <int KIND>
__global__ __launch_bounds__(SC_BLOCK) void score_kernel(int n, const double* __restrict__ a, const double* __restrict__ b,
                                                         const double* __restrict__ models, const double* __restrict__ Kdev,
                                                         int normalise, float threshold, float* __restrict__ errors,
                                                         int* __restrict__ counts, float* __restrict__ medians, int keys_in_lds) {
    extern __shared__ unsigned keys[];  // [n] when keys_in_lds
    __shared__ unsigned hist[256], sh[2];
    __shared__ int wsum[SC_BLOCK / 64];
    constexpr int MA = KIND == 2 ? 3 : 2, MM = KIND == 2 ? 12 : 9;
    const int m = blockIdx.x;
    double M[MM], K[4] = {1, 1, 0, 0};
#pragma unroll
    for (int k = 0; k < MM; ++k) M[k] = models[(size_t)MM * m + k];
    if (Kdev) {
#pragma unroll
        for (int k = 0; k < 4; ++k) K[k] = Kdev[k];
    }
    float* erow = errors ? errors + (size_t)m * n : nullptr;
    int c = 0;
    for (int i = threadIdx.x; i < n; i += SC_BLOCK) {
        double pa[MA], pb[2] = {b[2 * (size_t)i], b[2 * (size_t)i + 1]};
#pragma unroll
        for (int k = 0; k < MA; ++k) pa[k] = a[(size_t)MA * i + k];
        const float e = score_one<KIND>(pa, pb, M, K, normalise != 0);
        c += e <= threshold;
        if (erow) erow[i] = e;
        if (keys_in_lds) keys[i] = fkey(e);
    }
    const int tot = block_count(c, wsum);
    if (threadIdx.x == 0 && counts) counts[m] = tot;
    if (!medians) return;
    if (n == 0) {
        if (threadIdx.x == 0) medians[m] = __uint_as_float(0x7fc00000u);
        return;
    }
    __syncthreads();  // keys / the error row are complete (the row was written by this workgroup: visible after the barrier)
    const float med = block_median([&](int i) { return keys_in_lds ? keys[i] : fkey(erow[i]); }, n, hist, sh);
    if (threadIdx.x == 0) medians[m] = med;
}

}  // namespace
}  // namespace eacham

using namespace eacham;

extern "C" int eacham_score_hypotheses(eacham_ctx* ctx, int kind, int n_points, const double* a, const double* b, int n_models,
                                       const double* models, const double* K, float threshold, float* errors,
                                       int32_t* inlier_counts, float* medians) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (kind < EACHAM_SCORE_ESSENTIAL || kind > EACHAM_SCORE_FUNDAMENTAL || n_points < 0 || n_models < 0)
        return ctx->fail(EACHAM_ERR_INVALID, "score: bad kind or negative size");
    if (n_models == 0) return EACHAM_OK;
    if (!models || (n_points > 0 && (!a || !b)) || (kind == EACHAM_SCORE_PNP && !K))
        return ctx->fail(EACHAM_ERR_INVALID, "score: null array");
    const long long total = (long long)n_points * n_models;
    const bool keys_in_lds = n_points <= SC_MAX_LDS;
    if (!keys_in_lds && medians && total > (1ll << 32)) return ctx->fail(EACHAM_ERR_CAPACITY, "score: error matrix too large");
    EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int ma = kind == EACHAM_SCORE_PNP ? 3 : 2, mm = kind == EACHAM_SCORE_PNP ? 12 : 9;
    const bool need_err = errors != nullptr || (!keys_in_lds && medians != nullptr);
    hipStream_t st = ctx->stream;
    IoStage io(ctx, st);
    const auto h_a = io.in<double>(a, ma * (size_t)n_points), h_b = io.in<double>(b, 2 * (size_t)n_points);
    const auto h_m = io.in<double>(models, mm * (size_t)n_models), h_K = io.in<double>(K, 4);
    const auto h_c = io.out<int>(inlier_counts, (size_t)n_models);
    const auto h_med = io.out<float>(medians, (size_t)n_models);
    // the error matrix: a result when asked for, else the scratch of the medians' selection beyond SC_MAX_LDS points
    const auto h_e = errors ? io.out<float>(errors, (size_t)total) : io.scratch<float>(need_err ? (size_t)total : 0);
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    const size_t smem = keys_in_lds && medians ? sizeof(unsigned) * (size_t)(n_points > 0 ? n_points : 1) : 0;
    {
        ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
#define EACHAM_SCORE_LAUNCH(KIND)                                                                                              \
    do {                                                                                                                       \
        if (smem > 48 * 1024)                                                                                                  \
            EACHAM_HIP_TRY(ctx, hipFuncSetAttribute((const void*)score_kernel<KIND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)); \
        score_kernel<KIND><<<n_models, SC_BLOCK, smem, st>>>(n_points, d(h_a), d(h_b), d(h_m), K ? d(h_K) : nullptr,                 \
                                                             K && kind == EACHAM_SCORE_ESSENTIAL ? 1 : 0, threshold,             \
                                                             need_err ? d(h_e) : nullptr, d(h_c), medians ? d(h_med) : nullptr,  \
                                                             keys_in_lds && medians ? 1 : 0);                                    \
    } while (0)
        if (kind == EACHAM_SCORE_ESSENTIAL) EACHAM_SCORE_LAUNCH(0);
        else if (kind == EACHAM_SCORE_HOMOGRAPHY) EACHAM_SCORE_LAUNCH(1);
        else if (kind == EACHAM_SCORE_PNP) EACHAM_SCORE_LAUNCH(2);
        else EACHAM_SCORE_LAUNCH(3);
#undef EACHAM_SCORE_LAUNCH
    }
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return io.finish();
}
