// p3p.hip — the MINIMAL hypothesis of the PnP RANSAC, gfx950: P3P on four-point samples (three points give up to four poses, the
// fourth picks one) where solve.hip / pnp_batch.hip run EPnP on five. What cv::solvePnPRansac(..., cv::SOLVEPNP_P3P) draws; the
// definition — Grunert's quartic, the project's Durand-Kerner recipe at degree 4, two Newton steps on the depths, the pose from the
// two triangle frames, the fourth point's PnP error — is stated with eacham_solve_p3p in include/eacham_hip.h and runs in ONE device
// function (p3p_sample, p3p_dev.hpp), which both kernels below call: the bits cannot differ between the entry points.
//
//   eacham_solve_p3p                  solve_p3p_kernel  a LANE per sample (a sample is a few hundred flops of scalar fp64 with no shared
//                                                       state: 10 000 samples are 157 waves), optionally every candidate
//   eacham_pnp_hypotheses_batch_p3p   p3p_count_kernel  a WAVE per sample, SOLVE_WAVES per workgroup (the shape of pb_count_kernel):
//                                                       the sample's problem by prim::segment_of in sample_ptr, the solve on every
//                                                       lane (identical values, so the candidates run in a row), then the count
//                                                       pb_count_kernel makes (pnp_count, pnp_dev.hpp) over the problem's own points,
//                                                       with the model passed from the solve to the count in registers. One RANSAC
//                                                       round is ONE launch and no scratch array, where EPnP's is three launches and two.
// The entry's checks and staging are eacham_pnp_hypotheses_batch's (PnpHypCall, solve_launch.hpp). The refit of the winner's inliers
// stays EPnP (eacham_pnp_refit_batch, pnp_batch.hip), as in OpenCV.
#include "context.hpp"
#include "devprim.hpp"
#include "p3p_dev.hpp"
#include "pnp_dev.hpp"
#include "solve_dev.hpp"
#include "solve_launch.hpp"

namespace eacham {
namespace {

__device__ __forceinline__ void p3p_gather(const int* __restrict__ idx, const double* __restrict__ obj, const double* __restrict__ img, double* X, double* x) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const size_t i = (size_t)idx[k];
#pragma unroll
        for (int e = 0; e < 3; ++e) X[3 * k + e] = obj[3 * i + e];
#pragma unroll
        for (int e = 0; e < 2; ++e) x[2 * k + e] = img[2 * i + e];
    }
}

// A lane per sample. candidates / n_candidates may be null (not wanted).
__global__ __launch_bounds__(64) void solve_p3p_kernel(const double* __restrict__ obj, const double* __restrict__ img, const double* __restrict__ Kdev,
                                                       int n_samples, const int* __restrict__ idx, double* __restrict__ models,
                                                       int* __restrict__ n_models, double* __restrict__ candidates, int* __restrict__ n_candidates) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_samples) return;
    const double K[4] = {Kdev[0], Kdev[1], Kdev[2], Kdev[3]};
    double X[12], x[8], M[12];
    p3p_gather(idx + 4 * (size_t)s, obj, img, X, x);
    int nc = 0;
    const int n = p3p_sample(X, x, K, M, candidates ? candidates + 48 * (size_t)s : nullptr, &nc);
#pragma unroll
    for (int k = 0; k < 12; ++k) models[12 * (size_t)s + k] = M[k];
    n_models[s] = n;
    if (n_candidates) n_candidates[s] = nc;
}

// A wave per sample: the problem, the solve, the count. models may be null (not wanted).
__global__ __launch_bounds__(64 * SOLVE_WAVES) void p3p_count_kernel(SolveSeg seg, const double* __restrict__ obj, const double* __restrict__ img,
                                                                    const double* __restrict__ Kdev, int n_samples, const int* __restrict__ idx,
                                                                    float threshold, double* __restrict__ models, int* __restrict__ n_models,
                                                                    int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * SOLVE_WAVES + (threadIdx.x >> 6);
    if (s >= n_samples) return;
    const int p = prim::segment_of(seg.sample_ptr, seg.n_problems, s);
    const long long base = seg.point_ptr[p];
    const int n = (int)(seg.point_ptr[p + 1] - base);
    double M[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = 0.0;
    int have = 0;
    const double K[4] = {Kdev[0], Kdev[1], Kdev[2], Kdev[3]};
    const double* pa = obj + 3 * base;
    const double* pb = img + 2 * base;
    if (n >= 4) {   // (wave-uniform) a problem with fewer points than a sample: its samples are not looked at
        double X[12], x[8];
        p3p_gather(idx + 4 * (size_t)s, pa, pb, X, x);
        int nc = 0;
        have = p3p_sample(X, x, K, M, nullptr, &nc);
    }
    if (models) pnp_write_model(lane, M, models + 12 * (size_t)s);   // (identical values in every lane)
    const int c = have ? pnp_count(lane, pa, pb, n, M, K, threshold) : 0;   // (wave-uniform)
    if (lane == 0) n_models[s] = have, counts[s] = c;
}

}  // namespace
}  // namespace eacham

using namespace eacham;

extern "C" int eacham_solve_p3p(eacham_ctx* ctx, int n_points, const double* object_points, const double* image_points, const double* K,
                                int n_samples, const int32_t* sample_idx, double* models, int32_t* n_models, double* candidates,
                                int32_t* n_candidates) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_points < 0 || n_samples < 0 || (n_samples > 0 && (!object_points || !image_points || !K || !sample_idx || !models || !n_models)))
        return ctx->fail(EACHAM_ERR_INVALID, "solve_p3p: null argument or negative size");
    if (n_samples == 0) return EACHAM_OK;
    if (int rc = check_sample_idx(ctx, "solve_p3p", -1, sample_idx, 4 * (long long)n_samples, n_points)) return rc;
    EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    IoStage io(ctx, st);
    const auto h_a = io.in<double>(object_points, 3 * (size_t)n_points), h_b = io.in<double>(image_points, 2 * (size_t)n_points);
    const auto h_K = io.in<double>(K, 4);
    const auto h_i = io.in<int>(sample_idx, 4 * (size_t)n_samples);
    const auto h_m = io.out<double>(models, 12 * (size_t)n_samples);
    const auto h_n = io.out<int>(n_models, (size_t)n_samples);
    const auto h_c = io.out<double>(candidates, candidates ? 48 * (size_t)n_samples : 0);
    const auto h_nc = io.out<int>(n_candidates, n_candidates ? (size_t)n_samples : 0);
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    {
        ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
        solve_p3p_kernel<<<(unsigned)((n_samples + 63) / 64), 64, 0, st>>>(d(h_a), d(h_b), d(h_K), n_samples, d(h_i), d(h_m), d(h_n),
                                                                          candidates ? d(h_c) : nullptr, n_candidates ? d(h_nc) : nullptr);
    }
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return io.finish();
}

extern "C" int eacham_pnp_hypotheses_batch_p3p(eacham_ctx* ctx, int n_problems, const int64_t* point_ptr, const double* object_points,
                                               const double* image_points, const double* K, const int64_t* sample_ptr,
                                               const int32_t* sample_idx, float threshold, double* models, int32_t* n_models,
                                               int32_t* inlier_counts) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    const char* call = "pnp_hypotheses_batch_p3p";
    if (n_problems < 0) return ctx->fail(EACHAM_ERR_INVALID, "%s: negative number of problems", call);
    if (n_problems == 0) return EACHAM_OK;
    PnpHypCall c{n_problems, 4, point_ptr, object_points, image_points, K, sample_ptr, sample_idx, models, n_models, inlier_counts};
    if (int rc = c.check(ctx, call)) return rc;
    if (c.S == 0) return EACHAM_OK;
    EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    IoStage io(ctx, st);
    c.stage(io);
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    {
        ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
        const unsigned gw = (unsigned)((c.S + SOLVE_WAVES - 1) / SOLVE_WAVES);
        p3p_count_kernel<<<gw, 64 * SOLVE_WAVES, 0, st>>>(SolveSeg{d(c.h_pp), d(c.h_sp), c.P, nullptr}, d(c.h_a), d(c.h_b), d(c.h_K), (int)c.S,
                                                         d(c.h_i), threshold, models ? d(c.h_m) : nullptr, d(c.h_n), d(c.h_c));
    }
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return io.finish();
}
