// pnp_batch.hip — cv::solvePnPRansac's two device stages for a whole LIST of problems per call, gfx950.
//
// What SolvePnPRansac (include/eacham/PnPHip.hpp) does for one frame with two blocking calls per chunk of samples (eacham_solve_pnp,
// eacham_score_hypotheses) and two more for the refit runs here for n_problems (map points, pixels) problems: the inputs go up
// once, the results come back once, and the number of launches does not depend on n_problems.
//
// eacham_pnp_hypotheses_batch — one RANSAC round:
//   solve_pnp_launch  (solve.hip, through solve_launch.hpp) the list instantiation of solve_pnp_front_kernel / solve_pnp_back_kernel — the
//                   kernels eacham_solve_pnp launches, not a copy of them — on the sample's own problem, found by a binary search in
//                   sample_ptr (left in sample_problem[])
//   pb_count        a wave per sample: the first strictly smallest error of the three starts (pnp_first_smallest, solve_dev.hpp)
//                   gives the model; pnp_count (pnp_dev.hpp: score_one<PNP> over the problem's own points, a ballot and a popcount
//                   per 64 points — the count p3p_count_kernel of p3p.hip makes too) gives its inlier count. The model passes
//                   from the choice to the count in registers.
// eacham_pnp_refit_batch — the tail of solvePnPRansac:
//   pb_refit        a workgroup per problem: scores the model, writes the mask, compacts the inlier indices IN ASCENDING ORDER
//                   into the problem's own row of a workspace (ballot prefix: EPnP's sums run in row order), then
//                   pnp_refit_body (solve_dev.hpp: the function solve_pnp_big_kernel runs) on that row — for every size of the
//                   inlier set: with at most 64 rows a lane holds one term and the partials are added in lane order, which is the
//                   sequential sum of the at-most-64-point form term by term.
// The hypotheses entry's checks and staging from the tables on are PnpHypCall's (solve_launch.hpp), shared with the P3P entry.
#include "context.hpp"
#include "pnp_dev.hpp"
#include "solve_dev.hpp"
#include "solve_launch.hpp"

#include <algorithm>

namespace eacham {
namespace {

// A wave per sample: the choice among the three starts, then the count. models may be null (not wanted).
__global__ __launch_bounds__(64 * SOLVE_WAVES) void pb_count_kernel(const long long* __restrict__ point_ptr, const double* __restrict__ obj,
                                                                   const double* __restrict__ img, const double* __restrict__ Kdev,
                                                                   int n_samples, const int* __restrict__ sample_problem,
                                                                   const double* __restrict__ tmp, float threshold,
                                                                   double* __restrict__ models, int* __restrict__ n_models,
                                                                   int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * SOLVE_WAVES + (threadIdx.x >> 6);
    if (s >= n_samples) return;
    const size_t ns = (size_t)n_samples;
    const int which = pnp_first_smallest(tmp[(size_t)s * 13], tmp[(ns + s) * 13], tmp[(2 * ns + s) * 13]);
    double M[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = which >= 0 ? tmp[((size_t)which * n_samples + s) * 13 + 1 + k] : 0.0;
    if (models && lane < 12) models[12 * (size_t)s + lane] = which >= 0 ? tmp[((size_t)which * n_samples + s) * 13 + 1 + lane] : 0.0;
    int c = 0;
    if (which >= 0) {   // (wave-uniform)
        const double K[4] = {Kdev[0], Kdev[1], Kdev[2], Kdev[3]};
        const long long base = point_ptr[sample_problem[s]];
        const int n = (int)(point_ptr[sample_problem[s] + 1] - base);
        c = pnp_count(lane, obj + 3 * base, img + 2 * base, n, M, K, threshold);
    }
    if (lane == 0) n_models[s] = which >= 0 ? 1 : 0, counts[s] = c;
}

constexpr int PB_REFIT_BLOCK = 256;   // four waves score and compact; three of them then take EPnP's three starts

__global__ __launch_bounds__(PB_REFIT_BLOCK) void pb_refit_kernel(const long long* __restrict__ point_ptr, const double* __restrict__ obj,
                                                                 const double* __restrict__ img, const double* __restrict__ Kdev,
                                                                 const double* __restrict__ models, const unsigned char* __restrict__ has_model,
                                                                 float threshold, unsigned char* __restrict__ mask, int* __restrict__ n_inliers,
                                                                 int* rows_all, double* __restrict__ refit, int* __restrict__ refit_ok) {
    __shared__ PnpRefitLds W;
    __shared__ int wcnt[PB_REFIT_BLOCK / 64];
    const int p = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long base = point_ptr[p];
    const int n = (int)(point_ptr[p + 1] - base);
    const bool has = has_model[p] != 0;
    const double K4[4] = {Kdev[0], Kdev[1], Kdev[2], Kdev[3]};
    obj += 3 * base, img += 2 * base;
    int* rows = rows_all + base;   // (not __restrict__: written here, read by EPnP below after a workgroup barrier)
    double M[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = has ? models[12 * (size_t)p + k] : 0.0;
    int m = 0;   // inliers so far = where the next trip's first inlier goes
    for (int i0 = 0; i0 < n; i0 += PB_REFIT_BLOCK) {   // (every thread takes every trip)
        const int i = i0 + (int)threadIdx.x;
        const bool in = has && i < n && pnp_inlier(obj, img, i, M, K4, threshold);
        if (i < n) mask[base + i] = in;
        const unsigned long long b = __ballot(in);
        if (lane == 0) wcnt[wave] = __popcll(b);
        __syncthreads();
        int before = __popcll(b & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
        for (int w = 0; w < PB_REFIT_BLOCK / 64; ++w) {
            if (w < wave) before += wcnt[w];
            all += wcnt[w];
        }
        if (in) rows[m + before] = i;   // m + before < n: one slot per inlier of the problem
        m += all;
        __syncthreads();   // wcnt is read before the next trip writes it; after the last trip: rows[] is complete and visible
    }
    if (threadIdx.x == 0) n_inliers[p] = m;
    int which = -1;
    if (m >= 5) which = pnp_refit_body(m, rows, obj, img, K4, W);   // (workgroup-uniform) EPnP on the row of inliers
    if (threadIdx.x == 0) {
        for (int k = 0; k < 12; ++k) refit[12 * (size_t)p + k] = which >= 0 ? W.result[which][1 + k] : 0.0;
        refit_ok[p] = which >= 0 ? 1 : 0;
    }
}

}  // namespace
}  // namespace eacham

using namespace eacham;

extern "C" int eacham_pnp_hypotheses_batch(eacham_ctx* ctx, int n_problems, const int64_t* point_ptr, const double* object_points,
                                           const double* image_points, const double* K, const int64_t* sample_ptr, int sample_size,
                                           const int32_t* sample_idx, float threshold, double* models, int32_t* n_models,
                                           int32_t* inlier_counts) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    const char* call = "pnp_hypotheses_batch";
    if (n_problems < 0) return ctx->fail(EACHAM_ERR_INVALID, "%s: negative number of problems", call);
    if (sample_size < 5 || sample_size > 64) return ctx->fail(EACHAM_ERR_INVALID, "%s: sample_size %d outside 5..64", call, sample_size);
    if (n_problems == 0) return EACHAM_OK;
    PnpHypCall c{n_problems, sample_size, point_ptr, object_points, image_points, K, sample_ptr, sample_idx, models, n_models, inlier_counts};
    if (int rc = c.check(ctx, call)) return rc;
    const long long S = c.S;
    if (S == 0) return EACHAM_OK;
    EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    IoStage io(ctx, st);
    c.stage(io);
    const auto h_f = io.scratch<double>(PNP_FRAME * (size_t)S);   // the samples' frames between the front and the back half
    const auto h_t = io.scratch<double>(3 * 13 * (size_t)S);      // error + pose of the three starts
    const auto h_sprob = io.scratch<int>((size_t)S);
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    {
        ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
        const unsigned gw = (unsigned)((S + SOLVE_WAVES - 1) / SOLVE_WAVES);
        solve_pnp_launch(st, PnpLaunch{SolveSeg{d(c.h_pp), d(c.h_sp), c.P, d(h_sprob)}, d(c.h_a), d(c.h_b), d(c.h_K), c.m, (int)S, d(c.h_i), d(h_f), d(h_t)});
        pb_count_kernel<<<gw, 64 * SOLVE_WAVES, 0, st>>>(d(c.h_pp), d(c.h_a), d(c.h_b), d(c.h_K), (int)S, d(h_sprob), d(h_t), threshold,
                                                         models ? d(c.h_m) : nullptr, d(c.h_n), d(c.h_c));
    }
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return io.finish();
}

extern "C" int eacham_pnp_refit_batch(eacham_ctx* ctx, int n_problems, const int64_t* point_ptr, const double* object_points,
                                      const double* image_points, const double* K, const double* models, const uint8_t* has_model,
                                      float threshold, uint8_t* inlier_mask, int32_t* n_inliers, double* refit, int32_t* refit_ok) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    const char* call = "pnp_refit_batch";
    if (n_problems < 0) return ctx->fail(EACHAM_ERR_INVALID, "%s: negative number of problems", call);
    if (n_problems == 0) return EACHAM_OK;
    const int P = n_problems;
    if (int rc = check_table(ctx, call, "point_ptr", P, point_ptr)) return rc;
    const long long NP = point_ptr[P];
    if (!K || !models || !has_model || !n_inliers || !refit || !refit_ok || (NP > 0 && (!object_points || !image_points || !inlier_mask)))
        return ctx->fail(EACHAM_ERR_INVALID, "%s: null array", call);
    EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    IoStage io(ctx, st);
    const auto h_mask = io.out<unsigned char>(inlier_mask, (size_t)NP);
    const auto h_ni = io.out<int>(n_inliers, (size_t)P), h_ok = io.out<int>(refit_ok, (size_t)P);
    const auto h_r = io.out<double>(refit, 12 * (size_t)P);
    const auto h_pp = io.in<long long>(point_ptr, (size_t)P + 1);
    const auto h_K = io.in<double>(K, 4);
    const auto h_a = io.in<double>(object_points, 3 * (size_t)NP), h_b = io.in<double>(image_points, 2 * (size_t)NP);
    const auto h_m = io.in<double>(models, 12 * (size_t)P);
    const auto h_has = io.in<unsigned char>(has_model, (size_t)P);
    const auto h_rows = io.scratch<int>((size_t)NP);   // problem p's inlier indices, ascending, from point_ptr[p]
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    {
        ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
        pb_refit_kernel<<<(unsigned)P, PB_REFIT_BLOCK, 0, st>>>(d(h_pp), d(h_a), d(h_b), d(h_K), d(h_m), d(h_has), threshold, d(h_mask), d(h_ni),
                                                               d(h_rows), d(h_r), d(h_ok));
    }
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return io.finish();
}
