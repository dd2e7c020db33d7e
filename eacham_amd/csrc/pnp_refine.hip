// pnp_refine.hip — cv::solvePnPRefineLM for a whole LIST of problems per call, gfx950: Levenberg-Marquardt on the reprojection error
// of a pose over the rows its caller names (the RANSAC winner's inliers), where eacham_pnp_refit_batch (pnp_batch.hip) ends on EPnP's
// algebraic fit. include/eacham_hip.h states the algorithm with eacham_pnp_refine_batch; its pieces are the device functions of
// pnp_dev.hpp; tests/cpp/pnp_refine_reference.c is the CPU restatement the kernel is held to as bytes.
//
//   pnp_refine_kernel   a WAVE per problem, PNP_REFINE_WAVES per workgroup, no barrier, no LDS (the mapping rb_count's A/B of DESIGN §7d
//                       found ahead at these sizes). The WHOLE loop runs here — one launch for the list, no host turn per try. H, g,
//                       the cost, the pose and lambda live in registers, identical in every lane; a try is the 6 x 6 solve on every
//                       lane (identical values), the retraction, and ONE pass over the problem's points that gives the candidate's
//                       cost together with its H and g (pnp_refine_sums: a trip per 64 rows, a lane's rows in ascending order, a
//                       fixed butterfly over the 28 partials), so an accepted step costs no second pass. After the loop the same
//                       wave recounts err <= threshold over ALL of the problem's points under the refined pose (pnp_inlier, the
//                       predicate pb_refit_kernel uses).
// A problem's result depends on its own rows only: not on the length of the list, nor on where in it the problem sits.
#include "context.hpp"
#include "pnp_dev.hpp"
#include "solve_launch.hpp"

#include <cmath>

namespace eacham {
namespace {

constexpr int PNP_REFINE_WAVES = 4;

__global__ __launch_bounds__(64 * PNP_REFINE_WAVES) void pnp_refine_kernel(int n_problems, const long long* __restrict__ point_ptr,
                                                                          const double* __restrict__ obj, const double* __restrict__ img,
                                                                          const double* __restrict__ Kdev, const double* __restrict__ poses,
                                                                          const unsigned char* __restrict__ has_pose,
                                                                          const unsigned char* __restrict__ use_mask, int max_tries, float threshold,
                                                                          double* __restrict__ refined, double* __restrict__ cost,
                                                                          int* __restrict__ tries, int* __restrict__ status,
                                                                          unsigned char* __restrict__ mask, int* __restrict__ n_inliers) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * PNP_REFINE_WAVES + (threadIdx.x >> 6);
    if (p >= n_problems) return;   // (wave-uniform; the kernel has no barrier)
    const long long base = point_ptr[p];
    const int n = (int)(point_ptr[p + 1] - base);
    const bool has = has_pose[p] != 0;
    const double K[4] = {Kdev[0], Kdev[1], Kdev[2], Kdev[3]};
    obj += 3 * base, img += 2 * base;
    const unsigned char* use = use_mask ? use_mask + base : nullptr;
    double M[12], S[PNP_REFINE_NS];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = has ? poses[12 * (size_t)p + k] : 0.0;
    double cost0 = 0.0;
    int t = 0, st = PNP_REFINE_NOT_REFINED;
    bool run = false;
    if (has) {   // (wave-uniform, as is every branch below: the values are the same in every lane)
        int used = 0;
        const bool bad = pnp_refine_sums(lane, obj, img, use, n, M, K, S, used);
        cost0 = S[27] == S[27] ? S[27] : __longlong_as_double(0x7ff8000000000000ll);   // a NaN cost leaves as ONE bit pattern
        run = used >= 3 && !bad && S[27] - S[27] == 0.0;
    }
    double cost1 = cost0;
    if (run) {
        double lambda = 1e-3;
        st = PNP_REFINE_CAP;
        while (t < max_tries) {
            double d[6], Mc[12], Sc[PNP_REFINE_NS];
            ++t;
            if (!pnp_refine_solve(S, lambda, d)) {
                lambda = 10.0 * lambda < 1e12 ? 10.0 * lambda : 1e12;
                continue;
            }
            double big = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const double a = d[k] < 0.0 ? -d[k] : d[k];
                if (!(a <= big)) big = a;   // (a NaN step is not small)
            }
            if (big <= 1e-10) {
                st = PNP_REFINE_CONVERGED;
                break;
            }
            pnp_refine_retract(M, d, Mc);
            int uc = 0;
            const bool badc = pnp_refine_sums(lane, obj, img, use, n, Mc, K, Sc, uc);
            if (!badc && Sc[27] < S[27]) {
                const double dec = S[27] - Sc[27];
#pragma unroll
                for (int k = 0; k < 12; ++k) M[k] = Mc[k];
#pragma unroll
                for (int k = 0; k < PNP_REFINE_NS; ++k) S[k] = Sc[k];
                lambda = lambda / 10.0 > 1e-12 ? lambda / 10.0 : 1e-12;
                if (dec <= 1e-9 * S[27]) {
                    st = PNP_REFINE_CONVERGED;
                    break;
                }
            } else {
                lambda = 10.0 * lambda < 1e12 ? 10.0 * lambda : 1e12;
            }
        }
        cost1 = S[27];
    }
    pnp_write_model(lane, M, refined + 12 * (size_t)p);
    if (lane == 0) cost[2 * (size_t)p] = cost0, cost[2 * (size_t)p + 1] = cost1, tries[p] = t, status[p] = st;
    if (!mask && !n_inliers) return;
    int c = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {   // (every lane takes every trip: the ballot sees the whole wave)
        const int i = i0 + lane;
        const bool in = has && i < n && pnp_inlier(obj, img, i, M, K, threshold);
        if (mask && i < n) mask[base + i] = in;
        c += __popcll(__ballot(in));
    }
    if (n_inliers && lane == 0) n_inliers[p] = c;
}

}  // namespace
}  // namespace eacham

using namespace eacham;

extern "C" int eacham_pnp_refine_batch(eacham_ctx* ctx, int n_problems, const int64_t* point_ptr, const double* object_points,
                                       const double* image_points, const double* K, const double* poses, const uint8_t* has_pose,
                                       const uint8_t* use_mask, int max_tries, float threshold, double* refined, double* cost, int32_t* tries,
                                       int32_t* status, uint8_t* inlier_mask, int32_t* n_inliers) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    const char* call = "pnp_refine_batch";
    if (n_problems < 0) return ctx->fail(EACHAM_ERR_INVALID, "%s: negative number of problems", call);
    if (max_tries < 1) return ctx->fail(EACHAM_ERR_INVALID, "%s: max_tries %d below 1", call, max_tries);
    if ((inlier_mask || n_inliers) && !(threshold >= 0.f)) return ctx->fail(EACHAM_ERR_INVALID, "%s: threshold is NaN or negative", call);
    if (n_problems == 0) return EACHAM_OK;
    const int P = n_problems;
    if (int rc = check_table(ctx, call, "point_ptr", P, point_ptr)) return rc;
    const long long NP = point_ptr[P];
    if (!K || !poses || !has_pose || !refined || !cost || !tries || !status || (NP > 0 && (!object_points || !image_points)))
        return ctx->fail(EACHAM_ERR_INVALID, "%s: null array", call);
    EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    IoStage io(ctx, st);
    const auto h_r = io.out<double>(refined, 12 * (size_t)P), h_c = io.out<double>(cost, 2 * (size_t)P);
    const auto h_t = io.out<int>(tries, (size_t)P), h_s = io.out<int>(status, (size_t)P);
    const auto h_mask = io.out<unsigned char>(inlier_mask, inlier_mask ? (size_t)NP : 0);
    const auto h_ni = io.out<int>(n_inliers, n_inliers ? (size_t)P : 0);
    const auto h_pp = io.in<long long>(point_ptr, (size_t)P + 1);
    const auto h_K = io.in<double>(K, 4);
    const auto h_a = io.in<double>(object_points, 3 * (size_t)NP), h_b = io.in<double>(image_points, 2 * (size_t)NP);
    const auto h_m = io.in<double>(poses, 12 * (size_t)P);
    const auto h_has = io.in<unsigned char>(has_pose, (size_t)P);
    const auto h_use = io.in<unsigned char>(use_mask, use_mask ? (size_t)NP : 0);
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    {
        ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
        const unsigned gw = (unsigned)((P + PNP_REFINE_WAVES - 1) / PNP_REFINE_WAVES);
        pnp_refine_kernel<<<gw, 64 * PNP_REFINE_WAVES, 0, st>>>(P, d(h_pp), d(h_a), d(h_b), d(h_K), d(h_m), d(h_has), use_mask ? d(h_use) : nullptr,
                                                               max_tries, threshold, d(h_r), d(h_c), d(h_t), d(h_s),
                                                               inlier_mask ? d(h_mask) : nullptr, n_inliers ? d(h_ni) : nullptr);
    }
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return io.finish();
}
