// solve.hip — batched MINIMAL SOLVERS of the robust estimators eacham calls (the scoring half is
// score.hip): one thread per caller-supplied minimal sample.
//
//   cv::findHomography(pts1, pts2, cv::LMEDS, 4.0, mask2, 100, 0.999)              ReconstructionManager.cpp:75
//       -> EACHAM_SOLVE_HOMOGRAPHY4: OpenCV 4.5.5 HomographyEstimatorCallback::runKernel (fundam.cpp): per-set point
//          normalisation, LtL of the 2 x 9 constraint rows, eigenvector of the smallest eigenvalue (cyclic Jacobi), denormalised, / H[8]
//   cv::findEssentialMat(pts1, pts2, focal, pp, cv::LMEDS, 0.99, 4.0, 1000, mask)  ReconstructionManager.cpp:57-61
//       -> EACHAM_SOLVE_ESSENTIAL5: EMEstimatorCallback::runKernel (five-point.cpp), Nister's five-point algorithm: null space of
//          the 5 x 9 epipolar system (Householder), the ten cubic constraints as a 10 x 20 matrix, Gauss-Jordan, det B(z) = a
//          degree-10 polynomial, its real roots (Durand-Kerner + Newton polish), up to ten unit-norm E per sample
//   cv::findFundamentalMat(pts1, pts2, cv::FM_LMEDS, 3.0, 0.99, 1000, mask)          (not a call of the reference: the estimator for
//                                                                                     image sets whose K is unknown or guessed)
//       -> EACHAM_SOLVE_FUNDAMENTAL7: run7Point (fundam.cpp) restated with two deliberate deviations — (1) Hartley normalisation of
//          each image's seven points (centroid, mean distance sqrt(2)) because the null space comes from the 9 x 9 Jacobi eigen-solver
//          on A^T A, not from an SVD of the 7 x 9 system on raw pixels; (2) unit Frobenius norm, not F[8] = 1. The cubic
//          det(z f1 + f2), its real roots by the five-point solver's Durand-Kerner recipe for degree <= 3, up to three F per sample
//          (solve_dev.hpp: fundamental7_wave)
//   cv::solvePnPRansac(pts3d, pts2d, K, dist, rvec, t, false, 10000, 4.0f, 0.999f, inliers, cv::SOLVEPNP_EPNP)   :227-228
//       -> eacham_solve_pnp: EPnP on every 5-point sample (the RANSAC kernel) and on the inlier set (the final refit): four control
//          points, M^T M of the projection system, its four smallest eigenvectors (Jacobi 12 x 12), the 6 x 10 distance system, three
//          linearised starts + Gauss-Newton, absolute orientation (Horn), smallest reprojection error; the point passes recompute the
//          barycentric coordinates, so a thread's state does not grow with the sample size
// OpenCV draws the samples from its own RNG: the sample INDICES are an argument here (what RANSACPointSetRegistrator /
// LMeDSPointSetRegistrator::getSubset produce), so "these correspondences -> these models" is what can be held against the
// CPU restatement the tests keep (solve_oracle.c, bit for bit: this file is compiled with -ffp-contract=off and uses only
// + - * / sqrt) — end-to-end parity with cv::findHomography / findEssentialMat cannot be pinned without that RNG stream.
// A sample is ~10^4-10^5 flops of branchy fp64 with kilobytes of private state: latency-bound, no roofline claim; the
// 1000 / 100 iterations the reference asks for are one launch.
#include "context.hpp"
#include "devprim.hpp"
#include "solve_dev.hpp"
#include "solve_launch.hpp"

#include <cstdint>

namespace eacham {
namespace {

// Every stage below is ONE kernel template with two instantiations: LIST = false, the one-problem calls of this file, and LIST = true,
// the list calls (lmeds_batch.hip, pnp_batch.hip through solve_launch.hpp). What the list form adds is sample_segment() and nothing
// else, so a sample gives the same bits through either and a change of a solver is made once.

// LIST: the problem of sample s by a binary search in sample_ptr, left in sample_problem[s]; base = where its points begin. False: the
// problem has fewer than m points, and its samples are not solved. (The one-problem calls have no such rule: they check the indices
// against n_points on the host and solve whatever valid sample they are given, repeated indices on a 2-point problem included.)
__device__ __forceinline__ bool sample_segment(const SolveSeg& g, int s, int m, long long& base) {
    const int p = prim::segment_of(g.sample_ptr, g.n_problems, s);
    base = g.point_ptr[p];
    if ((threadIdx.x & 63) == 0) g.sample_problem[s] = p;
    return g.point_ptr[p + 1] - base >= m;   // (wave-uniform)
}

// Samples of at most 64 points (the RANSAC loop's five-point samples) in two launches. Front: ONE WAVE per sample, SOLVE_WAVES samples
// per workgroup (no workgroup barrier anywhere: waves return on their own), leaving the sample's frame — 130 doubles: c0 3, axes 9,
// lengths 3, rho 6, null vectors 48, distance system 60, valid 1 — in the batch's arrays, field-major (element e of sample s at
// frame[e * n_samples + s]: the back half's lanes read neighbouring words). Back: ONE LANE per sample. The back half is scalar work
// with ~380 live registers: run by a whole wave per sample it held the kernel at one wave per SIMD and 64 lanes repeated every
// operation (2.0 ms for 10 000 samples); by lanes, 10 000 samples are 157 waves. (The EPnP device code itself — epnp_front,
// epnp_back_variant, the frame's named offsets and its one pack — is in solve_dev.hpp; its one unpack is solve_pnp_back_body's.)
template <bool LIST>
__global__ __launch_bounds__(64 * SOLVE_WAVES) void solve_pnp_front_kernel(SolveSeg seg, const double* __restrict__ obj, const double* __restrict__ img,
                                                                          const double* __restrict__ K, int sample_size, int n_samples,
                                                                          const int* __restrict__ idx, double* __restrict__ frame) {
    __shared__ PnpLds lds[SOLVE_WAVES];
    extern __shared__ double rows_dyn[];   // SOLVE_WAVES x sample_size x 24: the two rows of every point of a wave's sample
    const int wave = threadIdx.x >> 6;
    const int s = blockIdx.x * SOLVE_WAVES + wave;
    if (s >= n_samples) return;
    bool solve = true;
    if constexpr (LIST) {
        long long base;
        solve = sample_segment(seg, s, sample_size, base);
        obj += 3 * base, img += 2 * base;
    }
    double* rows = rows_dyn + (size_t)wave * 24 * sample_size;
    const double K4[4] = {K[0], K[1], K[2], K[3]};
    PnpFrame F;
    PnpLds& S = lds[wave];
    int ok = 0;
    if (solve) ok = epnp_front<false>(sample_size, idx + (size_t)s * sample_size, obj, img, K4, F, S, rows, nullptr);
    pnp_frame_pack(frame + s, (size_t)n_samples, ok, F, S);
}

// A lane per (sample, linearised start): blockIdx.y is the start (0..2), ONE launch — as one lane per sample with the three starts in
// a row the kernel needed ~380 registers, spilled 122 of them (324 B of scratch per lane) and ran one wave per SIMD; as three launches
// (one instantiation each) the starts waited for one another on the stream: 36 + 32 + 32 us per RANSAC chunk of the incremental loop,
// where a chunk is four waves per start. The starts' errors and poses go to `tmp` ([start][sample][13]); pnp_first_smallest
// (solve_pnp_select_kernel here, pb_count_kernel of pnp_batch.hip) takes the first strictly smallest, as the CPU restatement's loop
// over the starts does.
template <bool LIST, int variant>
__device__ __forceinline__ void solve_pnp_back_body(const double* __restrict__ obj, const double* __restrict__ img,
                                                    const double* __restrict__ K, int sample_size, int n_samples,
                                                    const int* __restrict__ idx, const double* __restrict__ frame,
                                                    double* __restrict__ tmp, const SolveSeg& seg) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_samples) return;
    const size_t ns = (size_t)n_samples;
    const double K4[4] = {K[0], K[1], K[2], K[3]};
    double cand[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) cand[k] = 0.0;
    double err = -1.0;
    const double* src = frame + s;
    if (src[PNP_F_VALID * ns] != 0.0) {   // the frame's one unpack (its one pack: pnp_frame_pack, solve_dev.hpp)
        PnpFrame F;
#pragma unroll
        for (int e = 0; e < 3; ++e) F.c0[e] = src[(PNP_F_C0 + e) * ns], F.sc[e] = src[(PNP_F_SC + e) * ns];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int e = 0; e < 3; ++e) F.ax[k][e] = src[(PNP_F_AX + 3 * k + e) * ns];
#pragma unroll
        for (int q = 0; q < 6; ++q) F.rho[q] = src[(PNP_F_RHO + q) * ns];
        F.planar = F.sc[2] == 0.0;
        if constexpr (LIST) {
            const long long base = seg.point_ptr[seg.sample_problem[s]];
            obj += 3 * base, img += 2 * base;
        }
        err = epnp_back_variant<true, variant>(sample_size, idx + (size_t)s * sample_size, obj, img, K4, F, src + PNP_F_EV * ns, src + PNP_F_L * ns, ns, nullptr, cand);
    }
    double* dst = tmp + ((size_t)variant * ns + s) * 13;
    dst[0] = err;
#pragma unroll
    for (int k = 0; k < 12; ++k) dst[1 + k] = cand[k];
}
template <bool LIST>
__global__ __launch_bounds__(64) void solve_pnp_back_kernel(const double* __restrict__ obj, const double* __restrict__ img,
                                                            const double* __restrict__ K, int sample_size, int n_samples,
                                                            const int* __restrict__ idx, const double* __restrict__ frame,
                                                            double* __restrict__ tmp, SolveSeg seg) {
    if (blockIdx.y == 0) solve_pnp_back_body<LIST, 0>(obj, img, K, sample_size, n_samples, idx, frame, tmp, seg);        // (workgroup-uniform)
    else if (blockIdx.y == 1) solve_pnp_back_body<LIST, 1>(obj, img, K, sample_size, n_samples, idx, frame, tmp, seg);
    else solve_pnp_back_body<LIST, 2>(obj, img, K, sample_size, n_samples, idx, frame, tmp, seg);
}
__global__ __launch_bounds__(256) void solve_pnp_select_kernel(int n_samples, const double* __restrict__ tmp, double* __restrict__ models, int* __restrict__ n_models) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_samples) return;
    const size_t ns = (size_t)n_samples;
    const int which = pnp_first_smallest(tmp[(size_t)s * 13], tmp[(ns + s) * 13], tmp[(2 * ns + s) * 13]);
    for (int k = 0; k < 12; ++k) models[12 * (size_t)s + k] = which >= 0 ? tmp[((size_t)which * ns + s) * 13 + 1 + k] : 0.0;
    n_models[s] = which >= 0 ? 1 : 0;
}

// samples of more than 64 points (the all-inlier refit): one workgroup of three waves per sample runs pnp_refit_body (solve_dev.hpp),
// as pb_refit_kernel of pnp_batch.hip does on its row of inliers.
__global__ __launch_bounds__(192) void solve_pnp_big_kernel(const double* __restrict__ obj, const double* __restrict__ img,
                                                            const double* __restrict__ K, int sample_size, const int* __restrict__ idx,
                                                            double* __restrict__ models, int* __restrict__ n_models) {
    __shared__ PnpRefitLds W;
    const int s = blockIdx.x;
    const double K4[4] = {K[0], K[1], K[2], K[3]};
    const int which = pnp_refit_body(sample_size, idx + (size_t)s * sample_size, obj, img, K4, W);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 12; ++k) models[12 * (size_t)s + k] = which >= 0 ? W.result[which][1 + k] : 0.0;
        n_models[s] = which >= 0 ? 1 : 0;
    }
}

template <bool LIST>
__global__ __launch_bounds__(64 * SOLVE_WAVES) void solve_h4_kernel(SolveSeg seg, const double* __restrict__ a, const double* __restrict__ b, int n_samples,
                                                                   const int* __restrict__ idx, double* __restrict__ models, int* __restrict__ n_models) {
    __shared__ double LtL[SOLVE_WAVES][81], V[SOLVE_WAVES][81];
    __shared__ JacRound R[SOLVE_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int s = blockIdx.x * SOLVE_WAVES + wave;
    if (s >= n_samples) return;
    if constexpr (LIST) {
        long long base;
        if (!sample_segment(seg, s, 4, base)) {   // no candidates
            if (lane == 0) n_models[s] = 0;
            return;
        }
        a += 2 * base, b += 2 * base;
    }
    double pa[8], pb[8], out[9];
    gather_sample<4>(idx + (size_t)s * 4, a, b, pa, pb);
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = 0.0;
    const int n = homography4_wave(pa, pb, out, LtL[wave], V[wave], R[wave]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) models[9 * (size_t)s + k] = out[k];
        n_models[s] = n;
    }
}

template <bool LIST>
__global__ __launch_bounds__(64 * SOLVE_WAVES) void solve_e5_kernel(SolveSeg seg, const double* __restrict__ a, const double* __restrict__ b,
                                                                   const double* __restrict__ K, int has_K, int n_samples, const int* __restrict__ idx,
                                                                   double* __restrict__ models, int* __restrict__ n_models) {
    __shared__ E5Lds lds[SOLVE_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int s = blockIdx.x * SOLVE_WAVES + wave;
    if (s >= n_samples) return;
    if constexpr (LIST) {
        long long base;
        if (!sample_segment(seg, s, 5, base)) {   // no candidates
            if (lane == 0) n_models[s] = 0;
            return;
        }
        a += 2 * base, b += 2 * base;
    }
    double pa[10], pb[10];
    gather_sample<5>(idx + (size_t)s * 5, a, b, pa, pb);
    double fx = 1, fy = 1, cx = 0, cy = 0;
    if (has_K) fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    double* dst = models + (size_t)s * 90;
    for (int k = lane; k < 90; k += 64) dst[k] = 0.0;  // (this wave's own stores below follow in program order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    const int n = essential5_wave(pa, pb, has_K != 0, fx, fy, cx, cy, dst, lds[wave]);
    if (lane == 0) n_models[s] = n;
}

// The seven-point solver (fundamental7_wave, solve_dev.hpp): the shape of solve_h4_kernel, up to 3 models of 9 doubles per sample,
// the slots behind n_models zero. K is not an argument: a fundamental matrix lives in pixels.
template <bool LIST>
__global__ __launch_bounds__(64 * SOLVE_WAVES) void solve_f7_kernel(SolveSeg seg, const double* __restrict__ a, const double* __restrict__ b, int n_samples,
                                                                   const int* __restrict__ idx, double* __restrict__ models, int* __restrict__ n_models) {
    __shared__ double AtA[SOLVE_WAVES][81], V[SOLVE_WAVES][81];
    __shared__ JacRound R[SOLVE_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int s = blockIdx.x * SOLVE_WAVES + wave;
    if (s >= n_samples) return;
    if constexpr (LIST) {
        long long base;
        if (!sample_segment(seg, s, 7, base)) {   // no candidates
            if (lane == 0) n_models[s] = 0;
            return;
        }
        a += 2 * base, b += 2 * base;
    }
    double pa[14], pb[14], out[27];
    gather_sample<7>(idx + (size_t)s * 7, a, b, pa, pb);
    const int n = fundamental7_wave(pa, pb, out, AtA[wave], V[wave], R[wave]);
    if (lane < 27) {   // (identical values in every lane: entry `lane` by selection)
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 27; ++k)
            if (k == lane) v = out[k];
        models[27 * (size_t)s + lane] = v;
    }
    if (lane == 0) n_models[s] = n;
}

}  // namespace

void solve_minimal_launch(hipStream_t st, const MinimalLaunch& L) {
    const unsigned grid = (unsigned)((L.n_samples + SOLVE_WAVES - 1) / SOLVE_WAVES);
    const bool list = L.seg.point_ptr != nullptr;
    if (L.kind == EACHAM_SOLVE_HOMOGRAPHY4)
        (list ? solve_h4_kernel<true> : solve_h4_kernel<false>)<<<grid, 64 * SOLVE_WAVES, 0, st>>>(L.seg, L.a, L.b, L.n_samples, L.sample_idx, L.models, L.n_models);
    else if (L.kind == EACHAM_SOLVE_FUNDAMENTAL7)
        (list ? solve_f7_kernel<true> : solve_f7_kernel<false>)<<<grid, 64 * SOLVE_WAVES, 0, st>>>(L.seg, L.a, L.b, L.n_samples, L.sample_idx, L.models, L.n_models);
    else
        (list ? solve_e5_kernel<true> : solve_e5_kernel<false>)<<<grid, 64 * SOLVE_WAVES, 0, st>>>(L.seg, L.a, L.b, L.K, L.has_K ? 1 : 0, L.n_samples, L.sample_idx,
                                                                                                 L.models, L.n_models);
}

void solve_pnp_launch(hipStream_t st, const PnpLaunch& L) {
    const bool list = L.seg.point_ptr != nullptr;
    const unsigned gw = (unsigned)((L.n_samples + SOLVE_WAVES - 1) / SOLVE_WAVES), gb = (unsigned)((L.n_samples + 63) / 64);
    (list ? solve_pnp_front_kernel<true> : solve_pnp_front_kernel<false>)<<<gw, 64 * SOLVE_WAVES, sizeof(double) * SOLVE_WAVES * 24 * (size_t)L.sample_size, st>>>(
        L.seg, L.obj, L.img, L.K, L.sample_size, L.n_samples, L.sample_idx, L.frame);
    (list ? solve_pnp_back_kernel<true> : solve_pnp_back_kernel<false>)<<<dim3(gb, 3), 64, 0, st>>>(L.obj, L.img, L.K, L.sample_size, L.n_samples, L.sample_idx, L.frame,
                                                                                                  L.tmp, L.seg);
}

}  // namespace eacham

using namespace eacham;

extern "C" int eacham_solve_minimal(eacham_ctx* ctx, int kind, int n_points, const double* a, const double* b, const double* K,
                                    int n_samples, const int32_t* sample_idx, double* models, int32_t* n_models) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (kind != EACHAM_SOLVE_HOMOGRAPHY4 && kind != EACHAM_SOLVE_ESSENTIAL5 && kind != EACHAM_SOLVE_FUNDAMENTAL7)
        return ctx->fail(EACHAM_ERR_INVALID, "solve_minimal: unknown kind %d", kind);
    if (n_points < 0 || n_samples < 0 || (n_samples > 0 && (!a || !b || !sample_idx || !models || !n_models)))
        return ctx->fail(EACHAM_ERR_INVALID, "solve_minimal: null argument or negative size");
    if (n_samples == 0) return EACHAM_OK;
    const int m = solve_sample_size(kind), maxm = solve_max_models(kind);
    if (int rc = check_sample_idx(ctx, "solve_minimal", -1, sample_idx, (long long)n_samples * m, n_points)) return rc;
    EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    IoStage io(ctx, st);
    const auto h_a = io.in<double>(a, 2 * (size_t)n_points), h_b = io.in<double>(b, 2 * (size_t)n_points);
    const auto h_K = io.in<double>(K, 4);
    const auto h_i = io.in<int>(sample_idx, (size_t)n_samples * m);
    const auto h_m = io.out<double>(models, 9 * (size_t)maxm * n_samples);
    const auto h_n = io.out<int>(n_models, (size_t)n_samples);
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    {
        ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
        solve_minimal_launch(st, MinimalLaunch{kind, SolveSeg{}, d(h_a), d(h_b), d(h_K), K != nullptr, n_samples, d(h_i), d(h_m), d(h_n)});
    }
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return io.finish();
}

extern "C" int eacham_solve_pnp(eacham_ctx* ctx, int n_points, const double* object_points, const double* image_points, const double* K,
                                int sample_size, int n_samples, const int32_t* sample_idx, double* models, int32_t* n_models) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_points < 0 || n_samples < 0 || (n_samples > 0 && (!object_points || !image_points || !K || !sample_idx || !models || !n_models)))
        return ctx->fail(EACHAM_ERR_INVALID, "solve_pnp: null argument or negative size");
    if (n_samples == 0) return EACHAM_OK;
    if (sample_size < 5) return ctx->fail(EACHAM_ERR_INVALID, "solve_pnp: EPnP needs at least 5 points per sample, got %d", sample_size);
    const long long total = (long long)n_samples * sample_size;
    if (int rc = check_sample_idx(ctx, "solve_pnp", -1, sample_idx, total, n_points)) return rc;
    EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    IoStage io(ctx, st);
    const auto h_a = io.in<double>(object_points, 3 * (size_t)n_points), h_b = io.in<double>(image_points, 2 * (size_t)n_points);
    const auto h_K = io.in<double>(K, 4);
    const auto h_i = io.in<int>(sample_idx, (size_t)total);
    const auto h_m = io.out<double>(models, 12 * (size_t)n_samples);
    const auto h_n = io.out<int>(n_models, (size_t)n_samples);
    const auto h_f = io.scratch<double>(sample_size <= 64 ? PNP_FRAME * (size_t)n_samples : 0);   // the samples' frames between the two launches
    const auto h_t = io.scratch<double>(sample_size <= 64 ? 3 * 13 * (size_t)n_samples : 0);      // error + pose of the three starts
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    {
        ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
        // Bit-identical with the CPU restatement either way: samples of at most 64 points — the RANSAC loop's — a wave per sample for the
        // shared front half, a lane per sample for the scalar back half; larger ones — the all-inlier refit — one wave for both.
        if (sample_size <= 64) {
            solve_pnp_launch(st, PnpLaunch{SolveSeg{}, d(h_a), d(h_b), d(h_K), sample_size, n_samples, d(h_i), d(h_f), d(h_t)});
            solve_pnp_select_kernel<<<(unsigned)((n_samples + 255) / 256), 256, 0, st>>>(n_samples, d(h_t), d(h_m), d(h_n));
        }
        else
            solve_pnp_big_kernel<<<(unsigned)n_samples, 192, 0, st>>>(d(h_a), d(h_b), d(h_K), sample_size, d(h_i), d(h_m), d(h_n));
    }
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return io.finish();
}
