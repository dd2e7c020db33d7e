// PnPHip.hpp — cv::solvePnPRansac as the reference calls it, on the device library.
//
//   cv::solvePnPRansac(pts3d1, pts2d2, K, distCoeffs /* zeros */, rvec, t, false, 10000, 4.0f, 0.999f, inliersPnP,
//                      cv::SOLVEPNP_EPNP);              /root/reference/modules/sfm/reconstruction/ReconstructionManager.cpp:227-228
//   cv::Rodrigues(rvec, R); factor.transform = ConvertToTransform(R, t);                                          :236-238
//
// OpenCV's loop is sequential: draw 5 points, EPnP, count the points within 4 px, shrink the iteration budget from the
// best inlier ratio and the confidence (RANSACUpdateNumIters), stop when the budget is used up, and run EPnP once more on
// the inliers of the winner. Here the samples are processed in CHUNKS of 256 — eacham_solve_pnp on the chunk's five-point
// rows, one eacham_score_hypotheses(kind PNP) call for its models against every point — and the sequential rule is replayed
// over the chunk's inlier counts in sample order, so the loop ends at exactly the sample OpenCV's would (`iterations`) and
// the winner is the best model among the samples before it; with 70 % inliers that is one chunk instead of the 10 000
// samples asked for. The last launch is EPnP on the one row of the winner's inliers. The samples are OpenCV's own stream by
// default (Sampling::OpenCV, CvSampling.hpp: cv::RNG seeded (uint64)-1, getSubset; from memory of the 4.5.5 sources, unverified:
// parity unpinned) or the counter-based generator seeded by the caller (Sampling::Counter); tests hold the result against the
// ground truth under both.
//
// The loop is written ONCE for one problem and once for a list (pnp_detail::ransac_single / ransac_batch, over replay_chunk), for any
// sample size m, the solver step handed in as a callable: SolvePnPRansac[Batch] are the EPnP instantiations (m = 5), PnPP3PHip.hpp
// holds the P3P ones (m = 4). This header names no P3P entry point: a program that includes only it links without them.
#pragma once

#include <algorithm>
#include <cmath>

#include "TwoViewHip.hpp"

namespace eacham {
namespace hip {

struct PnPResult {
    bool ok = false;              // false: fewer than 5 points, or no sample gave a model with >= 5 inliers (cv returns false)
    Mat3 R{};                     // cv::Rodrigues(rvec)
    Vec3 rvec{};                  // axis * angle, what solvePnPRansac hands back
    Vec3 t{};
    std::vector<int> inliers;     // indices within 4 px of the RANSAC winner (OpenCV's `inliers` output)
    int iterations = 0;           // samples the sequential rule consumed before RANSACUpdateNumIters stopped it
};

// What one SolvePnPRansac run decided on the way, for whoever wants to replay it (tests): every sample it drew (whole chunks:
// more than the `iterations` the sequential rule consumed) and the sample whose model won (-1: none).
struct PnPTrace {
    std::vector<int32_t> samples;
    int winner = -1;
};

// One (map points, pixels) problem of SolvePnPRansacBatch: object n x 3, image n x 2 (pixels).
struct PnPProblem {
    std::vector<double> object, image;
};

inline Vec3 RodriguesFromMatrix(const Mat3& R) {   // rotation matrix -> axis * angle
    const double c = std::min(1.0, std::max(-1.0, (R[0] + R[4] + R[8] - 1.0) * 0.5));
    const double theta = std::acos(c);
    Vec3 ax{R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double s = twoview_detail::norm(ax) * 0.5;   // sin(theta)
    if (s > 1e-9) {
        for (double& x : ax) x *= theta / (2.0 * s);
        return ax;
    }
    if (c > 0.0) return {0.0, 0.0, 0.0};
    // theta = pi: axis from the diagonal of (R + I) / 2
    Vec3 v{std::sqrt(std::max(0.0, (R[0] + 1.0) * 0.5)), std::sqrt(std::max(0.0, (R[4] + 1.0) * 0.5)), std::sqrt(std::max(0.0, (R[8] + 1.0) * 0.5))};
    if (R[1] + R[3] < 0.0) v[1] = -v[1];
    if (R[2] + R[6] < 0.0) v[2] = -v[2];
    if (v[0] == 0.0 && R[5] + R[7] < 0.0) v[2] = -v[2];
    const double n = twoview_detail::norm(v);
    for (double& x : v) x *= theta / (n > 0.0 ? n : 1.0);
    return v;
}

namespace pnp_detail {

const int kChunk = 256;   // samples solved and scored per launch

// Samples first .. first + count - 1 of one RANSACPointSetRegistrator::run, count rows of m indices out of n. Sampling::OpenCV
// continues `rng` (one stream for the whole call: ask for the samples in order); Sampling::Counter is indexed by the global
// sample number; `given`, when set, is the whole run's list and is read in place of either (rows past its end repeat its last).
inline std::vector<int32_t> pnp_samples(int n, int m, int first, int count, CvRNG& rng, uint64_t seed, Sampling sampling,
                                        const std::vector<int32_t>* given = nullptr) {
    std::vector<int32_t> idx;
    if (given) {
        const int rows = (int)(given->size() / m);
        idx.resize((size_t)count * m);
        for (int k = 0; k < count; ++k) std::copy_n(&(*given)[(size_t)std::min(first + k, rows - 1) * m], m, &idx[(size_t)k * m]);
    } else if (sampling == Sampling::OpenCV) {
        idx.resize((size_t)count * m);
        for (int k = 0; k < count; ++k) (void)cv_get_subset(rng, n, m, &idx[(size_t)k * m], 10000, [](const int32_t*) { return true; });
    } else {
        idx = twoview_detail::draw_samples(n, m, count, seed, first);
    }
    return idx;
}

// The sequential rule over one chunk's results (sample first + k is row k), in sample order and while the budget lasts: a model
// with strictly more inliers than the best so far (and at least a sample's worth) replaces it and shrinks the budget.
inline void replay_chunk(int n, int m, double confidence, int first, int cnt, const int32_t* ok, const int32_t* inl, const double* models,
                         int& budget, int& best_inl, double* best_model, int& iterations, PnPTrace* trace) {
    for (int k = 0; k < cnt && first + k < budget; ++k) {
        iterations = first + k + 1;
        if (!ok[k]) continue;
        if (inl[k] > std::max(best_inl, m - 1)) {
            best_inl = inl[k];
            if (trace) trace->winner = first + k;
            std::copy_n(&models[(size_t)k * 12], 12, best_model);
            budget = twoview_detail::ransac_update_num_iters(confidence, (double)(n - inl[k]) / n, m, budget);
        }
    }
}

inline void set_pose(PnPResult& r, const double* pose) {   // R | t of the refit, or of the winner where there is none
    for (int e = 0; e < 9; ++e) r.R[e] = pose[e];
    for (int e = 0; e < 3; ++e) r.t[e] = pose[9 + e];
    r.rvec = RodriguesFromMatrix(r.R);
    r.ok = true;
}

// One problem, samples of m points. solve(ctx, n, object, image, K4, count, idx, models, ok) is the chunk's solver call: `count`
// rows of m indices -> models [count][12] and ok [count]; it returns the library's error code.
template <class Solve>
inline PnPResult ransac_single(Context& ctx, int m, Solve&& solve, const std::vector<double>& object, const std::vector<double>& image,
                               const double* K9, int iterations, float reprojectionError, double confidence, uint64_t seed, Sampling sampling,
                               PnPTrace* trace, const std::vector<int32_t>* samples) {
    PnPResult out;
    const int n = (int)(image.size() / 2);
    if (n < m || object.size() != (size_t)3 * n || iterations <= 0 || (samples && samples->size() < (size_t)m)) return out;
    const double K4[4] = {K9[0], K9[4], K9[2], K9[5]};
    const float thr = reprojectionError * reprojectionError;   // PnPRansacCallback::computeError returns squared pixels
    const int chunk = kChunk;
    std::vector<double> models((size_t)chunk * 12), best_model(12, 0.0);
    std::vector<int32_t> okv(chunk), inl(chunk);
    int best_inl = -1, budget = iterations;
    CvRNG rng(0xffffffffffffffffull);   // RANSACPointSetRegistrator::run: RNG rng((uint64)-1), one stream for the whole call
    for (int first = 0; first < budget; first += chunk) {
        const int cnt = std::min(chunk, iterations - first);
        // sample s of the whole run is row (s - first) of this chunk: OpenCV's stream is drawn in sample order (a chunk draws ahead
        // of the budget, which only shrinks: the samples the sequential rule consumes are the stream's prefix); the counter-based
        // generator is indexed by the global sample number
        const std::vector<int32_t> idx = pnp_samples(n, m, first, cnt, rng, seed, sampling, samples);
        if (trace) trace->samples.insert(trace->samples.end(), idx.begin(), idx.end());
        ctx.check(solve(ctx.get(), n, object.data(), image.data(), K4, cnt, idx.data(), models.data(), okv.data()));
        ctx.check(eacham_score_hypotheses(ctx.get(), EACHAM_SCORE_PNP, n, object.data(), image.data(), cnt, models.data(), K4, thr, nullptr,
                                          inl.data(), nullptr));
        replay_chunk(n, m, confidence, first, cnt, okv.data(), inl.data(), models.data(), budget, best_inl, best_model.data(), out.iterations, trace);
    }
    if (best_inl < m) return out;
    std::vector<float> err(n);
    int32_t cnt = 0;
    ctx.check(eacham_score_hypotheses(ctx.get(), EACHAM_SCORE_PNP, n, object.data(), image.data(), 1, best_model.data(), K4, thr,
                                      err.data(), &cnt, nullptr));
    std::vector<int32_t> rows;
    for (int i = 0; i < n; ++i)
        if (err[i] <= thr) rows.push_back(i);
    out.inliers.assign(rows.begin(), rows.end());
    double refit[12];
    int32_t rok = 0;
    if (rows.size() >= 5)   // the refit is EPnP, which needs five rows: a four-inlier winner (m = 4) keeps its own pose
        ctx.check(eacham_solve_pnp(ctx.get(), n, object.data(), image.data(), K4, (int)rows.size(), 1, rows.data(), refit, &rok));
    set_pose(out, rok ? refit : best_model.data());   // (a collinear inlier set cannot be refitted: keep the winner)
    return out;
}

// A LIST of problems in rounds + 1 device calls, whatever the length of the list. In round r every problem still running draws
// its rows [256 r, min(256 (r + 1), iterations)) from its OWN stream (Sampling::OpenCV: a CvRNG seeded (uint64)-1 per problem,
// kept across the rounds; Sampling::Counter: seeds[p]) and ONE call of round(ctx, P, point_ptr, object, image, K4, sample_ptr, idx,
// thr, models, ok, counts) — an eacham_pnp_hypotheses_batch* entry with its sample size m bound — solves and counts them all; the
// sequential rule is then replayed per problem on the host over that problem's counts (ransac_update_num_iters uses the host's log
// and pow: a device libm may round differently at a knife edge). A problem leaves the list when its budget is within the samples
// already seen. After the last round ONE eacham_pnp_refit_batch call (EPnP) serves every problem whose best count is >= m; where it
// gives no pose — fewer than 5 inliers, a degenerate set — the winner's stays.
template <class Round>
inline std::vector<PnPResult> ransac_batch(Context& ctx, int m, Round&& round, const std::vector<PnPProblem>& problems, const double* K9,
                                           int iterations, float reprojectionError, double confidence, const std::vector<uint64_t>& seeds,
                                           Sampling sampling, std::vector<PnPTrace>* traces) {
    const size_t P = problems.size();
    const int chunk = kChunk;
    std::vector<PnPResult> out(P);
    if (traces) traces->assign(P, PnPTrace{});
    const double K4[4] = {K9[0], K9[4], K9[2], K9[5]};
    const float thr = reprojectionError * reprojectionError;
    std::vector<int64_t> point_ptr(P + 1, 0), sample_ptr(P + 1, 0);
    std::vector<double> object, image;
    std::vector<int> npts(P), budget(P), best_inl(P, -1);
    std::vector<CvRNG> rng(P, CvRNG(0xffffffffffffffffull));
    for (size_t p = 0; p < P; ++p) {
        npts[p] = (int)(problems[p].image.size() / 2);
        // (what ransac_single turns away takes part with its points and never with a sample)
        budget[p] = npts[p] >= m && problems[p].object.size() == (size_t)3 * npts[p] && iterations > 0 ? iterations : 0;
        point_ptr[p + 1] = point_ptr[p] + npts[p];
        object.insert(object.end(), problems[p].object.begin(), problems[p].object.end());
        object.resize((size_t)3 * point_ptr[p + 1], 0.0);
        image.insert(image.end(), problems[p].image.begin(), problems[p].image.begin() + 2 * (size_t)npts[p]);
    }
    std::vector<double> best_model(12 * P, 0.0), models;
    std::vector<int32_t> idx, okv, inl;
    for (int first = 0;; first += chunk) {
        idx.clear();
        for (size_t p = 0; p < P; ++p) {
            const int cnt = first < budget[p] ? std::min(chunk, iterations - first) : 0;
            if (cnt > 0) {
                const std::vector<int32_t> rows = pnp_samples(npts[p], m, first, cnt, rng[p], p < seeds.size() ? seeds[p] : 1, sampling);
                if (traces) (*traces)[p].samples.insert((*traces)[p].samples.end(), rows.begin(), rows.end());
                idx.insert(idx.end(), rows.begin(), rows.end());
            }
            sample_ptr[p + 1] = sample_ptr[p] + cnt;
        }
        const size_t S = (size_t)sample_ptr[P];
        if (S == 0) break;
        models.resize(12 * S), okv.resize(S), inl.resize(S);
        ctx.check(round(ctx.get(), (int)P, point_ptr.data(), object.data(), image.data(), K4, sample_ptr.data(), idx.data(), thr, models.data(),
                        okv.data(), inl.data()));
        for (size_t p = 0; p < P; ++p) {
            const size_t s0 = (size_t)sample_ptr[p];
            replay_chunk(npts[p], m, confidence, first, (int)(sample_ptr[p + 1] - sample_ptr[p]), okv.data() + s0, inl.data() + s0,
                         models.data() + 12 * s0, budget[p], best_inl[p], &best_model[12 * p], out[p].iterations, traces ? &(*traces)[p] : nullptr);
        }
    }
    std::vector<uint8_t> has(P, 0), mask((size_t)point_ptr[P], 0);
    bool any = false;
    for (size_t p = 0; p < P; ++p) any |= (has[p] = best_inl[p] >= m) != 0;
    if (!any) return out;
    std::vector<int32_t> n_inl(P), rok(P);
    std::vector<double> refit(12 * P);
    ctx.check(eacham_pnp_refit_batch(ctx.get(), (int)P, point_ptr.data(), object.data(), image.data(), K4, best_model.data(), has.data(), thr,
                                     mask.data(), n_inl.data(), refit.data(), rok.data()));
    for (size_t p = 0; p < P; ++p) {
        if (!has[p]) continue;
        for (int i = 0; i < npts[p]; ++i)
            if (mask[(size_t)point_ptr[p] + i]) out[p].inliers.push_back(i);
        set_pose(out[p], rok[p] ? &refit[12 * p] : &best_model[12 * p]);
    }
    return out;
}

}  // namespace pnp_detail

// object: n x 3, image: n x 2 (pixels), K9: row-major 3 x 3 (no distortion — the reference passes zeros).
inline PnPResult SolvePnPRansac(Context& ctx, const std::vector<double>& object, const std::vector<double>& image, const double* K9,
                                int iterations = 10000, float reprojectionError = 4.0f, double confidence = 0.999, uint64_t seed = 1,
                                Sampling sampling = Sampling::OpenCV, PnPTrace* trace = nullptr, const std::vector<int32_t>* samples = nullptr) {
    const auto solve = [](eacham_ctx* c, int n, const double* obj, const double* img, const double* K4, auto... rows) {
        return eacham_solve_pnp(c, n, obj, img, K4, 5, rows...);   // (the sample size goes in front of the rows)
    };
    return pnp_detail::ransac_single(ctx, 5, solve, object, image, K9, iterations, reprojectionError, confidence, seed, sampling, trace, samples);
}

// SolvePnPRansac for a LIST of problems (pnp_detail::ransac_batch, the round one eacham_pnp_hypotheses_batch call). result[p] — and
// traces[p], when asked for — equal what SolvePnPRansac returns for problem p alone with seeds[p] and the same arguments, field for field.
inline std::vector<PnPResult> SolvePnPRansacBatch(Context& ctx, const std::vector<PnPProblem>& problems, const double* K9, int iterations = 10000,
                                                  float reprojectionError = 4.0f, double confidence = 0.999,
                                                  const std::vector<uint64_t>& seeds = {}, Sampling sampling = Sampling::OpenCV,
                                                  std::vector<PnPTrace>* traces = nullptr) {
    const auto round = [](eacham_ctx* c, int P, const int64_t* pp, const double* obj, const double* img, const double* K4, const int64_t* sp, auto... rest) {
        return eacham_pnp_hypotheses_batch(c, P, pp, obj, img, K4, sp, 5, rest...);   // (the sample size goes in front of the rows)
    };
    return pnp_detail::ransac_batch(ctx, 5, round, problems, K9, iterations, reprojectionError, confidence, seeds, sampling, traces);
}

// ---- the polish: cv::solvePnPRefineLM on the inliers (eacham_pnp_refine_batch, include/eacham_hip.h states the loop) --------------
// SolvePnPRansac[Batch] end on EPnP's algebraic fit, as cv::solvePnPRansac(..., SOLVEPNP_EPNP) does; the calls below add what
// SOLVEPNP_ITERATIVE and COLMAP add after it: Levenberg-Marquardt on the reprojection error over the winner's inliers, for the whole
// list in ONE device call. The functions above, their defaults and their results are unchanged.

// A PnPResult whose pose has been polished. `inliers` keeps its meaning (the rows within the threshold of the RANSAC winner: the
// rows the polish ran on); a result that is not ok, or whose status is NOT_REFINED (fewer than 3 inliers, a point behind the
// camera), keeps the pose it came with.
struct PnPRefined : PnPResult {
    double cost_before = 0.0, cost_after = 0.0;   // sum of squared pixel residuals over the inliers
    int tries = 0;
    int status = EACHAM_PNP_REFINE_NOT_REFINED;   // EACHAM_PNP_REFINE_CONVERGED / _CAP / _NOT_REFINED
};

namespace pnp_detail {

// One eacham_pnp_refine_batch call for the list: problem p is refined from poses[p] (R, t; skipped unless ok) over poses[p].inliers.
inline std::vector<PnPRefined> refine_batch(Context& ctx, const std::vector<PnPProblem>& problems, const double* K9,
                                            const std::vector<PnPResult>& poses, int maxTries) {
    const size_t P = problems.size();
    std::vector<PnPRefined> out(P);
    if (P == 0 || poses.size() != P) return out;
    const double K4[4] = {K9[0], K9[4], K9[2], K9[5]};
    std::vector<int64_t> point_ptr(P + 1, 0);
    std::vector<double> object, image, in(12 * P, 0.0);
    std::vector<uint8_t> has(P, 0);
    for (size_t p = 0; p < P; ++p) {
        static_cast<PnPResult&>(out[p]) = poses[p];
        const int n = (int)(problems[p].image.size() / 2);
        point_ptr[p + 1] = point_ptr[p] + n;
        object.insert(object.end(), problems[p].object.begin(), problems[p].object.end());
        object.resize((size_t)3 * point_ptr[p + 1], 0.0);
        image.insert(image.end(), problems[p].image.begin(), problems[p].image.begin() + 2 * (size_t)n);
        has[p] = poses[p].ok && problems[p].object.size() == (size_t)3 * n;
        for (int e = 0; e < 9; ++e) in[12 * p + e] = poses[p].R[e];
        for (int e = 0; e < 3; ++e) in[12 * p + 9 + e] = poses[p].t[e];
    }
    std::vector<uint8_t> use((size_t)point_ptr[P], 0);
    for (size_t p = 0; p < P; ++p)
        for (const int i : poses[p].inliers)
            if (i >= 0 && i < point_ptr[p + 1] - point_ptr[p]) use[(size_t)point_ptr[p] + i] = 1;
    std::vector<double> refined(12 * P), cost(2 * P);
    std::vector<int32_t> tries(P), status(P);
    ctx.check(eacham_pnp_refine_batch(ctx.get(), (int)P, point_ptr.data(), object.data(), image.data(), K4, in.data(), has.data(), use.data(), maxTries,
                                      0.f, refined.data(), cost.data(), tries.data(), status.data(), nullptr, nullptr));
    for (size_t p = 0; p < P; ++p) {
        out[p].cost_before = cost[2 * p], out[p].cost_after = cost[2 * p + 1], out[p].tries = tries[p], out[p].status = status[p];
        if (has[p] && status[p] != EACHAM_PNP_REFINE_NOT_REFINED) set_pose(out[p], &refined[12 * p]);
    }
    return out;
}

}  // namespace pnp_detail

// The polish for a LIST: poses[p] is what a SolvePnPRansac* call returned for problems[p] (or any pose R, t with ok set and the rows
// to use in `inliers`). result[p] equals what RefinePnP returns for problem p alone, field for field.
inline std::vector<PnPRefined> RefinePnPBatch(Context& ctx, const std::vector<PnPProblem>& problems, const double* K9,
                                              const std::vector<PnPResult>& poses, int maxTries = 20) {
    return pnp_detail::refine_batch(ctx, problems, K9, poses, maxTries);
}

// The polish for one problem: Levenberg-Marquardt from `pose` (R, t) over the rows pose.inliers of object / image.
inline PnPRefined RefinePnP(Context& ctx, const std::vector<double>& object, const std::vector<double>& image, const double* K9,
                            const PnPResult& pose, int maxTries = 20) {
    return pnp_detail::refine_batch(ctx, {PnPProblem{object, image}}, K9, {pose}, maxTries)[0];
}

// SolvePnPRansac, then the polish on its inliers (arguments and defaults of SolvePnPRansac; maxTries = the cap of the LM loop).
inline PnPRefined SolvePnPRansacRefined(Context& ctx, const std::vector<double>& object, const std::vector<double>& image, const double* K9,
                                        int iterations = 10000, float reprojectionError = 4.0f, double confidence = 0.999, uint64_t seed = 1,
                                        Sampling sampling = Sampling::OpenCV, int maxTries = 20) {
    return RefinePnP(ctx, object, image, K9, SolvePnPRansac(ctx, object, image, K9, iterations, reprojectionError, confidence, seed, sampling), maxTries);
}

// SolvePnPRansacBatch, then ONE more device call for every polish. result[p] equals SolvePnPRansacRefined on problem p with seeds[p].
inline std::vector<PnPRefined> SolvePnPRansacRefinedBatch(Context& ctx, const std::vector<PnPProblem>& problems, const double* K9,
                                                          int iterations = 10000, float reprojectionError = 4.0f, double confidence = 0.999,
                                                          const std::vector<uint64_t>& seeds = {}, Sampling sampling = Sampling::OpenCV,
                                                          int maxTries = 20) {
    return RefinePnPBatch(ctx, problems, K9, SolvePnPRansacBatch(ctx, problems, K9, iterations, reprojectionError, confidence, seeds, sampling), maxTries);
}

}  // namespace hip
}  // namespace eacham
