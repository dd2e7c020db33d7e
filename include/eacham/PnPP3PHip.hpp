// PnPP3PHip.hpp — cv::solvePnPRansac with cv::SOLVEPNP_P3P on the device library: the PnP RANSAC on its minimal sample.
//
// SolvePnPRansac (PnPHip.hpp) draws five-point EPnP samples, as the reference asks for; here a sample is FOUR correspondences —
// three give up to four poses, the fourth picks one (eacham_solve_p3p, include/eacham_hip.h states the solver and how it differs from
// OpenCV's p3p.cpp: the same solution set, not the same bits) — so the budget for a given confidence is smaller, a frame with
// exactly four correspondences gets a pose at all, and a round of the list form is ONE launch (eacham_pnp_hypotheses_batch_p3p) where
// EPnP's is three. The loops are pnp_detail::ransac_single / ransac_batch of PnPHip.hpp with m = 4 and the two P3P entry points as the
// solver step: the same arguments, defaults and results. The REFIT is EPnP on the winner's inliers (from memory of OpenCV 4.5.5,
// which refits the P3P winner with EPnP; parity unpinned); with fewer than 5 inliers, or an inlier set EPnP calls degenerate, the
// winner's pose is returned. ok needs a winner with >= 4 inliers. A header of its own: only what includes it needs the P3P entries.
#pragma once

#include "PnPHip.hpp"

namespace eacham {
namespace hip {

// object: n x 3, image: n x 2 (pixels), K9: row-major 3 x 3 (no distortion).
inline PnPResult SolvePnPRansacP3P(Context& ctx, const std::vector<double>& object, const std::vector<double>& image, const double* K9,
                                   int iterations = 10000, float reprojectionError = 4.0f, double confidence = 0.999, uint64_t seed = 1,
                                   Sampling sampling = Sampling::OpenCV, PnPTrace* trace = nullptr, const std::vector<int32_t>* samples = nullptr) {
    const auto solve = [](auto... a) { return eacham_solve_p3p(a..., nullptr, nullptr); };   // (the candidates are not wanted)
    return pnp_detail::ransac_single(ctx, 4, solve, object, image, K9, iterations, reprojectionError, confidence, seed, sampling, trace, samples);
}

// SolvePnPRansacP3P for a LIST of problems in rounds + 1 device calls: the round is ONE eacham_pnp_hypotheses_batch_p3p launch. result[p]
// — and traces[p], when asked for — equal what SolvePnPRansacP3P returns for problem p alone with seeds[p] and the same arguments.
inline std::vector<PnPResult> SolvePnPRansacP3PBatch(Context& ctx, const std::vector<PnPProblem>& problems, const double* K9, int iterations = 10000,
                                                     float reprojectionError = 4.0f, double confidence = 0.999,
                                                     const std::vector<uint64_t>& seeds = {}, Sampling sampling = Sampling::OpenCV,
                                                     std::vector<PnPTrace>* traces = nullptr) {
    return pnp_detail::ransac_batch(ctx, 4, eacham_pnp_hypotheses_batch_p3p, problems, K9, iterations, reprojectionError, confidence, seeds,
                                    sampling, traces);
}

// SolvePnPRansacP3P, then the polish of PnPHip.hpp (RefinePnP: Levenberg-Marquardt on the reprojection error) on its inliers. EPnP's
// refit needs five rows, the polish three: under this call a frame registered from exactly FOUR correspondences, or a winner with four
// inliers, comes back polished where SolvePnPRansacP3P returns the raw minimal pose.
inline PnPRefined SolvePnPRansacP3PRefined(Context& ctx, const std::vector<double>& object, const std::vector<double>& image, const double* K9,
                                           int iterations = 10000, float reprojectionError = 4.0f, double confidence = 0.999, uint64_t seed = 1,
                                           Sampling sampling = Sampling::OpenCV, int maxTries = 20) {
    return RefinePnP(ctx, object, image, K9, SolvePnPRansacP3P(ctx, object, image, K9, iterations, reprojectionError, confidence, seed, sampling), maxTries);
}

// SolvePnPRansacP3PBatch, then ONE more device call for every polish. result[p] equals SolvePnPRansacP3PRefined on problem p with seeds[p].
inline std::vector<PnPRefined> SolvePnPRansacP3PRefinedBatch(Context& ctx, const std::vector<PnPProblem>& problems, const double* K9,
                                                             int iterations = 10000, float reprojectionError = 4.0f, double confidence = 0.999,
                                                             const std::vector<uint64_t>& seeds = {}, Sampling sampling = Sampling::OpenCV,
                                                             int maxTries = 20) {
    return RefinePnPBatch(ctx, problems, K9, SolvePnPRansacP3PBatch(ctx, problems, K9, iterations, reprojectionError, confidence, seeds, sampling),
                          maxTries);
}

}  // namespace hip
}  // namespace eacham
