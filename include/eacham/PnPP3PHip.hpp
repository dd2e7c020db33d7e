// PnPP3PHip.hpp — cv::solvePnPRansac with cv::SOLVEPNP_P3P on the device library: the PnP RANSAC on its minimal sample.
//
// SolvePnPRansac (PnPHip.hpp) draws five-point EPnP samples, as the reference asks for; here a sample is FOUR correspondences —
// three give up to four poses, the fourth picks one (eacham_solve_p3p, include/eacham_hip.h states the solver and how it differs from
// OpenCV's p3p.cpp: the same solution set, not the same bits) — so the budget for a given confidence is smaller, a frame with
// exactly four correspondences gets a pose at all, and a round of the list form is ONE launch (eacham_pnp_hypotheses_batch_p3p) where
// EPnP's is three. Everything else is SolvePnPRansac[Batch] with m = 4: the same arguments and defaults, the same PnPResult /
// PnPTrace, chunks of 256 samples, the sequential rule replayed over the chunk's counts (a count > max(best, 3) replaces the model,
// ransac_update_num_iters(..., 4, ...)), the samples from pnp_detail::pnp_samples(n, 4, ...) under both samplings. The REFIT is
// EPnP on the winner's inliers through the existing calls (from memory of OpenCV 4.5.5, which refits the P3P winner with EPnP;
// parity unpinned); with fewer than 5 inliers, or an inlier set EPnP calls degenerate, the winner's pose is returned — the rule the
// EPnP form already has for a failed refit. ok needs a winner with >= 4 inliers.
//
// A header of its own: nothing that includes PnPHip.hpp needs the two new entry points.
#pragma once

#include "PnPHip.hpp"

namespace eacham {
namespace hip {

// object: n x 3, image: n x 2 (pixels), K9: row-major 3 x 3 (no distortion).
inline PnPResult SolvePnPRansacP3P(Context& ctx, const std::vector<double>& object, const std::vector<double>& image, const double* K9,
                                   int iterations = 10000, float reprojectionError = 4.0f, double confidence = 0.999, uint64_t seed = 1,
                                   Sampling sampling = Sampling::OpenCV, PnPTrace* trace = nullptr, const std::vector<int32_t>* samples = nullptr) {
    PnPResult out;
    const int n = (int)(image.size() / 2), m = 4;
    if (n < m || object.size() != (size_t)3 * n || iterations <= 0 || (samples && samples->size() < (size_t)m)) return out;
    const double K4[4] = {K9[0], K9[4], K9[2], K9[5]};
    const float thr = reprojectionError * reprojectionError;
    const int chunk = pnp_detail::kChunk;
    std::vector<double> models((size_t)chunk * 12), best_model(12, 0.0);
    std::vector<int32_t> okv(chunk), inl(chunk);
    int best_inl = -1, budget = iterations, done = 0;
    CvRNG rng(0xffffffffffffffffull);
    for (int first = 0; first < budget; first += chunk) {
        const int cnt = std::min(chunk, iterations - first);
        const std::vector<int32_t> idx = pnp_detail::pnp_samples(n, m, first, cnt, rng, seed, sampling, samples);
        if (trace) trace->samples.insert(trace->samples.end(), idx.begin(), idx.end());
        ctx.check(eacham_solve_p3p(ctx.get(), n, object.data(), image.data(), K4, cnt, idx.data(), models.data(), okv.data(), nullptr, nullptr));
        ctx.check(eacham_score_hypotheses(ctx.get(), EACHAM_SCORE_PNP, n, object.data(), image.data(), cnt, models.data(), K4, thr, nullptr,
                                          inl.data(), nullptr));
        for (int k = 0; k < cnt && first + k < budget; ++k) {
            done = first + k + 1;
            if (!okv[k]) continue;
            if (inl[k] > std::max(best_inl, m - 1)) {   // strictly more inliers (and at least a sample's worth) replaces the model
                best_inl = inl[k];
                if (trace) trace->winner = first + k;
                std::copy(&models[(size_t)k * 12], &models[(size_t)k * 12] + 12, best_model.begin());
                budget = twoview_detail::ransac_update_num_iters(confidence, (double)(n - inl[k]) / n, m, budget);
            }
        }
    }
    out.iterations = done;
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
    if (rows.size() >= 5)   // EPnP needs five: a four-inlier winner keeps its own pose
        ctx.check(eacham_solve_pnp(ctx.get(), n, object.data(), image.data(), K4, (int)rows.size(), 1, rows.data(), refit, &rok));
    const double* pose = rok ? refit : best_model.data();
    for (int e = 0; e < 9; ++e) out.R[e] = pose[e];
    for (int e = 0; e < 3; ++e) out.t[e] = pose[9 + e];
    out.rvec = RodriguesFromMatrix(out.R);
    out.ok = true;
    return out;
}

// SolvePnPRansacP3P for a LIST of problems in rounds + 1 device calls: SolvePnPRansacBatch with the round served by ONE
// eacham_pnp_hypotheses_batch_p3p launch and the tail by eacham_pnp_refit_batch, unchanged. result[p] — and traces[p], when asked for —
// equal what SolvePnPRansacP3P returns for problem p alone with seeds[p] and the same arguments, field for field.
inline std::vector<PnPResult> SolvePnPRansacP3PBatch(Context& ctx, const std::vector<PnPProblem>& problems, const double* K9, int iterations = 10000,
                                                     float reprojectionError = 4.0f, double confidence = 0.999,
                                                     const std::vector<uint64_t>& seeds = {}, Sampling sampling = Sampling::OpenCV,
                                                     std::vector<PnPTrace>* traces = nullptr) {
    const size_t P = problems.size();
    const int m = 4, chunk = pnp_detail::kChunk;
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
        // (what SolvePnPRansacP3P turns away takes part with its points and never with a sample)
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
                const std::vector<int32_t> rows = pnp_detail::pnp_samples(npts[p], m, first, cnt, rng[p], p < seeds.size() ? seeds[p] : 1, sampling);
                if (traces) (*traces)[p].samples.insert((*traces)[p].samples.end(), rows.begin(), rows.end());
                idx.insert(idx.end(), rows.begin(), rows.end());
            }
            sample_ptr[p + 1] = sample_ptr[p] + cnt;
        }
        const size_t S = (size_t)sample_ptr[P];
        if (S == 0) break;
        models.resize(12 * S), okv.resize(S), inl.resize(S);
        ctx.check(eacham_pnp_hypotheses_batch_p3p(ctx.get(), (int)P, point_ptr.data(), object.data(), image.data(), K4, sample_ptr.data(), idx.data(),
                                                  thr, models.data(), okv.data(), inl.data()));
        for (size_t p = 0; p < P; ++p) {
            const size_t s0 = (size_t)sample_ptr[p];
            const int cnt = (int)(sample_ptr[p + 1] - sample_ptr[p]), n = npts[p];
            for (int k = 0; k < cnt && first + k < budget[p]; ++k) {
                out[p].iterations = first + k + 1;
                if (!okv[s0 + k]) continue;
                if (inl[s0 + k] > std::max(best_inl[p], m - 1)) {
                    best_inl[p] = inl[s0 + k];
                    if (traces) (*traces)[p].winner = first + k;
                    std::copy_n(&models[12 * (s0 + k)], 12, &best_model[12 * p]);
                    budget[p] = twoview_detail::ransac_update_num_iters(confidence, (double)(n - inl[s0 + k]) / n, m, budget[p]);
                }
            }
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
        const double* pose = rok[p] ? &refit[12 * p] : &best_model[12 * p];   // (fewer than 5 inliers, or a degenerate set: the winner stays)
        for (int e = 0; e < 9; ++e) out[p].R[e] = pose[e];
        for (int e = 0; e < 3; ++e) out[p].t[e] = pose[9 + e];
        out[p].rvec = RodriguesFromMatrix(out[p].R);
        out[p].ok = true;
    }
    return out;
}

}  // namespace hip
}  // namespace eacham
