// GraphVerifyHip.hpp — geometric verification of a RESIDENT match graph (eacham_graph_set_keypoints / eacham_graph_verify /
// eacham_graph_tracks_verified of eacham_hip.h).
//
// FindEssentialMatBatch / FindHomographyBatch (TwoViewHip.hpp) take the matches of every pair as host arrays: the caller walks the
// graph and gathers (uv1, uv2), the samples are drawn on the host, 32 bytes per match go up and a mask byte per match comes back —
// to go up again as the `keep` of the track builder. With the graph resident all of that happens on the device:
//
//   ResidentMatchGraph rg(ctx, pairs, g, keypointsPerFrame);
//   SetKeypoints(rg, keypoints);                                   // keypoints[f] = x0 y0 x1 y1 ... (pixels), uploaded once
//   std::vector<RobustModel> E = VerifyEssential(rg, K4);          // == FindEssentialMatBatch on the host-gathered points, field for field
//   Tracks tr = TracksVerified(rg);                                // == rg.Tracks(the masks of that call), nothing uploaded
//
// A header of its own: drivers that include TwoViewHip.hpp or TracksHip.hpp alone link what they linked before.
#pragma once

#include "TracksHip.hpp"
#include "TwoViewHip.hpp"

namespace eacham {
namespace hip {

// keypoints[f] holds frame f's pixels as x0 y0 x1 y1 ...; every frame's full keypoint count
template <class Frames>
inline void SetKeypoints(ResidentMatchGraph& rg, const Frames& keypoints) {
    std::vector<double> xy;
    xy.reserve(2 * (size_t)rg.nodes() + 2);
    for (const auto& kp : keypoints) xy.insert(xy.end(), kp.begin(), kp.end());
    if (xy.size() != 2 * (size_t)rg.nodes()) throw std::invalid_argument("SetKeypoints: the frames do not hold the graph's keypoints");
    xy.resize(xy.size() + 2);   // (no null data() for a graph without keypoints)
    rg.context().check(eacham_graph_set_keypoints(rg.get(), xy.data()));
}

namespace graphverify_detail {

// the host's walk over pair p's matches: uv1 / uv2 = x y x y ... of its keypoints in frame pairs[p].first / .second
template <class Frames>
inline void gather_pair(const std::vector<std::pair<unsigned, unsigned>>& pairs, const MatchGraph& g, const Frames& keypoints, size_t p,
                        std::vector<double>& uv1, std::vector<double>& uv2) {
    const size_t n = (size_t)std::max(g.counts[p], 0);
    uv1.resize(2 * n), uv2.resize(2 * n);
    const auto &k1 = keypoints[pairs[p].first], &k2 = keypoints[pairs[p].second];
    for (size_t i = 0; i < n; ++i) {
        const size_t a = g.q[(size_t)g.offsets[p] + i], b = g.t[(size_t)g.offsets[p] + i];
        uv1[2 * i] = k1[2 * a], uv1[2 * i + 1] = k1[2 * a + 1];
        uv2[2 * i] = k2[2 * b], uv2[2 * i + 1] = k2[2 * b + 1];
    }
}
// the refit of cv::findHomography on every pair with a model and more than 4 matches, on host-gathered points
template <class Frames>
inline void refit_homographies(std::vector<RobustModel>& r, const std::vector<std::pair<unsigned, unsigned>>& pairs, const MatchGraph& g,
                               const Frames& keypoints) {
    std::vector<double> uv1, uv2;
    for (size_t p = 0; p < r.size(); ++p) {
        if (!r[p].ok || g.counts[p] <= 4) continue;
        gather_pair(pairs, g, keypoints, p, uv1, uv2);
        Mat3 H;
        if (RefitHomography(uv1, uv2, r[p].mask, H)) r[p].model = H;
    }
}

// twoview_detail::lmeds_batch with the gather, the draws and the mask left on the device. seeds: empty = 12345 for every pair.
inline std::vector<RobustModel> verify(ResidentMatchGraph& rg, int solve_kind, int m, const double* K4, int maxIters, double confidence,
                                       const std::vector<uint64_t>& seeds, Sampling sampling, bool retain, std::vector<LmedsTrace>* traces) {
    const size_t P = rg.counts().size();
    std::vector<RobustModel> out(P);
    if (traces) traces->assign(P, LmedsTrace());
    if (!seeds.empty() && seeds.size() != P) throw std::invalid_argument("graph verify: one seed per pair");
    if (P == 0) return out;
    const int iterations = maxIters > 0 ? std::min(maxIters, std::max(twoview_detail::ransac_update_num_iters(confidence, 0.45, m, maxIters), 3)) : 0;
    int64_t n_src = 0;
    for (size_t p = 0; p < P; ++p)
        if (rg.counts()[p] > 0) n_src = std::max<int64_t>(n_src, rg.offsets()[p] + rg.counts()[p]);
    std::vector<double> models(P * 9);
    std::vector<float> med(P), thr(P);
    std::vector<int32_t> inl(P), win(P * 3), ncand(P), nsamp(P), samples(traces ? P * (size_t)iterations * m + 1 : 0);
    std::vector<uint8_t> masks((size_t)n_src + 1);
    rg.context().check(eacham_graph_verify(rg.get(), solve_kind, K4, sampling == Sampling::OpenCV ? EACHAM_SAMPLING_OPENCV : EACHAM_SAMPLING_COUNTER,
                                           iterations, seeds.empty() ? nullptr : seeds.data(), retain ? 1 : 0, models.data(), med.data(), thr.data(),
                                           inl.data(), masks.data(), win.data(), ncand.data(), nsamp.data(), traces ? samples.data() : nullptr));
    for (size_t p = 0; p < P; ++p) {
        const int n = rg.counts()[p];
        RobustModel& r = out[p];
        r.iterations = nsamp[p];
        if (traces) {
            LmedsTrace& t = (*traces)[p];
            const int32_t* s = &samples[p * (size_t)iterations * m];
            t.samples.assign(s, s + (size_t)nsamp[p] * m);
            t.candidates = ncand[p];
        }
        if (win[3 * p] < 0) continue;
        for (int e = 0; e < 9; ++e) r.model[e] = models[9 * p + e];
        r.median = med[p];
        r.mask.assign(masks.begin() + rg.offsets()[p], masks.begin() + rg.offsets()[p] + n);
        r.inliers = inl[p];
        r.ok = true;
        if (traces) {
            LmedsTrace& t = (*traces)[p];
            t.candidate = win[3 * p], t.sample = win[3 * p + 1], t.root = win[3 * p + 2];
            t.sigma = std::max(2.5 * 1.4826 * (1.0 + 5.0 / std::max(n - m, 1)) * std::sqrt((double)med[p]), 0.001);   // as lmeds() states it
            t.threshold = thr[p];
            t.winner = r.model;
        }
    }
    return out;
}

}  // namespace graphverify_detail

// FindEssentialMatBatch for every pair of the resident graph: result[p] (and traces[p]) equal FindEssentialMatBatch(ctx, uv1, uv2,
// K4, [seeds,] maxIters, prob, sampling, traces)[p] on the points gathered from the graph's matches on the host, field for field.
// retain: the inlier mask stays in the graph for TracksVerified. seeds: empty = 12345 for every pair.
inline std::vector<RobustModel> VerifyEssential(ResidentMatchGraph& rg, const double* K4, int maxIters = 1000, double prob = 0.99,
                                                Sampling sampling = Sampling::OpenCV, std::vector<LmedsTrace>* traces = nullptr,
                                                bool retain = true, const std::vector<uint64_t>& seeds = {}) {
    return graphverify_detail::verify(rg, EACHAM_SOLVE_ESSENTIAL5, 5, K4, maxIters, prob, seeds, sampling, retain, traces);
}

// FindFundamentalMatBatch for every pair of the resident graph — the verification that reads no intrinsics: result[p] (and traces[p])
// equal FindFundamentalMatBatch(ctx, uv1, uv2, [seeds,] maxIters, prob, sampling, traces)[p] on the host-gathered points, field for
// field. There is no refit. retain and seeds as for VerifyEssential.
inline std::vector<RobustModel> VerifyFundamental(ResidentMatchGraph& rg, int maxIters = 1000, double prob = 0.99, Sampling sampling = Sampling::OpenCV,
                                                  std::vector<LmedsTrace>* traces = nullptr, bool retain = true, const std::vector<uint64_t>& seeds = {}) {
    return graphverify_detail::verify(rg, EACHAM_SOLVE_FUNDAMENTAL7, 7, nullptr, maxIters, prob, seeds, sampling, retain, traces);
}

// FindHomographyBatch for every pair of the resident graph. The refit of cv::findHomography on the winner's inliers stays a host
// step on the returned mask (RefitHomography), so the matches and pixels it reads are given again: `pairs` and `g` as the graph was
// made from them, keypoints[f] = x0 y0 x1 y1 ... Only pairs with a model and more than 4 matches are gathered for it.
template <class Frames>
inline std::vector<RobustModel> VerifyHomography(ResidentMatchGraph& rg, const std::vector<std::pair<unsigned, unsigned>>& pairs, const MatchGraph& g,
                                                 const Frames& keypoints, int maxIters = 100, double confidence = 0.999,
                                                 Sampling sampling = Sampling::OpenCV, std::vector<LmedsTrace>* traces = nullptr,
                                                 bool retain = true, const std::vector<uint64_t>& seeds = {}) {
    if (pairs.size() != rg.counts().size()) throw std::invalid_argument("VerifyHomography: not the pairs the graph was made from");
    std::vector<RobustModel> r = graphverify_detail::verify(rg, EACHAM_SOLVE_HOMOGRAPHY4, 4, nullptr, maxIters, confidence, seeds, sampling, retain, traces);
    graphverify_detail::refit_homographies(r, pairs, g, keypoints);
    return r;
}

namespace graphverify_detail {

// twoview_detail::ransac_batch with the gather, the draws and the mask left on the device (eacham_graph_verify_ransac). A pair with
// exactly m matches goes through the device's rule like every other pair; the registrator's n == m shortcut, which ransac_batch
// applies on the host, needs the pair's points: all_points_pairs below applies it where the caller gives them again.
// seeds: empty = 12345 for every pair.
inline std::vector<RobustModel> verify_ransac(ResidentMatchGraph& rg, int solve_kind, const double* K4, int maxIters, float threshold_sq, double confidence,
                                              const std::vector<uint64_t>& seeds, Sampling sampling, bool retain, int stage1) {
    const size_t P = rg.counts().size();
    std::vector<RobustModel> out(P);
    if (!seeds.empty() && seeds.size() != P) throw std::invalid_argument("graph verify: one seed per pair");
    if (P == 0) return out;
    int64_t n_src = 0;
    for (size_t p = 0; p < P; ++p)
        if (rg.counts()[p] > 0) n_src = std::max<int64_t>(n_src, rg.offsets()[p] + rg.counts()[p]);
    std::vector<double> models(P * 9);
    std::vector<int32_t> inl(P), win(P * 3), ncand(P), used(P), nsamp(P);
    std::vector<uint8_t> masks((size_t)n_src + 1);
    rg.context().check(eacham_graph_verify_ransac(rg.get(), solve_kind, K4, sampling == Sampling::OpenCV ? EACHAM_SAMPLING_OPENCV : EACHAM_SAMPLING_COUNTER,
                                                  std::max(maxIters, 0), seeds.empty() ? nullptr : seeds.data(), retain ? 1 : 0, threshold_sq, confidence,
                                                  stage1, models.data(), inl.data(), masks.data(), win.data(), ncand.data(), used.data(), nsamp.data(),
                                                  nullptr));
    for (size_t p = 0; p < P; ++p) {
        RobustModel& r = out[p];
        r.iterations = used[p];
        if (win[3 * p] < 0) continue;
        for (int e = 0; e < 9; ++e) r.model[e] = models[9 * p + e];
        r.mask.assign(masks.begin() + rg.offsets()[p], masks.begin() + rg.offsets()[p] + rg.counts()[p]);
        r.inliers = inl[p];
        r.ok = true;
    }
    return out;
}

// result[p] of every pair with exactly m matches as twoview_detail::ransac_batch gives it (ransac_all_points on host-gathered points).
// The mask RETAINED in the graph stays the device rule's for such a pair.
template <class Frames>
inline void all_points_pairs(Context& ctx, std::vector<RobustModel>& r, int solve_kind, int m, const double* K4,
                             const std::vector<std::pair<unsigned, unsigned>>& pairs, const MatchGraph& g, const Frames& keypoints, int maxIters) {
    if (pairs.size() != r.size()) throw std::invalid_argument("graph verify: not the pairs the graph was made from");
    std::vector<double> uv1, uv2;
    for (size_t p = 0; p < r.size(); ++p) {
        if (g.counts[p] != m || maxIters <= 0) continue;
        gather_pair(pairs, g, keypoints, p, uv1, uv2);
        r[p] = twoview_detail::ransac_all_points(ctx, solve_kind, m, uv1, uv2, K4);
    }
}

}  // namespace graphverify_detail

// FindEssentialMatRansacBatch for every pair of the resident graph: result[p] equals FindEssentialMatRansacBatch(...)[p] on the points
// gathered from the graph's matches on the host, field for field, for every pair with more than 5 matches (see verify_ransac).
// retain: the inlier mask stays in the graph for TracksVerified. seeds: empty = 12345 for every pair.
inline std::vector<RobustModel> VerifyEssentialRansac(ResidentMatchGraph& rg, const double* K4, double threshold = 1.0, double prob = 0.999,
                                                      int maxIters = 1000, Sampling sampling = Sampling::OpenCV, bool retain = true,
                                                      const std::vector<uint64_t>& seeds = {}, int stage1 = 0) {
    return graphverify_detail::verify_ransac(rg, EACHAM_SOLVE_ESSENTIAL5, K4, maxIters, twoview_detail::ransac_threshold_sq(threshold, K4), prob, seeds,
                                             sampling, retain, stage1);
}
// ... with `pairs`, `g` and keypoints[f] = x0 y0 x1 y1 ... given again, as VerifyHomography takes them: every pair field for field, the
// pairs of exactly 5 matches by the registrator's shortcut on the host.
template <class Frames>
inline std::vector<RobustModel> VerifyEssentialRansac(ResidentMatchGraph& rg, const std::vector<std::pair<unsigned, unsigned>>& pairs, const MatchGraph& g,
                                                      const Frames& keypoints, const double* K4, double threshold = 1.0, double prob = 0.999,
                                                      int maxIters = 1000, Sampling sampling = Sampling::OpenCV, bool retain = true,
                                                      const std::vector<uint64_t>& seeds = {}, int stage1 = 0) {
    std::vector<RobustModel> r = VerifyEssentialRansac(rg, K4, threshold, prob, maxIters, sampling, retain, seeds, stage1);
    graphverify_detail::all_points_pairs(rg.context(), r, EACHAM_SOLVE_ESSENTIAL5, 5, K4, pairs, g, keypoints, maxIters);
    return r;
}
// FindFundamentalMatRansacBatch for every pair of the resident graph (more than 7 matches: field for field). No intrinsics, no refit.
inline std::vector<RobustModel> VerifyFundamentalRansac(ResidentMatchGraph& rg, double threshold = 3.0, double confidence = 0.99, int maxIters = 1000,
                                                        Sampling sampling = Sampling::OpenCV, bool retain = true,
                                                        const std::vector<uint64_t>& seeds = {}, int stage1 = 0) {
    return graphverify_detail::verify_ransac(rg, EACHAM_SOLVE_FUNDAMENTAL7, nullptr, maxIters, twoview_detail::ransac_threshold_sq(threshold, nullptr),
                                             confidence, seeds, sampling, retain, stage1);
}
// ... with the points given again: every pair field for field, the pairs of exactly 7 matches by the shortcut on the host.
template <class Frames>
inline std::vector<RobustModel> VerifyFundamentalRansac(ResidentMatchGraph& rg, const std::vector<std::pair<unsigned, unsigned>>& pairs, const MatchGraph& g,
                                                        const Frames& keypoints, double threshold = 3.0, double confidence = 0.99, int maxIters = 1000,
                                                        Sampling sampling = Sampling::OpenCV, bool retain = true,
                                                        const std::vector<uint64_t>& seeds = {}, int stage1 = 0) {
    std::vector<RobustModel> r = VerifyFundamentalRansac(rg, threshold, confidence, maxIters, sampling, retain, seeds, stage1);
    graphverify_detail::all_points_pairs(rg.context(), r, EACHAM_SOLVE_FUNDAMENTAL7, 7, nullptr, pairs, g, keypoints, maxIters);
    return r;
}
// FindHomographyRansacBatch for every pair of the resident graph, field for field: the points are given again (`pairs`, `g`,
// `keypoints`, as for VerifyHomography) for the shortcut on pairs of exactly 4 matches and for the refit on the winner's inliers.
template <class Frames>
inline std::vector<RobustModel> VerifyHomographyRansac(ResidentMatchGraph& rg, const std::vector<std::pair<unsigned, unsigned>>& pairs, const MatchGraph& g,
                                                       const Frames& keypoints, double threshold = 3.0, int maxIters = 2000, double confidence = 0.995,
                                                       Sampling sampling = Sampling::OpenCV, bool retain = true,
                                                       const std::vector<uint64_t>& seeds = {}, int stage1 = 0) {
    if (pairs.size() != rg.counts().size()) throw std::invalid_argument("VerifyHomographyRansac: not the pairs the graph was made from");
    std::vector<RobustModel> r = graphverify_detail::verify_ransac(rg, EACHAM_SOLVE_HOMOGRAPHY4, nullptr, maxIters,
                                                                   twoview_detail::ransac_threshold_sq(threshold, nullptr), confidence, seeds, sampling,
                                                                   retain, stage1);
    graphverify_detail::all_points_pairs(rg.context(), r, EACHAM_SOLVE_HOMOGRAPHY4, 4, nullptr, pairs, g, keypoints, maxIters);
    graphverify_detail::refit_homographies(r, pairs, g, keypoints);
    return r;
}

// ResidentMatchGraph::Tracks with the mask the last Verify...(retain = true) left in the graph as `keep`: nothing is uploaded
inline Tracks TracksVerified(ResidentMatchGraph& rg, int min_len = 2, int conflict_policy = 0) {
    return detail::run_tracks(rg.context(), rg.nodes(), rg.matches(), [&](int64_t capObs, int32_t capTracks, int32_t* nT, int64_t* nO, int64_t* ptr,
                                                                          uint32_t* of, uint32_t* ok, uint8_t* fl, int32_t* nt) {
        return eacham_graph_tracks_verified(rg.get(), min_len, conflict_policy, capObs, capTracks, nT, nO, ptr, of, ok, fl, nt);
    });
}

}  // namespace hip
}  // namespace eacham
