// GuidedMatchHip.hpp — guided matching (eacham_match_guided / eacham_graph_match_guided of eacham_hip.h): the pairs of a verified
// match graph matched again, with only the candidates admitted that agree with the pair's two-view model.
//
//   MatchGraph g = MatchAllPairs(ctx, frames, pairs);                       // blind: the ratio test over the whole train frame
//   ResidentMatchGraph rg(ctx, pairs, g, keypointsPerFrame);
//   SetKeypoints(rg, keypoints);
//   std::vector<RobustModel> F = VerifyFundamentalRansac(rg);              // what the verification found, per pair
//   GuidedMatchGraph g2 = MatchGuided(rg, F, EACHAM_SCORE_FUNDAMENTAL, 4.0f);   // every pair again, gated by its own model
//   ResidentMatchGraph rg2(ctx, pairs, g2, keypointsPerFrame);              // g2 is the wire format the graph and the tracks take
//
// The descriptors are the frames resident in the context (MatchAllPairs left them there, frame f under id f). A pair without a
// model (RobustModel::ok == false) goes down as the all-zero "none" record and gets no match.
// A header of its own: drivers that include the other headers alone link what they linked before.
#pragma once

#include "GraphVerifyHip.hpp"

namespace eacham {
namespace hip {

struct GuidedMatchGraph : MatchGraph {
    std::vector<uint32_t> d2;      // d2[k] = squared L2 of the descriptors of q[k] -> t[k]
    std::vector<int32_t> stats;    // per pair |m12|, |m21| (0 without the cross-check), |result|
};

namespace guided_detail {

inline std::vector<double> flat_models(const std::vector<RobustModel>& models) {
    std::vector<double> m(9 * models.size() + 9, 0.0);
    for (size_t p = 0; p < models.size(); ++p)
        if (models[p].ok)
            for (int e = 0; e < 9; ++e) m[9 * p + e] = models[p].model[e];
    return m;
}

// call(cap, g, total): the C-ABI call on buffers of `cap` matches. The capacity that always suffices is the sum of the query
// frames' rows; where the caller does not know it the first answer says what is needed (EACHAM_ERR_CAPACITY writes nothing else).
template <class Call>
inline GuidedMatchGraph run(Context& ctx, size_t npairs, int64_t cap, Call call) {
    GuidedMatchGraph g;
    g.counts.assign(npairs + 1, 0), g.offsets.assign(npairs + 1, 0), g.stats.assign(3 * npairs + 3, 0);
    int64_t total = 0;
    for (int attempt = 0;; ++attempt) {
        g.q.assign((size_t)cap + 1, 0), g.t.assign((size_t)cap + 1, 0), g.d2.assign((size_t)cap + 1, 0);
        const int rc = call(cap, g, &total);
        if (rc == EACHAM_ERR_CAPACITY && attempt == 0) {
            cap = total;
            continue;
        }
        ctx.check(rc);
        break;
    }
    g.counts.resize(npairs), g.stats.resize(3 * npairs);
    g.q.resize((size_t)total), g.t.resize((size_t)total), g.d2.resize((size_t)total);
    return g;
}

}  // namespace guided_detail

// The list form. pairs: ordered (f1, f2) of resident int8 frames; models[p]: pair p's model of `kind` (EACHAM_SCORE_ESSENTIAL with
// K4 = fx fy cx cy or null for normalised points, EACHAM_SCORE_HOMOGRAPHY, EACHAM_SCORE_FUNDAMENTAL); keypoints[f] = x0 y0 x1 y1 ...
// of frame f, as many points as the frame has rows. maxError in the error's own unit (squared pixels for H and F; +inf: no gate).
template <class Frames>
inline GuidedMatchGraph MatchGuided(Context& ctx, const std::vector<std::pair<unsigned, unsigned>>& pairs, const std::vector<RobustModel>& models,
                                    const Frames& keypoints, int kind, float maxError, const double* K4 = nullptr, double ratio = 0.8,
                                    uint32_t maxD2 = 0, bool crossCheck = true) {
    if (models.size() != pairs.size()) throw std::invalid_argument("MatchGuided: one model per pair");
    std::vector<int32_t> flat(2 * pairs.size() + 2);
    std::vector<int64_t> kpo{0};
    std::vector<double> xy;
    for (const auto& kp : keypoints) {
        xy.insert(xy.end(), kp.begin(), kp.end());
        kpo.push_back((int64_t)(xy.size() / 2));
    }
    xy.resize(xy.size() + 2);   // (no null data() without keypoints)
    int64_t cap = 0;
    for (size_t p = 0; p < pairs.size(); ++p) {
        flat[2 * p] = (int32_t)pairs[p].first, flat[2 * p + 1] = (int32_t)pairs[p].second;
        if ((size_t)pairs[p].first + 1 >= kpo.size() || (size_t)pairs[p].second + 1 >= kpo.size()) throw std::invalid_argument("MatchGuided: a pair names a frame without keypoints");
        cap += kpo[pairs[p].first + 1] - kpo[pairs[p].first];
    }
    const std::vector<double> m = guided_detail::flat_models(models);
    return guided_detail::run(ctx, pairs.size(), cap, [&](int64_t c, GuidedMatchGraph& g, int64_t* total) {
        return eacham_match_guided(ctx.get(), kind, flat.data(), (int)pairs.size(), m.data(), K4, kpo.data(), xy.data(), maxError, ratio, maxD2,
                                   crossCheck ? 1 : 0, g.counts.data(), g.offsets.data(), g.q.data(), g.t.data(), g.d2.data(), c, total, g.stats.data());
    });
}

// The resident form: pairs and keypoints are the graph's (SetKeypoints), models what a Verify... call on this graph returned. A free
// function over the graph's accessors, like the Verify... calls of GraphVerifyHip.hpp.
inline GuidedMatchGraph MatchGuided(ResidentMatchGraph& rg, const std::vector<RobustModel>& models, int kind, float maxError, const double* K4 = nullptr,
                                    double ratio = 0.8, uint32_t maxD2 = 0, bool crossCheck = true) {
    if (models.size() != rg.counts().size()) throw std::invalid_argument("MatchGuided: one model per pair of the graph");
    const std::vector<double> m = guided_detail::flat_models(models);
    return guided_detail::run(rg.context(), rg.counts().size(), std::max<int64_t>(4 * rg.matches(), 4096), [&](int64_t c, GuidedMatchGraph& g, int64_t* total) {
        return eacham_graph_match_guided(rg.get(), kind, m.data(), K4, maxError, ratio, maxD2, crossCheck ? 1 : 0, g.counts.data(), g.offsets.data(),
                                         g.q.data(), g.t.data(), g.d2.data(), c, total, g.stats.data());
    });
}

}  // namespace hip
}  // namespace eacham
