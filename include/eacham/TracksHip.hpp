// TracksHip.hpp — multi-view tracks from the match graph (eacham_tracks_build / eacham_graph_tracks of eacham_hip.h).
//
// The stage between the batch estimators and triangulation / bundle adjustment: the reference forms a star around one frame's
// keypoints with hash maps, frame by frame (TriangulateFrame, modules/sfm/reconstruction/Triangulator.cpp:202-241);
// a caller that holds the whole match graph — and perhaps the inlier masks of its edges from FindEssentialMatBatch — gets every
// track at once:
//
//   MatchGraph g = MatchAllPairs(ctx, frames, pairs);
//   Tracks tr = BuildTracks(ctx, pairs, g, keypointsPerFrame, keep);          // or ResidentMatchGraph::Tracks(keep)
//   std::vector<double> uv = GatherTrackPixels(tr, keypoints);               // keypoints[f] = x0 y0 x1 y1 ...
//   std::vector<int32_t> ptr = tr.TrackPtr32();
//   eacham_triangulate_tracks(ctx.get(), T, nFrames, (int)tr.size(), ptr.data(), tr.obs_frame.data(), uv.data(), K, ...);
//
// and (camera = obs_frame[o], landmark = the track of o, pixel = uv[o]) are the observations of eacham_ba_solve.
// A track is a connected component of kept matches over (frame, keypoint) with at least min_len keypoints; tracks are ordered by
// their smallest (frame, keypoint), the observations of a track frame-major. A track with two keypoints of one frame is a conflict:
// flags bit 0 (conflict_policy 0) or dropped whole (1).
#pragma once

#include <algorithm>

#include "FeatureMatcherHip.hpp"

namespace eacham {
namespace hip {

struct Tracks {
    std::vector<int64_t> track_ptr{0};       // n + 1 CSR offsets into the observation arrays
    std::vector<uint32_t> obs_frame, obs_kp; // frame and keypoint-in-frame per observation
    std::vector<uint8_t> flags;              // per track: bit 0 = two keypoints of one frame
    std::vector<int32_t> node_track;         // per keypoint (frames one behind the other): its track, -1 = none
    size_t size() const { return flags.size(); }
    std::vector<int32_t> TrackPtr32() const { return std::vector<int32_t>(track_ptr.begin(), track_ptr.end()); }   // what eacham_triangulate_tracks takes
};

namespace detail {
// sizes the outputs by the bounds that always suffice (n_obs <= min(nodes, 2 x matches), n_tracks <= n_obs / 2), calls, trims
template <class Call>
inline Tracks run_tracks(Context& ctx, int64_t nodes, int64_t matches, Call call) {
    const int64_t capObs = std::min<int64_t>(nodes, 2 * matches);
    const int32_t capTracks = (int32_t)(capObs / 2);
    Tracks tr;
    tr.track_ptr.assign((size_t)capTracks + 1, 0);
    tr.obs_frame.resize((size_t)capObs + 1);
    tr.obs_kp.resize((size_t)capObs + 1);
    tr.flags.resize((size_t)capTracks + 1);
    tr.node_track.resize((size_t)nodes + 1);
    int32_t nTracks = 0;
    int64_t nObs = 0;
    ctx.check(call(capObs, capTracks, &nTracks, &nObs, tr.track_ptr.data(), tr.obs_frame.data(), tr.obs_kp.data(), tr.flags.data(),
                   tr.node_track.data()));
    tr.track_ptr.resize((size_t)nTracks + 1);
    tr.obs_frame.resize((size_t)nObs);
    tr.obs_kp.resize((size_t)nObs);
    tr.flags.resize((size_t)nTracks);
    tr.node_track.resize((size_t)nodes);
    return tr;
}
}  // namespace detail

// keep: optional, one byte per match of g (g.q.size() of them)
inline Tracks BuildTracks(Context& ctx, const std::vector<std::pair<unsigned, unsigned>>& pairs, const MatchGraph& g,
                          const std::vector<size_t>& keypointsPerFrame, const uint8_t* keep = nullptr, int min_len = 2,
                          int conflict_policy = 0) {
    std::vector<int32_t> flat(2 * pairs.size());
    for (size_t p = 0; p < pairs.size(); ++p) flat[2 * p] = (int32_t)pairs[p].first, flat[2 * p + 1] = (int32_t)pairs[p].second;
    std::vector<int64_t> kpo(keypointsPerFrame.size() + 1, 0);
    for (size_t f = 0; f < keypointsPerFrame.size(); ++f) kpo[f + 1] = kpo[f] + (int64_t)keypointsPerFrame[f];
    int64_t matches = 0;
    for (int32_t c : g.counts) matches += c > 0 ? c : 0;
    return detail::run_tracks(ctx, kpo.back(), matches, [&](int64_t capObs, int32_t capTracks, int32_t* nT, int64_t* nO, int64_t* ptr,
                                                            uint32_t* of, uint32_t* ok, uint8_t* fl, int32_t* nt) {
        return eacham_tracks_build(ctx.get(), (int)keypointsPerFrame.size(), flat.data(), (int)pairs.size(), g.counts.data(), g.offsets.data(),
                                   g.q.data(), g.t.data(), kpo.data(), keep, min_len, conflict_policy, capObs, capTracks, nT, nO, ptr, of, ok,
                                   fl, nt);
    });
}

inline struct Tracks ResidentMatchGraph::Tracks(const uint8_t* keep, int min_len, int conflict_policy) {
    return detail::run_tracks(ctx_, nodes_, matches_, [&](int64_t capObs, int32_t capTracks, int32_t* nT, int64_t* nO, int64_t* ptr,
                                                          uint32_t* of, uint32_t* ok, uint8_t* fl, int32_t* nt) {
        return eacham_graph_tracks(h_, keep, min_len, conflict_policy, capObs, capTracks, nT, nO, ptr, of, ok, fl, nt);
    });
}

// obs_uv (x, y per observation) from per-frame keypoint arrays: keypoints[f] holds frame f's pixels as x0 y0 x1 y1 ...
template <class Frames>
inline std::vector<double> GatherTrackPixels(const Tracks& tr, const Frames& keypoints) {
    std::vector<double> uv(2 * tr.obs_frame.size());
    for (size_t o = 0; o < tr.obs_frame.size(); ++o) {
        const auto& kp = keypoints[tr.obs_frame[o]];
        uv[2 * o] = kp[2 * (size_t)tr.obs_kp[o]];
        uv[2 * o + 1] = kp[2 * (size_t)tr.obs_kp[o] + 1];
    }
    return uv;
}

}  // namespace hip
}  // namespace eacham
