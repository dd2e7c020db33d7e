// tracks_driver.cpp — the C++ adapters of the track building (include/eacham/TracksHip.hpp) on a match graph read from a file:
// BuildTracks and ResidentMatchGraph::Tracks, written out field by field; with geometry in the file, GatherTrackPixels' output is
// fed unchanged to eacham_triangulate_tracks. `uf` as third argument instead times a single-threaded union-find over the same
// arrays on the host (tools/tracks_rate.py prints it beside the device's figures, for reference only).
//
// in : i32 n_frames | i64 kp[n_frames] | i32 npairs | i32 pairs[2 npairs] | i32 counts[npairs] | i64 offsets[npairs + 1] |
//      i64 m | u32 q[m] | u32 t[m] | i32 has_keep | u8 keep[m] | i32 min_len | i32 policy |
//      i32 has_geometry | f64 K[4] | f64 T[16 n_frames] | f64 xy[2 kp[f]] per frame | f32 max_repr_error | f32 min_tri_angle
// out: per adapter the five fields of Tracks, each as i64 count | i64 element size | bytes; with geometry then uv, the
//      triangulation's return code (one i32), status, points — same framing.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "eacham/TracksHip.hpp"

using namespace eacham::hip;

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return v;
}
template <class T>
static T rd1(FILE* f) { return rd<T>(f, 1)[0]; }
template <class T>
static void wr(FILE* f, const std::vector<T>& v) {
    const int64_t head[2] = {(int64_t)v.size(), (int64_t)sizeof(T)};
    fwrite(head, sizeof(int64_t), 2, f);
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}
static void wr_tracks(FILE* f, const Tracks& tr) {
    wr(f, tr.track_ptr), wr(f, tr.obs_frame), wr(f, tr.obs_kp), wr(f, tr.flags), wr(f, tr.node_track);
}

// the host's way: union-find with the smaller root kept, then the nodes bucketed by label
static double union_find_ms(const std::vector<int64_t>& kpo, const std::vector<int32_t>& pairs, const MatchGraph& g, const uint8_t* keep,
                            size_t* n_tracks) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> parent((size_t)kpo.back());
    std::iota(parent.begin(), parent.end(), 0u);
    std::vector<uint8_t> touched(parent.size(), 0);
    auto find = [&](uint32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    for (size_t p = 0; p < g.counts.size(); ++p)
        for (int64_t k = g.offsets[p]; k < g.offsets[p] + g.counts[p]; ++k) {
            if (keep && !keep[k]) continue;
            const uint32_t u = (uint32_t)(kpo[pairs[2 * p]] + g.q[k]), v = (uint32_t)(kpo[pairs[2 * p + 1]] + g.t[k]);
            touched[u] = touched[v] = 1;
            const uint32_t ru = find(u), rv = find(v);
            if (ru != rv) parent[std::max(ru, rv)] = std::min(ru, rv);
        }
    std::vector<uint32_t> len(parent.size(), 0);
    for (size_t i = 0; i < parent.size(); ++i)
        if (touched[i]) ++len[find((uint32_t)i)];
    size_t n = 0;
    for (uint32_t l : len) n += l >= 2;
    *n_tracks = n;
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    const int nFrames = rd1<int32_t>(in);
    const auto kp = rd<int64_t>(in, nFrames);
    const int nPairs = rd1<int32_t>(in);
    const auto flat = rd<int32_t>(in, 2 * (size_t)nPairs);
    MatchGraph g;
    g.counts = rd<int32_t>(in, nPairs);
    g.offsets = rd<int64_t>(in, (size_t)nPairs + 1);
    const int64_t m = rd1<int64_t>(in);
    g.q = rd<uint32_t>(in, m);
    g.t = rd<uint32_t>(in, m);
    const bool hasKeep = rd1<int32_t>(in) != 0;
    const auto keepv = rd<uint8_t>(in, hasKeep ? m : 0);
    const uint8_t* keep = hasKeep ? keepv.data() : nullptr;
    const int minLen = rd1<int32_t>(in), policy = rd1<int32_t>(in);
    std::vector<std::pair<unsigned, unsigned>> pairs(nPairs);
    for (int p = 0; p < nPairs; ++p) pairs[p] = {(unsigned)flat[2 * p], (unsigned)flat[2 * p + 1]};
    std::vector<size_t> perFrame(kp.begin(), kp.end());

    if (argc > 3 && std::string(argv[3]) == "uf") {
        std::vector<int64_t> kpo(nFrames + 1, 0);
        for (int f = 0; f < nFrames; ++f) kpo[f + 1] = kpo[f] + kp[f];
        size_t n = 0;
        for (int rep = 0; rep < 5; ++rep) std::printf("union_find_ms %.3f\n", union_find_ms(kpo, flat, g, keep, &n));
        std::printf("union_find_tracks %zu\n", n);
        return 0;
    }

    const bool hasGeometry = rd1<int32_t>(in) != 0;
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    try {
        Context ctx(0);
        const Tracks built = BuildTracks(ctx, pairs, g, perFrame, keep, minLen, policy);
        wr_tracks(out, built);
        {
            ResidentMatchGraph graph(ctx, pairs, g, perFrame);
            wr_tracks(out, graph.Tracks(keep, minLen, policy));
        }
        if (hasGeometry) {
            const auto K = rd<double>(in, 4);
            const auto T = rd<double>(in, 16 * (size_t)nFrames);
            std::vector<std::vector<double>> keypoints(nFrames);
            for (int f = 0; f < nFrames; ++f) keypoints[f] = rd<double>(in, 2 * (size_t)kp[f]);
            const float maxReprError = rd1<float>(in), minTriAngle = rd1<float>(in);
            const std::vector<double> uv = GatherTrackPixels(built, keypoints);
            const std::vector<int32_t> ptr = built.TrackPtr32();
            std::vector<double> points(3 * built.size() + 3, 0.0);
            std::vector<int32_t> status(built.size(), -1);
            std::vector<uint8_t> masks(built.obs_frame.size() + 1);
            const int32_t rc = eacham_triangulate_tracks(ctx.get(), T.data(), nFrames, (int)built.size(), ptr.data(), built.obs_frame.data(), uv.data(),
                                                         K.data(), maxReprError, minTriAngle, points.data(), status.data(), masks.data());
            points.resize(3 * built.size());
            wr(out, uv), wr(out, std::vector<int32_t>{rc}), wr(out, status), wr(out, points);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    fclose(out);
    fclose(in);
    return 0;
}
