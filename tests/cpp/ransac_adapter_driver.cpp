// ransac_adapter_driver.cpp — the threshold-RANSAC adapters of include/eacham/TwoViewHip.hpp and GraphVerifyHip.hpp, linked with
// libeacham_hip.so (tests/test_ransac_adapters_cpp_gpu.py). argv[1]: a graph case file (tests/test_graph_verify_gpu.py: write_case).
//   Find{EssentialMat,FundamentalMat,Homography}RansacBatch against the single-pair forms pair by pair, every RobustModel field,
//   under both sample streams and for stage1 = 0 (the default), 3 and a single pass;
//   Verify{Essential,Fundamental,Homography}Ransac on the resident graph against the batch forms on host-gathered points: with the
//   points given again every pair field for field (a pair of exactly m matches by the n == m shortcut in both families), without
//   them every pair but those;
//   TracksVerified against ResidentMatchGraph::Tracks(the masks).
// Prints one line per comparison; exit status 1 if any differs.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "eacham/GraphVerifyHip.hpp"

using namespace eacham::hip;

namespace {

template <class T>
std::vector<T> read_vec(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) throw std::runtime_error("short case file");
    return v;
}
template <class T>
T read_one(FILE* f) { return read_vec<T>(f, 1)[0]; }

int failures = 0;
void report(const std::string& what, bool same) {
    std::printf("%s %s\n", same ? "same" : "DIFFERENT", what.c_str());
    failures += same ? 0 : 1;
}
template <class T>
bool bits(const T& a, const T& b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

bool same_model(const RobustModel& a, const RobustModel& b) {
    return bits(a.model, b.model) && a.mask == b.mask && a.inliers == b.inliers && bits(a.median, b.median) && a.iterations == b.iterations && a.ok == b.ok;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    try {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        const int n_frames = read_one<int32_t>(f);
        const auto kp = read_vec<int64_t>(f, (size_t)n_frames);
        const int npairs = read_one<int32_t>(f);
        const auto flat = read_vec<int32_t>(f, 2 * (size_t)npairs);
        MatchGraph g;
        g.counts = read_vec<int32_t>(f, (size_t)npairs);
        g.offsets = read_vec<int64_t>(f, (size_t)npairs);
        const size_t n_src = (size_t)read_one<int64_t>(f);
        g.q = read_vec<uint32_t>(f, n_src);
        g.t = read_vec<uint32_t>(f, n_src);
        std::vector<std::vector<double>> keypoints((size_t)n_frames);
        std::vector<size_t> per_frame((size_t)n_frames);
        for (int fr = 0; fr < n_frames; ++fr) keypoints[fr] = read_vec<double>(f, 2 * (size_t)kp[fr]), per_frame[fr] = (size_t)kp[fr];
        const auto K4 = read_vec<double>(f, 4);
        const auto seeds = read_vec<uint64_t>(f, (size_t)npairs);
        std::fclose(f);
        std::vector<std::pair<unsigned, unsigned>> pairs((size_t)npairs);
        for (int p = 0; p < npairs; ++p) pairs[p] = {(unsigned)flat[2 * p], (unsigned)flat[2 * p + 1]};
        std::vector<std::vector<double>> uv1((size_t)npairs), uv2((size_t)npairs);
        for (int p = 0; p < npairs; ++p)
            for (int i = 0; i < g.counts[p]; ++i) {
                const size_t a = g.q[(size_t)g.offsets[p] + i], b = g.t[(size_t)g.offsets[p] + i];
                uv1[p].push_back(keypoints[pairs[p].first][2 * a]), uv1[p].push_back(keypoints[pairs[p].first][2 * a + 1]);
                uv2[p].push_back(keypoints[pairs[p].second][2 * b]), uv2[p].push_back(keypoints[pairs[p].second][2 * b + 1]);
            }

        Context ctx(0);
        ResidentMatchGraph rg(ctx, pairs, g, per_frame);
        SetKeypoints(rg, keypoints);
        const int ITERS = 200;   // (the adapters' defaults are 1000 / 2000: fewer keep the host's draws of the single-pair forms short)
        for (Sampling sampling : {Sampling::OpenCV, Sampling::Counter}) {
            const std::string s = sampling == Sampling::OpenCV ? "opencv" : "counter";
            for (int stage1 : {0, 3, 1 << 20}) {
                const std::string at = s + " stage1 " + std::to_string(stage1);
                const auto E = FindEssentialMatRansacBatch(ctx, uv1, uv2, K4.data(), 1.0, 0.999, ITERS, sampling, seeds, stage1);
                const auto F = FindFundamentalMatRansacBatch(ctx, uv1, uv2, 3.0, 0.99, ITERS, sampling, seeds, stage1);
                const auto H = FindHomographyRansacBatch(ctx, uv1, uv2, 3.0, ITERS, 0.995, sampling, seeds, stage1);
                int okE = 0, okF = 0, okH = 0;
                for (int p = 0; p < npairs; ++p) {
                    const std::string pair = " pair " + std::to_string(p);
                    report("essential/" + at + pair, same_model(E[p], FindEssentialMatRansac(ctx, uv1[p], uv2[p], K4.data(), 1.0, 0.999, ITERS, sampling, seeds[p])));
                    report("fundamental/" + at + pair, same_model(F[p], FindFundamentalMatRansac(ctx, uv1[p], uv2[p], 3.0, 0.99, ITERS, sampling, seeds[p])));
                    report("homography/" + at + pair, same_model(H[p], FindHomographyRansac(ctx, uv1[p], uv2[p], 3.0, ITERS, 0.995, sampling, seeds[p])));
                    okE += E[p].ok, okF += F[p].ok, okH += H[p].ok;
                }
                std::printf("info %s pairs_with_a_model essential %d fundamental %d homography %d of %d\n", at.c_str(), okE, okF, okH, npairs);
                // the resident graph, the points given again: the same answers for EVERY pair, those of exactly m matches (the registrator's
                // shortcut, applied on the host by both families) included
                const auto VF = VerifyFundamentalRansac(rg, pairs, g, keypoints, 3.0, 0.99, ITERS, sampling, true, seeds, stage1);
                const auto VH = VerifyHomographyRansac(rg, pairs, g, keypoints, 3.0, ITERS, 0.995, sampling, true, seeds, stage1);
                const auto VE = VerifyEssentialRansac(rg, pairs, g, keypoints, K4.data(), 1.0, 0.999, ITERS, sampling, true, seeds, stage1);   // the later mask is the one retained
                // ... and without the points: the same but for the pairs of exactly m matches, which the device's rule answers
                const auto VE0 = VerifyEssentialRansac(rg, K4.data(), 1.0, 0.999, ITERS, sampling, true, seeds, stage1);
                const auto VF0 = VerifyFundamentalRansac(rg, 3.0, 0.99, ITERS, sampling, false, seeds, stage1);
                for (int p = 0; p < npairs; ++p) {
                    const std::string pair = " pair " + std::to_string(p);
                    report("verify essential/" + at + pair, same_model(VE[p], E[p]));
                    report("verify fundamental/" + at + pair, same_model(VF[p], F[p]));
                    report("verify homography/" + at + pair, same_model(VH[p], H[p]));
                    if (g.counts[p] != 5) report("verify essential, no points/" + at + pair, same_model(VE0[p], E[p]));
                    if (g.counts[p] != 7) report("verify fundamental, no points/" + at + pair, same_model(VF0[p], F[p]));
                }
                std::vector<uint8_t> keep(n_src + 1, 0);
                for (int p = 0; p < npairs; ++p)   // (VE0's call retained last; a pair of exactly 5 matches: the device rule's mask, VE0's)
                    if (VE0[p].ok) std::copy(VE0[p].mask.begin(), VE0[p].mask.end(), keep.begin() + g.offsets[p]);
                const Tracks a = TracksVerified(rg, 2, 0), b = rg.Tracks(keep.data(), 2, 0);
                report("tracks/" + at, a.track_ptr == b.track_ptr && a.obs_frame == b.obs_frame && a.obs_kp == b.obs_kp && a.flags == b.flags &&
                                           a.node_track == b.node_track);
                std::printf("info tracks/%s tracks %zu\n", at.c_str(), b.size());
            }
        }
    } catch (const std::exception& e) {
        std::printf("DIFFERENT exception %s\n", e.what());
        return 1;
    }
    return failures ? 1 : 0;
}
