// graph_verify_driver.cpp — two programs for the graph-verification tests.
//
// -DGRAPH_VERIFY_HOST_ONLY (tests/graph_verify_cases.py: host_samples; no library is linked): the project's own sample streams.
//   stdin:  "m check sampling iterations P", then per pair "n seed" and n lines "x1 y1 x2 y2"
//   stdout: per pair the number of samples twoview_detail::lmeds_samples(n, m, iterations, check, uv1, uv2, seed, sampling) drew and
//           their indices (a pair with n < m draws nothing, as lmeds() returns at once)
//
// Otherwise (tests/test_graph_verify_gpu.py, linked with libeacham_hip.so): the C++ adapters of include/eacham/GraphVerifyHip.hpp
// against FindEssentialMatBatch / FindHomographyBatch on host-gathered points, every RobustModel field and every trace field, under
// both sample streams, and TracksVerified against ResidentMatchGraph::Tracks(the masks). argv[1]: the case file
// (test_graph_verify_gpu.py: write_case). Prints one line per comparison; exit status 1 if any differs.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#ifdef GRAPH_VERIFY_HOST_ONLY

#include "eacham/TwoViewHip.hpp"

int main() {
    using namespace eacham::hip;
    int m, check, sampling, iterations, P;
    if (!(std::cin >> m >> check >> sampling >> iterations >> P)) return 2;
    for (int p = 0; p < P; ++p) {
        long long n;
        unsigned long long seed;
        if (!(std::cin >> n >> seed)) return 2;
        std::vector<double> uv1(2 * (size_t)n), uv2(2 * (size_t)n);
        for (long long i = 0; i < n; ++i)
            if (!(std::cin >> uv1[2 * i] >> uv1[2 * i + 1] >> uv2[2 * i] >> uv2[2 * i + 1])) return 2;
        std::vector<int32_t> s;
        if (n >= m) s = twoview_detail::lmeds_samples((int)n, m, iterations, check != 0, uv1, uv2, seed, sampling ? Sampling::Counter : Sampling::OpenCV);
        std::printf("%zu\n", s.size() / m);
        for (size_t k = 0; k < s.size(); ++k) std::printf("%d%c", s[k], (k + 1) % m ? ' ' : '\n');
    }
    return 0;
}

#else

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
bool same_trace(const LmedsTrace& a, const LmedsTrace& b) {
    return a.samples == b.samples && a.candidates == b.candidates && a.candidate == b.candidate && a.sample == b.sample && a.root == b.root &&
           bits(a.sigma, b.sigma) && bits(a.threshold, b.threshold) && bits(a.winner, b.winner);
}
void compare(const std::string& label, const std::vector<RobustModel>& got, const std::vector<RobustModel>& want, const std::vector<LmedsTrace>& tg,
             const std::vector<LmedsTrace>& tw) {
    bool sizes = got.size() == want.size() && tg.size() == tw.size() && tg.size() == got.size();
    report(label + " sizes", sizes);
    if (!sizes) return;
    int ok = 0;
    for (size_t p = 0; p < got.size(); ++p) {
        report(label + " pair " + std::to_string(p) + " model", same_model(got[p], want[p]));
        report(label + " pair " + std::to_string(p) + " trace", same_trace(tg[p], tw[p]));
        ok += want[p].ok;
    }
    std::printf("info %s pairs_with_a_model %d of %zu\n", label.c_str(), ok, want.size());
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

        // the host's walk over the matches
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
        for (Sampling sampling : {Sampling::OpenCV, Sampling::Counter}) {
            const std::string s = sampling == Sampling::OpenCV ? "opencv" : "counter";
            std::vector<LmedsTrace> tg, tw;
            const auto He = VerifyHomography(rg, pairs, g, keypoints, 100, 0.999, sampling, &tg, true, seeds);
            compare("homography/" + s, He, FindHomographyBatch(ctx, uv1, uv2, seeds, 100, 0.999, sampling, &tw), tg, tw);
            const auto E = VerifyEssential(rg, K4.data(), 1000, 0.99, sampling, &tg, true, seeds);   // the later mask is the one retained
            compare("essential/" + s, E, FindEssentialMatBatch(ctx, uv1, uv2, K4.data(), seeds, 1000, 0.99, sampling, &tw), tg, tw);
            std::vector<uint8_t> keep(n_src + 1, 0);
            for (int p = 0; p < npairs; ++p)
                if (E[p].ok) std::copy(E[p].mask.begin(), E[p].mask.end(), keep.begin() + g.offsets[p]);
            for (int policy = 0; policy < 2; ++policy) {
                const Tracks a = TracksVerified(rg, 2, policy), b = rg.Tracks(keep.data(), 2, policy);
                report("tracks/" + s + " policy " + std::to_string(policy), a.track_ptr == b.track_ptr && a.obs_frame == b.obs_frame && a.obs_kp == b.obs_kp &&
                                                                                 a.flags == b.flags && a.node_track == b.node_track);
                std::printf("info tracks/%s policy %d tracks %zu\n", s.c_str(), policy, b.size());
            }
        }
        // the default seed: no seed array at all
        std::vector<LmedsTrace> tg, tw;
        const auto E = VerifyEssential(rg, K4.data(), 1000, 0.99, Sampling::Counter, &tg, false);
        compare("essential/counter default seed", E, FindEssentialMatBatch(ctx, uv1, uv2, K4.data(), 1000, 0.99, Sampling::Counter, &tw), tg, tw);
    } catch (const std::exception& e) {
        std::printf("DIFFERENT exception %s\n", e.what());
        return 1;
    }
    return failures ? 1 : 0;
}

#endif
