// fundamental_driver.cpp — two programs for the tests of the fundamental-matrix kind.
//
// -DFUNDAMENTAL_HOST_ONLY (tests/test_fundamental_reference.py, tests/test_fundamental_gpu.py; no library is linked):
//   argv[1] = "check":   stdin lines of 28 numbers, src x0 y0 .. x6 y6 then dst; stdout per line cv_check_subset_fundamental's verdict
//   argv[1] = "samples": stdin "sampling iterations P", then per pair "n seed" and n lines "x1 y1 x2 y2"; stdout per pair the number
//                        of samples twoview_detail::lmeds_samples(n, 7, iterations, SubsetCheck::Fundamental, ...) drew and their
//                        indices (a pair with n < 7 draws nothing, as lmeds() returns at once)
//
// Otherwise (tests/test_fundamental_gpu.py, linked with libeacham_hip.so): FindFundamentalMat per pair against
// FindFundamentalMatBatch against VerifyFundamental on the same pairs — every RobustModel field and every trace field, both sample
// streams — and EssentialFromFundamental of the true F with the true K against the essential-matrix constraint. argv[1]: the case
// file (test_graph_verify_gpu.py: write_case, then 9 doubles of a true F and 4 of its K). Prints one line per comparison; exit
// status 1 if any differs.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#ifdef FUNDAMENTAL_HOST_ONLY

#include "eacham/TwoViewHip.hpp"

int main(int argc, char** argv) {
    using namespace eacham::hip;
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "check") {
        double v[28];
        for (;;) {
            for (int k = 0; k < 28; ++k)
                if (!(std::cin >> v[k])) return 0;
            float src[14], dst[14];
            for (int k = 0; k < 14; ++k) src[k] = (float)v[k], dst[k] = (float)v[14 + k];
            std::printf("%d\n", cv_check_subset_fundamental(src, dst, 7) ? 1 : 0);
        }
    }
    if (mode != "samples") return 2;
    int sampling, iterations, P;
    if (!(std::cin >> sampling >> iterations >> P)) return 2;
    for (int p = 0; p < P; ++p) {
        long long n;
        unsigned long long seed;
        if (!(std::cin >> n >> seed)) return 2;
        std::vector<double> uv1(2 * (size_t)n), uv2(2 * (size_t)n);
        for (long long i = 0; i < n; ++i)
            if (!(std::cin >> uv1[2 * i] >> uv1[2 * i + 1] >> uv2[2 * i] >> uv2[2 * i + 1])) return 2;
        std::vector<int32_t> s;
        if (n >= 7)
            s = twoview_detail::lmeds_samples((int)n, 7, iterations, twoview_detail::SubsetCheck::Fundamental, uv1, uv2, seed,
                                              sampling ? Sampling::Counter : Sampling::OpenCV);
        std::printf("%zu\n", s.size() / 7);
        for (size_t k = 0; k < s.size(); ++k) std::printf("%d%c", s[k], (k + 1) % 7 ? ' ' : '\n');
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
        read_vec<double>(f, 4);   // the graph's K: a fundamental matrix does not read it
        const auto seeds = read_vec<uint64_t>(f, (size_t)npairs);
        const auto Ftrue = read_vec<double>(f, 9);
        const auto Ktrue = read_vec<double>(f, 4);
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
            std::vector<LmedsTrace> tb, tv;
            const auto batch = FindFundamentalMatBatch(ctx, uv1, uv2, seeds, 1000, 0.99, sampling, &tb);
            const auto verified = VerifyFundamental(rg, 1000, 0.99, sampling, &tv, true, seeds);
            const bool sizes = batch.size() == (size_t)npairs && verified.size() == (size_t)npairs && tb.size() == (size_t)npairs && tv.size() == (size_t)npairs;
            report(s + " sizes", sizes);
            if (!sizes) continue;
            int ok = 0;
            for (int p = 0; p < npairs; ++p) {
                LmedsTrace t1;
                const RobustModel one = FindFundamentalMat(ctx, uv1[p], uv2[p], 1000, 0.99, seeds[p], sampling, &t1);
                const std::string at = s + " pair " + std::to_string(p);
                report(at + " single = batch model", same_model(one, batch[p]));
                report(at + " batch = verify model", same_model(batch[p], verified[p]));
                // (a pair that lmeds() leaves at once has no trace to compare: the batch forms record its candidates all the same)
                if (one.ok) report(at + " single = batch trace", same_trace(t1, tb[p]));
                report(at + " batch = verify trace", same_trace(tb[p], tv[p]));
                ok += one.ok;
            }
            std::printf("info %s pairs_with_a_model %d of %d\n", s.c_str(), ok, npairs);
            // the default seed of the overloads without a seed list
            const auto b0 = FindFundamentalMatBatch(ctx, uv1, uv2, 1000, 0.99, sampling);
            const auto v0 = VerifyFundamental(rg, 1000, 0.99, sampling, nullptr, false);
            bool same = b0.size() == v0.size();
            for (size_t p = 0; same && p < b0.size(); ++p) same = same_model(b0[p], v0[p]);
            report(s + " default seed batch = verify", same);
        }
        // E = K^T F K of a true F with its true K is an essential matrix: 2 E E^T E - tr(E E^T) E = 0
        Mat3 F;
        for (int k = 0; k < 9; ++k) F[k] = Ftrue[k];
        const Mat3 E = EssentialFromFundamental(F, Ktrue.data());
        const Mat3 EEt = twoview_detail::mul(E, twoview_detail::transpose(E)), EEtE = twoview_detail::mul(EEt, E);
        const double tr = EEt[0] + EEt[4] + EEt[8];
        double worst = 0.0, scale = 0.0;
        for (int k = 0; k < 9; ++k) worst = std::max(worst, std::fabs(2.0 * EEtE[k] - tr * E[k])), scale = std::max(scale, std::fabs(tr * E[k]));
        std::printf("info essential constraint %.3e relative\n", worst / scale);
        report("EssentialFromFundamental satisfies the essential constraint to 1e-9", scale > 0.0 && worst <= 1e-9 * scale);
    } catch (const std::exception& e) {
        std::printf("DIFFERENT exception %s\n", e.what());
        return 1;
    }
    return failures ? 1 : 0;
}

#endif
