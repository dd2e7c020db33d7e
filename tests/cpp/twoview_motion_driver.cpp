// Test driver for the batch adapters of the second half of RecoverPoseTwoView (include/eacham/TwoViewHip.hpp: RecoverPoseBatch,
// TwoViewMotionBatch; include/eacham/ReconstructionHip.hpp: RecoverPoseTwoViewBatch) on the stand-ins of ref_standins.hpp:
//   twoview_motion_driver <in.bin> <out.bin>
// in:  int32 pairs, 4 doubles K (fx fy cx cy), then per pair int32 n, n x 2 doubles uv1, n x 2 doubles uv2.
// Pair p becomes the nodes 2p and 2p + 1 of a graph (match i of the list joins keypoint i of the first with keypoint n - 1 - i of the
// second), connected both ways; the directed pairs are (2p, 2p + 1), (2p + 1, 2p), ...
// out: one group of records after the other, one record per directed pair in each:
//   "single"  RecoverPoseTwoView pair by pair                       : transform, match ids, points, branch
//   "pose1"   RecoverPose on the E RecoverPoseTwoView estimates     : R, t, good, mask
// and, unless built with -DEACHAM_MOTION_SINGLE_ONLY (the CPU build over tests/cpp/oracle_abi.cpp, which has no batch entry point):
//   "batch"   RecoverPoseTwoViewBatch over all directed pairs       : as "single"
//   "motion"  TwoViewMotionBatch on the E / H of the single path    : as "single"
//   "poseB"   RecoverPoseBatch on the same E                        : as "pose1"
// tests/test_twoview_motion_gpu.py compares the batch records with the single ones byte for byte.
#include <cstdio>
#include <fstream>
#include <memory>
#include <vector>

#include "ref_standins.hpp"
#include "eacham/ReconstructionHip.hpp"

using namespace eacham;
using namespace eacham::hip;

template <class T> static void wr(std::ofstream& f, const T* v, size_t n) {
    int64_t c = (int64_t)n;
    f.write((const char*)&c, sizeof(c));
    f.write((const char*)v, sizeof(T) * n);
}

static void record(std::ofstream& f, const glue::MatchTwoViewHip& r, int32_t branch) {
    std::vector<uint32_t> ids;
    std::vector<double> pts;
    for (const auto& m : r.matches) {
        ids.push_back(std::get<0>(m)), ids.push_back(std::get<1>(m));
        pts.insert(pts.end(), std::get<2>(m).begin(), std::get<2>(m).end());
    }
    wr(f, r.transform.data(), 16);
    wr(f, ids.data(), ids.size());
    wr(f, pts.data(), pts.size());
    wr(f, &branch, 1);
}

static void record(std::ofstream& f, const RecoveredPose& p) {
    const int32_t good = p.good;
    wr(f, p.R.data(), 9);
    wr(f, p.t.data(), 3);
    wr(f, &good, 1);
    wr(f, p.mask.data(), p.mask.size());
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    int32_t pairs = 0;
    double K4[4];
    in.read((char*)&pairs, sizeof(pairs));
    in.read((char*)K4, sizeof(K4));
    auto graph = std::make_shared<graph_t>();
    auto map = std::make_shared<Map>();
    std::vector<std::pair<unsigned, unsigned>> directed;
    for (int p = 0; p < pairs; ++p) {
        int32_t n = 0;
        in.read((char*)&n, sizeof(n));
        std::vector<double> uv1(2 * (size_t)n), uv2(2 * (size_t)n);
        in.read((char*)uv1.data(), sizeof(double) * uv1.size());
        in.read((char*)uv2.data(), sizeof(double) * uv2.size());
        std::vector<cv::Point2f> k1(n), k2(n);
        match_t m12, m21;
        for (int i = 0; i < n; ++i) {
            k1[i].x = (float)uv1[2 * i], k1[i].y = (float)uv1[2 * i + 1];
            k2[n - 1 - i].x = (float)uv2[2 * i], k2[n - 1 - i].y = (float)uv2[2 * i + 1];
            m12[(unsigned)i] = (unsigned)(n - 1 - i), m21[(unsigned)(n - 1 - i)] = (unsigned)i;
        }
        const unsigned a = 2 * (unsigned)p, b = a + 1;
        graph->TestCreate(a)->TestSetFeatures(k1);
        graph->TestCreate(b)->TestSetFeatures(k2);
        graph->Connect(graph->Get(a), graph->Get(b), std::move(m12));
        graph->Connect(graph->Get(b), graph->Get(a), std::move(m21));
        directed.push_back({a, b}), directed.push_back({b, a});
    }
    if (!in) return 3;
    cv::Mat K;
    K.at<double>(0, 0) = K4[0], K.at<double>(1, 1) = K4[1], K.at<double>(0, 2) = K4[2], K.at<double>(1, 2) = K4[3], K.at<double>(2, 2) = 1.0;
    const double K9[9] = {K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1};
    const double Kff[4] = {K4[0], K4[0], K4[2], K4[3]};   // findEssentialMat's focal / pp form, as RecoverPoseTwoView passes it
    const float maxReprError = 4.0f, minTriAngle = 0.0174532925f;
    const uint64_t seed = 12345;
    try {
        Context ctx(0);
        glue::ReconstructionManagerHip<graph_t, Map> rec(ctx, graph, map, maxReprError, minTriAngle, 30, seed);
        const size_t D = directed.size();
        // the inputs and the estimates of the single path, restated as RecoverPoseTwoView gathers them
        std::vector<std::vector<std::pair<unsigned, unsigned>>> ms(D);
        std::vector<std::vector<double>> pts1(D), pts2(D);
        std::vector<RobustModel> E(D), H(D);
        std::vector<int> eIn(D), hIn(D);
        std::vector<int32_t> branch(D);
        for (size_t d = 0; d < D; ++d) {
            const unsigned id1 = directed[d].first, id2 = directed[d].second;
            auto* n1 = graph->Get(id1);
            auto* n2 = graph->Get(id2);
            for (const auto& m : n1->GetFactor(id2).matches) ms[d].emplace_back(m.first, m.second);
            std::sort(ms[d].begin(), ms[d].end());
            for (const auto& m : ms[d]) {
                const auto& a = n1->GetKeyPoint(m.first);
                const auto& b = n2->GetKeyPoint(m.second);
                pts1[d].push_back(a.x), pts1[d].push_back(a.y), pts2[d].push_back(b.x), pts2[d].push_back(b.y);
            }
            const uint64_t s = seed + 0x9E3779B97F4A7C15ull * ((uint64_t)id1 * 65536 + id2);
            E[d] = FindEssentialMat(ctx, pts1[d], pts2[d], Kff, 1000, s, 0.99);
            H[d] = FindHomography(ctx, pts1[d], pts2[d], 100, s + 1, 0.999);
            eIn[d] = E[d].inliers, hIn[d] = H[d].ok ? H[d].inliers : 0;
            const float ratio = hIn[d] > 0 && eIn[d] > 0 ? (float)hIn[d] / (float)eIn[d] : 0.0f;
            branch[d] = !E[d].ok ? -1 : ratio > 0.9f ? 1 : 0;
        }
        for (size_t d = 0; d < D; ++d) record(out, rec.RecoverPoseTwoView(directed[d].first, directed[d].second, K), branch[d]);
        for (size_t d = 0; d < D; ++d) record(out, RecoverPose(ctx, E[d].model, pts1[d], pts2[d], K9, 50.0, E[d].ok ? &E[d].mask : nullptr));
#ifndef EACHAM_MOTION_SINGLE_ONLY
        const auto batch = rec.RecoverPoseTwoViewBatch(directed, K);
        for (size_t d = 0; d < D; ++d) record(out, batch[d], branch[d]);
        const auto motion = TwoViewMotionBatch(ctx, pts1, pts2, K9, E, H, eIn, hIn, maxReprError, minTriAngle);
        for (size_t d = 0; d < D; ++d) {
            glue::MatchTwoViewHip r;
            for (const auto& m : motion[d].matches) r.matches.emplace_back(ms[d][m.first].first, ms[d][m.first].second, m.second);
            r.transform = motion[d].transform;
            record(out, r, motion[d].branch);
        }
        std::vector<Mat3> Em(D);
        std::vector<const std::vector<uint8_t>*> masks(D, nullptr);
        for (size_t d = 0; d < D; ++d) {
            Em[d] = E[d].model;
            if (E[d].ok) masks[d] = &E[d].mask;
        }
        const auto poses = RecoverPoseBatch(ctx, Em, pts1, pts2, K9, 50.0, &masks);
        for (size_t d = 0; d < D; ++d) record(out, poses[d]);
#endif
    } catch (const std::exception& e) {
        std::fprintf(stderr, "twoview_motion_driver: %s\n", e.what());
        return 1;
    }
    return out ? 0 : 4;
}
