// Test driver for the batch adapters of PnP registration (include/eacham/PnPHip.hpp: SolvePnPRansacBatch;
// include/eacham/ReconstructionHip.hpp: PnPBatch / RecoverPosePnPBatch) on the stand-ins of ref_standins.hpp:
//   pnp_batch_driver <in.bin> <out.bin>
// in:  int32 problems, 4 doubles K (fx fy cx cy), int32 iterations, int32 minPnpInliers, then per problem int32 n, n x 3 doubles
//      object points, n x 2 doubles pixels.
// out: blobs (int64 count, int64 element size, payload), one group of records after the other:
//   for Sampling::OpenCV, then Sampling::Counter:
//     "single"  SolvePnPRansac problem by problem            : ok, R, rvec, t, inliers, iterations, trace samples, trace winner
//     "batch"   SolvePnPRansacBatch over the whole list      : the same
//   "seq"     RecoverPosePnP on the pairs (0, p + 1) one after another : flag, node transform, node validity, factor transform
//   "batchG"  RecoverPosePnPBatch over the same pairs on a second, identical graph : the same
// The graph: node 0 holds one keypoint per correspondence of every problem, each with its map point; problem p is frame p + 1,
// whose keypoint i is the problem's pixel i, matched from node 0's keypoint (offset of p) + i.
// tests/test_pnp_batch_cpp_gpu.py compares the batch records with the single ones byte for byte.
#include <cstdio>
#include <fstream>
#include <memory>
#include <vector>

#include "ref_standins.hpp"
#include "eacham/ReconstructionHip.hpp"

using namespace eacham;
using namespace eacham::hip;

template <class T> static void wr(std::ofstream& f, const T* v, size_t n) {
    const int64_t c[2] = {(int64_t)n, (int64_t)sizeof(T)};
    f.write((const char*)c, sizeof(c));
    f.write((const char*)v, sizeof(T) * n);
}

static void record(std::ofstream& f, const PnPResult& r, const PnPTrace& t) {
    const int32_t ok = r.ok, it = r.iterations, win = t.winner;
    wr(f, &ok, 1);
    wr(f, r.R.data(), 9);
    wr(f, r.rvec.data(), 3);
    wr(f, r.t.data(), 3);
    wr(f, r.inliers.data(), r.inliers.size());
    wr(f, &it, 1);
    wr(f, t.samples.data(), t.samples.size());
    wr(f, &win, 1);
}

struct World {
    std::shared_ptr<graph_t> graph = std::make_shared<graph_t>();
    std::shared_ptr<Map> map = std::make_shared<Map>();
};

static World build(const std::vector<PnPProblem>& problems) {
    World w;
    std::vector<cv::Point2f> k0;
    node_t* n0 = w.graph->TestCreate(0);
    for (size_t p = 0; p < problems.size(); ++p) {
        const size_t n = problems[p].image.size() / 2, off = k0.size();
        std::vector<cv::Point2f> kp(n);
        match_t m;
        for (size_t i = 0; i < n; ++i) {
            kp[i].x = (float)problems[p].image[2 * i], kp[i].y = (float)problems[p].image[2 * i + 1];
            const unsigned id3d = w.map->Add(Eigen::Vector3d(problems[p].object[3 * i], problems[p].object[3 * i + 1], problems[p].object[3 * i + 2]));
            n0->SetPoint3d((unsigned)(off + i), id3d, false);
            m[(unsigned)(off + i)] = (unsigned)i;
        }
        k0.resize(off + n);
        node_t* nf = w.graph->TestCreate((unsigned)p + 1);
        nf->TestSetFeatures(kp);
        w.graph->Connect(n0, nf, std::move(m));
    }
    n0->TestSetFeatures(k0);
    n0->TestSetValid(true);
    return w;
}

static void record(std::ofstream& f, World& w, unsigned id, bool flag) {
    const int32_t fl = flag, valid = w.graph->Get(id)->IsValid();
    double T[16], F[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) T[4 * r + c] = w.graph->Get(id)->GetTransform()(r, c), F[4 * r + c] = w.graph->Get(0)->GetFactor(id).transform(r, c);
    wr(f, &fl, 1);
    wr(f, T, 16);
    wr(f, &valid, 1);
    wr(f, F, 16);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    int32_t P = 0, iterations = 0, minPnpInliers = 0;
    double K4[4];
    in.read((char*)&P, sizeof(P));
    in.read((char*)K4, sizeof(K4));
    in.read((char*)&iterations, sizeof(iterations));
    in.read((char*)&minPnpInliers, sizeof(minPnpInliers));
    std::vector<PnPProblem> problems((size_t)P);
    for (auto& pr : problems) {
        int32_t n = 0;
        in.read((char*)&n, sizeof(n));
        pr.object.resize(3 * (size_t)n), pr.image.resize(2 * (size_t)n);
        in.read((char*)pr.object.data(), sizeof(double) * pr.object.size());
        in.read((char*)pr.image.data(), sizeof(double) * pr.image.size());
    }
    if (!in) return 3;
    cv::Mat K;
    K.at<double>(0, 0) = K4[0], K.at<double>(1, 1) = K4[1], K.at<double>(0, 2) = K4[2], K.at<double>(1, 2) = K4[3], K.at<double>(2, 2) = 1.0;
    const double K9[9] = {K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1};
    try {
        Context ctx(0);
        std::vector<uint64_t> seeds((size_t)P);
        for (int p = 0; p < P; ++p) seeds[p] = 1000 + 7 * (uint64_t)p;
        for (const Sampling sampling : {Sampling::OpenCV, Sampling::Counter}) {
            for (int p = 0; p < P; ++p) {
                PnPTrace t;
                const PnPResult r = SolvePnPRansac(ctx, problems[p].object, problems[p].image, K9, iterations, 4.0f, 0.999, seeds[p], sampling, &t);
                record(out, r, t);
            }
            std::vector<PnPTrace> traces;
            const std::vector<PnPResult> rs = SolvePnPRansacBatch(ctx, problems, K9, iterations, 4.0f, 0.999, seeds, sampling, &traces);
            for (int p = 0; p < P; ++p) record(out, rs[p], traces[p]);
        }
        std::vector<std::pair<unsigned, unsigned>> pairs;
        for (int p = 0; p < P; ++p) pairs.push_back({0u, (unsigned)p + 1});
        World a = build(problems), b = build(problems);
        glue::ReconstructionManagerHip<graph_t, Map> seq(ctx, a.graph, a.map, 4.0f, 0.0174532925f, minPnpInliers, 12345);
        glue::ReconstructionManagerHip<graph_t, Map> bat(ctx, b.graph, b.map, 4.0f, 0.0174532925f, minPnpInliers, 12345);
        std::vector<bool> flags;
        for (const auto& pr : pairs) flags.push_back(seq.RecoverPosePnP(pr.first, pr.second, K));
        for (int p = 0; p < P; ++p) record(out, a, pairs[p].second, flags[p]);
        const std::vector<bool> done = bat.RecoverPosePnPBatch(pairs, K);
        for (int p = 0; p < P; ++p) record(out, b, pairs[p].second, done[p]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "pnp_batch_driver: %s\n", e.what());
        return 1;
    }
    return out ? 0 : 4;
}
