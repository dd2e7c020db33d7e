// Test driver for the batch adapters of include/eacham/TwoViewHip.hpp:
//   twoview_batch_driver <in.bin> <out.bin>
// in:  int32 pairs, 4 doubles K (fx fy cx cy), then per pair int32 n, n x 2 doubles uv1, n x 2 doubles uv2.
// out: for the essential matrix and then for the homography — FindEssentialMatBatch / FindHomographyBatch over all pairs, then
//      FindEssentialMat / FindHomography pair by pair — one record per pair: every RobustModel field and every LmedsTrace field.
// tests/test_twoview_batch_gpu.py compares the batch records with the single ones byte for byte.
#include <cstdio>
#include <fstream>
#include <vector>

#include "eacham/TwoViewHip.hpp"

using namespace eacham::hip;

template <class T> static void wr(std::ofstream& f, const T* v, size_t n) {
    int64_t c = (int64_t)n;
    f.write((const char*)&c, sizeof(c));
    f.write((const char*)v, sizeof(T) * n);
}

static void record(std::ofstream& f, const RobustModel& r, const LmedsTrace& t) {
    const int32_t ints[7] = {r.inliers, r.iterations, r.ok ? 1 : 0, t.candidates, t.candidate, t.sample, t.root};
    wr(f, r.model.data(), 9);
    wr(f, r.mask.data(), r.mask.size());
    wr(f, ints, 7);
    wr(f, &r.median, 1);
    wr(f, t.samples.data(), t.samples.size());
    wr(f, &t.sigma, 1);
    wr(f, &t.threshold, 1);
    wr(f, t.winner.data(), 9);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    int32_t pairs = 0;
    double K4[4];
    in.read((char*)&pairs, sizeof(pairs));
    in.read((char*)K4, sizeof(K4));
    std::vector<std::vector<double>> uv1(pairs), uv2(pairs);
    for (int p = 0; p < pairs; ++p) {
        int32_t n = 0;
        in.read((char*)&n, sizeof(n));
        uv1[p].resize(2 * (size_t)n), uv2[p].resize(2 * (size_t)n);
        in.read((char*)uv1[p].data(), sizeof(double) * uv1[p].size());
        in.read((char*)uv2[p].data(), sizeof(double) * uv2[p].size());
    }
    if (!in) return 3;
    try {
        Context ctx(0);
        std::vector<LmedsTrace> traces;
        const std::vector<RobustModel> eb = FindEssentialMatBatch(ctx, uv1, uv2, K4, 1000, 0.99, Sampling::OpenCV, &traces);
        for (int p = 0; p < pairs; ++p) record(out, eb[p], traces[p]);
        for (int p = 0; p < pairs; ++p) {
            LmedsTrace t;
            const RobustModel r = FindEssentialMat(ctx, uv1[p], uv2[p], K4, 1000, 12345, 0.99, Sampling::OpenCV, &t);
            record(out, r, t);
        }
        const std::vector<RobustModel> hb = FindHomographyBatch(ctx, uv1, uv2, 100, 0.999, Sampling::OpenCV, &traces);
        for (int p = 0; p < pairs; ++p) record(out, hb[p], traces[p]);
        for (int p = 0; p < pairs; ++p) {
            LmedsTrace t;
            const RobustModel r = FindHomography(ctx, uv1[p], uv2[p], 100, 12345, 0.999, Sampling::OpenCV, &t);
            record(out, r, t);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "twoview_batch_driver: %s\n", e.what());
        return 1;
    }
    return out ? 0 : 4;
}
