// Test driver for the polishing adapters (include/eacham/PnPHip.hpp: SolvePnPRansacRefined[Batch], RefinePnP[Batch];
// include/eacham/PnPP3PHip.hpp: SolvePnPRansacP3PRefined[Batch]):
//   pnp_refine_driver <in.bin> <out.bin>
// in:  the file of p3p_driver: int32 problems, 4 doubles K (fx fy cx cy), int32 iterations, then per problem int32 n, n x 3 doubles
//      object points, n x 2 doubles pixels.
// out: blobs (int64 count, int64 element size, payload), one group of records (one per problem) after the other, Sampling::Counter:
//        "plain p3p"     SolvePnPRansacP3P problem by problem                  : ok, R, rvec, t, inliers, iterations
//        "single p3p"    SolvePnPRansacP3PRefined problem by problem           : the same, then cost_before, cost_after, tries, status
//        "batch p3p"     SolvePnPRansacP3PRefinedBatch over the whole list     : as "single p3p"
//        "single epnp"   SolvePnPRansacRefined problem by problem              : as "single p3p"
//        "batch epnp"    SolvePnPRansacRefinedBatch over the whole list        : as "single p3p"
//        "refine batch"  RefinePnPBatch on the "plain p3p" results             : as "single p3p"
// tests/test_pnp_refine_cpp_gpu.py compares the batch records with the single ones byte for byte and the polish with the restatement.
#include <cstdio>
#include <fstream>
#include <vector>

#include "eacham/PnPP3PHip.hpp"

using namespace eacham;
using namespace eacham::hip;

template <class T> static void wr(std::ofstream& f, const T* v, size_t n) {
    const int64_t c[2] = {(int64_t)n, (int64_t)sizeof(T)};
    f.write((const char*)c, sizeof(c));
    f.write((const char*)v, sizeof(T) * n);
}

static void record(std::ofstream& f, const PnPResult& r) {
    const int32_t ok = r.ok, it = r.iterations;
    wr(f, &ok, 1);
    wr(f, r.R.data(), 9);
    wr(f, r.rvec.data(), 3);
    wr(f, r.t.data(), 3);
    wr(f, r.inliers.data(), r.inliers.size());
    wr(f, &it, 1);
}

static void record(std::ofstream& f, const PnPRefined& r) {
    record(f, static_cast<const PnPResult&>(r));
    const int32_t tries = r.tries, status = r.status;
    wr(f, &r.cost_before, 1);
    wr(f, &r.cost_after, 1);
    wr(f, &tries, 1);
    wr(f, &status, 1);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    int32_t P = 0, iterations = 0;
    double K4[4];
    in.read((char*)&P, sizeof(P));
    in.read((char*)K4, sizeof(K4));
    in.read((char*)&iterations, sizeof(iterations));
    std::vector<PnPProblem> problems((size_t)P);
    for (auto& pr : problems) {
        int32_t n = 0;
        in.read((char*)&n, sizeof(n));
        pr.object.resize(3 * (size_t)n), pr.image.resize(2 * (size_t)n);
        in.read((char*)pr.object.data(), sizeof(double) * pr.object.size());
        in.read((char*)pr.image.data(), sizeof(double) * pr.image.size());
    }
    if (!in) return 3;
    const double K9[9] = {K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1};
    const Sampling sampling = Sampling::Counter;
    try {
        Context ctx(0);
        std::vector<uint64_t> seeds((size_t)P);
        for (int p = 0; p < P; ++p) seeds[p] = 1000 + 7 * (uint64_t)p;
        std::vector<PnPResult> plain;
        for (int p = 0; p < P; ++p) {
            plain.push_back(SolvePnPRansacP3P(ctx, problems[p].object, problems[p].image, K9, iterations, 4.0f, 0.999, seeds[p], sampling));
            record(out, plain.back());
        }
        for (int p = 0; p < P; ++p)
            record(out, SolvePnPRansacP3PRefined(ctx, problems[p].object, problems[p].image, K9, iterations, 4.0f, 0.999, seeds[p], sampling));
        for (const PnPRefined& r : SolvePnPRansacP3PRefinedBatch(ctx, problems, K9, iterations, 4.0f, 0.999, seeds, sampling)) record(out, r);
        for (int p = 0; p < P; ++p)
            record(out, SolvePnPRansacRefined(ctx, problems[p].object, problems[p].image, K9, iterations, 4.0f, 0.999, seeds[p], sampling));
        for (const PnPRefined& r : SolvePnPRansacRefinedBatch(ctx, problems, K9, iterations, 4.0f, 0.999, seeds, sampling)) record(out, r);
        for (const PnPRefined& r : RefinePnPBatch(ctx, problems, K9, plain)) record(out, r);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "pnp_refine_driver: %s\n", e.what());
        return 1;
    }
    return out ? 0 : 4;
}
