// MatchAllPairsDot of include/eacham/FeatureMatcherHip.hpp with screened = true, then with its default (false), on one context.
//   match_dot_screen_driver <in.bin> <out.bin> <min_score> <min_dir> <min_mutual>
// in : int32 F, int32 dim, then per frame int32 n + n*dim floats.
// out: for screened = true, false: counts, q, t, scores over the pairs i < j (each int64 length + values).
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "eacham/FeatureMatcherHip.hpp"

using namespace eacham::hip;

template <class T> static T rd1(std::ifstream& f) { T v; f.read((char*)&v, sizeof(T)); return v; }
template <class T> static void wr(std::ofstream& f, const std::vector<T>& v) {
    const int64_t n = (int64_t)v.size();
    f.write((const char*)&n, sizeof(n));
    f.write((const char*)v.data(), sizeof(T) * v.size());
}

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    const float minScore = (float)std::atof(argv[3]);
    const int minDir = std::atoi(argv[4]), minMutual = std::atoi(argv[5]);
    const int F = rd1<int32_t>(in), dim = rd1<int32_t>(in);
    std::vector<std::vector<float>> store(F);
    std::vector<DescriptorView> frames(F);
    for (int f = 0; f < F; ++f) {
        const int n = rd1<int32_t>(in);
        store[f].resize((size_t)n * dim);
        in.read((char*)store[f].data(), sizeof(float) * store[f].size());
        frames[f] = DescriptorView{store[f].data(), n, dim};
    }
    try {
        Context ctx(0);
        std::vector<std::pair<unsigned, unsigned>> pairs;
        for (int i = 0; i < F; ++i)
            for (int j = i + 1; j < F; ++j) pairs.push_back({(unsigned)i, (unsigned)j});
        for (int screened = 1; screened >= 0; --screened) {
            const MatchGraphDot g = screened ? MatchAllPairsDot(ctx, frames, pairs, minScore, minDir, minMutual, true)
                                             : MatchAllPairsDot(ctx, frames, pairs, minScore, minDir, minMutual);
            wr(out, g.counts);
            wr(out, g.q);
            wr(out, g.t);
            wr(out, g.scores);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "match_dot_screen_driver: %s\n", e.what());
        return 6;
    }
    return 0;
}
