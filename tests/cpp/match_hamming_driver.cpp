// FeatureMatcherHammingHip under the reference's call pattern (apps/sfm/main.cpp:84-109): every ORDERED frame pair is one Match() from
// a pool of worker threads on ONE shared instance — once directed, once with the mutual check — then MatchAllPairsHamming.
//   match_hamming_driver <in.bin> <out.bin> <threads> <ratio> <min_dir> <min_mutual>
// in : int32 F, int32 bytes per row, then per frame int32 n + n * bytes.
// out: for mutual = 0, 1: per ordered pair (i != j, i-major) int64 n, n x {q, t} sorted by q, n int32 distances;
//      then of MatchAllPairsHamming over the pairs i < j: counts, q, t, distances (each int64 length + values).
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <thread>

#include "eacham/FeatureMatcherHip.hpp"

using namespace eacham::hip;

template <class T> static T rd1(std::ifstream& f) { T v; f.read((char*)&v, sizeof(T)); return v; }
template <class T> static void wr(std::ofstream& f, const std::vector<T>& v) {
    const int64_t n = (int64_t)v.size();
    f.write((const char*)&n, sizeof(n));
    f.write((const char*)v.data(), sizeof(T) * v.size());
}

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    const int threads = std::atoi(argv[3]);
    const double ratio = std::atof(argv[4]);
    const int minDir = std::atoi(argv[5]), minMutual = std::atoi(argv[6]);
    const int F = rd1<int32_t>(in), bytes = rd1<int32_t>(in);
    std::vector<std::vector<uint8_t>> store(F);
    std::vector<BinaryDescriptorView> frames(F);
    for (int f = 0; f < F; ++f) {
        const int n = rd1<int32_t>(in);
        store[f].resize((size_t)n * bytes);
        in.read((char*)store[f].data(), store[f].size());
        frames[f] = BinaryDescriptorView{store[f].data(), n, bytes};
    }
    std::vector<std::pair<int, int>> ordered;
    for (int i = 0; i < F; ++i)
        for (int j = 0; j < F; ++j)
            if (i != j) ordered.push_back({i, j});
    try {
        for (int mutual = 0; mutual <= 1; ++mutual) {
            FeatureMatcherHammingHip matcher(ratio, mutual != 0);
            std::vector<FeatureMatcherHammingHip::MatchType> res(ordered.size());
            std::vector<FeatureMatcherHammingHip::DistanceType> ds(ordered.size());
            std::atomic<size_t> next{0};
            std::atomic<int> failed{0};
            std::vector<std::thread> pool;
            for (int w = 0; w < threads; ++w)
                pool.emplace_back([&] {
                    try {
                        for (size_t p = next.fetch_add(1); p < ordered.size(); p = next.fetch_add(1))
                            res[p] = matcher.Match(frames[ordered[p].first], frames[ordered[p].second], &ds[p]);
                    } catch (const std::exception& e) {
                        std::fprintf(stderr, "Match failed: %s\n", e.what());
                        failed.fetch_add(1);
                    }
                });
            for (auto& t : pool) t.join();
            if (failed.load()) return 3;
            for (size_t p = 0; p < ordered.size(); ++p) {
                std::vector<uint32_t> flat;
                std::vector<int32_t> dist;
                for (unsigned q = 0; q < (unsigned)frames[ordered[p].first].rows; ++q) {
                    auto it = res[p].find(q);
                    if (it == res[p].end()) continue;
                    flat.push_back(q);
                    flat.push_back(it->second);
                    dist.push_back(ds[p].at(q));
                }
                if (ds[p].size() != res[p].size()) return 4;
                const int64_t n = (int64_t)dist.size();
                out.write((const char*)&n, sizeof(n));
                out.write((const char*)flat.data(), sizeof(uint32_t) * flat.size());
                out.write((const char*)dist.data(), sizeof(int32_t) * dist.size());
            }
            // the accessor form, single caller: the distances of the call just made
            const auto m = matcher.Match(frames[0], frames[1]);
            const auto last = matcher.LastDistances();
            if (last.size() != m.size()) return 5;
            for (const auto& kv : m)
                if (!last.count(kv.first)) return 5;
        }
        Context ctx(0);
        std::vector<std::pair<unsigned, unsigned>> pairs;
        for (int i = 0; i < F; ++i)
            for (int j = i + 1; j < F; ++j) pairs.push_back({(unsigned)i, (unsigned)j});
        const MatchGraphHamming g = MatchAllPairsHamming(ctx, frames, pairs, ratio, minDir, minMutual);
        wr(out, g.counts);
        wr(out, g.q);
        wr(out, g.t);
        wr(out, g.distances);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "match_hamming_driver: %s\n", e.what());
        return 6;
    }
    std::printf("match_hamming_driver: %zu ordered pairs x 2 forms, %d threads\n", ordered.size(), threads);
    return 0;
}
