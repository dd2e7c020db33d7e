// guided_driver.cpp — the C++ adapters of include/eacham/GuidedMatchHip.hpp on one case of tests/guided_cases.py
// (tests/test_match_guided_cpp_gpu.py writes the case file, runs this program linked with libeacham_hip.so and compares what it
// writes with the Python mirror's arrays, byte for byte).
//
// argv[1]: the case — int32 dim, n_frames; per frame int32 rows, rows x dim float descriptors, rows x 2 double keypoints; int32
//          npairs, npairs x 2 int32 pairs, npairs x 9 double models; int32 kind, has_K; 4 double K; float max_error; double ratio;
//          uint32 max_d2; int32 cross_check
// argv[2]: the result — for the list form, then for the resident form: int64 total, counts, offsets (npairs + 1), q, t, d2, stats
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "eacham/GuidedMatchHip.hpp"

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
template <class T>
void write_vec(FILE* f, const std::vector<T>& v) {
    if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) throw std::runtime_error("short write");
}
void write_graph(FILE* f, const GuidedMatchGraph& g) {
    const std::vector<int64_t> total{(int64_t)g.q.size()};
    write_vec(f, total), write_vec(f, g.counts), write_vec(f, g.offsets), write_vec(f, g.q), write_vec(f, g.t), write_vec(f, g.d2), write_vec(f, g.stats);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    try {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        const int dim = read_one<int32_t>(f), n_frames = read_one<int32_t>(f);
        std::vector<std::vector<float>> descs((size_t)n_frames);
        std::vector<std::vector<double>> keypoints((size_t)n_frames);
        std::vector<size_t> per_frame((size_t)n_frames);
        for (int fr = 0; fr < n_frames; ++fr) {
            const size_t rows = (size_t)read_one<int32_t>(f);
            per_frame[fr] = rows;
            descs[fr] = read_vec<float>(f, rows * (size_t)dim);
            keypoints[fr] = read_vec<double>(f, 2 * rows);
        }
        const int npairs = read_one<int32_t>(f);
        const auto flat = read_vec<int32_t>(f, 2 * (size_t)npairs);
        const auto m = read_vec<double>(f, 9 * (size_t)npairs);
        const int kind = read_one<int32_t>(f), has_K = read_one<int32_t>(f);
        const auto K4 = read_vec<double>(f, 4);
        const float max_error = read_one<float>(f);
        const double ratio = read_one<double>(f);
        const uint32_t max_d2 = read_one<uint32_t>(f);
        const bool cross = read_one<int32_t>(f) != 0;
        std::fclose(f);

        std::vector<std::pair<unsigned, unsigned>> pairs((size_t)npairs);
        std::vector<RobustModel> models((size_t)npairs);
        for (int p = 0; p < npairs; ++p) {
            pairs[p] = {(unsigned)flat[2 * p], (unsigned)flat[2 * p + 1]};
            for (int e = 0; e < 9; ++e) models[p].model[e] = m[9 * (size_t)p + e];
            models[p].ok = true;
        }
        Context ctx(0);
        for (int fr = 0; fr < n_frames; ++fr) {
            descs[fr].resize(descs[fr].size() + 1);   // (no null data() for an empty frame)
            ctx.check(eacham_upload_descriptors(ctx.get(), fr, descs[fr].data(), (int)per_frame[fr], dim));
        }
        FILE* out = std::fopen(argv[2], "wb");
        if (!out) return 2;
        write_graph(out, MatchGuided(ctx, pairs, models, keypoints, kind, max_error, has_K ? K4.data() : nullptr, ratio, max_d2, cross));
        MatchGraph empty;
        empty.counts.assign((size_t)npairs + 1, 0), empty.offsets.assign((size_t)npairs + 1, 0), empty.q.assign(1, 0), empty.t.assign(1, 0);
        ResidentMatchGraph rg(ctx, pairs, empty, per_frame);
        SetKeypoints(rg, keypoints);
        write_graph(out, MatchGuided(rg, models, kind, max_error, has_K ? K4.data() : nullptr, ratio, max_d2, cross));
        std::fclose(out);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "guided_driver: %s\n", e.what());
        return 1;
    }
}
