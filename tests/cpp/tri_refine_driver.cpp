// Test driver for the polishing adapters of include/eacham/TriangulatorHip.hpp (TriangulateTracksRefined, RefineTrackPoints, RefinePoint):
//   tri_refine_driver <in.bin> <out.bin>
// in:  int32 tracks, int32 frames, int32 max_tries, float max_repr_error, float min_tri_angle, 4 doubles K (fx fy cx cy),
//      int64 track_ptr [tracks + 1], transforms [16 frames], uint32 obs_frame [obs], obs_uv [2 obs].
// out: blobs (int64 count, int64 element size, payload), one group after the other:
//        "plain"    eacham_triangulate_tracks alone                                 : points, status, masks
//        "adapter"  TriangulateTracksRefined                                        : points, status, masks, then refined, cost_before,
//                                                                                     cost_after, tries, refine_status, inliers, n_inliers
//        "by hand"  eacham_triangulate_tracks, then eacham_triangulate_refine_tracks
//                   with has_point = (status == 3) and use_mask = masks             : as "adapter", the cost as the call's [tracks, 2]
//        "single"   RefinePoint track by track from the plain point over the plain mask (tracks of status 3; the others copy the
//                   plain point and say NOT_REFINED)                                : refined, cost_before, cost_after, refine_status
// tests/test_tri_refine_cpp_gpu.py compares the groups byte for byte.
#include <cstdio>
#include <fstream>
#include <vector>

#include "eacham/TriangulatorHip.hpp"

using namespace eacham;
using namespace eacham::hip;

template <class T> static void wr(std::ofstream& f, const std::vector<T>& v) {
    const int64_t c[2] = {(int64_t)v.size(), (int64_t)sizeof(T)};
    f.write((const char*)c, sizeof(c));
    f.write((const char*)v.data(), sizeof(T) * v.size());
}

template <class T> static void rd(std::ifstream& f, std::vector<T>& v, size_t n) {
    v.resize(n);
    f.read((char*)v.data(), sizeof(T) * n);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    int32_t head[3] = {0, 0, 0};
    float thr[2] = {0, 0};
    double K4[4];
    in.read((char*)head, sizeof(head));
    in.read((char*)thr, sizeof(thr));
    in.read((char*)K4, sizeof(K4));
    const int n = head[0], frames = head[1], maxTries = head[2];
    TrackList tl;
    rd(in, tl.trackPtr, (size_t)n + 1);
    if (!in) return 3;
    const size_t nObs = (size_t)tl.trackPtr[n];
    rd(in, tl.transforms, 16 * (size_t)frames);
    rd(in, tl.obsFrame, nObs);
    rd(in, tl.obsUv, 2 * nObs);
    if (!in) return 3;
    const double K9[9] = {K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1};
    std::vector<int32_t> ptr32(tl.trackPtr.begin(), tl.trackPtr.end());
    try {
        Context ctx(0);
        // plain
        std::vector<double> points(3 * (size_t)n);
        std::vector<int32_t> status(n);
        std::vector<uint8_t> masks(nObs);
        ctx.check(eacham_triangulate_tracks(ctx.get(), tl.transforms.data(), frames, n, ptr32.data(), tl.obsFrame.data(), tl.obsUv.data(), K4, thr[0],
                                            thr[1], points.data(), status.data(), masks.data()));
        wr(out, points), wr(out, status), wr(out, masks);
        // adapter
        const TriangulatedTracks a = TriangulateTracksRefined(ctx, tl, K9, thr[0], thr[1], maxTries);
        wr(out, a.points), wr(out, a.status), wr(out, a.masks);
        wr(out, a.refined.points), wr(out, a.refined.costBefore), wr(out, a.refined.costAfter), wr(out, a.refined.tries), wr(out, a.refined.status);
        wr(out, a.refined.inliers), wr(out, a.refined.nInliers);
        // by hand
        std::vector<double> p2(3 * (size_t)n), refined(3 * (size_t)n), cost(2 * (size_t)n);
        std::vector<int32_t> s2(n), tries(n), rstatus(n), ni(n);
        std::vector<uint8_t> m2(nObs), has(n), rmask(nObs);
        ctx.check(eacham_triangulate_tracks(ctx.get(), tl.transforms.data(), frames, n, ptr32.data(), tl.obsFrame.data(), tl.obsUv.data(), K4, thr[0],
                                            thr[1], p2.data(), s2.data(), m2.data()));
        for (int t = 0; t < n; ++t) has[t] = s2[t] == 3;
        ctx.check(eacham_triangulate_refine_tracks(ctx.get(), tl.transforms.data(), frames, n, tl.trackPtr.data(), tl.obsFrame.data(), tl.obsUv.data(),
                                                   K4, p2.data(), has.data(), m2.data(), maxTries, thr[0], refined.data(), cost.data(), tries.data(),
                                                   rstatus.data(), rmask.data(), ni.data()));
        wr(out, p2), wr(out, s2), wr(out, m2);
        wr(out, refined), wr(out, cost), wr(out, tries), wr(out, rstatus), wr(out, rmask), wr(out, ni);
        // single
        std::vector<double> sp(points), cb(n, 0.0), ca(n, 0.0);
        std::vector<int32_t> ss(n, EACHAM_TRI_REFINE_NOT_REFINED);
        for (int t = 0; t < n; ++t) {
            if (status[t] != 3) continue;
            std::vector<EstimatorData> data;
            std::vector<bool> inl;
            for (int64_t i = tl.trackPtr[t]; i < tl.trackPtr[t + 1]; ++i) {
                EstimatorData d;
                for (int k = 0; k < 16; ++k) d.transform[k] = tl.transforms[16 * (size_t)tl.obsFrame[i] + k];
                d.point2d[0] = tl.obsUv[2 * i], d.point2d[1] = tl.obsUv[2 * i + 1];
                data.push_back(d), inl.push_back(masks[i] != 0);
            }
            ss[t] = RefinePoint(ctx, data, K9, &sp[3 * (size_t)t], inl, thr[0], maxTries, &cb[t], &ca[t]);
        }
        wr(out, sp), wr(out, cb), wr(out, ca), wr(out, ss);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "tri_refine_driver: %s\n", e.what());
        return 1;
    }
    return out ? 0 : 4;
}
