// Test driver for include/eacham/TwoViewHip.hpp and PnPHip.hpp.
//   twoview_driver decompose   < "H(9) K(9)", "E(9)" or "R(9)" lines -> prints the decompositions / the Rodrigues vector (host-only math)
//   twoview_driver iters <in.bin> <out.bin>                        -> ransac_update_num_iters on a list of (p, ep, m, maxIters) (host-only)
//   twoview_driver refit <in.bin> <out.bin>                        -> RefitHomography on records of points + mask (host-only)
//   twoview_driver pnp <in.bin> <out.bin>                          -> SolvePnPRansac through the C-ABI
//   twoview_driver pipeline <in.bin> <out.bin>                    -> FindEssentialMat / FindHomography / RecoverPose /
//                                                                    DecomposeHomographyMat through the C-ABI
// The C-ABI is whatever the driver is linked with: libeacham_hip.so (GPU), tests/cpp/oracle_abi.cpp (the CPU oracle behind the
// same entry points) or tests/cpp/stub_abi.cpp (fake results, for the sanitizer builds).
// A pnp / pipeline record that starts with n = -1 carries its own parameters (below) in place of the reference's literals, and
// its output record is followed by what the loops decided on the way (the samples, the winner's place, sigma, ...): that is
// what tests/test_estimators.py replays step by step.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>

#include "eacham/PnPHip.hpp"
#include "eacham/TwoViewHip.hpp"

using namespace eacham::hip;

template <class T> static std::vector<T> rd(std::ifstream& f, size_t n) {
    std::vector<T> v(n);
    f.read((char*)v.data(), sizeof(T) * n);
    return v;
}
template <class T> static void wr(std::ofstream& f, const std::vector<T>& v) {
    int64_t n = (int64_t)v.size();
    f.write((char*)&n, sizeof(n));
    f.write((const char*)v.data(), sizeof(T) * v.size());
}

static Sampling sampling_of(double v) { return v == 0.0 ? Sampling::OpenCV : Sampling::Counter; }   // (2: a given list, passed beside it)

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "decompose")) {
        std::string kind;
        while (std::cin >> kind) {
            if (kind == "H") {
                Mat3 H;
                double K[9];
                for (double& x : H) std::cin >> x;
                for (double& x : K) std::cin >> x;
                const auto sols = DecomposeHomographyMat(H, K);
                std::printf("H %zu\n", sols.size());
                for (const auto& m : sols) {
                    for (double x : m.R) std::printf("%.17g ", x);
                    for (double x : m.t) std::printf("%.17g ", x);
                    for (double x : m.n) std::printf("%.17g ", x);
                    std::printf("\n");
                }
            } else if (kind == "R") {
                Mat3 R;
                for (double& x : R) std::cin >> x;
                const Vec3 r = RodriguesFromMatrix(R);
                std::printf("R %.17g %.17g %.17g\n", r[0], r[1], r[2]);
            } else {
                Mat3 E, R1, R2;
                Vec3 t;
                for (double& x : E) std::cin >> x;
                DecomposeEssentialMat(E, R1, R2, t);
                std::printf("E\n");
                for (double x : R1) std::printf("%.17g ", x);
                for (double x : R2) std::printf("%.17g ", x);
                for (double x : t) std::printf("%.17g ", x);
                std::printf("\n");
            }
        }
        return 0;
    }
    if (argc < 4) return 2;
    std::ifstream in(argv[2], std::ios::binary);
    std::ofstream out(argv[3], std::ios::binary);
    if (!strcmp(argv[1], "iters")) {   // count, count x (p, ep, m, maxIters) as doubles -> count results
        int32_t count;
        in.read((char*)&count, sizeof(count));
        const auto a = rd<double>(in, 4 * (size_t)count);
        std::vector<int32_t> res(count);
        for (int k = 0; k < count; ++k) res[k] = twoview_detail::ransac_update_num_iters(a[4 * k], a[4 * k + 1], (int)a[4 * k + 2], (int)a[4 * k + 3]);
        wr(out, res);
        std::printf("twoview driver ok\n");
        return 0;
    }
    if (!strcmp(argv[1], "refit")) {   // records of n, uv1, uv2, mask (n bytes; n = 0 bytes when the record says so) -> ok, H
        for (;;) {
            int32_t n, nmask;
            if (!in.read((char*)&n, sizeof(n))) break;
            in.read((char*)&nmask, sizeof(nmask));
            const auto uv1 = rd<double>(in, 2 * (size_t)n), uv2 = rd<double>(in, 2 * (size_t)n);
            const auto mask = rd<uint8_t>(in, (size_t)nmask);
            Mat3 H{};
            const bool ok = RefitHomography(uv1, uv2, mask, H);
            std::vector<double> res{(double)ok};
            res.insert(res.end(), H.begin(), H.end());
            wr(out, res);
        }
        std::printf("twoview driver ok\n");
        return 0;
    }
    Context ctx(0);
    if (!strcmp(argv[1], "pnp")) {   // n, object (n x 3), image (n x 2), K9 -> ok, iterations, R, rvec, t, inliers
        for (;;) {
            int32_t n;
            if (!in.read((char*)&n, sizeof(n))) break;
            // n = -1: 8 doubles (n, sampling 0 OpenCV / 1 counter / 2 given, seed, iterations, reprojection error, confidence, number of
            // given samples, 0), the given samples (5 indices each), then the record; the output gains the samples drawn and the winner
            const bool ext = n < 0;
            std::vector<double> par{0, 0, 5, 10000, 4.0, 0.999, 0, 0};
            std::vector<int32_t> given;
            if (ext) {
                par = rd<double>(in, 8);
                n = (int32_t)par[0];
                given = rd<int32_t>(in, 5 * (size_t)par[6]);
            }
            const auto obj = rd<double>(in, 3 * (size_t)n), img = rd<double>(in, 2 * (size_t)n), K9 = rd<double>(in, 9);
            PnPTrace trace;
            const PnPResult r = SolvePnPRansac(ctx, obj, img, K9.data(), (int)par[3], (float)par[4], par[5], (uint64_t)par[2], sampling_of(par[1]),
                                               &trace, par[1] == 2.0 ? &given : nullptr);
            std::vector<double> pose{(double)r.ok, (double)r.iterations};
            pose.insert(pose.end(), r.R.begin(), r.R.end());
            pose.insert(pose.end(), r.rvec.begin(), r.rvec.end());
            pose.insert(pose.end(), r.t.begin(), r.t.end());
            wr(out, pose);
            wr(out, std::vector<int32_t>(r.inliers.begin(), r.inliers.end()));
            if (ext) {
                wr(out, trace.samples);
                wr(out, std::vector<double>{(double)trace.winner});
            }
        }
        std::printf("twoview driver ok\n");
        return 0;
    }
    for (;;) {   // one scene per record (a general one: E branch, a planar one: H branch, ...)
        int32_t n;
        if (!in.read((char*)&n, sizeof(n))) break;
        // n = -1: 12 doubles (n, sampling 0 OpenCV / 1 counter / 2 given, seed, E maxIters, E confidence, H maxIters, H confidence,
        // recoverPose's distance threshold, its mask 0 E's / 1 none / 2 all zero, number of given E samples, of given H samples, 0),
        // the given samples (5 resp. 4 indices each), then the record; the output gains the traces (see below)
        const bool ext = n < 0;
        std::vector<double> par{0, 0, 7, 1000, 0.99, 100, 0.999, 50.0, 0, 0, 0, 0};
        std::vector<int32_t> givenE, givenH;
        if (ext) {
            par = rd<double>(in, 12);
            n = (int32_t)par[0];
            givenE = rd<int32_t>(in, 5 * (size_t)par[9]);
            givenH = rd<int32_t>(in, 4 * (size_t)par[10]);
        }
        const bool given = par[1] == 2.0;
        const auto uv1 = rd<double>(in, 2 * (size_t)n), uv2 = rd<double>(in, 2 * (size_t)n), K9 = rd<double>(in, 9);
        const double K4[4] = {K9[0], K9[4], K9[2], K9[5]};
        LmedsTrace Et, Ht;
        const RobustModel Em = FindEssentialMat(ctx, uv1, uv2, K4, (int)par[3], (uint64_t)par[2], par[4], sampling_of(par[1]), &Et, given ? &givenE : nullptr);
        const RobustModel Hm = FindHomography(ctx, uv1, uv2, (int)par[5], (uint64_t)par[2], par[6], sampling_of(par[1]), &Ht, given ? &givenH : nullptr);
        if (ext) {   // (a record of its own layout: a failed estimate has no mask to hand on and no model to decompose)
            std::vector<double> meta{(double)Em.ok, (double)Em.inliers, (double)Em.median, (double)Hm.ok, (double)Hm.inliers, (double)Hm.median,
                                     (double)Em.iterations, (double)Hm.iterations};
            wr(out, meta);
            wr(out, std::vector<double>(Em.model.begin(), Em.model.end()));
            wr(out, std::vector<double>(Hm.model.begin(), Hm.model.end()));
            wr(out, Em.mask);
            wr(out, Hm.mask);
            wr(out, Et.samples);
            wr(out, Ht.samples);
            wr(out, std::vector<double>{(double)Et.candidates, (double)Et.candidate, (double)Et.sample, (double)Et.root, Et.sigma, (double)Et.threshold,
                                        (double)Ht.candidates, (double)Ht.candidate, (double)Ht.sample, (double)Ht.root, Ht.sigma, (double)Ht.threshold});
            wr(out, std::vector<double>(Ht.winner.begin(), Ht.winner.end()));
            std::vector<double> pose, dec;
            std::vector<uint8_t> pmask;
            if (Em.ok) {
                Mat3 R1, R2;
                Vec3 t;
                DecomposeEssentialMat(Em.model, R1, R2, t);
                dec.insert(dec.end(), R1.begin(), R1.end());
                dec.insert(dec.end(), R2.begin(), R2.end());
                dec.insert(dec.end(), t.begin(), t.end());
                const std::vector<uint8_t> none(n, 0);
                const RecoveredPose rp = RecoverPose(ctx, Em.model, uv1, uv2, K9.data(), par[7], par[8] == 0.0 ? &Em.mask : par[8] == 2.0 ? &none : nullptr);
                pose.assign(rp.R.begin(), rp.R.end());
                pose.insert(pose.end(), rp.t.begin(), rp.t.end());
                pose.push_back(rp.good);
                pmask = rp.mask;
            }
            wr(out, dec);
            wr(out, pose);
            wr(out, pmask);
            continue;
        }
        std::vector<double> meta{(double)Em.ok, (double)Em.inliers, (double)Em.median, (double)Hm.ok, (double)Hm.inliers, (double)Hm.median,
                                 (double)Em.iterations, (double)Hm.iterations};
        wr(out, meta);
        wr(out, std::vector<double>(Em.model.begin(), Em.model.end()));
        wr(out, std::vector<double>(Hm.model.begin(), Hm.model.end()));
        wr(out, Em.mask);
        wr(out, Hm.mask);
        const RecoveredPose rp = RecoverPose(ctx, Em.model, uv1, uv2, K9.data(), 50.0, &Em.mask);
        std::vector<double> pose(rp.R.begin(), rp.R.end());
        pose.insert(pose.end(), rp.t.begin(), rp.t.end());
        pose.push_back(rp.good);
        wr(out, pose);
        // the homography branch of RecoverPoseTwoView (:92-150): decompose, triangulate every match under each solution, best count
        const auto sols = DecomposeHomographyMat(Hm.model, K9.data());
        std::vector<double> T;
        for (const auto& m : sols) {
            const double M[16] = {m.R[0], m.R[1], m.R[2], m.t[0], m.R[3], m.R[4], m.R[5], m.t[1], m.R[6], m.R[7], m.R[8], m.t[2], 0, 0, 0, 1};
            T.insert(T.end(), M, M + 16);
        }
        const auto tv = TwoViewPoints(ctx, uv1, uv2, K9.data(), T, 4.0f, 0.0174533f, true);
        const int best = BestTwoViewSolution(tv);
        std::vector<double> hb{(double)sols.size(), (double)best};
        for (const auto& s : tv) hb.push_back((double)s.matches.size());
        for (const auto& m : sols) {
            hb.insert(hb.end(), m.R.begin(), m.R.end());
            hb.insert(hb.end(), m.t.begin(), m.t.end());
        }
        wr(out, hb);
    }
    std::printf("twoview driver ok\n");
    return 0;
}
