// graph_verify_host.cpp — the host half of verifying a match graph through eacham_lmeds_batch, as a C++ caller does it
// (ReconstructionManagerHip::RecoverPoseTwoViewBatch): walk the matches and gather (uv1, uv2) per pair, draw every pair's minimal
// samples with twoview_detail::lmeds_samples, pack both into the wire form of eacham_lmeds_batch. tools/graph_verify_rate.py compiles
// this into a shared object with g++ and times it as part of the host composition.
#include <cstdint>
#include <vector>

#include "eacham/TwoViewHip.hpp"

extern "C" long long gv_host_pack(int npairs, const int32_t* pairs, const int32_t* counts, const int64_t* offsets, const uint32_t* q, const uint32_t* t,
                                  const int64_t* kp_offsets, const double* xy, int m, int homography, int sampling, int iterations, const uint64_t* seeds,
                                  int64_t* point_ptr, double* a, double* b, int64_t* sample_ptr, int32_t* idx) {
    using namespace eacham::hip;
    int64_t np = 0, ns = 0;
    point_ptr[0] = sample_ptr[0] = 0;
    std::vector<double> uv1, uv2;
    for (int p = 0; p < npairs; ++p) {
        const int n = counts[p];
        const double *x1 = xy + 2 * kp_offsets[pairs[2 * p]], *x2 = xy + 2 * kp_offsets[pairs[2 * p + 1]];
        uv1.resize(2 * (size_t)n), uv2.resize(2 * (size_t)n);
        for (int i = 0; i < n; ++i) {
            const size_t k1 = q[offsets[p] + i], k2 = t[offsets[p] + i];
            uv1[2 * i] = x1[2 * k1], uv1[2 * i + 1] = x1[2 * k1 + 1];
            uv2[2 * i] = x2[2 * k2], uv2[2 * i + 1] = x2[2 * k2 + 1];
        }
        std::copy(uv1.begin(), uv1.end(), a + 2 * np);
        std::copy(uv2.begin(), uv2.end(), b + 2 * np);
        np += n;
        if (n >= m && iterations > 0) {
            const std::vector<int32_t> s = twoview_detail::lmeds_samples(n, m, iterations, homography != 0, uv1, uv2, seeds ? seeds[p] : 12345,
                                                                         sampling ? Sampling::Counter : Sampling::OpenCV);
            std::copy(s.begin(), s.end(), idx + ns * m);
            ns += (int64_t)(s.size() / m);
        }
        point_ptr[p + 1] = np;
        sample_ptr[p + 1] = ns;
    }
    return ns;
}
