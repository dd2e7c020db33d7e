// CvSampling.hpp — the SAMPLE STREAM of OpenCV's robust estimators, restated.
//
// cv::findEssentialMat / cv::findHomography (cv::LMEDS) and cv::solvePnPRansac, as the reference calls them
// (/root/reference/modules/sfm/reconstruction/ReconstructionManager.cpp:57-61, :75, :227-228), draw their minimal samples
// inside LMeDSPointSetRegistrator::run / RANSACPointSetRegistrator::run (OpenCV 4.5.5, modules/calib3d/src/ptsetreg.cpp):
//   * both seed a fresh generator per call:          RNG rng((uint64)-1);
//   * cv::RNG is a multiply-with-carry generator:    state = (uint64)(unsigned)state * 4164903690U + (unsigned)(state >> 32);
//                                                    next() = (unsigned)state;   uniform(a, b) = a + next() % (b - a)
//   * getSubset draws modelPoints indices one by one with rng.uniform(0, count), drawing again while the index repeats one
//     already in the subset; the finished subset goes through the callback's checkSubset and is drawn afresh when that
//     refuses it (at most 1000 attempts under LMedS, 10 000 under RANSAC). Of the reference's calls only
//     HomographyEstimatorCallback has a checkSubset (fundam.cpp): the last point must not be collinear with any two earlier
//     ones, in either image, and the four correspondences must keep their orientation (the sign test of Marquez-Neila et al.).
//     FMEstimatorCallback (cv::findFundamentalMat, the library's uncalibrated kind) has the collinearity half alone.
// OpenCV is not in this image and none of it could be run here: everything above is written FROM MEMORY of the 4.5.5 sources
// and is unverified ("parity unpinned", like the rest of the estimators). What it buys is that the documented deviation
// "the samples come from the library's own counter-based generator" is gone by default: with OpenCV at hand, E / H / the PnP
// pose can be compared model for model. tests/test_cv_sampling.py pins the generator's first draws against an independent
// statement of the recurrence.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

// The streams below are stated ONCE for the host and for the kernels that draw on the device (eacham_amd/csrc/graph_verify.hip):
// EACHAM_HD marks what both compile; the unroll hint lets the 4 - 7 indices of a subset stay in registers there.
#if defined(__HIPCC__)
#define EACHAM_HD __host__ __device__
#define EACHAM_UNROLL _Pragma("unroll")
#else
#define EACHAM_HD
#define EACHAM_UNROLL
#endif

namespace eacham {
namespace hip {

enum class Sampling {
    OpenCV,   // cv::RNG((uint64)-1) + getSubset (+ checkSubset for the homography): the default
    Counter   // the counter-based generator of rounds 1-3 (splitmix64 of (seed, sample, draw)), seeded by the caller
};

struct CvRNG {   // cv::RNG (core/include/opencv2/core.hpp, core/operations.hpp)
    uint64_t state;
    EACHAM_HD explicit CvRNG(uint64_t s = 0xffffffffu) : state(s ? s : 0xffffffffu) {}
    EACHAM_HD unsigned next() {
        state = (uint64_t)(unsigned)state * 4164903690u + (unsigned)(state >> 32);
        return (unsigned)state;
    }
    EACHAM_HD int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a) + a); }
};

namespace cvsampling_detail {

// haveCollinearPoints (fundam.cpp): only the LAST point of the subset is tested against the lines through two earlier ones
EACHAM_HD inline bool have_collinear_points(const float* p /* count x 2 */, int count) {
    const int i = count - 1;
    EACHAM_UNROLL
    for (int j = 0; j < i; ++j) {
        const double dx1 = p[2 * j] - p[2 * i], dy1 = p[2 * j + 1] - p[2 * i + 1];   // (float differences, widened)
        EACHAM_UNROLL
        for (int k = 0; k < j; ++k) {
            const double dx2 = p[2 * k] - p[2 * i], dy2 = p[2 * k + 1] - p[2 * i + 1];
            if (std::fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (std::fabs(dx1) + std::fabs(dy1) + std::fabs(dx2) + std::fabs(dy2))) return true;
        }
    }
    return false;
}
EACHAM_HD inline double det3(const double* m) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

}  // namespace cvsampling_detail

// HomographyEstimatorCallback::checkSubset for a subset of `count` correspondences (src, dst: count x 2, cv::Point2f values)
EACHAM_HD inline bool cv_check_subset_homography(const float* src, const float* dst, int count) {
    using namespace cvsampling_detail;
    if (have_collinear_points(src, count) || have_collinear_points(dst, count)) return false;
    if (count == 4) {
        constexpr int tt[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
        int negative = 0;
        EACHAM_UNROLL
        for (int i = 0; i < 4; ++i) {
            const int* t = tt[i];
            const double A[9] = {src[2 * t[0]], src[2 * t[0] + 1], 1.0, src[2 * t[1]], src[2 * t[1] + 1], 1.0, src[2 * t[2]], src[2 * t[2] + 1], 1.0};
            const double B[9] = {dst[2 * t[0]], dst[2 * t[0] + 1], 1.0, dst[2 * t[1]], dst[2 * t[1] + 1], 1.0, dst[2 * t[2]], dst[2 * t[2] + 1], 1.0};
            negative += det3(A) * det3(B) < 0;
        }
        if (negative != 0 && negative != 4) return false;
    }
    return true;
}

// FMEstimatorCallback::checkSubset (fundam.cpp) for a subset of `count` correspondences: the last point must not be collinear with
// any two earlier ones, in either image. No orientation test.
EACHAM_HD inline bool cv_check_subset_fundamental(const float* src, const float* dst, int count) {
    using namespace cvsampling_detail;
    return !have_collinear_points(src, count) && !have_collinear_points(dst, count);
}

// One getSubset call: m distinct indices out of n into idx[0..m). `check(idx)` is the callback's checkSubset (may be empty).
// Returns false when maxAttempts subsets were refused (the registrator then stops: found == false).
template <class Check>
EACHAM_HD inline bool cv_get_subset(CvRNG& rng, int n, int m, int32_t* idx, int maxAttempts, Check check) {
    for (int iters = 0; iters < maxAttempts; ++iters) {
        EACHAM_UNROLL
        for (int i = 0; i < m; ++i) {
            int v = rng.uniform(0, n);
            for (;;) {
                bool dup = false;
                EACHAM_UNROLL
                for (int j = 0; j < i; ++j) dup = dup || idx[j] == v;
                if (!dup) break;
                v = rng.uniform(0, n);
            }
            idx[i] = v;
        }
        if (check(idx)) return true;
    }
    return false;
}

// ---- the library's counter-based stream (Sampling::Counter): splitmix64 of (seed, sample, draw) ----
EACHAM_HD inline uint64_t mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// sample number `sample` of the stream of `seed`: m distinct indices out of n (n >= m) into idx[0..m)
EACHAM_HD inline void counter_sample(int n, int m, uint64_t seed, int sample, int32_t* idx) {
    uint64_t ctr = 0;
    EACHAM_UNROLL
    for (int k = 0; k < m; ++k) {
        for (;;) {
            const int v = (int)(mix(seed * 0x100000001B3ull + ((uint64_t)sample << 20) + ctr++) % (uint64_t)n);
            bool dup = false;
            EACHAM_UNROLL
            for (int j = 0; j < k; ++j) dup = dup || idx[j] == v;
            if (!dup) {
                idx[k] = v;
                break;
            }
        }
    }
}

}  // namespace hip
}  // namespace eacham
