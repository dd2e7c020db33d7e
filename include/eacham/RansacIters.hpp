// RansacIters.hpp — RANSACUpdateNumIters, on its own so that the library's host code (csrc/ransac_rule.hpp builds the budget rows of
// eacham_ransac_batch with it) and the adapters (TwoViewHip.hpp, PnPHip.hpp, GraphVerifyHip.hpp) evaluate the SAME function.
#pragma once

#include <algorithm>
#include <cmath>
#include <limits>

namespace eacham {
namespace hip {
namespace twoview_detail {

// RANSACUpdateNumIters (ptsetreg.cpp): iterations after which a sample of m inliers has been drawn with probability p at
// outlier ratio ep, capped by maxIters
inline int ransac_update_num_iters(double p, double ep, int m, int maxIters) {
    p = std::min(std::max(p, 0.0), 1.0);
    ep = std::min(std::max(ep, 0.0), 1.0);
    const double num = std::max(1.0 - p, std::numeric_limits<double>::min());
    const double denom = 1.0 - std::pow(1.0 - ep, m);
    if (denom < std::numeric_limits<double>::min()) return 0;
    const double ln = std::log(num), ld = std::log(denom);
    return ld >= 0 || -ln >= maxIters * (-ld) ? maxIters : (int)std::lround(ln / ld);
}

}  // namespace twoview_detail
}  // namespace hip
}  // namespace eacham
