// ransac_rule.hpp — the selection rule of threshold RANSAC (RANSACPointSetRegistrator::run) on inlier counts that are already
// there, as the device (ransac_batch.hip: rb_rule_kernel) and the host (tests/cpp/ransac_rule_driver.cpp) both run it.
//
// The sequential statement, per problem of n points, sample size m and S samples in order:
//     budget = S, best = m - 1;  for s = 0, 1, .. while s < budget:  for every root r of sample s, in root order:
//         if count(s, r) > best:  best = count, winner = (s, r), budget = ransac_update_num_iters(confidence, (n - count) / n, m, budget)
// ransac_update_num_iters (include/eacham/RansacIters.hpp) is pow, log and lround: the host's libm decides, never the device's. The
// device sees the function only as the integer row B[g] = ransac_update_num_iters(confidence, (double)(n - g) / n, m, cap), g = 0 .. n,
// that ransac_budget_row builds on the host with that function, for a cap no smaller than any budget of the call. Two facts carry it
// (tests/test_ransac_reference.py holds both on the rows this file builds):
//     ransac_update_num_iters(confidence, (n - g) / n, m, cur) == min(cur, B[g])  for every cur <= cap,      B is non-increasing in g.
// With the row the walk below is integer-only. The budget is tested per SAMPLE: a record in root 0 that drops the budget below s + 1
// does not keep the later roots of sample s from being counted, and they may win.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EACHAM_RULE_HD __host__ __device__
#else
#define EACHAM_RULE_HD
#endif

#include "../../include/eacham/RansacIters.hpp"

namespace eacham {

struct RansacPick {
    int budget;        // the sample budget when the walk ended
    int n_used;        // samples whose roots were looked at
    int n_candidates;  // candidates of those samples
    int best;          // the winner's count (m - 1: no record)
    int candidate, sample, root;   // the winner: its place among the consumed samples' candidates, its sample, its root (-1 -1 -1: none)
};

// Src: roots(s) = candidates of sample s, count(s, r) = inliers of root r of sample s. `avail`: the samples whose counts exist (the
// walk ends there at the latest; after every stage of ransac_launch avail covers the budget, so the final walk is the full rule).
template <class Src>
EACHAM_RULE_HD inline RansacPick ransac_rule_walk(int S, int avail, int m, const int* B /* [n + 1] */, const Src& src) {
    RansacPick r{S, 0, 0, m - 1, -1, -1, -1};
    int s = 0;
    for (; s < r.budget && s < avail; ++s) {
        const int k = src.roots(s);
        for (int j = 0; j < k; ++j) {
            const int c = src.count(s, j);
            if (c > r.best) {   // strictly more: the earlier candidate stays
                r.best = c, r.candidate = r.n_candidates + j, r.sample = s, r.root = j;
                const int b = B[c];
                if (b < r.budget) r.budget = b;
            }
        }
        r.n_candidates += k;
    }
    r.n_used = s;
    return r;
}

// B[g], g = 0 .. n, by the host's ransac_update_num_iters (n > 0).
inline void ransac_budget_row(double confidence, int n, int m, int cap, int* B) {
    for (int g = 0; g <= n; ++g) B[g] = hip::twoview_detail::ransac_update_num_iters(confidence, (double)(n - g) / n, m, cap);
}

}  // namespace eacham
