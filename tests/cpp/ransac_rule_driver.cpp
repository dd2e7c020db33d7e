// ransac_rule_driver.cpp — eacham_amd/csrc/ransac_rule.hpp on the host, judged by tests/test_ransac_reference.py (no GPU, no library).
//   ransac_rule_driver row <confidence> <n> <m> <cap>     -> the budget row ransac_budget_row builds, n + 1 integers on one line
//   ransac_rule_driver fuzz <seed> <trials>               -> random count sequences (samples with 0 .. max_models roots): the table walk,
//                                                            the order-free form and the two-pass use of the walk against the sequential
//                                                            loop that calls ransac_update_num_iters itself; one summary line, exit 1 on
//                                                            any difference
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../eacham_amd/csrc/ransac_rule.hpp"

using eacham::RansacPick;

struct Seq {
    std::vector<int> first, counts;   // roots of sample s: counts[first[s] .. first[s + 1])
    int roots(int s) const { return first[s + 1] - first[s]; }
    int count(int s, int r) const { return counts[first[s] + r]; }
};

// RANSACPointSetRegistrator::run on the counts, the budget by the function itself
static RansacPick loop(const Seq& q, int S, int n, int m, double confidence) {
    RansacPick r{S, 0, 0, m - 1, -1, -1, -1};
    int best = -1, s = 0;
    for (; s < r.budget; ++s) {
        for (int j = 0; j < q.roots(s); ++j) {
            const int c = q.count(s, j);
            if (c > std::max(best, m - 1)) {
                best = c, r.best = c, r.candidate = r.n_candidates + j, r.sample = s, r.root = j;
                r.budget = eacham::hip::twoview_detail::ransac_update_num_iters(confidence, (double)(n - c) / n, m, r.budget);
            }
        }
        r.n_candidates += q.roots(s);
    }
    r.n_used = s;
    return r;
}

// The same decisions in the order-free form, a second statement the walk is held to: M_s = the largest count of
// sample s, P_s = the largest M before s floored at m - 1; sample s is reached iff s < (P_s > m - 1 ? min(S, B[P_s]) : S); the reached samples are a prefix (B is non-increasing);
// the winner is the first candidate with the largest count of that prefix, if that count exceeds m - 1.
template <class Src>
static RansacPick rule_prefix(int S, int m, const int* B, const Src& src) {
    RansacPick r{S, 0, 0, m - 1, -1, -1, -1};
    int P = m - 1, reached = 0;
    for (int s = 0; s < S; ++s) {   // (every test below reads only counts of samples before s: the tests are independent of each other)
        const int lim = P > m - 1 ? (B[P] < S ? B[P] : S) : S;
        if (s < lim) reached = s + 1;
        for (int j = 0, k = src.roots(s); j < k; ++j)
            if (src.count(s, j) > P) P = src.count(s, j);
    }
    for (int s = 0; s < reached; ++s) {
        const int k = src.roots(s);
        for (int j = 0; j < k; ++j)
            if (src.count(s, j) > r.best) r.best = src.count(s, j), r.candidate = r.n_candidates + j, r.sample = s, r.root = j;
        r.n_candidates += k;
    }
    r.n_used = reached;
    r.budget = r.best > m - 1 ? (B[r.best] < S ? B[r.best] : S) : S;
    return r;
}

static bool same(const RansacPick& a, const RansacPick& b) {
    return a.budget == b.budget && a.n_used == b.n_used && a.n_candidates == b.n_candidates && a.best == b.best && a.candidate == b.candidate &&
           a.sample == b.sample && a.root == b.root;
}

int main(int argc, char** argv) {
    if (argc == 6 && !std::strcmp(argv[1], "row")) {
        const int n = std::atoi(argv[3]), m = std::atoi(argv[4]), cap = std::atoi(argv[5]);
        std::vector<int> B((size_t)n + 1);
        eacham::ransac_budget_row(std::atof(argv[2]), n, m, cap, B.data());
        for (int g = 0; g <= n; ++g) std::printf("%d%c", B[g], g == n ? '\n' : ' ');
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "fuzz")) {
        std::mt19937_64 rng(std::strtoull(argv[2], nullptr, 10));
        const int trials = std::atoi(argv[3]);
        const int ms[3] = {4, 5, 7}, maxms[3] = {1, 10, 3}, ns[6] = {0, 8, 31, 64, 257, 300};
        const double confs[3] = {0.99, 0.995, 0.999};
        long long bad = 0, multi = 0, early = 0, late_root = 0;
        auto pick = [&](int k) { return (int)(rng() % (unsigned long long)k); };
        for (int t = 0; t < trials; ++t) {
            const int k = pick(3), m = ms[k], maxm = maxms[k];
            int n = ns[pick(6)];
            if (n == 0) n = m;
            const double confidence = confs[pick(3)];
            const int S = pick(4) == 0 ? pick(4) : 1 + pick(80);
            // counts that climb: mostly poor candidates, now and then one near the best so far or above it
            Seq q;
            q.first.push_back(0);
            int top = pick(n + 1) / 4;
            bool several = false;
            for (int s = 0; s < S; ++s) {
                const int roots = pick(5) == 0 ? 0 : 1 + pick(maxm);
                several |= roots > 1;
                for (int j = 0; j < roots; ++j) {
                    int c = pick(top + 1);
                    const int kind = pick(8);
                    if (kind == 0) c = std::min(n, top + 1 + pick(1 + (n - top) / 3)), top = std::max(top, c);
                    else if (kind == 1) c = top;
                    q.counts.push_back(c);
                }
                q.first.push_back((int)q.counts.size());
            }
            std::vector<int> B((size_t)n + 1);
            eacham::ransac_budget_row(confidence, n, m, std::max(S, 1), B.data());
            const RansacPick want = loop(q, S, n, m, confidence);
            bool ok = same(eacham::ransac_rule_walk(S, S, m, B.data(), q), want) && same(rule_prefix(S, m, B.data(), q), want);
            const int stages[5] = {1, 3, 16, 1 + pick(S + 1), S + 1};
            for (int stage1 : stages) {   // pass 1 = ranks < stage1, pass 2 = ranks .. budget1 - 1, then the walk over what exists
                const int c1 = std::min(S, stage1);
                const int budget1 = eacham::ransac_rule_walk(S, c1, m, B.data(), q).budget;
                ok = ok && same(eacham::ransac_rule_walk(S, std::max(c1, budget1), m, B.data(), q), want);
            }
            bad += !ok;
            multi += several;
            early += want.n_used < S;
            late_root += want.root > 0 && want.budget < want.sample + 1;
        }
        std::printf("{\"trials\": %d, \"mismatches\": %lld, \"multi_root\": %lld, \"early_stop\": %lld, \"late_root_past_budget\": %lld}\n", trials, bad, multi,
                    early, late_root);
        return bad ? 1 : 0;
    }
    std::fprintf(stderr, "usage: ransac_rule_driver row <confidence> <n> <m> <cap> | fuzz <seed> <trials>\n");
    return 2;
}
