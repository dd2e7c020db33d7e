// ransac_launch.hpp — threshold RANSAC as the translation units share it: ransac_batch.hip defines the launch sequence, its host-pointer
// entry and eacham_graph_verify_ransac (graph_verify.hip) stage its arrays and call it. lmeds_launch.hpp is its LMedS counterpart.
#pragma once

#include "context.hpp"
#include "devprim.hpp"
#include "solve_launch.hpp"

namespace eacham {

// ransac_batch.hip: the launch sequence of eacham_ransac_batch on device pointers — threshold RANSAC in two passes. Pass 1 solves and
// counts ranks < stage1 of every problem, the rule (ransac_rule.hpp) gives every problem's budget so far, pass 2 solves and counts
// ranks stage1 .. budget - 1 (its sample list is built on the device, its total read back once through total2_host), the rule runs
// over everything solved, the winner's model, mask and count are written. single: stage1 covers every problem's samples, pass 1
// reads sample_ptr / sample_idx as they are and there is no pass 2 and no read-back. The host-pointer entry and
// eacham_graph_verify_ransac (graph_verify.hip) both call it. Pass 2's scratch is ctx->ws, sized after the read-back.
struct RansacLaunch {
    int kind, P;                 // EACHAM_SOLVE_*, problems (> 0)
    long long S1;                // samples of pass 1: sum of min(S_p, stage1), or sample_ptr[P] when single
    int stage1;                  // > 0
    bool single;
    float threshold;
    const long long *point_ptr, *sample_ptr;
    const double *a, *b;
    CallK K;
    const int* sample_idx;
    const int *tab_off, *table;  // problem p's budget row begins at table[tab_off[p]] (ransac_budget_row; unread for a problem below m points)
    // scratch of pass 1: P + 1 three times, scan_ws_elems(P + 1); S1 x m (unless single), 9 x S1 x maxm, S1 x 3, 1, scan_ws_elems(S1), S1 x maxm
    long long *sp1, *sp2, *stage_cnt, *stage_ws;
    int* idx1;
    double* cand1;
    int *n_models1, *first1, *sample_problem1, *total1, *scan_ws1, *counts1;
    int *budget, *win_at;        // P, 2 x P: the winner's pass (0 / 1, -1 none) and its place in that pass's candidate list
    long long *total2, *total2_host;   // pass 2's samples on the device, and the pinned word it is read back through
    // results, per problem (masks: per point, in the layout of a / b)
    double* models;
    int* inliers;
    unsigned char* masks;
    int *winner, *n_candidates, *n_used;
    bool s1_known = true;        // false: S1 is an upper bound (the scratch's size), the pass's total is read back like pass 2's
};
// pass 1's scratch as both callers stage it (six arrays of the call's IoStage), and its hand-over to the launch
struct RansacScratch {
    IoArray<long long> ll;   // sp1, sp2, stage_cnt: 3 x (P + 1), then the scan's workspace
    IoArray<int> idx1, per_sample, per_cand, per_problem;
    IoArray<double> cand;
    size_t P, S1, maxm, ws_ll;
    RansacScratch(IoStage& io, int P_, long long S1_, int m, int maxm_, bool single) : P((size_t)P_), S1((size_t)S1_), maxm((size_t)maxm_) {
        ws_ll = prim::scan_ws_elems(P + 1);
        ll = io.scratch<long long>(3 * (P + 1) + ws_ll);
        idx1 = io.scratch<int>(single ? 0 : S1 * m);
        cand = io.scratch<double>(9 * S1 * maxm);
        per_sample = io.scratch<int>(3 * S1 + 1 + prim::scan_ws_elems(S1));   // n_models, first, sample_problem, total, the scan's workspace
        per_cand = io.scratch<int>(S1 * maxm);
        per_problem = io.scratch<int>(3 * P);
    }
    void bind(RansacLaunch& L, const IoDev& d) const {
        L.sp1 = d(ll), L.sp2 = L.sp1 + P + 1, L.stage_cnt = L.sp2 + P + 1, L.stage_ws = L.stage_cnt + P + 1;
        L.idx1 = d(idx1), L.cand1 = d(cand);
        L.n_models1 = d(per_sample), L.first1 = L.n_models1 + S1, L.sample_problem1 = L.first1 + S1, L.total1 = L.sample_problem1 + S1, L.scan_ws1 = L.total1 + 1;
        L.counts1 = d(per_cand);
        L.budget = d(per_problem), L.win_at = L.budget + P;
    }
};
int ransac_default_stage1();
int ransac_launch(eacham_ctx* ctx, hipStream_t st, const RansacLaunch& L);
// the budget rows of a call, one per distinct n >= m: rows appended to `table`, tab_off[p] set (0 for a problem below m points); the host
// time it takes is left in ctx->ransac_table_ms
void ransac_build_table(eacham_ctx* ctx, double confidence, int m, int cap, const int* n_of, int P, std::vector<int>& tab_off, std::vector<int>& table);

}  // namespace eacham
