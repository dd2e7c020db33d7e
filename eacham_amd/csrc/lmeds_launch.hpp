// lmeds_launch.hpp — LMedS as the translation units share it, the counterpart of ransac_launch.hpp: lmeds_batch.hip defines the
// launch sequence, its host-pointer entry and eacham_graph_verify (graph_verify.hip) stage its arrays and call it.
#pragma once

#include "context.hpp"
#include "devprim.hpp"
#include "solve_launch.hpp"

namespace eacham {

// lmeds_batch.hip: the launch sequence of eacham_lmeds_batch on device pointers — solve every sample, scan the root counts, score
// every candidate (keys in LDS up to SC_MAX_LDS points, in error rows beyond, by max_n), select per problem. S = the samples
// sample_ptr[P] names; the scratch arrays may be larger.
struct LmedsLaunch {
    int kind, P;                 // EACHAM_SOLVE_*, problems (> 0)
    long long S, max_n;          // samples in this call; the largest problem with at least a minimal sample's worth of points
    const long long *point_ptr, *sample_ptr;
    const double *a, *b;
    CallK K;
    const int* sample_idx;
    // scratch (LmedsScratch): 9 x S x maxm, S, S, S, 1, scan_ws_elems(S), S x maxm, need_rows ? score_grid x max_n : 0
    int score_grid;              // lmeds_score_grid(...): the workgroups of the scorer, and the rows `rows` holds beyond SC_MAX_LDS
    double* cand_models;
    int *n_models, *first, *sample_problem, *total, *scan_ws;
    float *cand_medians, *rows;
    // results, per problem (masks: per point, in the layout of a / b)
    double* models;
    float *medians, *thresholds;
    int* inliers;
    unsigned char* masks;
    int *winner, *n_candidates;
};
int lmeds_score_grid(long long cand_cap, long long max_n);
bool lmeds_needs_rows(long long max_n);
int lmeds_launch(eacham_ctx* ctx, hipStream_t st, const LmedsLaunch& L);

// the scratch as both callers stage it (eight arrays of the call's IoStage, sized by the sample bound S_cap), and its hand-over
struct LmedsScratch {
    IoArray<double> cand;
    IoArray<int> n_models, first, sample_problem, total, scan_ws;
    IoArray<float> cand_medians, rows;
    int score_grid;
    LmedsScratch(IoStage& io, long long S_cap, int maxm, long long max_n) : score_grid(lmeds_score_grid(S_cap * maxm, max_n)) {
        const size_t S = (size_t)S_cap, cand_cap = S * (size_t)maxm;
        cand = io.scratch<double>(9 * cand_cap);
        n_models = io.scratch<int>(S), first = io.scratch<int>(S), sample_problem = io.scratch<int>(S);
        total = io.scratch<int>(1), scan_ws = io.scratch<int>(prim::scan_ws_elems(S));
        cand_medians = io.scratch<float>(cand_cap);
        rows = io.scratch<float>(lmeds_needs_rows(max_n) ? (size_t)score_grid * (size_t)max_n : 0);
    }
    void bind(LmedsLaunch& L, const IoDev& d) const {
        L.score_grid = score_grid, L.cand_models = d(cand);
        L.n_models = d(n_models), L.first = d(first), L.sample_problem = d(sample_problem), L.total = d(total), L.scan_ws = d(scan_ws);
        L.cand_medians = d(cand_medians), L.rows = d(rows);
    }
};

}  // namespace eacham
