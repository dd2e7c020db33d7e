// solve_launch.hpp — the minimal-solver kernels of solve.hip as the other translation units launch them: every stage is ONE kernel
// template with a one-problem and a list instantiation, and eacham_solve_minimal / eacham_solve_pnp (solve.hip), lmeds_launch
// (lmeds_batch.hip) and eacham_pnp_hypotheses_batch (pnp_batch.hip) go through the two functions below on device pointers.
#pragma once

#include "context.hpp"

namespace eacham {

// Where a sample's points are. point_ptr == nullptr: ONE problem, every sample indexes a / b (obj / img) as given. Else the list
// form: sample s belongs to the problem p with sample_ptr[p] <= s < sample_ptr[p + 1] (left in sample_problem[s] for the later
// stages), its indices count from point_ptr[p], and a problem with fewer points than a sample has is not solved (n_models = 0).
struct SolveSeg {
    const long long *point_ptr, *sample_ptr;
    int n_problems;
    int* sample_problem;
};

// A minimal sample's points and the models it can give, per kind (EACHAM_SOLVE_*): homography 4 / 1, essential 5 / 10, fundamental 7 / 3.
inline int solve_sample_size(int kind) { return kind == EACHAM_SOLVE_HOMOGRAPHY4 ? 4 : (kind == EACHAM_SOLVE_FUNDAMENTAL7 ? 7 : 5); }
inline int solve_max_models(int kind) { return kind == EACHAM_SOLVE_HOMOGRAPHY4 ? 1 : (kind == EACHAM_SOLVE_FUNDAMENTAL7 ? 3 : 10); }

// Every minimal sample -> its model(s): models [n_samples][1, 10 or 3][9], n_models [n_samples] (kind: EACHAM_SOLVE_*).
struct MinimalLaunch {
    int kind;
    SolveSeg seg;
    const double *a, *b, *K;   // K: device copy of fx fy cx cy, read when has_K
    bool has_K;
    int n_samples;             // > 0
    const int* sample_idx;
    double* models;
    int* n_models;
};
void solve_minimal_launch(hipStream_t st, const MinimalLaunch& L);

// EPnP on samples of 5..64 points, front and back half: tmp [3][n_samples][13] = error (< 0: no pose) and pose of each linearised
// start; frame = PNP_FRAME x n_samples doubles of scratch between the two launches.
struct PnpLaunch {
    SolveSeg seg;
    const double *obj, *img, *K;
    int sample_size, n_samples;   // n_samples > 0
    const int* sample_idx;
    double *frame, *tmp;
};
void solve_pnp_launch(hipStream_t st, const PnpLaunch& L);

// Every one of `count` sample indices lies in 0 .. n - 1 (problem < 0: a one-problem call, its message names no problem).
inline int check_sample_idx(eacham_ctx* ctx, const char* call, int problem, const int32_t* idx, long long count, long long n) {
    for (long long k = 0; k < count; ++k)
        if (idx[k] < 0 || idx[k] >= n) {
            if (problem < 0) return ctx->fail(EACHAM_ERR_INVALID, "%s: sample index %d of %lld points", call, (int)idx[k], n);
            return ctx->fail(EACHAM_ERR_INVALID, "%s: problem %d: sample index %d of %lld points", call, problem, (int)idx[k], n);
        }
    return EACHAM_OK;
}

}  // namespace eacham
