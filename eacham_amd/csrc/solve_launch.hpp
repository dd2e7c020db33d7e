// solve_launch.hpp — the minimal-solver kernels of solve.hip as the other translation units launch them: every stage is ONE kernel
// template with a one-problem and a list instantiation, and eacham_solve_minimal / eacham_solve_pnp (solve.hip), lmeds_launch
// (lmeds_batch.hip), rb_pass (ransac_batch.hip) and eacham_pnp_hypotheses_batch (pnp_batch.hip) go through the two functions below on
// device pointers. With them, what the estimators above the solver share on the host: the kind dispatcher (with_solve_kind), the
// call's K (CallK), the entry check and input staging of the two two-view list calls (check_list_call, ListCall) and of the two PnP
// hypotheses calls (PnpHypCall, with the PnP calls' table check, check_table).
#pragma once

#include "context.hpp"

#include <climits>

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
// f(SolveKind<...>{}) for a checked two-view kind: what the estimators' kernel templates take — M the sample size, SCORE score_one's
// KIND, CHECK the checkSubset of the OpenCV sample stream (graph_verify.hip). Returns what f returns.
template <int M_, int SCORE_, int CHECK_>
struct SolveKind { static constexpr int M = M_, SCORE = SCORE_, CHECK = CHECK_; };
template <class F>
inline auto with_solve_kind(int kind, F&& f) {
    if (kind == EACHAM_SOLVE_HOMOGRAPHY4) return f(SolveKind<4, 1, 1>{});
    if (kind == EACHAM_SOLVE_FUNDAMENTAL7) return f(SolveKind<7, 3, 2>{});
    return f(SolveKind<5, 0, 0>{});
}
// The call's K as the estimators carry it: the staged copy of fx fy cx cy (always there) and whether the caller gave one. The solver
// takes both; the scorer a null pointer for "none", and normalises the points only for the essential kind.
struct CallK {
    const double* dev;
    bool given;
    const double* scorer() const { return given ? dev : nullptr; }
    int normalise(int kind) const { return given && kind == EACHAM_SOLVE_ESSENTIAL5 ? 1 : 0; }
};

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

inline int check_solve_kind(eacham_ctx* ctx, const char* call, int kind) {
    if (kind == EACHAM_SOLVE_HOMOGRAPHY4 || kind == EACHAM_SOLVE_ESSENTIAL5 || kind == EACHAM_SOLVE_FUNDAMENTAL7) return EACHAM_OK;
    return ctx->fail(EACHAM_ERR_INVALID, "%s: unknown kind %d", call, kind);
}

// The lists of eacham_lmeds_batch / eacham_ransac_batch: what check_list_call learns of them, and their six input arrays on the call's
// IoStage, declared in the order they always were — the tables and K, (the entry's own small inputs,) the points and the sample indices.
struct ListCall {
    long long NP = 0, S = 0;          // points and samples of the whole call
    long long max_n = 0, max_S = 0;   // the largest problem with at least a minimal sample's worth of points; the most samples of any
    IoArray<long long> point_ptr, sample_ptr;
    IoArray<double> K, a, b;
    IoArray<int> sample_idx;
    void stage_tables(IoStage& io, int P, const int64_t* pp, const int64_t* sp, const double* K_) {
        point_ptr = io.in<long long>(pp, (size_t)P + 1), sample_ptr = io.in<long long>(sp, (size_t)P + 1), K = io.in<double>(K_, 4);
    }
    void stage_points(IoStage& io, int m, const double* a_, const double* b_, const int32_t* idx) {
        a = io.in<double>(a_, 2 * (size_t)NP), b = io.in<double>(b_, 2 * (size_t)NP), sample_idx = io.in<int>(idx, (size_t)S * m);
    }
};
// The checks both entries make of their lists, in their order and wording (kind: checked, by check_solve_kind ahead of the entry's own
// scalar checks). No problems: EACHAM_OK before any table is looked at, and nothing else for the entry to do.
inline int check_list_call(eacham_ctx* ctx, const char* call, int kind, int n_problems, const int64_t* point_ptr, const int64_t* sample_ptr,
                           const double* a, const double* b, const int32_t* sample_idx, ListCall& c, std::vector<int>* n_of = nullptr) {
    if (n_problems < 0) return ctx->fail(EACHAM_ERR_INVALID, "%s: negative number of problems", call);
    if (n_problems == 0) return EACHAM_OK;
    if (!point_ptr || !sample_ptr) return ctx->fail(EACHAM_ERR_INVALID, "%s: null offset table", call);
    const int P = n_problems, m = solve_sample_size(kind), maxm = solve_max_models(kind);
    if (point_ptr[0] != 0 || sample_ptr[0] != 0) return ctx->fail(EACHAM_ERR_INVALID, "%s: an offset table does not start at 0", call);
    for (int p = 0; p < P; ++p)
        if (point_ptr[p + 1] < point_ptr[p] || sample_ptr[p + 1] < sample_ptr[p])
            return ctx->fail(EACHAM_ERR_INVALID, "%s: problem %d: offset table not monotone", call, p);
    c.NP = point_ptr[P], c.S = sample_ptr[P];
    if (c.NP > INT_MAX / 2 || c.S * m > INT_MAX || c.S * maxm > INT_MAX)
        return ctx->fail(EACHAM_ERR_CAPACITY, "%s: %lld points / %lld samples in one call", call, c.NP, c.S);
    if ((c.NP > 0 && (!a || !b)) || (c.S > 0 && !sample_idx)) return ctx->fail(EACHAM_ERR_INVALID, "%s: null array", call);
    if (n_of) n_of->resize((size_t)P);
    for (int p = 0; p < P; ++p) {
        const long long n = point_ptr[p + 1] - point_ptr[p], Sp = sample_ptr[p + 1] - sample_ptr[p];
        if (n_of) (*n_of)[p] = (int)n;
        c.max_S = std::max(c.max_S, Sp);
        if (n < m) continue;   // its samples are not looked at: the problem gets the "none" record
        c.max_n = std::max(c.max_n, n);
        if (int rc = check_sample_idx(ctx, call, p, sample_idx + sample_ptr[p] * m, Sp * m, n)) return rc;
    }
    return EACHAM_OK;
}

// One offset table of a PnP list call (eacham_pnp_hypotheses_batch[_p3p], eacham_pnp_refit_batch): given, from 0, never decreasing, its
// end within an int.
inline int check_table(eacham_ctx* ctx, const char* call, const char* what, int n_problems, const int64_t* ptr) {
    if (!ptr) return ctx->fail(EACHAM_ERR_INVALID, "%s: null %s", call, what);
    if (ptr[0] != 0) return ctx->fail(EACHAM_ERR_INVALID, "%s: %s does not start at 0", call, what);
    for (int p = 0; p < n_problems; ++p)
        if (ptr[p + 1] < ptr[p]) return ctx->fail(EACHAM_ERR_INVALID, "%s: problem %d: %s decreases", call, p, what);
    if (ptr[n_problems] > INT_MAX) return ctx->fail(EACHAM_ERR_CAPACITY, "%s: %s ends at %lld: more than 2^31 - 1 in one call", call, what, (long long)ptr[n_problems]);
    return EACHAM_OK;
}

// eacham_pnp_hypotheses_batch / eacham_pnp_hypotheses_batch_p3p from the tables on: the caller's arguments (P > 0 problems, samples of m
// points: the entry's own checks come first), check() — the tables, the null arrays, every sample index of a problem that has a
// sample's worth of points, in that order and wording; it leaves the totals NP and S — and stage(): the nine arrays on the call's
// IoStage in the order they always were, the three results, the tables and K, the points, the sample indices.
struct PnpHypCall {
    int P, m;
    const int64_t* point_ptr;
    const double *obj, *img, *K;
    const int64_t* sample_ptr;
    const int32_t* sample_idx;
    double* models;   // may be null (not wanted)
    int32_t *n_models, *counts;
    long long NP = 0, S = 0;   // points and samples of the whole call
    IoArray<double> h_m, h_K, h_a, h_b;
    IoArray<int> h_n, h_c, h_i;
    IoArray<long long> h_pp, h_sp;
    int check(eacham_ctx* ctx, const char* call) {
        if (int rc = check_table(ctx, call, "point_ptr", P, point_ptr)) return rc;
        if (int rc = check_table(ctx, call, "sample_ptr", P, sample_ptr)) return rc;
        NP = point_ptr[P], S = sample_ptr[P];
        if (!K || (NP > 0 && (!obj || !img)) || (S > 0 && (!sample_idx || !n_models || !counts)))
            return ctx->fail(EACHAM_ERR_INVALID, "%s: null array", call);
        for (int p = 0; p < P; ++p) {
            const long long n = point_ptr[p + 1] - point_ptr[p];
            if (n < m) continue;   // its samples are not looked at: each gets n_models = 0
            if (int rc = check_sample_idx(ctx, call, p, sample_idx + sample_ptr[p] * m, (sample_ptr[p + 1] - sample_ptr[p]) * m, n)) return rc;
        }
        return EACHAM_OK;
    }
    void stage(IoStage& io) {
        h_m = io.out<double>(models, models ? 12 * (size_t)S : 0);
        h_n = io.out<int>(n_models, (size_t)S), h_c = io.out<int>(counts, (size_t)S);
        h_pp = io.in<long long>(point_ptr, (size_t)P + 1), h_sp = io.in<long long>(sample_ptr, (size_t)P + 1);
        h_K = io.in<double>(K, 4);
        h_a = io.in<double>(obj, 3 * (size_t)NP), h_b = io.in<double>(img, 2 * (size_t)NP);
        h_i = io.in<int>(sample_idx, (size_t)S * m);
    }
};

}  // namespace eacham
