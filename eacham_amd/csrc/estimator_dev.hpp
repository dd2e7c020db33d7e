// estimator_dev.hpp — what the kernels of the robust two-view estimators (lmeds_batch.hip, ransac_batch.hip) share above the scorer:
// the call's K, a candidate of a flattened list, and the winner's tail (model, mask bytes, inlier count), each written once.
// It runs score_one: only translation units compiled with -ffp-contract=off (csrc/Makefile) may include it.
#pragma once

#include "devprim.hpp"
#include "score_dev.hpp"

namespace eacham {
namespace {

// fx fy cx cy as score_one reads them: the caller's four doubles, or {1, 1, 0, 0} when the call has none
__device__ __forceinline__ void load_K(const double* __restrict__ Kdev, double* K) {
    K[0] = K[1] = 1.0, K[2] = K[3] = 0.0;
    if (Kdev) {
#pragma unroll
        for (int k = 0; k < 4; ++k) K[k] = Kdev[k];
    }
}

// Candidate c of a flattened list (sample order, then root order): first[s] = candidates before sample s (the exclusive scan of
// n_models over the list's n_samples samples), the models where the solver wrote them — sample-major, max_models slots per sample.
struct Candidate {
    int s;              // its sample: first[s] <= c < first[s + 1]
    const double* pm;   // its model
    __device__ __forceinline__ Candidate(const int* __restrict__ first, int n_samples, const double* __restrict__ models, int max_models, int c)
        : s(prim::segment_of(first, n_samples, c)), pm(models + 9 * ((size_t)s * max_models + (c - first[s]))) {}
    __device__ __forceinline__ void load(double* M) const {
#pragma unroll
        for (int k = 0; k < 9; ++k) M[k] = pm[k];
    }
};
// The points of problem p (a candidate's: p = sample_problem[s], and n >= m since the sample was solved): where they begin, how many
struct Points {
    long long base;
    int n;
    const double *pa, *pb;
    __device__ __forceinline__ Points(const long long* __restrict__ point_ptr, const double* __restrict__ a, const double* __restrict__ b, int p)
        : base(point_ptr[p]), n((int)(point_ptr[p + 1] - base)), pa(a + 2 * base), pb(b + 2 * base) {}
};

// A workgroup of SC_BLOCK threads on a problem's points: the winner's model pm (null: no winner, zeros) to out_model, every point's
// `error <= thr` as its mask byte (no winner: 0), the inliers counted and returned to thread 0 (block_count: ends past a workgroup
// barrier; wsum: [SC_BLOCK / 64] LDS).
template <int KIND>
__device__ __forceinline__ int classify_winner(const double* __restrict__ pm, const double* __restrict__ Kdev, int normalise, const Points& q, float thr,
                                               double* __restrict__ out_model, unsigned char* __restrict__ out_masks, int* wsum) {
    const bool none = pm == nullptr;
    double M[9], K[4];
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = none ? 0.0 : pm[k];
    load_K(none ? nullptr : Kdev, K);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) out_model[k] = M[k];
    }
    int cnt = 0;
    for (int i = threadIdx.x; i < q.n; i += SC_BLOCK) {
        unsigned char in = 0;
        if (!none) {
            const double xa[2] = {q.pa[2 * (size_t)i], q.pa[2 * (size_t)i + 1]}, xb[2] = {q.pb[2 * (size_t)i], q.pb[2 * (size_t)i + 1]};
            in = score_one<KIND>(xa, xb, M, K, normalise != 0) <= thr;
        }
        out_masks[q.base + i] = in;
        cnt += in;
    }
    return block_count(cnt, wsum);
}

}  // namespace
}  // namespace eacham
