// lmeds_batch.hip — LMedS two-view estimation for a whole LIST of pairs in one call (eacham_lmeds_batch), gfx950.
//
// What twoview_detail::lmeds (include/eacham/TwoViewHip.hpp) does for one pair with three blocking calls — solve every minimal
// sample, score every candidate's median, keep the first smallest, derive the threshold from sigma, classify the points by the
// winner — runs here for n_problems pairs with no host turn between the stages: the inputs go up once, the results come back
// once, and the number of launches does not depend on n_problems.
//
//   solve_minimal_launch        (solve.hip, through solve_launch.hpp) the list instantiation of solve_h4_kernel / solve_e5_kernel / solve_f7_kernel — the
//                               kernels eacham_solve_minimal launches, not a copy of them: a wave per sample on the sample's own
//                               problem, found by a binary search in sample_ptr (and left in sample_problem[] for the stages below);
//                               a problem with fewer points than a minimal sample has no candidates
//   prim::exclusive_scan        of n_models over all samples (devprim.hpp: one launch up to 16 384 samples, three beyond): candidate c
//                               of the flattened list (sample order, then root order) is root c - first[s] of the sample s with
//                               first[s] <= c < first[s + 1] — the models stay where the solver wrote them, nothing is copied
//   lb_score<KIND>              a workgroup per candidate over its own problem's points: score_one, the key transform and the radix
//                               select of score_kernel (score_dev.hpp: block_median), so the medians are the same bits. The number of candidates
//                               is only known on the device: a fixed grid strides over them. Keys live in LDS up to SC_MAX_LDS
//                               points (dynamic LDS sized by the largest problem of the call) and in the workgroup's own error row
//                               beyond it.
//   lb_select<KIND>             a workgroup per problem: first smallest non-NaN median (strict < over ascending candidate index),
//                               sigma and the threshold in fp64 in the host's order of operations, then the winner's errors
//                               against the threshold: the mask bytes and the inlier count (estimator_dev.hpp: classify_winner, the
//                               tail rb_finish of ransac_batch.hip runs too).
// The launch struct and the scratch's staging are lmeds_launch.hpp's. The entry's checks and input staging are the ones
// eacham_ransac_batch makes (solve_launch.hpp: check_list_call, ListCall): they keep their own wording ("not monotone", one
// message for both tables) and their own order, so they are not pnp_batch.hip's check_table, whose messages its tests hold.
#include "estimator_dev.hpp"
#include "lmeds_launch.hpp"

namespace eacham {
namespace {

// KIND 0 = essential (Sampson distance, fp64), 1 = homography (transfer error, fp32), 3 = fundamental (the larger epipolar-line
// distance, fp64, K ignored): score_one's kinds.
// first[s] = candidates before sample s (the exclusive scan of n_models), *total = all of them; max_models = 10 / 1 / 3.
template <int KIND>
__global__ __launch_bounds__(SC_BLOCK) void lb_score_kernel(const long long* __restrict__ point_ptr, const double* __restrict__ a,
                                                            const double* __restrict__ b, const double* __restrict__ Kdev, int normalise,
                                                            int n_samples, const int* __restrict__ first, const int* __restrict__ total,
                                                            const int* __restrict__ sample_problem, const double* __restrict__ models,
                                                            int max_models, float* __restrict__ medians, float* __restrict__ rows,
                                                            size_t row_stride) {
    extern __shared__ unsigned keys[];  // [min(largest problem, SC_MAX_LDS)]
    __shared__ unsigned hist[256], sh[2];
    double K[4];
    load_K(Kdev, K);
    float* erow = rows ? rows + (size_t)blockIdx.x * row_stride : nullptr;
    const int ncand = *total;
    for (int c = blockIdx.x; c < ncand; c += gridDim.x) {   // (c, and every barrier below, is uniform over the workgroup)
        const Candidate cand(first, n_samples, models, max_models, c);
        const Points q(point_ptr, a, b, sample_problem[cand.s]);
        const int n = q.n;
        double M[9];
        cand.load(M);
        const bool keys_in_lds = n <= SC_MAX_LDS;
        for (int i = threadIdx.x; i < n; i += SC_BLOCK) {
            const double xa[2] = {q.pa[2 * (size_t)i], q.pa[2 * (size_t)i + 1]}, xb[2] = {q.pb[2 * (size_t)i], q.pb[2 * (size_t)i + 1]};
            const float e = score_one<KIND>(xa, xb, M, K, normalise != 0);
            if (keys_in_lds) keys[i] = fkey(e);
            else erow[i] = e;
        }
        __syncthreads();  // keys / the error row are complete (the row was written by this workgroup: visible after the barrier)
        const float med = block_median([&](int i) { return keys_in_lds ? keys[i] : fkey(erow[i]); }, n, hist, sh);
        if (threadIdx.x == 0) medians[c] = med;
        // (radix_select ends on a barrier: every read of this candidate's keys is done before the next one's are written)
    }
}

// sigma of LMeDSPointSetRegistrator::run as the host evaluates `std::max(2.5 * 1.4826 * (1.0 + 5.0 / std::max(n - m, 1)) *
// std::sqrt((double)median), 0.001)`: the constant product folded, then left to right, every operation rounded on its own.
__device__ __forceinline__ double lmeds_sigma(float median, int n, int m) {
    const int d = n - m > 1 ? n - m : 1;
    const double f = __dadd_rn(1.0, __ddiv_rn(5.0, (double)d));
    const double s = __dmul_rn(__dmul_rn(2.5 * 1.4826, f), __dsqrt_rn((double)median));
    return s < 0.001 ? 0.001 : s;
}

struct Best {
    float med;
    int at;   // candidate index in the call's flattened list, -1 = none yet
};
// `o` replaces `b` iff it holds a candidate and b does not, or its median is smaller, or equal with the smaller index
__device__ __forceinline__ Best first_smallest(Best b, Best o) {
    const bool take = o.at >= 0 && (b.at < 0 || o.med < b.med || (o.med == b.med && o.at < b.at));
    return take ? o : b;
}

template <int KIND>
__global__ __launch_bounds__(SC_BLOCK) void lb_select_kernel(const long long* __restrict__ point_ptr, const long long* __restrict__ sample_ptr,
                                                             const double* __restrict__ a, const double* __restrict__ b,
                                                             const double* __restrict__ Kdev, int normalise, int n_samples,
                                                             const int* __restrict__ first, const int* __restrict__ total,
                                                             const double* __restrict__ models, int max_models, const float* __restrict__ cmed,
                                                             double* __restrict__ out_models, float* __restrict__ out_medians,
                                                             float* __restrict__ out_thresholds, int* __restrict__ out_inliers,
                                                             unsigned char* __restrict__ out_masks, int* __restrict__ out_winner,
                                                             int* __restrict__ out_ncand) {
    constexpr int m = KIND == 0 ? 5 : (KIND == 3 ? 7 : 4);
    __shared__ Best wbest[SC_BLOCK / 64];
    __shared__ int wsum[SC_BLOCK / 64];
    const int p = blockIdx.x;
    const Points q(point_ptr, a, b, p);
    const long long s0 = sample_ptr[p], s1 = sample_ptr[p + 1];
    const int c0 = s0 < n_samples ? first[s0] : *total, c1 = s1 < n_samples ? first[s1] : *total;
    Best best{0.f, -1};
    for (int c = c0 + (int)threadIdx.x; c < c1; c += SC_BLOCK) {   // ascending in every thread: strict < keeps the first
        const float v = cmed[c];
        if (v == v && (best.at < 0 || v < best.med)) best = Best{v, c};
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Best o;
        o.med = __shfl_down(best.med, off);
        o.at = __shfl_down(best.at, off);
        best = first_smallest(best, o);
    }
    if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
    __syncthreads();
    best = wbest[0];
#pragma unroll
    for (int w = 1; w < SC_BLOCK / 64; ++w) best = first_smallest(best, wbest[w]);   // (every thread: the same values)
    const bool none = best.at < 0;
    const double* pm = nullptr;
    float thr = 0.f;
    int s = 0;
    if (!none) {
        const Candidate w(first, n_samples, models, max_models, best.at);
        s = w.s, pm = w.pm;
        const double sigma = lmeds_sigma(best.med, q.n, m);
        thr = (float)__dmul_rn(sigma, sigma);
    }
    if (threadIdx.x == 0) {
        out_medians[p] = none ? __uint_as_float(0x7fc00000u) : best.med;
        out_thresholds[p] = thr;
        out_winner[3 * (size_t)p] = none ? -1 : best.at - c0;
        out_winner[3 * (size_t)p + 1] = none ? -1 : s - (int)s0;
        out_winner[3 * (size_t)p + 2] = none ? -1 : best.at - first[s];
        out_ncand[p] = c1 - c0;
    }
    const int tot = classify_winner<KIND>(pm, Kdev, normalise, q, thr, out_models + 9 * (size_t)p, out_masks, wsum);
    if (threadIdx.x == 0) out_inliers[p] = tot;
}

constexpr int LB_SCORE_GRID = 4096;      // workgroups striding over the candidates (~2 resident rounds of 256 CUs x 8)
constexpr int LB_SCORE_GRID_ROWS = 1024; // ... when each carries an error row of the largest problem (> SC_MAX_LDS points)

}  // namespace

bool lmeds_needs_rows(long long max_n) { return max_n > SC_MAX_LDS; }
int lmeds_score_grid(long long cand_cap, long long max_n) {
    return (int)std::max<long long>(1, std::min<long long>(cand_cap, lmeds_needs_rows(max_n) ? LB_SCORE_GRID_ROWS : LB_SCORE_GRID));
}

int lmeds_launch(eacham_ctx* ctx, hipStream_t st, const LmedsLaunch& L) {
    const int P = L.P, S = (int)L.S, maxm = solve_max_models(L.kind), normalise = L.K.normalise(L.kind);
    const double* d_K = L.K.scorer();
    ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
    if (S > 0) {
        solve_minimal_launch(st, MinimalLaunch{L.kind, SolveSeg{L.point_ptr, L.sample_ptr, P, L.sample_problem}, L.a, L.b, L.K.dev, L.K.given, S, L.sample_idx,
                                               L.cand_models, L.n_models});
    }
    prim::exclusive_scan<int>(st, L.n_models, L.first, S, L.scan_ws, L.total);   // (no samples: *total = 0)
    const size_t smem = sizeof(unsigned) * (size_t)std::max<long long>(1, std::min<long long>(L.max_n, SC_MAX_LDS));
    if (int rc = with_solve_kind(L.kind, [&](auto k) -> int {
            constexpr int KIND = decltype(k)::SCORE;
            if (S > 0) {
                if (smem > 48 * 1024)
                    EACHAM_HIP_TRY(ctx, hipFuncSetAttribute((const void*)lb_score_kernel<KIND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
                lb_score_kernel<KIND><<<L.score_grid, SC_BLOCK, smem, st>>>(L.point_ptr, L.a, L.b, d_K, normalise, S, L.first, L.total, L.sample_problem,
                                                                            L.cand_models, maxm, L.cand_medians,
                                                                            lmeds_needs_rows(L.max_n) ? L.rows : nullptr, (size_t)L.max_n);
            }
            lb_select_kernel<KIND><<<P, SC_BLOCK, 0, st>>>(L.point_ptr, L.sample_ptr, L.a, L.b, d_K, normalise, S, L.first, L.total, L.cand_models, maxm,
                                                           L.cand_medians, L.models, L.medians, L.thresholds, L.inliers, L.masks, L.winner,
                                                           L.n_candidates);
            return EACHAM_OK;
        }))
        return rc;
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return EACHAM_OK;
}

}  // namespace eacham

using namespace eacham;

extern "C" int eacham_lmeds_batch(eacham_ctx* ctx, int kind, int n_problems, const int64_t* point_ptr, const double* a, const double* b,
                                  const double* K, const int64_t* sample_ptr, const int32_t* sample_idx, double* models, float* medians,
                                  float* thresholds, int32_t* inliers, uint8_t* masks, int32_t* winner, int32_t* n_candidates) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    ListCall c;
    if (int rc = check_solve_kind(ctx, "lmeds_batch", kind)) return rc;
    if (int rc = check_list_call(ctx, "lmeds_batch", kind, n_problems, point_ptr, sample_ptr, a, b, sample_idx, c)) return rc;
    if (n_problems == 0) return EACHAM_OK;
    const int P = n_problems, m = solve_sample_size(kind);
    EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    IoStage io(ctx, st);
    const auto h_om = io.out<double>(models, 9 * (size_t)P);
    const auto h_omed = io.out<float>(medians, (size_t)P), h_othr = io.out<float>(thresholds, (size_t)P);
    const auto h_oinl = io.out<int>(inliers, (size_t)P), h_owin = io.out<int>(winner, 3 * (size_t)P), h_onc = io.out<int>(n_candidates, (size_t)P);
    const auto h_omask = io.out<unsigned char>(masks, (size_t)c.NP);
    c.stage_tables(io, P, point_ptr, sample_ptr, K);
    c.stage_points(io, m, a, b, sample_idx);
    const LmedsScratch sc(io, c.S, solve_max_models(kind), c.max_n);
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    LmedsLaunch L{kind, P, c.S, c.max_n, d(c.point_ptr), d(c.sample_ptr), d(c.a), d(c.b), CallK{d(c.K), K != nullptr}, d(c.sample_idx)};
    sc.bind(L, d);
    L.models = d(h_om), L.medians = d(h_omed), L.thresholds = d(h_othr), L.inliers = d(h_oinl), L.masks = d(h_omask), L.winner = d(h_owin), L.n_candidates = d(h_onc);
    if (int rc = lmeds_launch(ctx, st, L)) return rc;
    return io.finish();
}
