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
//                               against the threshold: the mask bytes and the inlier count (score_dev.hpp: block_count).
// The offset-table checks of the entry point keep their own wording ("not monotone", one message for both tables) and their own
// order, so they are not pnp_batch.hip's check_table; the sample indices go through check_sample_idx (solve_launch.hpp).
#include "context.hpp"
#include "devprim.hpp"
#include "score_dev.hpp"
#include "solve_launch.hpp"

#include <climits>

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
    double K[4] = {1, 1, 0, 0};
    if (Kdev) {
#pragma unroll
        for (int k = 0; k < 4; ++k) K[k] = Kdev[k];
    }
    float* erow = rows ? rows + (size_t)blockIdx.x * row_stride : nullptr;
    const int ncand = *total;
    for (int c = blockIdx.x; c < ncand; c += gridDim.x) {   // (c, and every barrier below, is uniform over the workgroup)
        const int s = prim::segment_of(first, n_samples, c);
        const long long base = point_ptr[sample_problem[s]];
        const int n = (int)(point_ptr[sample_problem[s] + 1] - base);   // >= m: the sample was solved
        const double* pm = models + 9 * ((size_t)s * max_models + (c - first[s]));
        const double* pa = a + 2 * base;
        const double* pb = b + 2 * base;
        double M[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) M[k] = pm[k];
        const bool keys_in_lds = n <= SC_MAX_LDS;
        for (int i = threadIdx.x; i < n; i += SC_BLOCK) {
            const double xa[2] = {pa[2 * (size_t)i], pa[2 * (size_t)i + 1]}, xb[2] = {pb[2 * (size_t)i], pb[2 * (size_t)i + 1]};
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
    const long long base = point_ptr[p];
    const int n = (int)(point_ptr[p + 1] - base);
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
    double M[9], K[4] = {1, 1, 0, 0};
    float thr = 0.f;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = 0.0;
    if (!none) {
        s = prim::segment_of(first, n_samples, best.at);
        const double* pm = models + 9 * ((size_t)s * max_models + (best.at - first[s]));
#pragma unroll
        for (int k = 0; k < 9; ++k) M[k] = pm[k];
        const double sigma = lmeds_sigma(best.med, n, m);
        thr = (float)__dmul_rn(sigma, sigma);
        if (Kdev) {
#pragma unroll
            for (int k = 0; k < 4; ++k) K[k] = Kdev[k];
        }
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) out_models[9 * (size_t)p + k] = M[k];
        out_medians[p] = none ? __uint_as_float(0x7fc00000u) : best.med;
        out_thresholds[p] = thr;
        out_winner[3 * (size_t)p] = none ? -1 : best.at - c0;
        out_winner[3 * (size_t)p + 1] = none ? -1 : s - (int)s0;
        out_winner[3 * (size_t)p + 2] = none ? -1 : best.at - first[s];
        out_ncand[p] = c1 - c0;
    }
    const double* pa = a + 2 * base;
    const double* pb = b + 2 * base;
    int cnt = 0;
    for (int i = threadIdx.x; i < n; i += SC_BLOCK) {
        unsigned char in = 0;
        if (!none) {
            const double xa[2] = {pa[2 * (size_t)i], pa[2 * (size_t)i + 1]}, xb[2] = {pb[2 * (size_t)i], pb[2 * (size_t)i + 1]};
            in = score_one<KIND>(xa, xb, M, K, normalise != 0) <= thr;
        }
        out_masks[base + i] = in;
        cnt += in;
    }
    const int tot = block_count(cnt, wsum);
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
    const int P = L.P, maxm = solve_max_models(L.kind);
    const long long S = L.S, max_n = L.max_n;
    const bool need_rows = lmeds_needs_rows(max_n);
    const double* d_K = L.has_K ? L.K : nullptr;
    const int normalise = L.has_K && L.kind == EACHAM_SOLVE_ESSENTIAL5 ? 1 : 0;
    ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
    if (S > 0) {
        solve_minimal_launch(st, MinimalLaunch{L.kind, SolveSeg{L.point_ptr, L.sample_ptr, P, L.sample_problem}, L.a, L.b, L.K, L.has_K, (int)S, L.sample_idx,
                                               L.cand_models, L.n_models});
    }
    prim::exclusive_scan<int>(st, L.n_models, L.first, (int)S, L.scan_ws, L.total);   // (no samples: *total = 0)
    const size_t smem = sizeof(unsigned) * (size_t)std::max<long long>(1, std::min<long long>(max_n, SC_MAX_LDS));
#define EACHAM_LB_LAUNCH(KIND)                                                                                                                     \
    do {                                                                                                                                           \
        if (S > 0) {                                                                                                                               \
            if (smem > 48 * 1024)                                                                                                                  \
                EACHAM_HIP_TRY(ctx, hipFuncSetAttribute((const void*)lb_score_kernel<KIND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)); \
            lb_score_kernel<KIND><<<L.score_grid, SC_BLOCK, smem, st>>>(L.point_ptr, L.a, L.b, d_K, normalise, (int)S, L.first, L.total,           \
                                                                        L.sample_problem, L.cand_models, maxm, L.cand_medians,                     \
                                                                        need_rows ? L.rows : nullptr, (size_t)max_n);                              \
        }                                                                                                                                          \
        lb_select_kernel<KIND><<<P, SC_BLOCK, 0, st>>>(L.point_ptr, L.sample_ptr, L.a, L.b, d_K, normalise, (int)S, L.first, L.total,              \
                                                       L.cand_models, maxm, L.cand_medians, L.models, L.medians, L.thresholds, L.inliers,          \
                                                       L.masks, L.winner, L.n_candidates);                                                         \
    } while (0)
    if (L.kind == EACHAM_SOLVE_ESSENTIAL5) EACHAM_LB_LAUNCH(0);
    else if (L.kind == EACHAM_SOLVE_FUNDAMENTAL7) EACHAM_LB_LAUNCH(3);
    else EACHAM_LB_LAUNCH(1);
#undef EACHAM_LB_LAUNCH
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
    if (kind != EACHAM_SOLVE_HOMOGRAPHY4 && kind != EACHAM_SOLVE_ESSENTIAL5 && kind != EACHAM_SOLVE_FUNDAMENTAL7)
        return ctx->fail(EACHAM_ERR_INVALID, "lmeds_batch: unknown kind %d", kind);
    if (n_problems < 0) return ctx->fail(EACHAM_ERR_INVALID, "lmeds_batch: negative number of problems");
    if (n_problems == 0) return EACHAM_OK;
    if (!point_ptr || !sample_ptr) return ctx->fail(EACHAM_ERR_INVALID, "lmeds_batch: null offset table");
    const int P = n_problems, m = solve_sample_size(kind), maxm = solve_max_models(kind);
    if (point_ptr[0] != 0 || sample_ptr[0] != 0) return ctx->fail(EACHAM_ERR_INVALID, "lmeds_batch: an offset table does not start at 0");
    for (int p = 0; p < P; ++p)
        if (point_ptr[p + 1] < point_ptr[p] || sample_ptr[p + 1] < sample_ptr[p])
            return ctx->fail(EACHAM_ERR_INVALID, "lmeds_batch: problem %d: offset table not monotone", p);
    const long long NP = point_ptr[P], S = sample_ptr[P];
    if (NP > INT_MAX / 2 || S * m > INT_MAX || S * maxm > INT_MAX) return ctx->fail(EACHAM_ERR_CAPACITY, "lmeds_batch: %lld points / %lld samples in one call", NP, S);
    if ((NP > 0 && (!a || !b)) || (S > 0 && !sample_idx)) return ctx->fail(EACHAM_ERR_INVALID, "lmeds_batch: null array");
    long long max_n = 0;
    for (int p = 0; p < P; ++p) {
        const long long n = point_ptr[p + 1] - point_ptr[p];
        if (n < m) continue;   // its samples are not looked at: the problem gets the "none" record
        max_n = std::max(max_n, n);
        if (int rc = check_sample_idx(ctx, "lmeds_batch", p, sample_idx + sample_ptr[p] * m, (sample_ptr[p + 1] - sample_ptr[p]) * m, n)) return rc;
    }
    EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool need_rows = lmeds_needs_rows(max_n);
    const long long cand_cap = S * maxm;
    const int score_grid = lmeds_score_grid(cand_cap, max_n);
    hipStream_t st = ctx->stream;
    IoStage io(ctx, st);
    const auto h_om = io.out<double>(models, 9 * (size_t)P);
    const auto h_omed = io.out<float>(medians, (size_t)P), h_othr = io.out<float>(thresholds, (size_t)P);
    const auto h_oinl = io.out<int>(inliers, (size_t)P), h_owin = io.out<int>(winner, 3 * (size_t)P), h_onc = io.out<int>(n_candidates, (size_t)P);
    const auto h_omask = io.out<unsigned char>(masks, (size_t)NP);
    const auto h_pp = io.in<long long>(point_ptr, (size_t)P + 1), h_sp = io.in<long long>(sample_ptr, (size_t)P + 1);
    const auto h_K = io.in<double>(K, 4);
    const auto h_a = io.in<double>(a, 2 * (size_t)NP), h_b = io.in<double>(b, 2 * (size_t)NP);
    const auto h_i = io.in<int>(sample_idx, (size_t)S * m);
    const auto h_m = io.scratch<double>(9 * (size_t)cand_cap);
    const auto h_n = io.scratch<int>((size_t)S), h_first = io.scratch<int>((size_t)S), h_sprob = io.scratch<int>((size_t)S);
    const auto h_tot = io.scratch<int>(1), h_ws = io.scratch<int>(prim::scan_ws_elems((size_t)S));
    const auto h_cmed = io.scratch<float>((size_t)cand_cap);
    const auto h_rows = io.scratch<float>(need_rows ? (size_t)score_grid * (size_t)max_n : 0);
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    const LmedsLaunch L{kind, P, S, max_n, score_grid, d(h_pp), d(h_sp), d(h_a), d(h_b), d(h_K), K != nullptr, d(h_i),
                        d(h_m), d(h_n), d(h_first), d(h_sprob), d(h_tot), d(h_ws), d(h_cmed), d(h_rows),
                        d(h_om), d(h_omed), d(h_othr), d(h_oinl), d(h_omask), d(h_owin), d(h_onc)};
    if (int rc = lmeds_launch(ctx, st, L)) return rc;
    return io.finish();
}
