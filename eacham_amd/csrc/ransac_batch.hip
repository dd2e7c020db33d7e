// ransac_batch.hip — threshold RANSAC two-view estimation for a whole LIST of pairs in one call (eacham_ransac_batch), gfx950.
//
// RANSACPointSetRegistrator::run per problem — the candidate with the most errors <= threshold wins, the earlier one on ties, and
// every new record shrinks the sample budget by the confidence — as ransac_rule.hpp states it on integer counts and a host-built
// budget row (no device pow / log / lround decides anything). What eacham_lmeds_batch does for the median rule, with one more idea:
// the samples behind a problem's budget are never needed, so they are not solved.
//
//   rb_stage / prim::exclusive_scan / rb_compact   the sample list of a pass: pass 1 = ranks < stage1 of every problem, pass 2 = ranks
//                               stage1 .. budget1 - 1 (count, scan, compact — gv_compact_kernel's pattern); pass 2's total is read back once
//   solve_minimal_launch        (solve.hip, through solve_launch.hpp) the kernels eacham_solve_minimal launches, on the pass's list
//   prim::exclusive_scan        of n_models: the pass's flattened candidate list, as in lmeds_batch.hip
//   rb_count<KIND>              a WAVE per candidate over its own problem's points: score_one (score_dev.hpp), err <= threshold, a ballot's
//                               popcount per trip — lb_score without keys, LDS, error rows or the radix select, so without a size limit
//                               or a barrier. A fixed grid strides over the device-side candidate total.
//   rb_rule                     a thread per problem: ransac_rule_walk over the problem's samples in rank order, wherever a pass left
//                               them; after pass 1 it only leaves the budget, at the end the budget, n_used, the winner and n_candidates
//   rb_finish<KIND>             a workgroup per problem: the winner's place from win_at, then lb_select's tail (estimator_dev.hpp:
//                               classify_winner) — the winner's model, its errors against the threshold (the mask bytes), the count
// Pass 2 may solve samples the sequential loop would not reach (a record inside pass 2 shrinks the budget further): the rule only ever
// reads a prefix of what was solved, so every output is the same for every stage1.
// K, the candidate lookup and the kind dispatch are the shared ones (estimator_dev.hpp, solve_launch.hpp), and the entry's list checks
// and input staging are eacham_lmeds_batch's (check_list_call, ListCall) behind the rule's own scalar checks.
#include "estimator_dev.hpp"
#include "ransac_launch.hpp"
#include "ransac_rule.hpp"

#include <chrono>
#include <cmath>
#include <map>

namespace eacham {
namespace {

constexpr int RB = 256;
constexpr int RB_COUNT_GRID = 4096;   // workgroups of four waves striding over the candidates
constexpr int RB_STAGE1 = 128;        // the library's stage1 (where it was measured)

// What a pass left on the device. sp[p] .. sp[p + 1]: its samples of problem p, consecutive ranks; a null sp: the pass did not run.
struct RbPass {
    const long long* sp;
    const int *n_models, *first, *counts;
    const double* models;
};

// stage 1: problem p contributes its first min(S_p, stage1) samples; stage 2: ranks min(S_p, stage1) .. budget[p] - 1 (budget <= S_p)
__global__ __launch_bounds__(RB) void rb_stage_kernel(int P, const long long* __restrict__ sample_ptr, int stage1, const int* __restrict__ budget,
                                                      long long* __restrict__ cnt) {
    const int p = blockIdx.x * RB + threadIdx.x;
    if (p > P) return;
    long long c = 0;
    if (p < P) {
        const long long S = sample_ptr[p + 1] - sample_ptr[p], c1 = S < stage1 ? S : stage1;
        c = budget ? (budget[p] > c1 ? budget[p] - c1 : 0) : c1;
    }
    cnt[p] = c;   // (entry P = 0: the scan's last output is the total's place)
}

// local sample s of the pass (problem p, rank s - sp[p] + the ranks pass 1 took) -> its m indices
template <int M>
__global__ __launch_bounds__(RB) void rb_compact_kernel(int P, long long n, const long long* __restrict__ sp, const long long* __restrict__ sample_ptr,
                                                        int skip, const int* __restrict__ sample_idx, int* __restrict__ out) {
    const long long s = (long long)blockIdx.x * RB + threadIdx.x;
    if (s >= n) return;
    const int p = prim::segment_of(sp, P, s);
    const long long S = sample_ptr[p + 1] - sample_ptr[p];
    const long long src = sample_ptr[p] + (s - sp[p]) + (S < skip ? S : skip);
#pragma unroll
    for (int k = 0; k < M; ++k) out[s * M + k] = sample_idx[src * M + k];
}

template <int KIND>
__global__ __launch_bounds__(RB) void rb_count_kernel(const long long* __restrict__ point_ptr, const double* __restrict__ a, const double* __restrict__ b,
                                                      const double* __restrict__ Kdev, int normalise, int n_samples, const int* __restrict__ first,
                                                      const int* __restrict__ total, const int* __restrict__ sample_problem,
                                                      const double* __restrict__ models, int max_models, float thr, int* __restrict__ counts) {
    double K[4];
    load_K(Kdev, K);
    const int lane = threadIdx.x & 63, waves = RB / 64;
    const int ncand = *total;
    for (int c = blockIdx.x * waves + (threadIdx.x >> 6); c < ncand; c += gridDim.x * waves) {   // (c is uniform over the wave)
        const Candidate cand(first, n_samples, models, max_models, c);
        const Points q(point_ptr, a, b, sample_problem[cand.s]);
        double M[9];
        cand.load(M);
        int cnt = 0;
        for (int i0 = 0; i0 < q.n; i0 += 64) {
            const int i = i0 + lane;
            bool in = false;
            if (i < q.n) {
                const double xa[2] = {q.pa[2 * (size_t)i], q.pa[2 * (size_t)i + 1]}, xb[2] = {q.pb[2 * (size_t)i], q.pb[2 * (size_t)i + 1]};
                in = score_one<KIND>(xa, xb, M, K, normalise != 0) <= thr;
            }
            cnt += __popcll(__ballot(in));
        }
        if (lane == 0) counts[c] = cnt;
    }
}

struct RbSrc {
    RbPass p1, p2;
    long long s1, s2;   // where the problem's samples begin in each pass
    int c1;             // ranks pass 1 holds
    __device__ int roots(int s) const { return s < c1 ? p1.n_models[s1 + s] : p2.n_models[s2 + (s - c1)]; }
    __device__ int count(int s, int r) const { return s < c1 ? p1.counts[p1.first[s1 + s] + r] : p2.counts[p2.first[s2 + (s - c1)] + r]; }
};

// final == 0: after pass 1, only budget[p]. final != 0: everything.
__global__ __launch_bounds__(RB) void rb_rule_kernel(int P, int m, const long long* __restrict__ point_ptr, const long long* __restrict__ sample_ptr,
                                                     RbPass p1, RbPass p2, const int* __restrict__ tab_off, const int* __restrict__ table, int final,
                                                     int* __restrict__ budget, int* __restrict__ n_used, int* __restrict__ winner,
                                                     int* __restrict__ n_candidates, int* __restrict__ win_at) {
    const int p = blockIdx.x * RB + threadIdx.x;
    if (p >= P) return;
    const int n = (int)(point_ptr[p + 1] - point_ptr[p]), S = (int)(sample_ptr[p + 1] - sample_ptr[p]);
    RansacPick r{S, 0, 0, m - 1, -1, -1, -1};
    RbSrc src{p1, p2, p1.sp[p], p2.sp ? p2.sp[p] : 0, (int)(p1.sp[p + 1] - p1.sp[p])};
    if (n >= m) {
        const int avail = src.c1 + (p2.sp ? (int)(p2.sp[p + 1] - p2.sp[p]) : 0);
        r = ransac_rule_walk(S, avail, m, table + tab_off[p], src);
    }
    budget[p] = n >= m ? r.budget : 0;   // (a problem below m points: nothing of it goes into pass 2)
    if (!final) return;
    const bool none = r.candidate < 0;
    n_used[p] = n >= m ? (none ? S : r.n_used) : 0;
    n_candidates[p] = r.n_candidates;
    winner[3 * (size_t)p] = r.candidate, winner[3 * (size_t)p + 1] = r.sample, winner[3 * (size_t)p + 2] = r.root;
    win_at[2 * (size_t)p] = none ? -1 : (r.sample < src.c1 ? 0 : 1);
    win_at[2 * (size_t)p + 1] = none ? 0 : (r.sample < src.c1 ? p1.first[src.s1 + r.sample] : p2.first[src.s2 + (r.sample - src.c1)]) + r.root;
}

// win_at: the winner's pass (-1: none) and its place in that pass's candidate list (n1 / n2 samples)
template <int KIND>
__global__ __launch_bounds__(SC_BLOCK) void rb_finish_kernel(const long long* __restrict__ point_ptr, const double* __restrict__ a,
                                                             const double* __restrict__ b, const double* __restrict__ Kdev, int normalise,
                                                             RbPass p1, RbPass p2, int n1, int n2, int max_models, float thr,
                                                             const int* __restrict__ win_at, double* __restrict__ out_models,
                                                             int* __restrict__ out_inliers, unsigned char* __restrict__ out_masks) {
    __shared__ int wsum[SC_BLOCK / 64];
    const int p = blockIdx.x;
    const int pass = win_at[2 * (size_t)p], at = win_at[2 * (size_t)p + 1];
    const double* pm = nullptr;   // pass < 0: no winner
    if (pass >= 0) {
        const RbPass& w = pass == 0 ? p1 : p2;
        pm = Candidate(w.first, pass == 0 ? n1 : n2, w.models, max_models, at).pm;
    }
    const int tot = classify_winner<KIND>(pm, Kdev, normalise, Points(point_ptr, a, b, p), thr, out_models + 9 * (size_t)p, out_masks, wsum);
    if (threadIdx.x == 0) out_inliers[p] = tot;
}

inline unsigned rb_blocks(long long n) { return (unsigned)((n + RB - 1) / RB); }
inline size_t rb_up(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// one pass over `S` samples (> 0): solve, scan the root counts, count every candidate
void rb_pass(hipStream_t st, const RansacLaunch& L, const long long* sp, const int* idx, int S, double* cand, int* n_models, int* first,
             int* sample_problem, int* total, int* scan_ws, int* counts) {
    const int maxm = solve_max_models(L.kind);
    solve_minimal_launch(st, MinimalLaunch{L.kind, SolveSeg{L.point_ptr, sp, L.P, sample_problem}, L.a, L.b, L.K.dev, L.K.given, S, idx, cand, n_models});
    prim::exclusive_scan<int>(st, n_models, first, S, scan_ws, total);
    const int grid = (int)std::max<long long>(1, std::min<long long>(((long long)S * maxm + RB / 64 - 1) / (RB / 64), RB_COUNT_GRID));
    with_solve_kind(L.kind, [&](auto k) {
        rb_count_kernel<decltype(k)::SCORE><<<grid, RB, 0, st>>>(L.point_ptr, L.a, L.b, L.K.scorer(), L.K.normalise(L.kind), S, first, total,
                                                                 sample_problem, cand, maxm, L.threshold, counts);
    });
}

void rb_compact_any(hipStream_t st, const RansacLaunch& L, long long n, const long long* sp, int skip, int* out) {
    with_solve_kind(L.kind, [&](auto k) {
        rb_compact_kernel<decltype(k)::M><<<rb_blocks(n), RB, 0, st>>>(L.P, n, sp, L.sample_ptr, skip, L.sample_idx, out);
    });
}

}  // namespace

int ransac_default_stage1() { return RB_STAGE1; }

void ransac_build_table(eacham_ctx* ctx, double confidence, int m, int cap, const int* n_of, int P, std::vector<int>& tab_off, std::vector<int>& table) {
    const auto t0 = std::chrono::steady_clock::now();
    std::map<int, int> row;   // n -> where its row begins
    tab_off.assign((size_t)P, 0);
    table.clear();
    for (int p = 0; p < P; ++p) {
        const int n = n_of[p];
        if (n < m) continue;
        auto it = row.find(n);
        if (it == row.end()) {
            it = row.emplace(n, (int)table.size()).first;
            table.resize(table.size() + (size_t)n + 1);
            ransac_budget_row(confidence, n, m, cap, table.data() + it->second);
        }
        tab_off[p] = it->second;
    }
    if (table.empty()) table.push_back(0);
    ctx->ransac_table_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int ransac_launch(eacham_ctx* ctx, hipStream_t st, const RansacLaunch& L) {
    const int P = L.P, m = solve_sample_size(L.kind), maxm = solve_max_models(L.kind);
    RbPass p1{L.single ? L.sample_ptr : L.sp1, L.n_models1, L.first1, L.counts1, L.cand1}, p2{nullptr, nullptr, nullptr, nullptr, nullptr};
    long long S1 = L.S1, S2 = 0;
    auto read_total = [&](long long& v) -> int {   // the 8-byte read-back of a pass's sample total
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(L.total2_host, L.total2, sizeof(long long), hipMemcpyDeviceToHost, st));
        EACHAM_HIP_TRY(ctx, hipStreamSynchronize(st));
        v = *(volatile const long long*)L.total2_host;
        return EACHAM_OK;
    };
    if (!L.single) {
        {
            ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
            rb_stage_kernel<<<rb_blocks(P + 1), RB, 0, st>>>(P, L.sample_ptr, L.stage1, nullptr, L.stage_cnt);
            prim::exclusive_scan<long long>(st, L.stage_cnt, L.sp1, P + 1, L.stage_ws, L.total2);
        }
        if (!L.s1_known) {   // (only the device knows how many samples every problem has: L.S1 is the bound the scratch was sized by)
            if (int rc = read_total(S1)) return rc;
            if (S1 < 0 || S1 > L.S1) return ctx->fail(EACHAM_ERR_HIP, "ransac_batch: %lld samples in the first pass, at most %lld possible", S1, L.S1);
        }
    }
    {
        ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
        const int* idx1 = L.sample_idx;
        if (!L.single) {
            if (S1 > 0) rb_compact_any(st, L, S1, L.sp1, 0, L.idx1);
            idx1 = L.idx1;
        }
        if (S1 > 0) rb_pass(st, L, p1.sp, idx1, (int)S1, L.cand1, L.n_models1, L.first1, L.sample_problem1, L.total1, L.scan_ws1, L.counts1);
        if (!L.single) {
            rb_rule_kernel<<<rb_blocks(P), RB, 0, st>>>(P, m, L.point_ptr, L.sample_ptr, p1, p2, L.tab_off, L.table, 0, L.budget, nullptr, nullptr, nullptr, nullptr);
            rb_stage_kernel<<<rb_blocks(P + 1), RB, 0, st>>>(P, L.sample_ptr, L.stage1, L.budget, L.stage_cnt);
            prim::exclusive_scan<long long>(st, L.stage_cnt, L.sp2, P + 1, L.stage_ws, L.total2);
        }
        EACHAM_HIP_TRY(ctx, hipGetLastError());
    }
    if (!L.single) {
        if (int rc = read_total(S2)) return rc;
        if (S2 < 0 || S2 * m > INT_MAX || S2 * maxm > INT_MAX) return ctx->fail(EACHAM_ERR_CAPACITY, "ransac_batch: %lld samples in the second pass", S2);
    }
    ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
    if (S2 > 0) {
        const size_t s = (size_t)S2, o_idx = 0, o_cand = o_idx + rb_up(sizeof(int) * s * m), o_n = o_cand + rb_up(sizeof(double) * 9 * s * maxm),
                     o_first = o_n + rb_up(sizeof(int) * s), o_prob = o_first + rb_up(sizeof(int) * s), o_tot = o_prob + rb_up(sizeof(int) * s),
                     o_ws = o_tot + rb_up(sizeof(int)), o_cnt = o_ws + rb_up(sizeof(int) * prim::scan_ws_elems(s)), end = o_cnt + rb_up(sizeof(int) * s * maxm);
        if (int rc = ensure_workspace(ctx, end)) return rc;
        char* w = (char*)ctx->ws;
        int* idx2 = (int*)(w + o_idx);
        rb_compact_any(st, L, S2, L.sp2, L.stage1, idx2);
        rb_pass(st, L, L.sp2, idx2, (int)S2, (double*)(w + o_cand), (int*)(w + o_n), (int*)(w + o_first), (int*)(w + o_prob), (int*)(w + o_tot),
                (int*)(w + o_ws), (int*)(w + o_cnt));
        p2 = RbPass{L.sp2, (const int*)(w + o_n), (const int*)(w + o_first), (const int*)(w + o_cnt), (const double*)(w + o_cand)};
    }
    ctx->ransac_solved = S1 + S2;
    rb_rule_kernel<<<rb_blocks(P), RB, 0, st>>>(P, m, L.point_ptr, L.sample_ptr, p1, p2, L.tab_off, L.table, 1, L.budget, L.n_used, L.winner, L.n_candidates,
                                               L.win_at);
    with_solve_kind(L.kind, [&](auto k) {
        rb_finish_kernel<decltype(k)::SCORE><<<P, SC_BLOCK, 0, st>>>(L.point_ptr, L.a, L.b, L.K.scorer(), L.K.normalise(L.kind), p1, p2, (int)S1, (int)S2,
                                                                     maxm, L.threshold, L.win_at, L.models, L.inliers, L.masks);
    });
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return EACHAM_OK;
}

}  // namespace eacham

using namespace eacham;

extern "C" int eacham_ransac_batch(eacham_ctx* ctx, int kind, int n_problems, const int64_t* point_ptr, const double* a, const double* b,
                                   const double* K, const int64_t* sample_ptr, const int32_t* sample_idx, float threshold, double confidence,
                                   int stage1, double* models, int32_t* inliers, uint8_t* masks, int32_t* winner, int32_t* n_candidates,
                                   int32_t* n_used) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (int rc = check_solve_kind(ctx, "ransac_batch", kind)) return rc;
    if (!(threshold >= 0.f)) return ctx->fail(EACHAM_ERR_INVALID, "ransac_batch: the threshold is negative or not a number");
    if (!(confidence > 0.0 && confidence < 1.0)) return ctx->fail(EACHAM_ERR_INVALID, "ransac_batch: confidence outside (0, 1)");
    if (stage1 < 0) return ctx->fail(EACHAM_ERR_INVALID, "ransac_batch: negative stage1");
    ListCall c;
    std::vector<int> n_of;
    if (int rc = check_list_call(ctx, "ransac_batch", kind, n_problems, point_ptr, sample_ptr, a, b, sample_idx, c, &n_of)) return rc;
    if (n_problems == 0) return EACHAM_OK;
    const int P = n_problems, m = solve_sample_size(kind), maxm = solve_max_models(kind);
    if (stage1 == 0) stage1 = ransac_default_stage1();
    const bool single = stage1 >= c.max_S;
    long long S1 = single ? c.S : 0;   // pass 1: every problem's first min(S_p, stage1) samples
    for (int p = 0; p < P && !single; ++p) S1 += std::min<long long>(sample_ptr[p + 1] - sample_ptr[p], stage1);
    std::vector<int> tab_off, table;
    ransac_build_table(ctx, confidence, m, (int)std::max<long long>(c.max_S, 1), n_of.data(), P, tab_off, table);
    EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    IoStage io(ctx, st);
    const auto h_total2 = io.out<long long>(nullptr, 1);   // first: offset 0, always inside the pinned mirror
    const auto h_om = io.out<double>(models, 9 * (size_t)P);
    const auto h_oinl = io.out<int>(inliers, (size_t)P), h_owin = io.out<int>(winner, 3 * (size_t)P), h_onc = io.out<int>(n_candidates, (size_t)P);
    const auto h_onu = io.out<int>(n_used, (size_t)P);
    const auto h_omask = io.out<unsigned char>(masks, (size_t)c.NP);
    c.stage_tables(io, P, point_ptr, sample_ptr, K);
    const auto h_toff = io.in<int>(tab_off.data(), (size_t)P), h_tab = io.in<int>(table.data(), table.size());
    c.stage_points(io, m, a, b, sample_idx);
    const RansacScratch sc(io, P, S1, m, maxm, single);
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    RansacLaunch L{kind, P, S1, stage1, single, threshold, d(c.point_ptr), d(c.sample_ptr), d(c.a), d(c.b), CallK{d(c.K), K != nullptr}, d(c.sample_idx),
                   d(h_toff), d(h_tab)};
    sc.bind(L, d);
    L.total2 = d(h_total2), L.total2_host = (long long*)((char*)ctx->io_host + io.lay.off[h_total2.k]);
    L.models = d(h_om), L.inliers = d(h_oinl), L.masks = d(h_omask), L.winner = d(h_owin), L.n_candidates = d(h_onc), L.n_used = d(h_onu);
    if (int rc = ransac_launch(ctx, st, L)) return rc;
    return io.finish();
}

extern "C" int eacham_ransac_debug_last(eacham_ctx* ctx, int64_t* samples_solved, double* table_ms) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (samples_solved) *samples_solved = ctx->ransac_solved;
    if (table_ms) *table_ms = ctx->ransac_table_ms;
    return EACHAM_OK;
}
