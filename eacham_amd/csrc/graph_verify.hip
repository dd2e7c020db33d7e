// graph_verify.hip — LMedS verification of every edge of a RESIDENT match graph (eacham_graph_set_keypoints, eacham_graph_verify), gfx950.
//
// What a caller of eacham_lmeds_batch does on the host for a whole graph — walk the matches and gather (uv1, uv2) per pair, draw
// every pair's minimal samples, pack and upload 32 bytes per match plus the sample lists, download a mask byte per match and upload
// it again as the `keep` of eacham_graph_tracks — happens here where the graph lives. A PROBLEM is a caller pair of
// eacham_graph_create, in the caller's order; its points are the pair's matches in the caller's order.
//
//   gv_gather           flat over the packed matches: the edge by prim::segment_of over the packed offsets, a = xy[kp_offsets[f1] + q],
//                       b = xy[kp_offsets[f2] + t] into the call's scratch (doubles copied, nothing computed)
//   gv_draw_counter     a thread per (pair, sample): counter_sample (include/eacham/CvSampling.hpp), the function draw_samples calls
//   gv_draw_opencv      a thread per pair — the stream restarts from (uint64)-1 for every pair and every draw depends on the ones
//                       before it: `iterations` cv_get_subset calls of at most 1000 attempts, for the homography with
//                       cv_check_subset_homography and for the fundamental matrix with cv_check_subset_fundamental on the pair's
//                       gathered points converted to float, as lmeds_samples does it; a pair stops where getSubset gives up
//                       both write the fixed-stride `samples` (npairs x iterations x m, -1 behind a pair's count) and the counts
//   prim::exclusive_scan of the counts (npairs + 1 entries, the last 0) -> sample_ptr;  gv_compact -> the packed sample_idx
//   lmeds_launch        (lmeds_batch.hip) the lb_* kernels, unchanged, on these device arrays; the per-problem results land in caller-pair
//                       order, the mask in the packed order of the points
//   gv_scatter_mask     the mask byte of packed match k of edge e to src_offsets[e] + k: the index space of the q / t the graph was made
//                       from, which is what eacham_graph_tracks takes as `keep` (bytes that belong to no pair: zero)
//
// eacham_graph_verify_ransac is the same call with ransac_launch (ransac_batch.hip: threshold RANSAC in two passes) in lmeds_launch's
// place: the checks, the gather, both draws, the packed sample list, the read-back below, the scatter and `retain` are ONE function,
// gv_verify, which both entries hand their own staged arrays and their estimator's launch. Each entry stages its estimator's scratch
// with the struct the list call uses (lmeds_launch.hpp: LmedsScratch, ransac_launch.hpp: RansacScratch); the kernels that depend on
// the kind are launched through with_solve_kind (solve_launch.hpp).
//
// READ-BACKS. The number of samples is known on the host — (pairs with n >= m) x iterations — except under the OpenCV stream for the
// homography and the fundamental matrix, where checkSubset can make getSubset give up: then the total (8 bytes) is read back once through the pinned mirror.
// The scratch is sized by the host-known bound either way; the launches cover exactly sample_ptr[npairs] samples.
#include "lmeds_launch.hpp"
#include "ransac_launch.hpp"
#include "../../include/eacham/CvSampling.hpp"

#include <climits>
#include <exception>
#include <memory>

namespace eacham {
namespace {

constexpr int GV = 256;
constexpr int GV_PAIR = 64;   // gv_draw_opencv: a thread per pair

__device__ __forceinline__ long long gv_gid(int block) { return (long long)blockIdx.x * block + threadIdx.x; }

__global__ __launch_bounds__(GV) void gv_gather_kernel(long long n_matches, const int2* __restrict__ pairs, int n_edges,
                                                       const long long* __restrict__ offsets, const unsigned* __restrict__ q,
                                                       const unsigned* __restrict__ t, const long long* __restrict__ kp_offsets,
                                                       const double2* __restrict__ xy, double2* __restrict__ a, double2* __restrict__ b) {
    const long long k = gv_gid(GV);
    if (k >= n_matches) return;
    const int2 pr = pairs[prim::segment_of(offsets, n_edges, k)];
    a[k] = xy[kp_offsets[pr.x] + q[k]];
    b[k] = xy[kp_offsets[pr.y] + t[k]];
}

// every pair with n >= M gets exactly `iterations` samples; the grid has max(iterations, 1) threads per pair so that the counts are
// written when no sample is asked for
template <int M>
__global__ __launch_bounds__(GV) void gv_draw_counter_kernel(int P, int iterations, const long long* __restrict__ pair_ptr,
                                                             const unsigned long long* __restrict__ seeds, int* __restrict__ samples,
                                                             int* __restrict__ n_samples, long long* __restrict__ cnt) {
    const int per = iterations > 0 ? iterations : 1;
    const long long g = gv_gid(GV);
    if (g >= (long long)P * per) return;
    const int p = (int)(g / per), it = (int)(g % per);
    const long long n = pair_ptr[p + 1] - pair_ptr[p];
    if (it == 0) {
        const int c = n >= M ? iterations : 0;
        n_samples[p] = c;
        cnt[p] = c;
        if (p == 0) cnt[P] = 0;
    }
    if (it >= iterations) return;
    int32_t idx[M];
#pragma unroll
    for (int k = 0; k < M; ++k) idx[k] = -1;
    if (n >= M) hip::counter_sample((int)n, M, seeds ? (uint64_t)seeds[p] : 12345ull, it, idx);
#pragma unroll
    for (int k = 0; k < M; ++k) samples[g * M + k] = idx[k];
}

// CHECK: the callback's checkSubset — 0 none (essential), 1 the homography's, 2 the fundamental matrix's
template <int M, int CHECK>
__global__ __launch_bounds__(GV_PAIR) void gv_draw_opencv_kernel(int P, int iterations, const long long* __restrict__ pair_ptr,
                                                                 const double* __restrict__ a, const double* __restrict__ b,
                                                                 int* __restrict__ samples, int* __restrict__ n_samples,
                                                                 long long* __restrict__ cnt) {
    const long long p = gv_gid(GV_PAIR);
    if (p >= P) return;
    const long long base = pair_ptr[p], n = pair_ptr[p + 1] - base;
    int* out = samples + (size_t)p * iterations * M;
    int done = 0;
    if (n >= M) {
        const double* pa = a + 2 * base;
        const double* pb = b + 2 * base;
        hip::CvRNG rng(0xffffffffffffffffull);
        for (; done < iterations; ++done) {
            int32_t idx[M];
            const bool found = hip::cv_get_subset(rng, (int)n, M, idx, 1000, [&](const int32_t* s) {
                if constexpr (CHECK == 0) {
                    return true;
                } else {
                    float fa[2 * M], fb[2 * M];
#pragma unroll
                    for (int k = 0; k < M; ++k) {
                        fa[2 * k] = (float)pa[2 * (size_t)s[k]], fa[2 * k + 1] = (float)pa[2 * (size_t)s[k] + 1];
                        fb[2 * k] = (float)pb[2 * (size_t)s[k]], fb[2 * k + 1] = (float)pb[2 * (size_t)s[k] + 1];
                    }
                    if constexpr (CHECK == 1) return hip::cv_check_subset_homography(fa, fb, M);
                    else return hip::cv_check_subset_fundamental(fa, fb, M);
                }
            });
            if (!found) break;
#pragma unroll
            for (int k = 0; k < M; ++k) out[done * M + k] = idx[k];
        }
    }
    for (int i = done * M; i < iterations * M; ++i) out[i] = -1;
    n_samples[p] = done;
    cnt[p] = done;
    if (p == 0) cnt[P] = 0;
}

// sample `it` of pair p, if the pair has that many, to its place in the packed list the lb_* kernels read
template <int M>
__global__ __launch_bounds__(GV) void gv_compact_kernel(int P, int iterations, const long long* __restrict__ sample_ptr,
                                                        const int* __restrict__ samples, int* __restrict__ sample_idx) {
    const long long g = gv_gid(GV);
    if (g >= (long long)P * iterations) return;
    const int p = (int)(g / iterations), it = (int)(g % iterations);
    const long long s0 = sample_ptr[p];
    if (it >= sample_ptr[p + 1] - s0) return;
#pragma unroll
    for (int k = 0; k < M; ++k) sample_idx[(s0 + it) * M + k] = samples[g * M + k];
}

__global__ __launch_bounds__(GV) void gv_scatter_mask_kernel(long long n_matches, int n_edges, const long long* __restrict__ offsets,
                                                             const long long* __restrict__ src_offsets,
                                                             const unsigned char* __restrict__ packed, unsigned char* __restrict__ out) {
    const long long k = gv_gid(GV);
    if (k >= n_matches) return;
    const int e = prim::segment_of(offsets, n_edges, k);
    out[src_offsets[e] + (k - offsets[e])] = packed[k];
}

inline unsigned gv_blocks(long long n, int block) { return (unsigned)((n + block - 1) / block); }

template <class Body>
int verify_entry(eacham_ctx* ctx, const char* what, Body body) {   // nothing may leave extern "C"
    std::lock_guard<std::mutex> lock(ctx->mu);
    try {
        return body();
    } catch (const std::exception& e) {
        return ctx->fail(EACHAM_ERR_INVALID, "%s: %s", what, e.what());
    } catch (...) {
        return ctx->fail(EACHAM_ERR_INVALID, "%s: unknown exception", what);
    }
}

}  // namespace
}  // namespace eacham

using namespace eacham;

extern "C" int eacham_graph_set_keypoints(eacham_graph* g, const double* xy) {
    if (!g) return EACHAM_ERR_INVALID;
    eacham_ctx* ctx = g->ctx;
    return verify_entry(ctx, "graph_set_keypoints", [&]() -> int {
        if (g->n_kp > 0 && !xy) return ctx->fail(EACHAM_ERR_INVALID, "graph_set_keypoints: null xy for a graph with %lld keypoints", g->n_kp);
        EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t bytes = 2 * sizeof(double) * (size_t)g->n_kp;
        if (!g->xy) EACHAM_HIP_TRY(ctx, hipMalloc((void**)&g->xy, std::max<size_t>(bytes, 16)));
        g->has_xy = g->has_keep = false;   // new coordinates: a mask retained for the old ones says nothing about them
        if (bytes) EACHAM_HIP_TRY(ctx, hipMemcpyAsync(g->xy, xy, bytes, hipMemcpyHostToDevice, ctx->stream));
        EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the caller's buffer may die when this call returns)
        g->has_xy = true;
        return EACHAM_OK;
    });
}

// What both verifications share, around the estimator of the call: the checks, the gather, the draw, the packed sample list, the
// read-back of the sample total where only the device knows it, then — behind `launch` — the mask's scatter into the caller's match
// index space and `retain`. declare(io, plan): the estimator's own staged arrays, before the upload; launch(d, plan, GvDev): its
// kernels on the device arrays.
struct GvDev {   // what gv_verify prepared on the device, as the estimator's launch finds it
    long long S;                           // the samples sample_ptr[npairs] names
    const double *a, *b, *K;               // gathered points (packed pair order), the staged K
    const long long* sample_ptr;
    const int* sample_idx;
    unsigned char* packed_mask;            // the estimator's mask output: a byte per packed match
    long long *total, *total_host;         // a device word and its pinned mirror, free for the estimator's own 8-byte read-backs
};
struct GvPlan {
    int kind, P, m, maxm, iterations;
    long long n_ok, max_n, NP, S_cap, slots;   // pairs with >= m matches, the largest of them, matches, n_ok x iterations, P x iterations
    bool count_known;                          // every pair with >= m matches has exactly `iterations` samples
};
template <class Declare, class Launch>
int gv_verify(eacham_graph* g, const char* what, int kind, const double* K, int sampling, int iterations, const uint64_t* seeds, int retain,
              uint8_t* masks, int32_t* n_samples, int32_t* samples, Declare declare, Launch launch) {
    eacham_ctx* ctx = g->ctx;
    if (!g->has_xy) return ctx->fail(EACHAM_ERR_INVALID, "%s: the graph has no keypoint coordinates (eacham_graph_set_keypoints)", what);
    if (int rc = check_solve_kind(ctx, what, kind)) return rc;
    if (sampling != EACHAM_SAMPLING_OPENCV && sampling != EACHAM_SAMPLING_COUNTER)
        return ctx->fail(EACHAM_ERR_INVALID, "%s: unknown sampling %d", what, sampling);
    if (iterations < 0) return ctx->fail(EACHAM_ERR_INVALID, "%s: negative iterations", what);
    const int P = g->npairs, m = solve_sample_size(kind), maxm = solve_max_models(kind);
    if (P == 0) return EACHAM_OK;
    long long n_ok = 0, max_n = 0;   // pairs with a minimal sample's worth of matches; the largest of them
    for (int p = 0; p < P; ++p)
        if (g->pair_counts_h[p] >= m) ++n_ok, max_n = std::max<long long>(max_n, g->pair_counts_h[p]);
    const long long NP = g->n_matches, S_cap = n_ok * iterations, slots = (long long)P * iterations;
    if (NP > INT_MAX / 2 || P == INT_MAX || slots * m > INT_MAX || S_cap * maxm > INT_MAX)
        return ctx->fail(EACHAM_ERR_CAPACITY, "%s: %lld points / %d pairs x %d samples in one call", what, NP, P, iterations);
    EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (retain && !g->keep_mask) EACHAM_HIP_TRY(ctx, hipMalloc((void**)&g->keep_mask, std::max<size_t>((size_t)g->n_src, 16)));
    const GvPlan plan{kind, P, m, maxm, iterations, n_ok, max_n, NP, S_cap, slots, kind == EACHAM_SOLVE_ESSENTIAL5 || sampling != EACHAM_SAMPLING_OPENCV};
    hipStream_t st = ctx->stream;
    IoStage io(ctx, st);
    const auto h_total = io.out<long long>(nullptr, 1);   // first: offset 0, always inside the pinned mirror
    const auto h_ons = io.out<int>(n_samples, (size_t)P), h_osamp = io.out<int>(samples, (size_t)slots * m);
    const auto h_omask = io.out<unsigned char>(masks, (size_t)g->n_src);
    const auto h_K = io.in<double>(K, 4);
    const auto h_seeds = io.in<unsigned long long>(seeds, (size_t)P);
    const auto h_a = io.scratch<double2>((size_t)NP), h_b = io.scratch<double2>((size_t)NP);
    const auto h_cnt = io.scratch<long long>((size_t)P + 1), h_sp = io.scratch<long long>((size_t)P + 1);
    const auto h_spws = io.scratch<long long>(prim::scan_ws_elems((size_t)P + 1));
    const auto h_i = io.scratch<int>((size_t)S_cap * m);
    const auto h_pmask = io.scratch<unsigned char>((size_t)NP);
    declare(io, plan);
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    const double* d_a = (const double*)d(h_a);
    const double* d_b = (const double*)d(h_b);
    {   // (profiling: the gather, the draws and the mask's scatter count with the scorer's stage, as the estimators' kernels do)
        ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
        if (NP > 0)
            gv_gather_kernel<<<gv_blocks(NP, GV), GV, 0, st>>>(NP, g->pairs, g->n_edges, g->offsets, g->q, g->t, g->kp_offsets, (const double2*)g->xy,
                                                               d(h_a), d(h_b));
        with_solve_kind(kind, [&](auto k) {
            using Kind = decltype(k);
            if (sampling == EACHAM_SAMPLING_COUNTER) {
                const unsigned grid = gv_blocks((long long)P * std::max(iterations, 1), GV);
                gv_draw_counter_kernel<Kind::M><<<grid, GV, 0, st>>>(P, iterations, g->pair_ptr, seeds ? d(h_seeds) : nullptr, d(h_osamp), d(h_ons), d(h_cnt));
            } else {
                gv_draw_opencv_kernel<Kind::M, Kind::CHECK><<<gv_blocks(P, GV_PAIR), GV_PAIR, 0, st>>>(P, iterations, g->pair_ptr, d_a, d_b, d(h_osamp),
                                                                                                     d(h_ons), d(h_cnt));
            }
            prim::exclusive_scan<long long>(st, d(h_cnt), d(h_sp), P + 1, d(h_spws), d(h_total));
            if (slots > 0) gv_compact_kernel<Kind::M><<<gv_blocks(slots, GV), GV, 0, st>>>(P, iterations, d(h_sp), d(h_osamp), d(h_i));
        });
    }
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    long long S = S_cap;
    long long* total_host = (long long*)((char*)ctx->io_host + io.lay.off[h_total.k]);
    if (!plan.count_known) {
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(total_host, d(h_total), sizeof(long long), hipMemcpyDeviceToHost, st));
        EACHAM_HIP_TRY(ctx, hipStreamSynchronize(st));
        S = *(volatile const long long*)total_host;
        if (S < 0 || S > S_cap) return ctx->fail(EACHAM_ERR_HIP, "%s: %lld samples drawn, at most %lld possible", what, S, S_cap);
    }
    if (int rc = launch(d, plan, GvDev{S, d_a, d_b, d(h_K), d(h_sp), d(h_i), d(h_pmask), d(h_total), total_host})) return rc;
    {
        ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
        if (g->n_src > 0) EACHAM_HIP_TRY(ctx, hipMemsetAsync(d(h_omask), 0, (size_t)g->n_src, st));
        if (NP > 0) gv_scatter_mask_kernel<<<gv_blocks(NP, GV), GV, 0, st>>>(NP, g->n_edges, g->offsets, g->src_offsets, d(h_pmask), d(h_omask));
        EACHAM_HIP_TRY(ctx, hipGetLastError());
        if (retain) {
            g->has_keep = false;
            if (g->n_src > 0) EACHAM_HIP_TRY(ctx, hipMemcpyAsync(g->keep_mask, d(h_omask), (size_t)g->n_src, hipMemcpyDeviceToDevice, st));
        }
    }
    if (int rc = io.finish()) return rc;
    if (retain) g->has_keep = true;
    return EACHAM_OK;
}

extern "C" int eacham_graph_verify(eacham_graph* g, int kind, const double* K, int sampling, int iterations, const uint64_t* seeds, int retain,
                                   double* models, float* medians, float* thresholds, int32_t* inliers, uint8_t* masks, int32_t* winner,
                                   int32_t* n_candidates, int32_t* n_samples, int32_t* samples) {
    if (!g) return EACHAM_ERR_INVALID;
    eacham_ctx* ctx = g->ctx;
    return verify_entry(ctx, "graph_verify", [&]() -> int {
        IoArray<double> h_om{};
        IoArray<float> h_omed{}, h_othr{};
        IoArray<int> h_oinl{}, h_owin{}, h_onc{};
        std::unique_ptr<LmedsScratch> sc;
        return gv_verify(
            g, "graph_verify", kind, K, sampling, iterations, seeds, retain, masks, n_samples, samples,
            [&](IoStage& io, const GvPlan& pl) {
                const size_t P = (size_t)pl.P;
                h_om = io.out<double>(models, 9 * P);
                h_omed = io.out<float>(medians, P), h_othr = io.out<float>(thresholds, P);
                h_oinl = io.out<int>(inliers, P), h_owin = io.out<int>(winner, 3 * P), h_onc = io.out<int>(n_candidates, P);
                sc.reset(new LmedsScratch(io, pl.S_cap, pl.maxm, pl.max_n));
            },
            [&](const IoDev& d, const GvPlan& pl, const GvDev& v) -> int {
                LmedsLaunch L{kind, pl.P, v.S, pl.max_n, g->pair_ptr, v.sample_ptr, v.a, v.b, CallK{v.K, K != nullptr}, v.sample_idx};
                sc->bind(L, d);
                L.models = d(h_om), L.medians = d(h_omed), L.thresholds = d(h_othr), L.inliers = d(h_oinl), L.masks = v.packed_mask, L.winner = d(h_owin), L.n_candidates = d(h_onc);
                return lmeds_launch(ctx, ctx->stream, L);
            });
    });
}

extern "C" int eacham_graph_verify_ransac(eacham_graph* g, int kind, const double* K, int sampling, int iterations, const uint64_t* seeds, int retain,
                                          float threshold, double confidence, int stage1, double* models, int32_t* inliers, uint8_t* masks,
                                          int32_t* winner, int32_t* n_candidates, int32_t* n_used, int32_t* n_samples, int32_t* samples) {
    if (!g) return EACHAM_ERR_INVALID;
    eacham_ctx* ctx = g->ctx;
    return verify_entry(ctx, "graph_verify_ransac", [&]() -> int {
        if (!(threshold >= 0.f)) return ctx->fail(EACHAM_ERR_INVALID, "graph_verify_ransac: the threshold is negative or not a number");
        if (!(confidence > 0.0 && confidence < 1.0)) return ctx->fail(EACHAM_ERR_INVALID, "graph_verify_ransac: confidence outside (0, 1)");
        if (stage1 < 0) return ctx->fail(EACHAM_ERR_INVALID, "graph_verify_ransac: negative stage1");
        if (stage1 == 0) stage1 = ransac_default_stage1();
        IoArray<double> h_om{};
        IoArray<int> h_oinl{}, h_owin{}, h_onc{}, h_onu{}, h_toff{}, h_tab{};
        std::vector<int> tab_off, table;
        std::unique_ptr<RansacScratch> sc;
        bool single = false;
        long long S1_cap = 0;
        return gv_verify(
            g, "graph_verify_ransac", kind, K, sampling, iterations, seeds, retain, masks, n_samples, samples,
            [&](IoStage& io, const GvPlan& pl) {
                const size_t P = (size_t)pl.P;
                single = stage1 >= pl.iterations;
                S1_cap = single ? pl.S_cap : pl.n_ok * stage1;   // (the budget rows are built here, on the host: the pairs' match counts are known)
                ransac_build_table(ctx, confidence, pl.m, std::max(pl.iterations, 1), g->pair_counts_h.data(), pl.P, tab_off, table);
                h_om = io.out<double>(models, 9 * P);
                h_oinl = io.out<int>(inliers, P), h_owin = io.out<int>(winner, 3 * P), h_onc = io.out<int>(n_candidates, P), h_onu = io.out<int>(n_used, P);
                h_toff = io.in<int>(tab_off.data(), P), h_tab = io.in<int>(table.data(), table.size());
                sc.reset(new RansacScratch(io, pl.P, S1_cap, pl.m, pl.maxm, single));
            },
            [&](const IoDev& d, const GvPlan& pl, const GvDev& v) -> int {
                RansacLaunch L{kind, pl.P, single ? v.S : S1_cap, stage1, single, threshold, g->pair_ptr, v.sample_ptr, v.a, v.b, CallK{v.K, K != nullptr},
                               v.sample_idx, d(h_toff), d(h_tab)};
                sc->bind(L, d);
                L.s1_known = single || pl.count_known;
                L.total2 = v.total, L.total2_host = v.total_host;
                L.models = d(h_om), L.inliers = d(h_oinl), L.masks = v.packed_mask, L.winner = d(h_owin), L.n_candidates = d(h_onc), L.n_used = d(h_onu);
                return ransac_launch(ctx, ctx->stream, L);
            });
    });
}
