// tri_refine.hip — the non-linear step after triangulation for a whole LIST of tracks per call, gfx950: Levenberg-Marquardt on the
// reprojection error of a 3-D point over the observations its caller names (the inliers of eacham_triangulate_tracks), the cameras
// held fixed, where eacham_triangulate_tracks ends on the two-view DLT point of the last pair tried. include/eacham_hip.h states the
// algorithm with eacham_triangulate_refine_tracks; tests/cpp/tri_refine_reference.c is the CPU restatement the kernel is held to as
// bytes.
//
//   tri_refine_kernel   a GROUP of 8 lanes per track, 8 tracks per wave, TRI_REFINE_WAVES waves per workgroup; no barrier, no LDS.
//                       Tracks are short (2-10 views as a rule): a wave per track, as pnp_refine_kernel has a wave per frame, would
//                       idle some 60 lanes. The WHOLE loop runs here. H, g, the cost, the point and lambda live in registers,
//                       identical in the 8 lanes of a group; a try is the 3 x 3 solve on every lane (identical values), the step, and
//                       ONE pass over the track's observations that gives the candidate's cost together with its H and g
//                       (tri_refine_sums: a trip per 8 observations, a lane's observations in ascending order, a fixed butterfly
//                       over the 8 partials), so an accepted step costs no second pass. After the loop the same group recounts
//                       is_inlier (the predicate of triangulate.hip, restated here with the same expression) over ALL of the
//                       track's observations at the refined point.
//
// The groups of a wave leave the loop after different numbers of tries, so the wave is NOT in step: every branch is uniform within
// a group (its condition is computed from values that are the same in the group's 8 lanes), every cross-lane read is a
// __shfl_xor by 4, 2 or 1, which never leaves the group, and nothing here is a wave-wide vote (no __ballot, no __any).
// A track's result depends on its own observations only: not on the length of the list, nor on where in it the track sits.
#include "context.hpp"

#include <climits>
#include <cmath>

namespace eacham {
namespace {

constexpr int TRI_REFINE_GROUP = 8;                      // lanes per track
constexpr int TRI_REFINE_WAVES = 4;                      // waves per workgroup
constexpr int TRI_REFINE_BLOCK = 64 * TRI_REFINE_WAVES;
constexpr int TRI_REFINE_TRACKS = TRI_REFINE_BLOCK / TRI_REFINE_GROUP;   // tracks per workgroup
constexpr int TRI_REFINE_NS = 10;                        // 6 entries of H (upper triangle, row by row), 3 of g, the cost
constexpr int TRI_REFINE_CONVERGED = 0, TRI_REFINE_CAP = 1, TRI_REFINE_NOT_REFINED = 2;   // EACHAM_TRI_REFINE_* of the header

__device__ constexpr int tri_hidx(int i, int j) { return i * 3 - i * (i - 1) / 2 + (j - i); }   // i <= j

// S += the terms of one observation (T, (u, v)) at X: J'J, J'r and r'r. Returns z.
__device__ __forceinline__ double tri_refine_row(const double* __restrict__ T, double u, double v, const double* X, const double* K, double* S) {
    const double xc = ((T[0] * X[0] + T[1] * X[1]) + T[2] * X[2]) + T[3];
    const double yc = ((T[4] * X[0] + T[5] * X[1]) + T[6] * X[2]) + T[7];
    const double zc = ((T[8] * X[0] + T[9] * X[1]) + T[10] * X[2]) + T[11];
    const double iz = 1.0 / zc;
    const double xn = xc * iz, yn = yc * iz;
    const double r0 = (K[0] * xn + K[2]) - u, r1 = (K[1] * yn + K[3]) - v;
    const double a = K[0] * iz, b = K[1] * iz;
    double Ju[3], Jv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        Ju[j] = a * (T[j] - xn * T[8 + j]);
        Jv[j] = b * (T[4 + j] - yn * T[8 + j]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) S[tri_hidx(i, j)] = S[tri_hidx(i, j)] + (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
#pragma unroll
    for (int i = 0; i < 3; ++i) S[6 + i] = S[6 + i] + (Ju[i] * r0 + Jv[i] * r1);
    S[9] = S[9] + (r0 * r0 + r1 * r1);
    return zc;
}

// H, g and the cost of X over the used observations (use null: every one) of a track's n, by ONE group of 8 lanes: lane l owns the
// observations i with i % 8 == l and adds the used ones in ascending order from zero; the 8 partials are folded 4, 2, 1 (a
// butterfly: a + b is b + a, so every lane ends with the sum lane 0 of a shuffle-down tree would hold). used = the number of used
// observations; returns true if one of them has !(z > 0). The same in every lane of the group; no lane outside it is read.
__device__ __forceinline__ bool tri_refine_sums(int l, const double* __restrict__ transforms, const unsigned* __restrict__ frame,
                                                const double2* __restrict__ uv, const unsigned char* __restrict__ use, int n, const double* X,
                                                const double* K, double* S, int& used) {
#pragma unroll
    for (int k = 0; k < TRI_REFINE_NS; ++k) S[k] = 0.0;
    int bad = 0, m = 0;
    for (int i = l; i < n; i += TRI_REFINE_GROUP) {
        if (use && !use[i]) continue;
        const double2 p = uv[i];
        const double z = tri_refine_row(transforms + 16 * (size_t)frame[i], p.x, p.y, X, K, S);
        bad |= !(z > 0.0);
        ++m;
    }
#pragma unroll
    for (int off = TRI_REFINE_GROUP / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < TRI_REFINE_NS; ++k) S[k] = S[k] + __shfl_xor(S[k], off);
        m += __shfl_xor(m, off);
        bad |= __shfl_xor(bad, off);
    }
    used = m;
    return bad != 0;
}

// (H + lambda diag H) d = -g by an unpivoted L D L' factorisation in registers, in the order of pnp_refine_solve; false if a pivot
// is not > 0.
__device__ __forceinline__ bool tri_refine_solve(const double* S, double lambda, double* d) {
    double L[3][3], D[3], y[3];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double v = S[tri_hidx(j, j)] + lambda * S[tri_hidx(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) v = v - L[j][k] * D[k] * L[j][k];
        ok = ok && v > 0.0;   // (the rest is computed and thrown away: no divergence, no early exit from an unrolled nest)
        D[j] = v;
#pragma unroll
        for (int i = j + 1; i < 3; ++i) {
            double w = S[tri_hidx(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) w = w - L[i][k] * D[k] * L[j][k];
            L[i][j] = w / v;
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double v = -S[6 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
        y[i] = v;
    }
#pragma unroll
    for (int i = 2; i >= 0; --i) {
        double v = y[i] / D[i];
#pragma unroll
        for (int k = i + 1; k < 3; ++k) v = v - L[k][i] * d[k];
        d[i] = v;
    }
    return ok;
}

__device__ __forceinline__ double tri_max_abs3(const double* v) {
    double big = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a = v[k] < 0.0 ? -v[k] : v[k];
        if (!(a <= big)) big = a;   // (a NaN is not small)
    }
    return big;
}

// is_inlier of triangulate.hip, the same expression (that file's bytes stay as they are; both files are built without contraction)
__device__ __forceinline__ bool tri_refine_inlier(const double* __restrict__ T, double u0, double v0, const double* K, const double* X, float max_err) {
    const double px = T[0] * X[0] + T[1] * X[1] + T[2] * X[2] + T[3];
    const double py = T[4] * X[0] + T[5] * X[1] + T[6] * X[2] + T[7];
    const double pz = T[8] * X[0] + T[9] * X[1] + T[10] * X[2] + T[11];
    const double u = (K[0] * px) / pz + K[2], v = (K[1] * py) / pz + K[3];
    const float err = (float)sqrt((u0 - u) * (u0 - u) + (v0 - v) * (v0 - v));
    return err < max_err && pz >= 2.220446049250313e-16;
}

__global__ __launch_bounds__(TRI_REFINE_BLOCK) void tri_refine_kernel(
    int n_tracks, const long long* __restrict__ track_ptr, const double* __restrict__ transforms, const unsigned* __restrict__ obs_frame,
    const double2* __restrict__ obs_uv, const double* __restrict__ Kdev, const double* __restrict__ points,
    const unsigned char* __restrict__ has_point, const unsigned char* __restrict__ use_mask, int max_tries, float max_err,
    double* __restrict__ refined, double* __restrict__ cost, int* __restrict__ tries, int* __restrict__ status,
    unsigned char* __restrict__ mask, int* __restrict__ n_inliers) {
    const int l = threadIdx.x & (TRI_REFINE_GROUP - 1);
    const long long tl = (long long)blockIdx.x * TRI_REFINE_TRACKS + (threadIdx.x / TRI_REFINE_GROUP);
    if (tl >= n_tracks) return;   // (group-uniform, as is every branch below: the kernel has no barrier and no wave-wide vote)
    const int t = (int)tl;
    const long long base = track_ptr[t];
    const int n = (int)(track_ptr[t + 1] - base);
    const bool has = has_point[t] != 0;
    const double K[4] = {Kdev[0], Kdev[1], Kdev[2], Kdev[3]};
    const unsigned* frame = obs_frame + base;
    const double2* uv = obs_uv + base;
    const unsigned char* use = use_mask ? use_mask + base : nullptr;
    double X[3], S[TRI_REFINE_NS];
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = has ? points[3 * (size_t)t + k] : 0.0;
    double cost0 = 0.0;
    int tr = 0, st = TRI_REFINE_NOT_REFINED;
    bool run = false;
    if (has) {
        int used = 0;
        const bool bad = tri_refine_sums(l, transforms, frame, uv, use, n, X, K, S, used);
        cost0 = S[9] == S[9] ? S[9] : __longlong_as_double(0x7ff8000000000000ll);   // a NaN cost leaves as ONE bit pattern
        run = used >= 2 && !bad && S[9] - S[9] == 0.0;
    }
    double cost1 = cost0;
    if (run) {
        double lambda = 1e-3;
        st = TRI_REFINE_CAP;
        while (tr < max_tries) {
            double d[3], Xc[3], Sc[TRI_REFINE_NS];
            ++tr;
            if (!tri_refine_solve(S, lambda, d)) {
                lambda = 10.0 * lambda < 1e12 ? 10.0 * lambda : 1e12;
                continue;
            }
            if (tri_max_abs3(d) <= 1e-10 * (1.0 + tri_max_abs3(X))) {
                st = TRI_REFINE_CONVERGED;
                break;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) Xc[k] = X[k] + d[k];
            int uc = 0;
            const bool badc = tri_refine_sums(l, transforms, frame, uv, use, n, Xc, K, Sc, uc);
            if (!badc && Sc[9] < S[9]) {
                const double dec = S[9] - Sc[9];
#pragma unroll
                for (int k = 0; k < 3; ++k) X[k] = Xc[k];
#pragma unroll
                for (int k = 0; k < TRI_REFINE_NS; ++k) S[k] = Sc[k];
                lambda = lambda / 10.0 > 1e-12 ? lambda / 10.0 : 1e-12;
                if (dec <= 1e-9 * S[9]) {
                    st = TRI_REFINE_CONVERGED;
                    break;
                }
            } else {
                lambda = 10.0 * lambda < 1e12 ? 10.0 * lambda : 1e12;
            }
        }
        cost1 = S[9];
    }
    if (l < 3) refined[3 * (size_t)t + l] = l == 0 ? X[0] : l == 1 ? X[1] : X[2];
    if (l == 0) cost[2 * (size_t)t] = cost0, cost[2 * (size_t)t + 1] = cost1, tries[t] = tr, status[t] = st;
    if (!mask && !n_inliers) return;
    int c = 0;
    for (int i0 = 0; i0 < n; i0 += TRI_REFINE_GROUP) {   // (every lane of the GROUP takes every trip; the other groups are elsewhere)
        const int i = i0 + l;
        bool in = false;
        if (has && i < n) {
            const double2 p = uv[i];
            in = tri_refine_inlier(transforms + 16 * (size_t)frame[i], p.x, p.y, K, X, max_err);
        }
        if (mask && i < n) mask[base + i] = in;
        c += in;
    }
#pragma unroll
    for (int off = TRI_REFINE_GROUP / 2; off > 0; off >>= 1) c += __shfl_xor(c, off);   // (integers: the order is free)
    if (n_inliers && l == 0) n_inliers[t] = c;
}

}  // namespace
}  // namespace eacham

using namespace eacham;

extern "C" int eacham_triangulate_refine_tracks(eacham_ctx* ctx, const double* transforms, int n_frames, int n_tracks, const int64_t* track_ptr,
                                                const uint32_t* obs_frame, const double* obs_uv, const double* K, const double* points,
                                                const uint8_t* has_point, const uint8_t* use_mask, int max_tries, float max_repr_error,
                                                double* refined, double* cost, int32_t* tries, int32_t* status, uint8_t* inlier_mask,
                                                int32_t* n_inliers) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    const char* call = "triangulate_refine_tracks";
    if (n_tracks < 0 || n_frames < 0) return ctx->fail(EACHAM_ERR_INVALID, "%s: negative number of tracks or frames", call);
    if (max_tries < 1) return ctx->fail(EACHAM_ERR_INVALID, "%s: max_tries %d below 1", call, max_tries);
    if ((inlier_mask || n_inliers) && !(max_repr_error >= 0.f))
        return ctx->fail(EACHAM_ERR_INVALID, "%s: max_repr_error is NaN or negative", call);
    if (n_tracks == 0) return EACHAM_OK;
    const int P = n_tracks;
    if (!track_ptr) return ctx->fail(EACHAM_ERR_INVALID, "%s: null track_ptr", call);
    if (track_ptr[0] != 0) return ctx->fail(EACHAM_ERR_INVALID, "%s: track_ptr does not start at 0", call);
    for (int t = 0; t < P; ++t)
        if (track_ptr[t + 1] < track_ptr[t]) return ctx->fail(EACHAM_ERR_INVALID, "%s: track %d: track_ptr decreases", call, t);
    if (track_ptr[P] > INT_MAX)
        return ctx->fail(EACHAM_ERR_CAPACITY, "%s: track_ptr ends at %lld: more than 2^31 - 1 observations in one call", call, (long long)track_ptr[P]);
    const long long NO = track_ptr[P];
    if (!K || !points || !has_point || !refined || !cost || !tries || !status || (NO > 0 && (!transforms || !obs_frame || !obs_uv)))
        return ctx->fail(EACHAM_ERR_INVALID, "%s: null array", call);
    for (int t = 0; t < P; ++t)
        for (long long i = track_ptr[t]; i < track_ptr[t + 1]; ++i)
            if (obs_frame[i] >= (uint32_t)n_frames)
                return ctx->fail(EACHAM_ERR_INVALID, "%s: track %d: observation %lld names frame %u of %d", call, t, i - track_ptr[t], obs_frame[i], n_frames);
    EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    IoStage io(ctx, st);
    const auto h_r = io.out<double>(refined, 3 * (size_t)P), h_c = io.out<double>(cost, 2 * (size_t)P);
    const auto h_t = io.out<int>(tries, (size_t)P), h_s = io.out<int>(status, (size_t)P);
    const auto h_mask = io.out<unsigned char>(inlier_mask, inlier_mask ? (size_t)NO : 0);
    const auto h_ni = io.out<int>(n_inliers, n_inliers ? (size_t)P : 0);
    const auto h_tp = io.in<long long>(track_ptr, (size_t)P + 1);
    const auto h_K = io.in<double>(K, 4);
    const auto h_T = io.in<double>(NO > 0 ? transforms : nullptr, 16 * (size_t)n_frames);
    const auto h_of = io.in<unsigned>(obs_frame, (size_t)NO);
    const auto h_uv = io.in<double2>(obs_uv, (size_t)NO);
    const auto h_p = io.in<double>(points, 3 * (size_t)P);
    const auto h_has = io.in<unsigned char>(has_point, (size_t)P);
    const auto h_use = io.in<unsigned char>(use_mask, use_mask ? (size_t)NO : 0);
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    {
        ProfileScope scope(ctx, EACHAM_KERNEL_TRIANGULATE);
        const unsigned gw = (unsigned)(((long long)P + TRI_REFINE_TRACKS - 1) / TRI_REFINE_TRACKS);
        tri_refine_kernel<<<gw, TRI_REFINE_BLOCK, 0, st>>>(P, d(h_tp), d(h_T), d(h_of), d(h_uv), d(h_K), d(h_p), d(h_has),
                                                          use_mask ? d(h_use) : nullptr, max_tries, max_repr_error, d(h_r), d(h_c), d(h_t), d(h_s),
                                                          inlier_mask ? d(h_mask) : nullptr, n_inliers ? d(h_ni) : nullptr);
    }
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return io.finish();
}
