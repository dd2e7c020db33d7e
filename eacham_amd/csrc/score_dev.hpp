// score_dev.hpp — the device functions of the hypothesis scoring that more than one translation unit runs: the error one
// model assigns to one correspondence (OpenCV 4.5.5's estimator callbacks, no fused operations), the order-preserving key of
// a float, the block-wide radix select, the median over it (block_median) and the block's inlier count (block_count). score.hip
// (eacham_score_hypotheses), pnp_batch.hip (the PnP rounds) and, through estimator_dev.hpp, lmeds_batch.hip and ransac_batch.hip
// (the two-view estimators, under the list calls and under graph_verify.hip's) inline the same bodies, so a model's errors and
// median are the same bits through every entry point. Every includer is compiled with -ffp-contract=off (csrc/Makefile).
#pragma once

#include <hip/hip_runtime.h>

namespace eacham {
namespace {

constexpr int SC_BLOCK = 256;
constexpr int SC_MAX_LDS = 16384;  // errors of one model kept in LDS (64 KB); larger n re-reads the error matrix

__device__ __forceinline__ double dmul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double dadd(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ float fmul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float fadd(float a, float b) { return __fadd_rn(a, b); }

template <int KIND>
__device__ __forceinline__ float score_one(const double* __restrict__ a, const double* __restrict__ b, const double* M,
                                           const double* K, bool normalise) {
    if (KIND == 0) {
        double x1[3] = {a[0], a[1], 1.0}, x2[3] = {b[0], b[1], 1.0};
        if (normalise) {
            x1[0] = __ddiv_rn(dadd(a[0], -K[2]), K[0]); x1[1] = __ddiv_rn(dadd(a[1], -K[3]), K[1]);
            x2[0] = __ddiv_rn(dadd(b[0], -K[2]), K[0]); x2[1] = __ddiv_rn(dadd(b[1], -K[3]), K[1]);
        }
        double Ex1[3], Etx2[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            Ex1[r] = dadd(dadd(dmul(M[3 * r], x1[0]), dmul(M[3 * r + 1], x1[1])), dmul(M[3 * r + 2], x1[2]));
            Etx2[r] = dadd(dadd(dmul(M[r], x2[0]), dmul(M[3 + r], x2[1])), dmul(M[6 + r], x2[2]));
        }
        const double x2tEx1 = dadd(dadd(dmul(x2[0], Ex1[0]), dmul(x2[1], Ex1[1])), dmul(x2[2], Ex1[2]));
        const double d = dadd(dadd(dadd(dmul(Ex1[0], Ex1[0]), dmul(Ex1[1], Ex1[1])), dmul(Etx2[0], Etx2[0])), dmul(Etx2[1], Etx2[1]));
        return (float)__ddiv_rn(dmul(x2tEx1, x2tEx1), d);
    } else if (KIND == 1) {
        const float x = (float)a[0], y = (float)a[1], mx = (float)b[0], my = (float)b[1];
        const float H0 = (float)M[0], H1 = (float)M[1], H2 = (float)M[2], H3 = (float)M[3], H4 = (float)M[4], H5 = (float)M[5],
                    H6 = (float)M[6], H7 = (float)M[7];
        const float ww = __fdiv_rn(1.f, fadd(fadd(fmul(H6, x), fmul(H7, y)), 1.f));
        const float dx = fadd(fmul(fadd(fadd(fmul(H0, x), fmul(H1, y)), H2), ww), -mx);
        const float dy = fadd(fmul(fadd(fadd(fmul(H3, x), fmul(H4, y)), H5), ww), -my);
        return fadd(fmul(dx, dx), fmul(dy, dy));
    } else if (KIND == 3) {
        // FMEstimatorCallback::computeError on pixels (K is ignored, nothing is normalised), x1 = (a, 1), x2 = (b, 1):
        //   l2 = F x1:   l2[r] = (F[3r] a0 + F[3r+1] a1) + F[3r+2]          l1 = F^T x2:   l1[r] = (F[r] b0 + F[3+r] b1) + F[6+r]
        //   d = (b0 l2[0] + b1 l2[1]) + l2[2],   d2 = d d
        //   err = (float)max(d2 / (l1[0]^2 + l1[1]^2), d2 / (l2[0]^2 + l2[1]^2))      every operation rounded on its own, no FMA
        double l2[3], l1[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            l2[r] = dadd(dadd(dmul(M[3 * r], a[0]), dmul(M[3 * r + 1], a[1])), M[3 * r + 2]);
            l1[r] = dadd(dadd(dmul(M[r], b[0]), dmul(M[3 + r], b[1])), M[6 + r]);
        }
        const double d = dadd(dadd(dmul(b[0], l2[0]), dmul(b[1], l2[1])), l2[2]);
        const double d2 = dmul(d, d);
        const double e1 = __ddiv_rn(d2, dadd(dmul(l1[0], l1[0]), dmul(l1[1], l1[1])));
        const double e2 = __ddiv_rn(d2, dadd(dmul(l2[0], l2[0]), dmul(l2[1], l2[1])));
        return (float)(e1 < e2 ? e2 : e1);   // std::max(e1, e2): e1 unless e2 is greater
    } else {
        const double X = dadd(dadd(dadd(dmul(M[0], a[0]), dmul(M[1], a[1])), dmul(M[2], a[2])), M[9]);
        const double Y = dadd(dadd(dadd(dmul(M[3], a[0]), dmul(M[4], a[1])), dmul(M[5], a[2])), M[10]);
        double Z = dadd(dadd(dadd(dmul(M[6], a[0]), dmul(M[7], a[1])), dmul(M[8], a[2])), M[11]);
        Z = Z != 0.0 ? __ddiv_rn(1.0, Z) : 1.0;
        const float u = (float)dadd(dmul(dmul(X, Z), K[0]), K[2]), v = (float)dadd(dmul(dmul(Y, Z), K[1]), K[3]);
        const float dx = fadd((float)b[0], -u), dy = fadd((float)b[1], -v);
        return fadd(fmul(dx, dx), fmul(dy, dy));
    }
}

// total order of floats as unsigned keys (negatives reversed, NaN with the sign bit clear sorts last)
__device__ __forceinline__ unsigned fkey(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// k-th smallest (0-based) of the n keys: 4 passes of an 8-bit radix histogram, block-wide. `load(i)` returns key i.
template <class Load>
__device__ unsigned radix_select(Load load, int n, int k, unsigned* hist /* [256] LDS */, unsigned* sh /* [2] LDS */) {
    unsigned prefix = 0, mask = 0;
    int want = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < 256; i += SC_BLOCK) hist[i] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += SC_BLOCK) {
            const unsigned key = load(i);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);  // integer counts: order-free
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int acc = 0, d = 0;
            for (; d < 255; ++d) {
                if (acc + (int)hist[d] > want) break;
                acc += (int)hist[d];
            }
            sh[0] = (unsigned)d;
            sh[1] = (unsigned)acc;
        }
        __syncthreads();
        prefix |= sh[0] << shift;
        mask |= 255u << shift;
        want -= (int)sh[1];
        __syncthreads();
    }
    return prefix;
}

// The median of the n > 0 keys as the float it stands for: the upper middle, averaged with the lower one when n is even.
template <class Load>
__device__ __forceinline__ float block_median(Load load, int n, unsigned* hist /* [256] LDS */, unsigned* sh /* [2] LDS */) {
    const unsigned hi = radix_select(load, n, n / 2, hist, sh);
    float med = fkey_inv(hi);
    if (n % 2 == 0) {
        const unsigned lo = radix_select(load, n, n / 2 - 1, hist, sh);
        med = fmul(fadd(fkey_inv(lo), med), 0.5f);
    }
    return med;
}

// The sum of one count per thread, returned to thread 0 (integers: exact in any order): a shuffle tree per wave, then the waves in
// order. Ends past a workgroup barrier.
__device__ __forceinline__ int block_count(int c, int* wsum /* [SC_BLOCK / 64] LDS */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    int tot = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < SC_BLOCK / 64; ++w) tot += wsum[w];
    return tot;
}

}  // namespace
}  // namespace eacham
