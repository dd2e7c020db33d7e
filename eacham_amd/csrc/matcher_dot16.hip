// matcher_dot16.hip — the screened form of the mutual dot-product matcher (eacham_match_all_pairs_dot_screened): an fp16 sweep on
// v_mfma_f32_32x32x16_f16 decides every row and column that a proven error bound lets it decide, exact fp32 work runs for the
// winners and the near-ties alone, and the result is the result of eacham_match_all_pairs_dot bit for bit.
//
//   s(q,t)   the fp32 k-ordered fmaf chain from 0 over the padded dimension (what match_tile_dot_kernel's MFMAs give)
//   s~(q,t)  the sweep's value: fp16 images of both rows, exact products, fp32 accumulation inside the MFMA
//   |s~ - s| <= E(q,t) = kappa N'_q N'_t + eps0,     kappa = 2^-10 + (D + 16) 2^-22,  eps0 = 2^-100,  D = padded dimension
// where N' is the stored per-row norm bound: an upper bound of |x|_2 + 2^-3 sqrt(f), f = the row's elements with 0 < |x| < 2^-14,
// which the image kernel FLUSHES to zero (so no fp16 subnormal ever reaches the MFMA, whatever the hardware does with them).
// A row uses E_q = kappa N'_q max_t N'_t, a column the same with the roles swapped. All of the bound's arithmetic rounds up.
//
// Image of a frame: frag16[tile][ks][lane] = 8 halves (16 bytes), row 32 tile + lane % 32, k = 16 ks + 8 (lane / 32) + j — the
// register image of the 32x32x16 operands (A and B use the same map, so any consistent map gives the dot product); one wave
// access is 1 KiB contiguous and LDS-DMA copies a tile unswizzled. Built lazily from the resident fp32 fragments on a frame's
// first screened call, dropped with the frame.
#include "context.hpp"
#include "match_plan.hpp"

#include <algorithm>
#include <cmath>

namespace eacham {

typedef float v16f __attribute__((ext_vector_type(16)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef const float __attribute__((address_space(1)))* gfloat_t;

constexpr int H_THREADS = 256, H_WAVES = 4;
constexpr float DOT16_EPS0 = 0x1p-100f;
#define EACHAM_NEG_INF (-__builtin_inff())

// device-side entry of a frame's fp16 image
struct Frame16Dev {
    const int4* frag16;
    const float* nrm;  // N' per padded row (0 for padding)
    float maxn;        // max of nrm over the frame
    int pad;
};

// next float towards +inf / -inf (finite input; the bound's arithmetic is rn followed by one of these)
__host__ __device__ inline float next_up(float x) {
    if (!(x == x) || x == __builtin_inff()) return x;
    if (x == 0.0f) return 0x1p-149f;
    int b;
    memcpy(&b, &x, 4);
    b += x > 0.0f ? 1 : -1;
    memcpy(&x, &b, 4);
    return x;
}
__host__ __device__ inline float next_down(float x) { return -next_up(-x); }

// value (row, k) of a frame's fp32 fragments: fragf[tile][k / 2][32 (k % 2) + row % 32]
__device__ __forceinline__ size_t fragf_index(int row, int k, int D2) {
    return ((size_t)(row >> 5) * D2 + (k >> 1)) * 64 + 32 * (k & 1) + (row & 31);
}

// ---- image ------------------------------------------------------------------------------------------
__global__ void pack_f16_kernel(const float* __restrict__ fragf, int D2, int ntiles, int4* __restrict__ frag16) {
    const int KS = D2 / 8;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)ntiles * KS * 64) return;
    const int lane = (int)(idx % 64);
    const long long rest = idx / 64;
    const int ks = (int)(rest % KS), tile = (int)(rest / KS);
    const int row = tile * 32 + (lane & 31), k0 = 16 * ks + 8 * (lane >> 5);
    union {
        _Float16 h[8];
        int4 v;
    } u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float x = fragf[fragf_index(row, k0 + j, D2)];
        const bool keep = fabsf(x) >= 0x1p-14f && fabsf(x) <= 65504.0f;  // below: flushed; above or not finite: the frame is not screened
        u.h[j] = keep ? (_Float16)x : (_Float16)0.0f;                    // round to nearest even
    }
    frag16[idx] = u.v;
}
// N' per row (rounded up), the frame's maximum and its "not screenable" flag: meta = {bits(max N'), flag}
__global__ void norm_f16_kernel(const float* __restrict__ fragf, int n, int D2, int npad, float* __restrict__ nrm, int* __restrict__ meta) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= npad) return;
    float np = 0.0f;
    if (row < n) {
        float ss = 0.0f;
        int flushed = 0;
        bool bad = false;
        for (int k = 0; k < 2 * D2; ++k) {
            const float x = fragf[fragf_index(row, k, D2)];
            const float ax = fabsf(x);
            bad |= !(ax <= 65504.0f);  // NaN, Inf, beyond the fp16 range
            flushed += ax > 0.0f && ax < 0x1p-14f;
            ss = next_up(__fmaf_rn(x, x, ss));
        }
        if (bad) {
            atomicOr(&meta[1], 1);
        } else {
            np = next_up(__fsqrt_rn(ss));
            if (flushed) np = next_up(np + next_up(0.125f * next_up(__fsqrt_rn((float)flushed))));
            atomicMax(&meta[0], __float_as_int(np));  // non-negative floats order like their bits; a maximum has no arrival order
        }
    }
    nrm[row] = np;
}

// ---- K1h: fp16 similarity tiles + fused row/column top-2 values ------------------------------------------
// rowres[p][q]       = {bits(v1), col1, bits(v2), 0}        final over the columns < B.n
// colpart[p][wb][c]  = {bits(v1), row1, bits(v2), 0}        over the rows < A.n of tile wb of frame A
// DUMP: every s~(q, t) of the pair goes to `dump` (n1 x n2, eacham_match_debug_dot_coarse); the MFMA sequence is the same.
template <int KS, bool DUMP>
__global__ __launch_bounds__(H_THREADS, 2) void match_tile_dot16_kernel(
    const FrameDev* __restrict__ frames, const Frame16Dev* __restrict__ frames16, const int2* __restrict__ pairs,
    const int2* __restrict__ pairs_fb, int empty_frame, int wgs_per_pair, int4* __restrict__ rowres, int4* __restrict__ colpart,
    int wb_stride, int row_stride, float* __restrict__ dump) {
    constexpr int TILE_V = 64 * KS;  // 16-byte vectors per 32-row tile
    constexpr int RING_B = 2 * TILE_V * 16;
    constexpr int SLABS_B = H_WAVES * 3 * 32 * 33 * 4;
    constexpr int LDS_B = RING_B > SLABS_B ? RING_B : SLABS_B;
    __shared__ __attribute__((aligned(16))) char sMem[LDS_B];  // 2-slot tile ring; after the sweep reused as the row slabs
    v8h (*sB)[TILE_V] = reinterpret_cast<v8h (*)[TILE_V]>(sMem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cl = lane & 31, h = lane >> 5;
    const int p = blockIdx.x / wgs_per_pair, rb = blockIdx.x % wgs_per_pair;
    if (pairs_fb && pairs_fb[p].x != empty_frame) return;  // a pair with an unscreenable frame: the fp32 tile kernel has it
    const int2 pr = pairs[p];
    const FrameDev A = frames[pr.x], B = frames[pr.y];
    if (rb * H_WAVES >= A.ntiles) return;  // workgroup-uniform
    const int wb = rb * H_WAVES + wave;    // 32-row tile of frame A owned by this wave
    const bool active = wb < A.ntiles;
    const int wbc = active ? wb : 0;
    const int T = B.ntiles;
    auto uniform_ptr = [](const void* q) {
        const unsigned long long u = (unsigned long long)q;
        return (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(u >> 32)) << 32 |
               (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)u);
    };
    const v8h* Af = (const v8h*)frames16[pr.x].frag16;
    const char __attribute__((address_space(1)))* Bf = (const char __attribute__((address_space(1)))*)uniform_ptr(frames16[pr.y].frag16);

    v8h a[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) a[ks] = Af[((size_t)wbc * KS + ks) * 64 + lane];
    float rv1[16], rv2[16];
    int rt[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        rv1[r] = EACHAM_NEG_INF;
        rv2[r] = EACHAM_NEG_INF;
        rt[r] = 0;
    }
    // accumulator register r of this lane is row 32 wb + (r & 3) + 8 (r >> 2) + 4 h: real iff that offset < rows_here
    const int rows_here = A.n - 32 * wb - 4 * h;
    const int cols_left = B.n - cl;  // column 32 t + cl is real iff 32 t < cols_left
    auto stage_tile = [&](int tile, int slot) {  // KS pieces of 1 KiB
#pragma unroll
        for (int i = 0; i < (KS + H_WAVES - 1) / H_WAVES; ++i) {
            const int piece = wave + i * H_WAVES;
            if (piece < KS)
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void*)(Bf + ((size_t)tile * TILE_V + piece * 64 + lane) * 16),
                    (__attribute__((address_space(3))) void*)(&sB[slot][piece * 64]), 16, 0, 0);
        }
    };
    if (T > 0) stage_tile(0, 0);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();

    int4* cp;  // wave-uniform: kept as a scalar base
    {
        const unsigned long long u = (unsigned long long)(colpart + ((size_t)p * wb_stride + wb) * row_stride);
        cp = (int4*)uniform_ptr((const void*)u);
    }
    for (int t = 0; t < T; ++t) {
        const int cur = t & 1;
        stage_tile(min(t + 1, T - 1), cur ^ 1);  // that slot was last read before the previous barrier
        if (active) {
            v16f acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[ks], sB[cur][ks * 64 + lane], acc, 0, 0, 0);
            const bool col_real = 32 * t < cols_left;
            float cv1 = EACHAM_NEG_INF, cv2 = EACHAM_NEG_INF;
            int cr = -1;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ro = (r & 3) + 8 * (r >> 2);
                const bool row_real = ro < rows_here;
                if (DUMP) {
                    if (row_real && col_real) dump[(size_t)(32 * wb + ro + 4 * h) * B.n + 32 * t + cl] = acc[r];
                }
                const float sr = col_real ? acc[r] : EACHAM_NEG_INF;
                const bool lr = sr > rv1[r];  // ascending t: strict '>' keeps the lower column
                rv2[r] = lr ? rv1[r] : fmaxf(rv2[r], sr);
                rt[r] = lr ? t : rt[r];
                rv1[r] = lr ? sr : rv1[r];
                const float sc = row_real ? acc[r] : EACHAM_NEG_INF;
                const bool lc = sc > cv1;     // ascending rows within the lane
                cv2 = lc ? cv1 : fmaxf(cv2, sc);
                cr = lc ? ro + 4 * h : cr;
                cv1 = lc ? sc : cv1;
            }
            // the two lane halves hold interleaved rows of the same column: (value, row) lexicographic merge
            const float ov1 = __shfl_xor(cv1, 32), ov2 = __shfl_xor(cv2, 32);
            const int orow = __shfl_xor(cr, 32);
            const bool take = ov1 > cv1 || (ov1 == cv1 && orow < cr);
            const float n1 = take ? ov1 : cv1, n2 = take ? fmaxf(cv1, ov2) : fmaxf(cv2, ov1);
            if (h == 0) cp[(unsigned)(32 * t + cl)] = make_int4(__float_as_int(n1), 32 * wb + (take ? orow : cr), __float_as_int(n2), 0);
        }
        __syncthreads();
    }
    if (!active) return;
    // every wave is past the last barrier: the tile ring is dead, reuse it for the row transposition
    float* sv1 = (float*)sMem + wave * (3 * 32 * 33);
    float* sv2 = sv1 + 32 * 33;
    int* sc1 = (int*)(sv2 + 32 * 33);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        sv1[row * 33 + cl] = rv1[r];
        sv2[row * 33 + cl] = rv2[r];
        sc1[row * 33 + cl] = 32 * rt[r] + cl;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float b1 = EACHAM_NEG_INF, b2 = EACHAM_NEG_INF;
    int bc = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int idx = cl * 33 + 16 * h + j;
        const float v1 = sv1[idx], v2 = sv2[idx];
        const int c = sc1[idx];
        const bool gt = v1 > b1 || (v1 == b1 && c < bc);
        b2 = gt ? fmaxf(b1, v2) : fmaxf(b2, v1);
        bc = gt ? c : bc;
        b1 = gt ? v1 : b1;
    }
    const float o1 = __shfl_xor(b1, 32), o2 = __shfl_xor(b2, 32);
    const int oc = __shfl_xor(bc, 32);
    if (h == 0) {
        const bool gt = o1 > b1 || (o1 == b1 && oc < bc);
        const float f1 = gt ? o1 : b1, f2 = gt ? fmaxf(b1, o2) : fmaxf(b2, o1);
        rowres[(size_t)p * row_stride + 32 * wb + cl] = make_int4(__float_as_int(f1), gt ? oc : bc, __float_as_int(f2), 0);
    }
}

// ---- K2h: dead / settled / open, the exact score of the settled, the ordered lists of the open -----------------
// s(q, t): the k-ordered fmaf chain from 0 over the padded dimension — the bits of match_tile_dot_kernel's accumulator
__device__ __forceinline__ float dot_chain(const float* __restrict__ fa, int ra, const float* __restrict__ fb, int rb, int D2) {
    float s = 0.0f;
    for (int k = 0; k < 2 * D2; ++k) s = __fmaf_rn(fa[fragf_index(ra, k, D2)], fb[fragf_index(rb, k, D2)], s);
    return s;
}
// 0 = dead, 1 = settled, 2 = open
__device__ __forceinline__ int dot16_state(float s1, float s2, float E, float min_score) {
    if (!(s1 > EACHAM_NEG_INF)) return 0;               // no neighbour at all
    if (next_up(s1 + E) <= min_score) return 0;         // s <= s~1 + E <= min_score: cannot pass the strict threshold
    if (s2 > EACHAM_NEG_INF && next_down(s1 - s2) > next_up(2.0f * E)) return 1;  // s(t~1) > s(t) for every other t
    return 2;
}
constexpr int CLS_T = 256;
// exclusive position of `flag` among the block's threads (ascending tid) and the block's total
__device__ __forceinline__ int block_rank(int flag, int* s_scan, int* total) {
    const int tid = threadIdx.x;
    s_scan[tid] = flag;
    __syncthreads();
    for (int off = 1; off < CLS_T; off <<= 1) {
        const int v = tid >= off ? s_scan[tid - off] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    const int incl = s_scan[tid];
    *total = s_scan[CLS_T - 1];
    __syncthreads();
    return incl - flag;
}
// rr / cpart: what match_finalize_dot_kernel reads — {bits(s), index}, -inf for dead items, the column result in partial 0 and
// -inf in the partials behind it. open_idx[p][0][..] rows, [p][1][..] columns, ascending; open_cnt[p] = their counts.
// tally: 6 x 64-bit {rows dead, settled, open, columns dead, settled, open} (sums: no arrival order reaches an output).
__global__ __launch_bounds__(CLS_T) void dot_screen_classify_kernel(
    const FrameDev* __restrict__ frames, const Frame16Dev* __restrict__ frames16, const int2* __restrict__ pairs,
    const int2* __restrict__ pairs_fb, int empty_frame, const int4* __restrict__ rowres16, const int4* __restrict__ colpart16,
    int wb_stride, int row_stride, int D2, float kappa, float min_score, int2* __restrict__ rr, int2* __restrict__ cpart,
    int* __restrict__ open_idx, int2* __restrict__ open_cnt, unsigned long long* __restrict__ tally) {
    __shared__ int s_scan[CLS_T];
    const int tid = threadIdx.x, p = blockIdx.x;
    if (pairs_fb[p].x != empty_frame) return;
    const int2 pr = pairs[p];
    const FrameDev A = frames[pr.x], B = frames[pr.y];
    const Frame16Dev A16 = frames16[pr.x], B16 = frames16[pr.y];
    const float* fa = (const float*)A.frag;
    const float* fb = (const float*)B.frag;
    const int na = A.n, nb = B.n;
    int cnt0 = 0, cnt1 = 0, cnt2 = 0;
    int base = 0;
    for (int q0 = 0; q0 < na; q0 += CLS_T) {
        const int q = q0 + tid;
        int st = -1;
        if (q < na) {
            const int4 r = rowres16[(size_t)p * row_stride + q];
            const float s1 = nb > 0 ? __int_as_float(r.x) : EACHAM_NEG_INF, s2 = __int_as_float(r.z);
            const float E = next_up(next_up(next_up(kappa * A16.nrm[q]) * B16.maxn) + DOT16_EPS0);
            st = dot16_state(s1, s2, E, min_score);
            if (st == 0) rr[(size_t)p * row_stride + q] = make_int2(__float_as_int(EACHAM_NEG_INF), 0);
            if (st == 1) rr[(size_t)p * row_stride + q] = make_int2(__float_as_int(dot_chain(fa, q, fb, r.y, D2)), r.y);
            cnt0 += st == 0, cnt1 += st == 1, cnt2 += st == 2;
        }
        int total;
        const int pos = block_rank(st == 2, s_scan, &total);
        if (st == 2) open_idx[((size_t)p * 2 + 0) * row_stride + base + pos] = q;
        base += total;
    }
    const int open_rows = base;
    const int wbs = (na + 31) / 32;  // tiles of frame A that hold a real row
    int ccnt0 = 0, ccnt1 = 0, ccnt2 = 0;
    base = 0;
    for (int c0 = 0; c0 < nb; c0 += CLS_T) {
        const int c = c0 + tid;
        int st = -1;
        if (c < nb) {
            float v1 = EACHAM_NEG_INF, v2 = EACHAM_NEG_INF;
            int r1 = -1;
            const int4* cp = colpart16 + (size_t)p * wb_stride * row_stride + c;
            for (int wb = 0; wb < wbs; ++wb) {  // ascending rows; strict '>' keeps the lower row on ties
                const int4 e = cp[(size_t)wb * row_stride];
                const float a1 = __int_as_float(e.x), a2 = __int_as_float(e.z);
                if (a1 > v1) {
                    v2 = fmaxf(v1, a2);
                    v1 = a1;
                    r1 = e.y;
                } else {
                    v2 = fmaxf(v2, a1);
                }
            }
            const float E = next_up(next_up(next_up(kappa * B16.nrm[c]) * A16.maxn) + DOT16_EPS0);
            st = dot16_state(v1, v2, E, min_score);
            int2* out = cpart + (size_t)p * wb_stride * row_stride + c;
            if (st == 1) out[0] = make_int2(__float_as_int(dot_chain(fa, r1, fb, c, D2)), r1);
            else if (st == 0) out[0] = make_int2(__float_as_int(EACHAM_NEG_INF), -1);
            for (int wb = 1; wb < wbs; ++wb) out[(size_t)wb * row_stride] = make_int2(__float_as_int(EACHAM_NEG_INF), -1);
            ccnt0 += st == 0, ccnt1 += st == 1, ccnt2 += st == 2;
        }
        int total;
        const int pos = block_rank(st == 2, s_scan, &total);
        if (st == 2) open_idx[((size_t)p * 2 + 1) * row_stride + base + pos] = c;
        base += total;
    }
    if (tid == 0) open_cnt[p] = make_int2(open_rows, base);
    const int tl[6] = {cnt0, cnt1, cnt2, ccnt0, ccnt1, ccnt2};
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (tl[k]) atomicAdd(&tally[k], (unsigned long long)tl[k]);
}

// ---- K3h: the exact chain of an open item against the whole other frame, one wave per item -----------------------
// Item i of pair p: an open row (i < open rows) against every row of B, or an open column against every row of A (the same
// code, the frames' roles swapped); argmax with strict '>' in ascending index, i.e. the lower index on equal similarity.
constexpr int EXACT_WGS = 8;  // workgroups per pair
__global__ __launch_bounds__(H_THREADS) void dot_exact_rows_kernel(
    const FrameDev* __restrict__ frames, const int2* __restrict__ pairs, const int2* __restrict__ pairs_fb, int empty_frame,
    const int* __restrict__ open_idx, const int2* __restrict__ open_cnt, int wb_stride, int row_stride, int D2,
    int2* __restrict__ rr, int2* __restrict__ cpart) {
    __shared__ float s_own[H_WAVES][256];
    const int p = blockIdx.x / EXACT_WGS, wg = blockIdx.x % EXACT_WGS;  // (grid.x: a launch may hold more than 65 535 pairs)
    if (pairs_fb[p].x != empty_frame) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int2 pr = pairs[p];
    const int2 oc = open_cnt[p];
    float* own = s_own[wave];
    for (int i = wg * H_WAVES + wave; i < oc.x + oc.y; i += EXACT_WGS * H_WAVES) {
        const bool is_row = i < oc.x;
        const FrameDev X = frames[is_row ? pr.x : pr.y], Y = frames[is_row ? pr.y : pr.x];
        const int item = is_row ? open_idx[((size_t)p * 2 + 0) * row_stride + i] : open_idx[((size_t)p * 2 + 1) * row_stride + i - oc.x];
        const float* fx = (const float*)X.frag;
        const float* fy = (const float*)Y.frag;
        __builtin_amdgcn_wave_barrier();  // the previous item's reads of `own` are done
        for (int k = lane; k < 2 * D2; k += 64) own[k] = fx[fragf_index(item, k, D2)];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float best = EACHAM_NEG_INF;
        int bi = 0x7fffffff;
        for (int t = lane; t < Y.n; t += 64) {  // ascending within the lane
            float s = 0.0f;
            // fmaf(x, y, s) == fmaf(y, x, s): the same similarity seen from either side
            for (int k = 0; k < 2 * D2; ++k) s = __fmaf_rn(own[k], fy[fragf_index(t, k, D2)], s);
            if (s > best) {
                best = s;
                bi = t;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ob = __shfl_xor(best, off);
            const int oi = __shfl_xor(bi, off);
            const bool take = ob > best || (ob == best && oi < bi);
            best = take ? ob : best;
            bi = take ? oi : bi;
        }
        if (lane == 0) {
            if (bi == 0x7fffffff) bi = is_row ? 0 : -1;  // nothing compared greater than -inf
            if (is_row) rr[(size_t)p * row_stride + item] = make_int2(__float_as_int(best), bi);
            else cpart[(size_t)p * wb_stride * row_stride + item] = make_int2(__float_as_int(best), bi);
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------
static float dot16_kappa(int D2) {
    // 2^-10 + (D + 16) 2^-22 is a dyadic rational with < 24 significant bits for D <= 256: exact in fp32; one step up anyway
    return next_up((float)(std::ldexp(1.0, -10) + (2.0 * D2 + 16.0) * std::ldexp(1.0, -22)));
}

void free_frame_image16(FrameHost& f) {
    if (f.img16) (void)hipFree(f.img16);
    f.img16 = nullptr;
    f.img16_ready = false;
}

// builds the fp16 image of every frame the pairs name that has none yet, and reads their {max N', flag} back (one wait, only
// on a call that built an image). A frame counts as imaged only once its read-back is in: on any failure every image of this
// call is dropped again, so a later call starts them afresh.
static int build_images16(eacham_ctx* ctx, const int32_t* pairs, int npairs, std::vector<int>& built) {
    for (int i = 0; i < 2 * npairs; ++i) {
        FrameHost& f = ctx->frames[pairs[i]];
        if (f.img16_ready || f.img16) continue;  // imaged, or allocated earlier in this loop
        const int npad = f.ntiles * 32, KS = f.ks / 8;
        if (npad == 0 || !f.frag) {  // an empty frame: nothing to build
            f.img16_maxn = 0.0f;
            f.img16_bad = false;
            f.img16_ready = true;
            continue;
        }
        const size_t frag_bytes = (size_t)f.ntiles * KS * 1024, nrm_bytes = (size_t)npad * sizeof(float);
        if (hipMalloc(&f.img16, frag_bytes + nrm_bytes + 256) != hipSuccess) {
            f.img16 = nullptr;
            return ctx->fail(EACHAM_ERR_HIP, "fp16 image of frame %d: allocation of %zu bytes failed", pairs[i], frag_bytes + nrm_bytes + 256);
        }
        built.push_back(pairs[i]);
        char* base = (char*)f.img16;
        int* meta = (int*)(base + frag_bytes + nrm_bytes);
        EACHAM_HIP_TRY(ctx, hipMemsetAsync(meta, 0, 2 * sizeof(int), ctx->stream));
        const long long work = (long long)f.ntiles * KS * 64;
        pack_f16_kernel<<<(unsigned)((work + 255) / 256), 256, 0, ctx->stream>>>((const float*)f.frag, f.ks, f.ntiles, (int4*)base);
        norm_f16_kernel<<<(npad + 255) / 256, 256, 0, ctx->stream>>>((const float*)f.frag, f.n, f.ks, npad, (float*)(base + frag_bytes), meta);
        EACHAM_HIP_TRY(ctx, hipGetLastError());
    }
    if (built.empty()) return EACHAM_OK;
    EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int> metas(2 * built.size());
    for (size_t k = 0; k < built.size(); ++k) {
        const FrameHost& f = ctx->frames[built[k]];
        const size_t meta_off = (size_t)f.ntiles * (f.ks / 8) * 1024 + (size_t)f.ntiles * 32 * sizeof(float);
        EACHAM_HIP_TRY(ctx, hipMemcpy(&metas[2 * k], (const char*)f.img16 + meta_off, 2 * sizeof(int), hipMemcpyDeviceToHost));
    }
    for (size_t k = 0; k < built.size(); ++k) {  // every read-back is in: now, and only now, the frames count as imaged
        FrameHost& f = ctx->frames[built[k]];
        memcpy(&f.img16_maxn, &metas[2 * k], sizeof(float));
        f.img16_bad = metas[2 * k + 1] != 0;
        f.img16_ready = true;
    }
    return EACHAM_OK;
}
static int ensure_images16(eacham_ctx* ctx, const int32_t* pairs, int npairs) {
    std::vector<int> built;
    const int rc = build_images16(ctx, pairs, npairs, built);
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);  // kernels of this call may still write into the images
        for (int id : built) free_frame_image16(ctx->frames[id]);
    }
    return rc;
}

// the device table of the images, rebuilt per call (a few hundred bytes)
static int sync_table16(eacham_ctx* ctx) {
    const int need = (int)ctx->frames.size() + 1;
    if (need > ctx->table16_cap) {
        if (ctx->table16_dev) {
            EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            EACHAM_HIP_TRY(ctx, hipFree(ctx->table16_dev));
            ctx->table16_dev = nullptr;
            ctx->table16_cap = 0;
        }
        const int cap = need < 64 ? 64 : need * 2;
        EACHAM_HIP_TRY(ctx, hipMalloc(&ctx->table16_dev, sizeof(Frame16Dev) * cap));
        ctx->table16_cap = cap;
    }
    std::vector<Frame16Dev> tab(need);
    for (int i = 0; i < need; ++i) {
        Frame16Dev& e = tab[i];
        e.frag16 = nullptr, e.nrm = nullptr, e.maxn = 0.0f, e.pad = 0;
        if (i + 1 == need) continue;  // the empty stand-in frame
        const FrameHost& f = ctx->frames[i];
        if (!f.img16) continue;
        e.frag16 = (const int4*)f.img16;
        e.nrm = (const float*)((const char*)f.img16 + (size_t)f.ntiles * (f.ks / 8) * 1024);
        e.maxn = f.img16_maxn;
    }
    // pageable source: hipMemcpyAsync stages it before returning, so `tab` may die here
    EACHAM_HIP_TRY(ctx, hipMemcpyAsync(ctx->table16_dev, tab.data(), sizeof(Frame16Dev) * need, hipMemcpyHostToDevice, ctx->stream));
    return EACHAM_OK;
}

static unsigned long long* dot16_tally(eacham_ctx* ctx) { return ctx->flag_dev->dot16; }

template <bool DUMP>
static void launch_tile16(eacham_ctx* ctx, int grid, const int2* pb, const int2* fb, int empty, const MatchPlanF32& pl, int4* rr16,
                          int4* cp16, float* dump) {
    const Frame16Dev* t16 = (const Frame16Dev*)ctx->table16_dev;
    switch (ctx->ks_common) {
        case 32: match_tile_dot16_kernel<4, DUMP><<<grid, H_THREADS, 0, ctx->stream>>>(ctx->frame_table_dev, t16, pb, fb, empty, pl.wgs_per_pair, rr16, cp16, pl.wb_stride, pl.row_stride, dump); break;
        case 64: match_tile_dot16_kernel<8, DUMP><<<grid, H_THREADS, 0, ctx->stream>>>(ctx->frame_table_dev, t16, pb, fb, empty, pl.wgs_per_pair, rr16, cp16, pl.wb_stride, pl.row_stride, dump); break;
        default: match_tile_dot16_kernel<16, DUMP><<<grid, H_THREADS, 0, ctx->stream>>>(ctx->frame_table_dev, t16, pb, fb, empty, pl.wgs_per_pair, rr16, cp16, pl.wb_stride, pl.row_stride, dump); break;
    }
}

// fills pairs_fb (npairs x 2): a pair with an unscreenable frame keeps its frames (the fp32 tile kernel runs it), every other
// pair names the empty stand-in frame twice (that kernel leaves at once); builds the images the screened pairs need
int prepare_match_dot_screened(eacham_ctx* ctx, const int32_t* pairs, int npairs, int32_t* pairs_fb, int* n_fallback) {
    int rc = ensure_images16(ctx, pairs, npairs);
    if (rc) return rc;
    const int empty = (int)ctx->frames.size();
    int nfb = 0;
    for (int p = 0; p < npairs; ++p) {
        const bool fb = ctx->frames[pairs[2 * p]].img16_bad || ctx->frames[pairs[2 * p + 1]].img16_bad;
        pairs_fb[2 * p] = fb ? pairs[2 * p] : empty;
        pairs_fb[2 * p + 1] = fb ? pairs[2 * p + 1] : empty;
        nfb += fb;
    }
    *n_fallback = nfb;
    return sync_table16(ctx);
}

// The mutual form only. pairs_fb_host is prepare_match_dot_screened's list (host copy: which launches need the fp32 kernel).
int run_match_dot_screened(eacham_ctx* ctx, const int2* pairs_dev, const int2* pairs_fb_dev, const int32_t* pairs_fb_host, int npairs,
                           int n_fallback, float min_score, int min_dir, int min_mutual, int* counts_dev, long long* offsets_dev,
                           uint2* edges_dev, float* scores_dev, long long edge_cap, long long* total_dev, int4* stats_dev) {
    const MatchPlanF32 pl = plan_match_f32(ctx, npairs);
    int rc = ensure_workspace(ctx, pl.total_screened);
    if (rc) return rc;
    const F32Arrays a = pl.carve(ctx->ws, true);   // (the {bits, index} arrays of the fp32 form are what the finalize pass reads)
    int2 *rr = a.rowres_dot, *cp = a.colpart_dot;
    const int empty = (int)ctx->frames.size();
    const int D2 = ctx->ks_common;
    const float kappa = dot16_kappa(D2);
    EACHAM_HIP_TRY(ctx, hipMemsetAsync(dot16_tally(ctx), 0, 6 * sizeof(unsigned long long), ctx->stream));
    ctx->dot16_fallback_pairs = n_fallback;
    for (int first = 0; first < npairs; first += pl.batch) {
        const int nb = std::min(pl.batch, npairs - first);
        const int2* pb = pairs_dev + first;
        const int2* fb = pairs_fb_dev + first;
        const int grid = nb * pl.wgs_per_pair;
        int fb_here = 0;
        for (int p = first; p < first + nb; ++p) fb_here += pairs_fb_host[2 * p] != empty;
        {
            ProfileScope ps(ctx, EACHAM_KERNEL_MATCH_TILE);
            if (fb_here < nb) {
                launch_tile16<false>(ctx, grid, pb, fb, empty, pl, a.rr16, a.cp16, nullptr);
                dot_screen_classify_kernel<<<nb, CLS_T, 0, ctx->stream>>>(ctx->frame_table_dev, (const Frame16Dev*)ctx->table16_dev, pb, fb, empty,
                                                                          a.rr16, a.cp16, pl.wb_stride, pl.row_stride, D2, kappa, min_score, rr, cp,
                                                                          a.open_idx, a.open_cnt, dot16_tally(ctx));
                dot_exact_rows_kernel<<<nb * EXACT_WGS, H_THREADS, 0, ctx->stream>>>(ctx->frame_table_dev, pb, fb, empty, a.open_idx, a.open_cnt,
                                                                                 pl.wb_stride, pl.row_stride, D2, rr, cp);
            }
            if (fb_here > 0) launch_match_tile_dot(ctx, fb, nb, pl, rr, cp);  // screened pairs name the empty frame there
        }
        rc = launch_match_dot_tail(ctx, pl, a, pb, nb, first, first + nb == npairs, min_score, min_dir, min_mutual, 0, counts_dev,
                                   offsets_dev, edges_dev, scores_dev, edge_cap, total_dev, stats_dev);
        if (rc) return rc;
    }
    return EACHAM_OK;
}

}  // namespace eacham

using namespace eacham;

extern "C" int eacham_match_debug_dot_screen(eacham_ctx* ctx, int64_t* out) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    if (!out) return ctx->fail(EACHAM_ERR_INVALID, "null output");
    unsigned long long t[6] = {0, 0, 0, 0, 0, 0};
    EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    EACHAM_HIP_TRY(ctx, hipMemcpy(t, dot16_tally(ctx), sizeof(t), hipMemcpyDeviceToHost));
    for (int k = 0; k < 6; ++k) out[k] = (int64_t)t[k];
    out[6] = ctx->dot16_fallback_pairs;
    return EACHAM_OK;
}

extern "C" int eacham_match_debug_dot_coarse(eacham_ctx* ctx, int f1, int f2, float* s_coarse, float* row_E, float* col_E) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    try {
        for (int f : {f1, f2})
            if (f < 0 || (size_t)f >= ctx->frames.size() || ctx->frames[f].n < 0)
                return ctx->fail(EACHAM_ERR_INVALID, "frame %d is not resident", f);
        if (ctx->kind_common != FRAME_F32)
            return ctx->fail(EACHAM_ERR_UNSUPPORTED, "dot-product matching needs float frames (eacham_upload_descriptors_f32); the resident frames are int8");
        const int n1 = ctx->frames[f1].n, n2 = ctx->frames[f2].n;
        if (n1 > 4096 || n2 > 4096) return ctx->fail(EACHAM_ERR_CAPACITY, "the coarse scores are for frames of <= 4096 rows (%d x %d)", n1, n2);
        if ((n1 > 0 && n2 > 0 && !s_coarse) || (n1 > 0 && !row_E) || (n2 > 0 && !col_E)) return ctx->fail(EACHAM_ERR_INVALID, "null output");
        int rc = sync_frame_table(ctx);
        if (rc) return rc;
        const int32_t pr[2] = {f1, f2};
        int32_t fbp[2];
        int nfb = 0;
        rc = prepare_match_dot_screened(ctx, pr, 1, fbp, &nfb);
        if (rc) return rc;
        if (nfb) return ctx->fail(EACHAM_ERR_UNSUPPORTED, "a frame of the pair holds a value that is not finite or beyond the fp16 range: it is not screened");
        const MatchPlanF32 pl = plan_match_f32(ctx, 1);
        // one pair's sweep arrays, its n1 x n2 coarse scores and the pair itself (a null base: the bytes)
        int4 *rr16, *cp16;
        float* dump;
        int2* pair;
        auto carve = [&](void* base) {
            Bump b(base);
            rr16 = b.take<int4>((size_t)pl.row_stride), cp16 = b.take<int4>((size_t)pl.wb_stride * pl.row_stride);
            dump = b.take<float>((size_t)n1 * n2), pair = b.take<int2>(1);
            return b.off;
        };
        rc = ensure_workspace(ctx, carve(nullptr));
        if (rc) return rc;
        carve(ctx->ws);
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(pair, pr, sizeof(pr), hipMemcpyHostToDevice, ctx->stream));
        launch_tile16<true>(ctx, pl.wgs_per_pair, pair, nullptr, 0, pl, rr16, cp16, dump);
        EACHAM_HIP_TRY(ctx, hipGetLastError());
        if (n1 > 0 && n2 > 0)
            EACHAM_HIP_TRY(ctx, hipMemcpyAsync(s_coarse, dump, (size_t)n1 * n2 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        // the bounds as the classify kernel computes them, from the stored norm bounds
        const FrameHost &A = ctx->frames[f1], &B = ctx->frames[f2];
        std::vector<float> na((size_t)std::max(n1, 1)), nb((size_t)std::max(n2, 1));
        if (n1 > 0) EACHAM_HIP_TRY(ctx, hipMemcpyAsync(na.data(), (char*)A.img16 + (size_t)A.ntiles * (A.ks / 8) * 1024, n1 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (n2 > 0) EACHAM_HIP_TRY(ctx, hipMemcpyAsync(nb.data(), (char*)B.img16 + (size_t)B.ntiles * (B.ks / 8) * 1024, n2 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const float kappa = dot16_kappa(ctx->ks_common);
        for (int q = 0; q < n1; ++q) row_E[q] = next_up(next_up(next_up(kappa * na[q]) * B.img16_maxn) + DOT16_EPS0);
        for (int c = 0; c < n2; ++c) col_E[c] = next_up(next_up(next_up(kappa * nb[c]) * A.img16_maxn) + DOT16_EPS0);
        return EACHAM_OK;
    } catch (const std::exception& e) {
        return ctx->fail(EACHAM_ERR_INVALID, "dot-product screen: %s", e.what());
    } catch (...) {
        return ctx->fail(EACHAM_ERR_INVALID, "dot-product screen: unknown exception");
    }
}
