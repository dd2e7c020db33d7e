// matcher_dot.hip — dot-product form of the float-descriptor matcher: mutual nearest neighbour on the similarity
//     s(q,t) = a_q . b_t      fp32, the k-ordered fmaf chain from 0 of v_mfma_f32_32x32x2_f32
// with a score threshold, the brute-force rule for SuperPoint-class descriptors (the reference's LightGlue plug-in keeps
// a match by its score, `mscores0 > 0.5`, FeatureMatcherLightglue.cpp:118, and hands the score on).
//
// Same frames, fragment layout, LDS ring, launch bounds and batch plan as the L2 form in matcher_f32.hip; what differs is
// the epilogue: row and column top-1 by MAXIMUM as (value, index) pairs, no norm loads, no second neighbour. Nothing is
// normalised: the caller's values are used as they are.
//
// Padding: a padded row has zero fragments and scores exactly 0, which beats every negative similarity, so rows and
// columns at or beyond the frame's n are excluded BY INDEX — in the row results, the column partials and the finalize
// pass (the L2 form keeps them out by their norm PAD_F instead). "No neighbour" is the pair (-inf, any index): every
// comparison is a strict '>', so -inf and NaN similarities never win and never pass a threshold; ties resolve to the
// lower index like every other path.
#include "context.hpp"
#include "match_plan.hpp"
#include "match_tail.hpp"

#include <algorithm>

namespace eacham {

typedef float v16f __attribute__((ext_vector_type(16)));
typedef const float __attribute__((address_space(1)))* gfloat_t;

constexpr int F_THREADS = 256, F_WAVES = 4;
static_assert(PLAN_F32_WG_TILES == F_WAVES, "match_plan.hpp plans for these kernels");
#define EACHAM_NEG_INF (-__builtin_inff())

// ---- K1d: similarity tiles + fused row/column top-1 ---------------------------------------------------
// rowres[p][q]       = {bits(s), col}     final over the columns < B.n
// colpart[p][wb][c]  = {bits(s), row}     over the rows < A.n of tile wb of frame A
template <int D2>
__global__ __launch_bounds__(F_THREADS, 2) void match_tile_dot_kernel(
    const FrameDev* __restrict__ frames, const int2* __restrict__ pairs, int wgs_per_pair,
    int2* __restrict__ rowres, int2* __restrict__ colpart, int wb_stride, int row_stride) {
    constexpr int TILE_F = 64 * D2;  // floats per 32-row tile
    constexpr int SLABS_F = F_WAVES * 2 * 32 * 33;
    constexpr int LDS_F = 2 * TILE_F > SLABS_F ? 2 * TILE_F : SLABS_F;
    __shared__ float sMem[LDS_F];    // 2-slot tile ring; after the sweep reused as the row slabs
    float (*sB)[TILE_F] = reinterpret_cast<float (*)[TILE_F]>(sMem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cl = lane & 31, h = lane >> 5;
    const int p = blockIdx.x / wgs_per_pair, rb = blockIdx.x % wgs_per_pair;
    const int2 pr = pairs[p];
    const FrameDev A = frames[pr.x], B = frames[pr.y];
    if (rb * F_WAVES >= A.ntiles) return;  // workgroup-uniform
    const int wb = rb * F_WAVES + wave;    // 32-row tile of frame A owned by this wave
    const bool active = wb < A.ntiles;
    const int wbc = active ? wb : 0;
    const int T = B.ntiles;
    auto uniform_ptr = [](const void* q) {
        const unsigned long long u = (unsigned long long)q;
        return (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(u >> 32)) << 32 |
               (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)u);
    };
    const gfloat_t Af = (gfloat_t)A.frag, Bf = (gfloat_t)uniform_ptr(B.frag);

    float a[D2];
#pragma unroll
    for (int k2 = 0; k2 < D2; ++k2) a[k2] = Af[((size_t)wbc * D2 + k2) * 64 + lane];
    float rv[16];
    int rt[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        rv[r] = EACHAM_NEG_INF;
        rt[r] = 0;
    }
    // accumulator register r of this lane is row 32 wb + (r & 3) + 8 (r >> 2) + 4 h: real iff that offset < rows_here
    const int rows_here = A.n - 32 * wb - 4 * h;
    const int cols_left = B.n - cl;  // column 32 t + cl is real iff 32 t < cols_left
    constexpr int PIECES = TILE_F / 256;  // 1 KiB LDS-DMA pieces per tile
    auto stage_tile = [&](int tile, int slot) {
#pragma unroll
        for (int i = 0; i < (PIECES + F_WAVES - 1) / F_WAVES; ++i) {
            const int piece = wave + i * F_WAVES;
            if (piece < PIECES)
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void*)(Bf + (size_t)tile * TILE_F + piece * 256 + lane * 4),
                    (__attribute__((address_space(3))) void*)(&sB[slot][piece * 256]), 16, 0, 0);
        }
    };
    if (T > 0) stage_tile(0, 0);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();

    int2* cp;  // wave-uniform: kept as a scalar base
    {
        const unsigned long long u = (unsigned long long)(colpart + ((size_t)p * wb_stride + wb) * row_stride);
        cp = (int2*)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(u >> 32)) << 32) |
                     (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)u));
    }
    for (int t = 0; t < T; ++t) {
        const int cur = t & 1;
        stage_tile(min(t + 1, T - 1), cur ^ 1);  // that slot was last read before the previous barrier
        if (active) {
            v16f acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int k2 = 0; k2 < D2; ++k2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k2], sB[cur][k2 * 64 + lane], acc, 0, 0, 0);
            const bool col_real = 32 * t < cols_left;
            float cv = EACHAM_NEG_INF;
            int cr = -1;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float s = acc[r];
                const bool lr = col_real && s > rv[r];  // ascending t: strict '>' keeps the lower column
                rt[r] = lr ? t : rt[r];
                rv[r] = lr ? s : rv[r];
                const int ro = (r & 3) + 8 * (r >> 2);
                const bool lc = ro < rows_here && s > cv;  // ascending rows within the lane
                cr = lc ? ro + 4 * h : cr;
                cv = lc ? s : cv;
            }
            // the two lane halves hold interleaved rows of the same column: (value, row) lexicographic merge
            const float ov = __shfl_xor(cv, 32);
            const int orow = __shfl_xor(cr, 32);
            const bool take = ov > cv || (ov == cv && orow < cr);
            if (h == 0) cp[(unsigned)(32 * t + cl)] = make_int2(__float_as_int(take ? ov : cv), 32 * wb + (take ? orow : cr));
        }
        __syncthreads();
    }
    if (!active) return;
    // every wave is past the last barrier: the tile ring is dead, reuse it for the row transposition
    float* sv = sMem + wave * (2 * 32 * 33);
    int* sc = (int*)(sv + 32 * 33);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        sv[row * 33 + cl] = rv[r];
        sc[row * 33 + cl] = 32 * rt[r] + cl;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float b = EACHAM_NEG_INF;
    int bc = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int idx = cl * 33 + 16 * h + j;
        const float v = sv[idx];
        const int c = sc[idx];
        const bool gt = v > b || (v == b && c < bc);
        bc = gt ? c : bc;
        b = gt ? v : b;
    }
    const float o = __shfl_xor(b, 32);
    const int oc = __shfl_xor(bc, 32);
    if (h == 0) {
        const bool gt = o > b || (o == b && oc < bc);
        rowres[(size_t)p * row_stride + 32 * wb + cl] = make_int2(__float_as_int(gt ? o : b), gt ? oc : bc);
    }
}

// ---- K2d: merge of the column partials, threshold, mutual check, thresholds, ordered compaction -------------
__global__ __launch_bounds__(FIN_THREADS) void match_finalize_dot_kernel(
    const FrameDev* __restrict__ frames, const int2* __restrict__ pairs, const int2* __restrict__ rowres,
    const int2* __restrict__ colpart, int wb_stride, int row_stride, float min_score, int min_dir, int min_mutual,
    int mode, uint2* __restrict__ out_matches, int* __restrict__ counts, int4* __restrict__ stats) {
    extern __shared__ int smem[];
    const int tid = threadIdx.x, p = blockIdx.x;
    const int2 pr = pairs[p];
    const FrameDev A = frames[pr.x], B = frames[pr.y];
    int* fwd = smem;
    int* bwd = smem + row_stride;
    __shared__ int s_cnt[2];
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    int c12 = 0, c21 = 0;
    const int na = A.n, nb = B.n;  // rows / columns at or beyond these are padding: never read
    for (int q = tid; q < na; q += FIN_THREADS) {
        const int2 r = rowres[(size_t)p * row_stride + q];
        const bool ok = nb > 0 && __int_as_float(r.x) > min_score;  // strict; -inf ("no neighbour") never passes
        fwd[q] = ok ? r.y : -1;
        c12 += ok;
    }
    if (mode == 0) {
        const int wbs = (na + 31) / 32;  // tiles of frame A that hold a real row
        for (int c = tid; c < nb; c += FIN_THREADS) {
            float v = EACHAM_NEG_INF;
            int r1 = -1;
            const int2* cp = colpart + (size_t)p * wb_stride * row_stride + c;
            for (int wb = 0; wb < wbs; ++wb) {  // ascending rows; strict '>' keeps the lower row on ties
                const int2 e = cp[(size_t)wb * row_stride];
                const float s = __int_as_float(e.x);
                if (s > v) {
                    v = s;
                    r1 = e.y;
                }
            }
            const bool ok = v > min_score;
            bwd[c] = ok ? r1 : -1;
            c21 += ok;
        }
    }
    atomicAdd(&s_cnt[0], c12);
    atomicAdd(&s_cnt[1], c21);
    __syncthreads();
    const int base = compact_kept_rows(na, tid, out_matches + (size_t)p * row_stride, [&](int q) {
        const int t = fwd[q];
        return t >= 0 && (mode == 1 || bwd[t] == q) ? t : -1;
    });
    if (tid == 0) write_pair_result(p, mode, s_cnt[0], s_cnt[1], base, min_dir, min_mutual, counts, stats);
}

// edges + scores of a launch into the CSR arrays; the score of (q, t) is the row result of q, still in the workspace
__global__ void compact_dot_kernel(const uint2* __restrict__ matches, const int2* __restrict__ rowres, const int* __restrict__ counts,
                                   const long long* __restrict__ offsets, int row_stride, uint2* __restrict__ edges,
                                   float* __restrict__ scores, long long edge_cap) {
    const int p = blockIdx.x;
    const int n = counts[p];
    const long long off = offsets[p];
    for (int k = threadIdx.x; k < n; k += blockDim.x)
        if (off + k < edge_cap) {
            const uint2 e = matches[(size_t)p * row_stride + k];
            edges[off + k] = e;
            scores[off + k] = __int_as_float(rowres[(size_t)p * row_stride + e.x].x);
        }
}

void launch_match_tile_dot(eacham_ctx* ctx, const int2* pb, int nb, const MatchPlanF32& pl, int2* rr, int2* cp) {
    const int grid = nb * pl.wgs_per_pair;
    switch (ctx->ks_common) {
        case 32: match_tile_dot_kernel<32><<<grid, F_THREADS, 0, ctx->stream>>>(ctx->frame_table_dev, pb, pl.wgs_per_pair, rr, cp, pl.wb_stride, pl.row_stride); break;
        case 64: match_tile_dot_kernel<64><<<grid, F_THREADS, 0, ctx->stream>>>(ctx->frame_table_dev, pb, pl.wgs_per_pair, rr, cp, pl.wb_stride, pl.row_stride); break;
        default: match_tile_dot_kernel<128><<<grid, F_THREADS, 0, ctx->stream>>>(ctx->frame_table_dev, pb, pl.wgs_per_pair, rr, cp, pl.wb_stride, pl.row_stride); break;
    }
}

// finalize, scan of the counts and compaction of one launch's pairs [first, first + nb)
int launch_match_dot_tail(eacham_ctx* ctx, const MatchPlanF32& pl, const F32Arrays& a, const int2* pb, int nb, int first, bool is_last,
                          float min_score, int min_dir, int min_mutual, int mode, int* counts_dev, long long* offsets_dev,
                          uint2* edges_dev, float* scores_dev, long long edge_cap, long long* total_dev, int4* stats_dev) {
    const size_t fin_smem = (size_t)2 * pl.row_stride * sizeof(int);
    if (fin_smem > 48 * 1024)
        EACHAM_HIP_TRY(ctx, hipFuncSetAttribute((const void*)match_finalize_dot_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fin_smem));
    int2 *rr = a.rowres_dot, *cp = a.colpart_dot;
    uint2* mt = a.matches;
    {
        ProfileScope ps(ctx, EACHAM_KERNEL_MATCH_FINALIZE);
        int* cnt = counts_dev + first;
        match_finalize_dot_kernel<<<nb, FIN_THREADS, fin_smem, ctx->stream>>>(ctx->frame_table_dev, pb, rr, cp, pl.wb_stride, pl.row_stride, min_score,
                                                                       min_dir, min_mutual, mode, mt, cnt, stats_dev ? stats_dev + first : nullptr);
        launch_scan_counts(ctx, cnt, nb, offsets_dev, total_dev, first, is_last);
        compact_dot_kernel<<<nb, 256, 0, ctx->stream>>>(mt, rr, cnt, offsets_dev + first, pl.row_stride, edges_dev, scores_dev, edge_cap);
    }
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return EACHAM_OK;
}

// mode 0 = mutual + thresholds, mode 1 = directed lists; CSR over the pairs either way
int run_match_dot(eacham_ctx* ctx, const int2* pairs_dev, int npairs, float min_score, int min_dir, int min_mutual, int mode,
                  int* counts_dev, long long* offsets_dev, uint2* edges_dev, float* scores_dev, long long edge_cap,
                  long long* total_dev, int4* stats_dev) {
    const MatchPlanF32 pl = plan_match_f32(ctx, npairs);
    int rc = ensure_workspace(ctx, pl.total);
    if (rc) return rc;
    const F32Arrays a = pl.carve(ctx->ws);
    for (int first = 0; first < npairs; first += pl.batch) {
        const int nb = std::min(pl.batch, npairs - first);
        const int2* pb = pairs_dev + first;
        {
            ProfileScope ps(ctx, EACHAM_KERNEL_MATCH_TILE);
            launch_match_tile_dot(ctx, pb, nb, pl, a.rowres_dot, a.colpart_dot);
        }
        rc = launch_match_dot_tail(ctx, pl, a, pb, nb, first, first + nb == npairs, min_score, min_dir, min_mutual, mode, counts_dev,
                                   offsets_dev, edges_dev, scores_dev, edge_cap, total_dev, stats_dev);
        if (rc) return rc;
    }
    return EACHAM_OK;
}

}  // namespace eacham
