// matcher_ham_wide.hip — binary descriptors of up to 512 bits (BRISK, FREAK: 64 bytes; AKAZE's default MLDB: 61 bytes) under
// Hamming distance, on the FP4 matrix cores. The results are those of the narrow kind (matcher_ham.hip), documented in
// include/eacham_hip.h: cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) + the ratio test on (float)h0 / (float)h1.
//
// The 0 / 255 embedding of matcher_ham.hip ends at 256 bits (the int8 sweeps' dimension, and 65025 h in fp32). Wide rows are a kind
// of their own (3) with a sweep of their own, Hamming-native:
//   a bit is the E2M1 number +1.0 (code 0x2) or -1.0 (0xA); padding bits and padding rows are 0.0 (0x0);
//   the query operand has its sign nibbles flipped at load, the train operand carries the E8M0 scale 2^13, the query operand 2^0:
//   a product is -2^13 where the bits agree, +2^13 where they differ, and a chain over a row sums to 2^14 h - 2^13 D, D = 8 bytes_per_row;
//   the accumulator starts at 2^13 D + idx, idx = the train row (< 2^14): it ends as the KEY 2^14 h + idx.
// Every partial sum is an integer in [0, 2^24): exact in f32 in any order (the property the FP6 screen of matcher.hip rests on), so
// there is no screen, no bound and no second pass. The float order of the keys is the order of (h, idx): ties go to the lower train
// index with no extra work, and the runner-up's distance is the second smallest key >> 14. A padding train row starts at 2^25 and
// stays there (its products are zeros): it never wins, and a key >= 2^24 reads "no neighbour".
//
// v_mfma_scale_f32_32x32x64_f8f6f4 with FP4 operands (cbsz 4, blgp 4) takes K = 64 in the cycles v_mfma_i32_32x32x32_i8 takes for
// K = 32: a 512-bit row costs the matrix pipe what a 256-D int8 row costs. The train tile is the A operand (its rows land in the 16
// accumulator registers), the wave's query rows the B operand (a lane is a query row): the top-2 update is in-lane, v_min_f32 +
// v_med3_f32 per accumulator; the two lane halves (which hold different train rows of the same query) merge once, after the sweep.
// Which k a nibble of a fragment stands for does not matter to a sum over k as long as both operands agree, and they do: one image,
// one layout, both roles.
//
// Resident image, per frame: [ntiles][KS][64] int4, KS = ceil(D / 64) in 1..8; lane l = 32 half + r of step s of tile t holds the 32
// codes of bits 64 s + 32 half .. + 31 of row 32 t + r. A step of a tile is one 1 KiB piece: global_load_lds width 16 stages it.
// The packed rows are kept too (16 words per row, FrameHost::bits, behind the image in frag's allocation) and give every emitted
// match its distance by popcount, a path independent of the sweep and shared with the narrow kind (hamming_distances, matcher_ham.hip).
// The frame slot, the frame table, the sanitised pair list and the pair tail (match_tail.hpp) are the shared ones.
//
// Both directions: the sweep runs on (f1, f2) and on (f2, f1) — see DESIGN.md 3.7.
#include "context.hpp"
#include "match_plan.hpp"
#include "match_tail.hpp"

#include <algorithm>

namespace eacham {

typedef int hw_v4i __attribute__((ext_vector_type(4)));
typedef int hw_v8i __attribute__((ext_vector_type(8)));
typedef float hw_v16f __attribute__((ext_vector_type(16)));
typedef const hw_v4i __attribute__((address_space(1)))* hw_gfrag_t;

constexpr int HW_THREADS = 256, HW_WAVES = 4;
constexpr int HW_NSUB = 2;                       // 32-row query tiles per wave
constexpr int HW_WG_TILES = HW_WAVES * HW_NSUB;  // query tiles per workgroup
constexpr int HW_MAX_ROWS = 16384;               // the key's index field is 14 bits
constexpr int HW_MAX_BYTES = 64;
constexpr float HW_PAD = 33554432.0f;            // 2^25: the C-init of a padding train row, and "no neighbour"
constexpr float HW_KEY_END = 16777216.0f;        // 2^24: real keys lie below
constexpr int HW_SCALE_TRAIN = (int)0x8c8c8c8cu; // E8M0 2^13 in every byte
constexpr int HW_SCALE_QUERY = 0x7f7f7f7f;       // E8M0 2^0

// thread per (stored row, k-step, lane half): four bytes of the packed row -> four words of eight codes each. Bytes at or beyond
// bytes_per_row and rows at or beyond n are the zero codes of the padding.
__global__ void ham_wide_image_kernel(const unsigned char* __restrict__ packed, int n, int bytes_per_row, int ks, int npad,
                                      int4* __restrict__ img) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)npad * ks * 2) return;
    const int half = (int)(idx & 1), s = (int)((idx >> 1) % ks), row = (int)((idx >> 1) / ks);
    unsigned w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = 8 * s + 4 * half + k;
        unsigned word = 0u;
        if (row < n && j < bytes_per_row) {
            const unsigned v = packed[(size_t)row * bytes_per_row + j];
#pragma unroll
            for (int i = 0; i < 8; ++i) word |= ((v >> (7 - i)) & 1u ? 0x2u : 0xAu) << (4 * i);
        }
        w[k] = word;
    }
    img[((size_t)(row >> 5) * ks + s) * 64 + 32 * half + (row & 31)] = make_int4((int)w[0], (int)w[1], (int)w[2], (int)w[3]);
}

// ---- the sweep: rowres[(p ndir + dir)][q] = {smallest key, second smallest key} of query row q over the train frame's rows ----
// dir 0 is (pairs[p].x -> pairs[p].y), dir 1 the reverse. A workgroup owns 8 query tiles (4 waves x 2) and sweeps every train tile
// through a two-slot LDS-DMA ring; the accumulators are double-buffered (the epilogue of tile t - 1 stands beside the chains of tile t).
template <int KS>
__global__ __launch_bounds__(HW_THREADS, 2) void ham_wide_sweep_kernel(const FrameDev* __restrict__ frames, const int2* __restrict__ pairs,
                                                                       int wgs_per_pair, int ndir, float2* __restrict__ rowres,
                                                                       int row_stride, float cbase) {
    constexpr int TILE_V4 = KS * 64;
    __shared__ hw_v4i sB[2][TILE_V4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cl = lane & 31, h = lane >> 5;
    const int rb = blockIdx.x % wgs_per_pair, pd = blockIdx.x / wgs_per_pair;
    const int p = pd / ndir, dir = pd % ndir;
    const int2 pr = pairs[p];
    const FrameDev A = frames[dir ? pr.y : pr.x], B = frames[dir ? pr.x : pr.y];
    const int A_tiles = (A.n + 31) >> 5, T = (B.n + 31) >> 5, Bn = B.n;
    if (rb * HW_WG_TILES >= A_tiles) return;  // workgroup-uniform
    const int wb = rb * HW_WAVES + wave;
    const bool active = HW_NSUB * wb < A_tiles;   // (a frame's allocated tiles are a multiple of HW_NSUB: tile HW_NSUB wb + 1 exists)
    const int wbc = active ? wb : 0;
    const hw_gfrag_t Af = (hw_gfrag_t)A.frag, Bf = (hw_gfrag_t)B.frag;

    hw_v4i q[HW_NSUB][KS];   // the wave's 64 query rows with the sign nibbles flipped: the B operand
#pragma unroll
    for (int s = 0; s < HW_NSUB; ++s)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const hw_v4i v = Af[((size_t)(HW_NSUB * wbc + s) * KS + ks) * 64 + lane];
            q[s][ks] = v ^ (int)0x88888888u;
        }
    float m1[HW_NSUB], m2[HW_NSUB];
    hw_v16f accA[HW_NSUB], accB[HW_NSUB];
#pragma unroll
    for (int s = 0; s < HW_NSUB; ++s) {
        m1[s] = HW_PAD, m2[s] = HW_PAD;
#pragma unroll
        for (int r = 0; r < 16; ++r) accA[s][r] = HW_PAD, accB[s][r] = HW_PAD;
    }
    auto stage_tile = [&](int tile, int slot) {
#pragma unroll
        for (int i = 0; i < (KS + HW_WAVES - 1) / HW_WAVES; ++i) {
            const int piece = wave + i * HW_WAVES;
            if (piece < KS)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Bf + ((size_t)tile * KS + piece) * 64 + lane),
                                                 (__attribute__((address_space(3))) void*)(&sB[slot][piece * 64]), 16, 0, 0);
        }
    };
    // C-init of the chains on train tile t: accumulator r is train row 32 t + (r & 3) + 8 (r >> 2) + 4 h
    auto cinit_of = [&](int t) {
        hw_v16f c;
        const int row0 = 32 * t + 4 * h;
        if (32 * t + 32 <= Bn) {
            const float base = cbase + (float)row0;
#pragma unroll
            for (int r = 0; r < 16; ++r) c[r] = base + (float)((r & 3) + 8 * (r >> 2));
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row0 + (r & 3) + 8 * (r >> 2);
                c[r] = row < Bn ? cbase + (float)row : HW_PAD;
            }
        }
        return c;
    };
    // chains of tile t (ring slot t & 1) into `nxt`, top-2 update from `cur` (tile t - 1; padding values ahead of tile 0)
    auto step = [&](hw_v16f(&nxt)[HW_NSUB], hw_v16f(&cur)[HW_NSUB], int t) {
        stage_tile(min(t + 1, T - 1), (t + 1) & 1);   // that slot was last read before the previous barrier
        if (active) {
            const hw_v16f c0 = cinit_of(t);
            const hw_v4i* sT = sB[t & 1];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const hw_v4i f = sT[ks * 64 + lane];
                const hw_v8i a8 = hw_v8i{f[0], f[1], f[2], f[3], 0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < HW_NSUB; ++s) {
                    const hw_v8i b8 = hw_v8i{q[s][ks][0], q[s][ks][1], q[s][ks][2], q[s][ks][3], 0, 0, 0, 0};
                    nxt[s] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, ks ? nxt[s] : c0, 4, 4, 0, HW_SCALE_TRAIN, 0, HW_SCALE_QUERY);
                }
            }
#pragma unroll
            for (int s = 0; s < HW_NSUB; ++s)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float x = cur[s][r];
                    m2[s] = __builtin_amdgcn_fmed3f(m1[s], m2[s], x);   // m1 <= m2: the median is the new second smallest
                    m1[s] = fminf(m1[s], x);
                }
        }
        __syncthreads();
    };
    auto consume_last = [&](hw_v16f(&cur)[HW_NSUB]) {
#pragma unroll
        for (int s = 0; s < HW_NSUB; ++s)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float x = cur[s][r];
                m2[s] = __builtin_amdgcn_fmed3f(m1[s], m2[s], x);
                m1[s] = fminf(m1[s], x);
            }
    };
    if (T > 0) {
        stage_tile(0, 0);
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        int t = 0;
        for (; t + 1 < T; t += 2) {
            step(accA, accB, t);
            step(accB, accA, t + 1);
        }
        if (t < T) step(accA, accB, t);
        if (active) {
            if (T & 1) consume_last(accA);
            else consume_last(accB);
        }
    }
    if (!active) return;
    // the partner lane holds the same query row against the other half of every tile's train rows
    float2* rr = rowres + (size_t)pd * row_stride + 32 * HW_NSUB * wb;
#pragma unroll
    for (int s = 0; s < HW_NSUB; ++s) {
        const float o1 = __shfl_xor(m1[s], 32), o2 = __shfl_xor(m2[s], 32);
        const float n1 = fminf(m1[s], o1), n2 = fminf(fmaxf(m1[s], o1), fminf(m2[s], o2));
        if (h == 0) rr[32 * s + cl] = make_float2(n1, n2);
    }
}

// (float)h0 / (float)h1 < ratio on the keys of a row; a row without two real neighbours fails; 0 / 0 is NaN and fails
__device__ __forceinline__ bool ham_wide_pass(float2 k, double ratio) {
    if (!(k.x < HW_KEY_END && k.y < HW_KEY_END)) return false;
    const int h0 = (int)k.x >> 14, h1 = (int)k.y >> 14;
    return (double)__fdiv_rn((float)h0, (float)h1) < ratio;
}

// ---- the tail: decode, predicate, directed lists, mutual check + thresholds (mode 0), stats; block per pair ----
__global__ __launch_bounds__(FIN_THREADS) void ham_wide_finalize_kernel(const FrameDev* __restrict__ frames, const int2* __restrict__ pairs,
                                                                     const float2* __restrict__ rowres, int ndir, int row_stride,
                                                                     double ratio, int min_dir, int min_mutual, int mode,
                                                                     uint2* __restrict__ out_matches, int* __restrict__ counts,
                                                                     int4* __restrict__ stats) {
    extern __shared__ int smem[];
    const int tid = threadIdx.x, p = blockIdx.x;
    const int2 pr = pairs[p];
    const int na = frames[pr.x].n, nb = frames[pr.y].n;
    int* fwd = smem;
    int* bwd = smem + row_stride;
    __shared__ int s_cnt[2];
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    int c12 = 0, c21 = 0;
    const float2* r12 = rowres + (size_t)p * ndir * row_stride;
    for (int q = tid; q < na; q += FIN_THREADS) {
        const float2 k = r12[q];
        const bool ok = nb >= 2 && ham_wide_pass(k, ratio);
        fwd[q] = ok ? ((int)k.x & (HW_MAX_ROWS - 1)) : -1;
        c12 += ok;
    }
    if (mode == 0) {
        const float2* r21 = r12 + row_stride;
        for (int c = tid; c < nb; c += FIN_THREADS) {
            const float2 k = r21[c];
            const bool ok = na >= 2 && ham_wide_pass(k, ratio);
            bwd[c] = ok ? ((int)k.x & (HW_MAX_ROWS - 1)) : -1;
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

// ---- host ------------------------------------------------------------------------------------------
int upload_frame_bits_wide(eacham_ctx* ctx, int frame_id, const unsigned char* packed_dev, int n, int bytes_per_row) {
    if (n < 0 || bytes_per_row <= 0) return ctx->fail(EACHAM_ERR_INVALID, "bad descriptor shape %d x %d bytes", n, bytes_per_row);
    if (n > 0 && !packed_dev) return ctx->fail(EACHAM_ERR_INVALID, "null descriptor pointer");
    const int ks = bytes_per_row <= HW_MAX_BYTES ? (8 * bytes_per_row + 63) / 64 : 0;
    FrameHost* slot = nullptr;
    if (int rc = open_frame_slot(ctx, frame_id, FRAME_BITS_WIDE, n, HW_MAX_ROWS, ks, bytes_per_row, &slot)) return rc;
    FrameHost& f = *slot;
    const int ntiles = ((n + 31) / 32 + HW_NSUB - 1) / HW_NSUB * HW_NSUB;
    const int npad = ntiles * 32;
    if (npad > 0) {
        // one allocation: the image (whole KiB) | the packed rows, 16 words each
        const size_t img_bytes = (size_t)ntiles * ks * 64 * sizeof(int4);
        EACHAM_HIP_TRY(ctx, hipMalloc((void**)&f.frag, img_bytes + (size_t)n * 16 * sizeof(unsigned)));
        f.bits = (unsigned*)((char*)f.frag + img_bytes);
        const long long work = (long long)npad * ks * 2;
        ham_wide_image_kernel<<<(unsigned)((work + 255) / 256), 256, 0, ctx->stream>>>(packed_dev, n, bytes_per_row, ks, npad, f.frag);
        launch_bits_store(ctx, packed_dev, n, bytes_per_row, 16, f.bits);
        EACHAM_HIP_TRY(ctx, hipGetLastError());
    }
    commit_frame(ctx, f, FRAME_BITS_WIDE, n, 8 * bytes_per_row, ks, ntiles, bytes_per_row);
    EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // orders reuse of the staging buffer (and of the caller's rows)
    return EACHAM_OK;
}

namespace {
static_assert(PLAN_HW_WG_TILES == HW_WG_TILES, "match_plan.hpp plans for these kernels");
HamWidePlan plan_ham_wide(const eacham_ctx* ctx, int npairs) {
    int max_tiles = HW_NSUB;
    for (const auto& f : ctx->frames)
        if (f.n >= 0) max_tiles = std::max(max_tiles, f.ntiles);
    return eacham::plan_ham_wide(max_tiles, npairs, ctx->wide_budget_bytes ? ctx->wide_budget_bytes : (size_t)ctx->match_budget_mb << 20);
}

void launch_ham_wide_sweep(eacham_ctx* ctx, const int2* pb, int nb, int ndir, const HamWidePlan& pl, float2* rr) {
    const int grid = nb * ndir * pl.wgs_per_pair;
    const float cbase = 8192.0f * (float)(8 * ctx->wide_bytes_common);   // 2^13 D
#define EACHAM_HW_CASE(K) \
    case K: ham_wide_sweep_kernel<K><<<grid, HW_THREADS, 0, ctx->stream>>>(ctx->frame_table_dev, pb, pl.wgs_per_pair, ndir, rr, pl.row_stride, cbase); break
    switch (ctx->ks_common) {
        EACHAM_HW_CASE(1);
        EACHAM_HW_CASE(2);
        EACHAM_HW_CASE(3);
        EACHAM_HW_CASE(4);
        EACHAM_HW_CASE(5);
        EACHAM_HW_CASE(6);
        EACHAM_HW_CASE(7);
        default: EACHAM_HW_CASE(8);
    }
#undef EACHAM_HW_CASE
}
}  // namespace

// mode 0 = mutual + thresholds, mode 1 = directed lists; CSR over the pairs either way. pairs_host (the same list, checked, or
// null) only feeds the tally of eacham_match_debug_hamming_wide; *pairs_used (may be null) is the list the kernels ran on.
int run_match_ham_wide(eacham_ctx* ctx, const int2* pairs_dev, int npairs, double ratio, int min_dir, int min_mutual, int mode,
                       int* counts_dev, long long* offsets_dev, uint2* edges_dev, long long edge_cap, long long* total_dev,
                       int4* stats_dev, const int32_t* pairs_host, const int2** pairs_used) {
    int rc = sync_frame_table(ctx);
    if (rc) return rc;
    if (npairs <= 0) return EACHAM_OK;
    if (mode == 0 && !(ratio <= 1.0))   // (as the narrow kind)
        return ctx->fail(EACHAM_ERR_INVALID, "ratio %g: mutual matching supports 0 < ratio <= 1 (the reference uses 0.8)", ratio);
    rc = sanitize_pairs(ctx, pairs_dev, npairs, &pairs_dev);  // a bad frame id in a device-side list must not reach the kernels
    if (rc) return rc;
    if (pairs_used) *pairs_used = pairs_dev;
    const HamWidePlan pl = plan_ham_wide(ctx, npairs);
    rc = ensure_workspace(ctx, pl.total);
    if (rc) return rc;
    const int ndir = mode == 0 ? 2 : 1;
    const size_t fin_smem = (size_t)2 * pl.row_stride * sizeof(int);
    if (fin_smem > 48 * 1024)
        EACHAM_HIP_TRY(ctx, hipFuncSetAttribute((const void*)ham_wide_finalize_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fin_smem));
    const HamWideArrays a = pl.carve(ctx->ws);
    float2* rr = a.rowres;
    uint2* mt = a.matches;
    long long batches = 0;
    for (int first = 0; first < npairs; first += pl.batch, ++batches) {
        const int nb = std::min(pl.batch, npairs - first);
        const int2* pb = pairs_dev + first;
        {
            ProfileScope ps(ctx, EACHAM_KERNEL_MATCH_TILE);
            launch_ham_wide_sweep(ctx, pb, nb, ndir, pl, rr);
        }
        {
            ProfileScope ps(ctx, EACHAM_KERNEL_MATCH_FINALIZE);
            int* cnt = counts_dev + first;
            ham_wide_finalize_kernel<<<nb, FIN_THREADS, fin_smem, ctx->stream>>>(ctx->frame_table_dev, pb, rr, ndir, pl.row_stride, ratio, min_dir,
                                                                          min_mutual, mode, mt, cnt, stats_dev ? stats_dev + first : nullptr);
            launch_scan_counts(ctx, cnt, nb, offsets_dev, total_dev, first, first + nb == npairs);
            launch_compact_edges(ctx, nb, mt, cnt, offsets_dev + first, pl.row_stride, edges_dev, edge_cap);
        }
        EACHAM_HIP_TRY(ctx, hipGetLastError());
    }
    long long rows = pairs_host ? 0 : -1;   // (a device-side pair list is not read back for a tally)
    for (int i = 0; pairs_host && i < npairs; ++i)
        rows += ctx->frames[pairs_host[2 * i]].n + (ndir == 2 ? ctx->frames[pairs_host[2 * i + 1]].n : 0);
    ctx->wide_debug[0] = batches;
    ctx->wide_debug[1] = pl.batch;
    ctx->wide_debug[2] = batches;   // one launch per batch covers its directions
    ctx->wide_debug[3] = rows;
    return EACHAM_OK;
}

// the sweep's own top-2 of the ordered pair (f1, f2), from the buffer the tail reads
int ham_wide_debug_pair(eacham_ctx* ctx, int f1, int f2, int32_t* best, int32_t* h0, int32_t* h1, int cap) {
    if (!best || !h0 || !h1 || cap < 0) return ctx->fail(EACHAM_ERR_INVALID, "null output");
    if (ctx->kind_common != FRAME_BITS_WIDE) return ctx->fail(EACHAM_ERR_UNSUPPORTED, "the wide Hamming sweep needs wide binary frames (eacham_upload_descriptors_bits_wide)");
    const FrameHost &A = ctx->frames[f1], &B = ctx->frames[f2];
    if (B.n < 2) return ctx->fail(EACHAM_ERR_INVALID, "frame %d has %d rows: a top-2 needs two or more", f2, B.n);
    if (cap < A.n) return ctx->fail(EACHAM_ERR_CAPACITY, "%d rows but capacity %d", A.n, cap);
    if (A.n == 0) return EACHAM_OK;
    int rc = sync_frame_table(ctx);
    if (rc) return rc;
    const HamWidePlan pl = plan_ham_wide(ctx, 1);
    rc = ensure_workspace(ctx, pl.total);
    if (rc) return rc;
    const int32_t pr[2] = {f1, f2};
    IoStage io(ctx, ctx->stream);
    const auto h_pair = io.in<int2>(pr, 1);
    IoDev d;
    rc = io.upload(d);
    if (rc) return rc;
    float2* rr = pl.carve(ctx->ws).rowres;
    launch_ham_wide_sweep(ctx, d(h_pair), 1, 1, pl, rr);
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    rc = io.finish();
    if (rc) return rc;
    std::vector<float2> res((size_t)A.n);
    EACHAM_HIP_TRY(ctx, hipMemcpy(res.data(), rr, sizeof(float2) * res.size(), hipMemcpyDeviceToHost));
    for (int q = 0; q < A.n; ++q) {
        const float2 k = res[q];
        const bool ok = k.x < HW_KEY_END && k.y < HW_KEY_END;
        best[q] = ok ? ((int)k.x & (HW_MAX_ROWS - 1)) : -1;
        h0[q] = ok ? (int)k.x >> 14 : -1;
        h1[q] = ok ? (int)k.y >> 14 : -1;
    }
    return EACHAM_OK;
}

}  // namespace eacham
