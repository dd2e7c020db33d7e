// matcher.hip — exact all-pairs descriptor matching for gfx950 (MI355X).
//
// Replaces   FeatureMatcherFlann::Match   modules/base/features/FeatureMatcherFlann.cpp:14-30
//            pair loop + mutual check     apps/sfm/main.cpp:84-147
//
// Data layout in HBM ("fragment-major int8"): descriptors are integers in [0,255] (OpenCV SIFT),
// stored centred (x-128) as int8 in the exact register image of v_mfma_i32_32x32x32_i8 operands:
//     frag[tile = row/32][ks = k/32][lane = 32*((k%32)/16) + row%32] = 16 bytes  (k%16 ascending)
// so one wave-wide 16-byte load is 1 KiB contiguous and needs no LDS swizzle. The same image
// serves as the A operand (queries, rows of the distance tile) and the B operand (train, columns).
//
// Arithmetic (all integer, hence independent of summation order => bit-exact vs the CPU oracle):
//     d2(q,t) = |a_q|^2 + |b_t|^2 - 2 a_q.b_t = 2 H + pa + pb
//     H = floor(|a_q|^2 / 2) + floor(|b_t|^2 / 2) - a_q.b_t   (int8 MFMA, int32 accumulate, C-init;
//         stored with a +1 bias so that it is never negative)
//     pa, pb = parities of the two squared norms
// One int32 key per distance serves BOTH directions:
//     key = (H << 8) | (pb << 7) | column-tile index
// Row direction (q -> best t): pa is constant, keys order by (2H + pb, tile) — exact, ties to the
// lower column. Column direction (t -> best q): pb and the tile are constant, keys order by H, which
// is the order of d2 as long as pa is constant among the rows compared — so frames are stored
// PARITY-SORTED (even squared norms first, each class padded to whole 32-row tiles): a sub-tile has
// one parity, and the one workgroup that may straddle the boundary keeps two column partials.
// The column direction only needs VALUES: a row q is column t's unique best
// iff d2(q,t) equals the column minimum and the column passes the ratio test (a tie gives quotient
// 1, which no ratio <= 1 accepts), so no row index is carried through the column reduction.
// A running top-2 costs two VALU ops:  m2 = med3(m1, m2, key); m1 = min(m1, key).
#include "context.hpp"
#include "match_plan.hpp"
#include "match_screen.hpp"
#include "match_tail.hpp"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <type_traits>

namespace eacham {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
// Pointers read out of the device-side frame table are generic to the compiler; casting them to the
// global address space turns flat_load (which ties vmcnt to lgkmcnt) into global_load.
typedef const v4i __attribute__((address_space(1)))* gfrag_t;
typedef const int __attribute__((address_space(1)))* gint_t;

// H constant of padding rows/columns: above any real H (<= 256*255^2/2 = 8,323,200) and small
// enough that pad x pad (2 * PADH) still fits the 24-bit H field of a key
constexpr int PADH = 8350000;
constexpr int KEY_SHIFT = 7;               // tile field; key >> 7 = 2H + pb
constexpr int KEY_MASK = (1 << KEY_SHIFT) - 1;
constexpr int CHUNK_TILES = 1 << KEY_SHIFT;  // column tiles one sweep can tag in a key: 128 * 32 = 4096 train rows
constexpr int MAX_ROWS = 16384;              // rows per frame (K2 keeps two int per stored row in LDS)
constexpr int WG_THREADS = 256;            // 4 waves (1 per SIMD); 2 workgroups per CU drift out of phase so MFMA and VALU overlap
constexpr int WAVES = WG_THREADS / 64;
constexpr int MATCH_NSUB = 2;                        // 32-row MFMA sub-tiles per wave (A fragments live in VGPRs)
constexpr int ROWS_PER_WAVE = 32 * MATCH_NSUB;
constexpr int ROWS_PER_WG = WAVES * ROWS_PER_WAVE;
constexpr int GROUP_TILES = MATCH_NSUB;              // tiles in use are padded to whole wave-blocks
static_assert(PLAN_WG_TILES == ROWS_PER_WG / 32 && PLAN_CHUNK_TILES == CHUNK_TILES, "match_plan.hpp plans for these kernels");

// ------------------------------------------------------------------------------------------------
// upload: fp32 row-major -> fragment-major int8 + squared norms
// ------------------------------------------------------------------------------------------------

// U1: per-row sum of squares / sum of the centred values + integrality flag (thread per 16 values)
__global__ void rowsum_kernel(const float* __restrict__ src, int n, int dim, int* __restrict__ s2,
                              int* __restrict__ s1, int* __restrict__ bad_flag) {
    const int chunks = (dim + 15) / 16;
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)n * chunks) return;
    const int row = (int)(idx / chunks), ch = (int)(idx % chunks);
    int sq = 0, sum = 0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int k = ch * 16 + j;
        if (k < dim) {
            const float v = src[(size_t)row * dim + k];
            if (!(v >= 0.0f && v <= 255.0f) || v != floorf(v)) bad = true;
            const int c = (int)v - 128;
            sq += c * c;
            sum += c;
        }
    }
    if (sq) atomicAdd(&s2[row], sq);
    if (sum) atomicAdd(&s1[row], sum);
    if (bad) atomicOr(bad_flag, 1);
}

// U2 (one workgroup): stable partition of the rows by the parity of |c|^2; fills the per-position
// constants and the two index maps. meta = {tiles of the even class, tiles in use}.
__global__ __launch_bounds__(1024) void partition_kernel(const int* __restrict__ s2, const int* __restrict__ s1, int n,
                                                         int npad, int group_rows, int* __restrict__ ca,
                                                         int* __restrict__ hb, int* __restrict__ orig,
                                                         int* __restrict__ pos, int* __restrict__ meta) {
    __shared__ int sc[1024];
    __shared__ int s_n0, s_carry;
    const int tid = threadIdx.x;
    for (int j = tid; j < npad; j += 1024) {
        ca[j] = PADH;
        hb[j] = PADH;
        orig[j] = -1;
    }
    if (tid == 0) s_n0 = 0, s_carry = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < n; i += 1024) mine += !(s2[i] & 1);
    atomicAdd(&s_n0, mine);
    __syncthreads();
    const int n0 = s_n0;
    const int even_pad = (n0 + 31) / 32 * 32;   // each parity class fills whole 32-row tiles
    const int odd_pad = (n - n0 + 31) / 32 * 32;
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + tid;
        const int even = i < n ? !(s2[i] & 1) : 0;
        sc[tid] = even;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
            const int v = tid >= off ? sc[tid - off] : 0;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        if (i < n) {
            const int rank_even = s_carry + sc[tid] - even;          // evens before row i
            const int j = even ? rank_even : even_pad + (i - rank_even);
            const int half = s2[i] >> 1;
            ca[j] = half + 1;  // +1 keeps H >= 0 when d2 = 0 between two odd-norm rows (d2 = 2 (H - 1) + pa + pb)
            hb[j] = half + s1[i];
            orig[j] = i;
            pos[i] = j;
        }
        __syncthreads();
        if (tid == 0) s_carry += sc[1023];
        __syncthreads();
    }
    if (tid == 0) {
        meta[0] = even_pad / 32;
        meta[1] = (even_pad + odd_pad + group_rows - 1) / group_rows * (group_rows / 32);  // whole wave-blocks
    }
}

// U3: fp32 row-major -> fragment-major int8 at the stored (parity-sorted) position
__global__ void quantize_kernel(const float* __restrict__ src, int dim, int KS, int npad,
                                const int* __restrict__ orig, v4i* __restrict__ frag) {
    const int chunks = KS * 2;
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)npad * chunks) return;
    const int j = (int)(idx / chunks), ch = (int)(idx % chunks);
    const int ks = ch >> 1, h = ch & 1, tile = j >> 5, r = j & 31;
    const int row = orig[j];
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (row >= 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int k = ks * 32 + h * 16 + e;
            const int c = k < dim ? (int)src[(size_t)row * dim + k] - 128 : 0;  // padded dimensions are centred zeros
            w[e >> 2] |= (unsigned)(c & 0xff) << (8 * (e & 3));
        }
    }
    const v4i out = {(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
    frag[((size_t)tile * KS + ks) * 64 + h * 32 + r] = out;
}

// U4 (frames above 128-D): the FP6 image of the screen sweep (match_screen.hpp), thread per stored row and 32 dimensions. A tile of
// 32 rows is 6 KiB: per K = 64 step a 16-byte plane and an 8-byte plane of 64 lanes (lane = 32 * ((k % 64) / 32) + row % 32 holds the
// 32 codes of k % 32 ascending, 24 bytes), so the LDS-DMA pieces of the sweep's ring stay 1 KiB and a lane's operand is two aligned
// reads. msq (zeroed) gathers |M|^2, sr (zeroed) s_r = sum (x - x~)^2.
constexpr float SCREEN_PAD = 8388608.0f;     // 2^23: exact in f32, above any n / 2 (n <= 256 * 120^2) and any partial sum of a real row
constexpr int SCREEN_KS = 4;                 // K = 64 steps of a 256-D row
constexpr int SCREEN_EXACT_KS = 8;           // int8 K = 32 steps of the same row: the exact pass behind the screen (frames_have_screen)
constexpr int SCREEN_STEP_BYTES = 1536, SCREEN_TILE_BYTES = SCREEN_KS * SCREEN_STEP_BYTES;
constexpr int SCREEN_CALL_TILES = 2;         // train tiles between two barriers of the screen sweep: 64 MFMAs of four passes per wave (128 query rows)
__global__ void quantize_screen_kernel(const float* __restrict__ src, int dim, int npad, const int* __restrict__ orig,
                                       char* __restrict__ image, int* __restrict__ msq, int* __restrict__ sr) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npad * 2 * SCREEN_KS) return;
    const int j = idx / (2 * SCREEN_KS), ch = idx % (2 * SCREEN_KS);
    const int ks = ch >> 1, h = ch & 1, tile = j >> 5, r = j & 31;
    const int row = orig[j];
    int m2 = 0, err = 0;
    unsigned char codes[32];
#pragma unroll
    for (int e = 0; e < 32; ++e) {
        const int k = ks * 64 + h * 32 + e;
        int code = 0;   // padded dimensions and padding rows: code 0, nothing towards a distance
        if (row >= 0 && k < dim) {
            const int x = min(max((int)src[(size_t)row * dim + k], 0), 255);   // (a value out of range fails the call elsewhere)
            code = screen::encode(x);
            const int m = screen::decode(code), d = x - screen::reconstruct(code);
            m2 += m * m;
            err += d * d;
        }
        codes[e] = (unsigned char)code;
    }
    uint32_t w[6];
    screen::pack32(codes, w);
    char* tb = image + (size_t)tile * SCREEN_TILE_BYTES + ks * SCREEN_STEP_BYTES;
    const int lane = 32 * h + r;
    *reinterpret_cast<v4i*>(tb + 16 * lane) = v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
    *reinterpret_cast<int2*>(tb + 1024 + 8 * lane) = make_int2((int)w[4], (int)w[5]);
    if (m2) atomicAdd(&msq[j], m2);
    if (err) atomicAdd(&sr[j], err);
}
// U5: hm = |M|^2 / 2 as float in msq's place (the C-init of the row as a train row, added once as a query row; padding rows:
// SCREEN_PAD, above every real value), eb[0] = the largest s_r of a real row, meta[2] (zeroed) = the stored tiles up to the last
// one that holds a real row: meta[1] without the tile that only rounds it up to whole wave-blocks. A class fills its tiles from
// their first row on, so a tile holds a real row where its first row is one. The screen sweep runs over these tiles as a train
// frame's: a tile of padding rows alone gives no subset a value below SCREEN_PAD, which the tail reads as no value at all.
__global__ void finish_screen_kernel(int npad, const int* __restrict__ orig, int* __restrict__ msq, const int* __restrict__ sr, int* __restrict__ eb,
                                     int* __restrict__ meta) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= npad) return;
    const bool real_row = orig[j] >= 0;
    reinterpret_cast<float*>(msq)[j] = real_row ? 0.5f * (float)msq[j] : SCREEN_PAD;
    if (real_row) atomicMax(eb, sr[j]);
    if (real_row && (j & 31) == 0) atomicMax(&meta[2], (j >> 5) + 1);
}

// ------------------------------------------------------------------------------------------------
// K1: distance tiles + fused row/column top-2
// ------------------------------------------------------------------------------------------------
//
// grid  = npairs * wgs_per_pair workgroups of 256 threads; workgroup (p, rb) owns rows
//         [256*rb, 256*rb+256) of frame A = pairs[p].x against ALL rows of frame B = pairs[p].y.
// wave  = 64 rows (two 32-row MFMA tiles): A fragments stay in VGPRs for the whole sweep
//         (A-stationary), B tiles (32 train rows = KS KiB) stream through LDS once per workgroup.
//
// The kernel is VALU-bound (each wave64 integer op costs 4 cycles per SIMD, the int8 MFMAs of a
// tile only 16 x 32), so the epilogue is cut to ~4.7 ops per distance:
//   * the query fragments are complemented once (a' = ~a = -a-1 per byte) and the accumulator starts
//     at floor(|a|^2/2) (C-init), so the MFMA returns acc = floor(|a|^2/2) - a.b - sum(b) and the
//     key is ONE v_lshl_add_u32:  key = (acc << 8) + ((hb_c << 8) | pb << 7 | t),
//     hb = floor(|b|^2/2) + sum(b) precomputed at upload;
//   * the row top-2 update is v_med3_u32 + v_min_u32 (2 ops per key);
//   * the column top-2 runs on the SAME keys, three at a time (5 ops per 3 keys).
// Measured on MI355X (tools/valu_ubench.hip, tools/mfma_ubench.hip): a wave64 integer VALU op costs
// ~4 cycles of its SIMD whatever the number of resident waves, the int8 32x32x32 MFMA 32 cycles, so
// the MFMA chains are software-pipelined UNDER the epilogue (see the main loop).
// out   rowres[p][cc][j]   = {v1, col1, v2, 0}   top-2 of stored row j over the columns of chunk cc,
//                                                v = 2H + pb = d2 - pa_j, col = stored column position
//       colpart[p][k][c]   = {key1, key2}        top-2 keys of stored column c over the rows of one
//                                                parity of a workgroup (d2 = 2 (key >> 8) + pa_k + pb_c - 2)
__device__ __forceinline__ unsigned vmed3(unsigned a, unsigned b, unsigned c) {
    unsigned d;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ unsigned umin(unsigned a, unsigned b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }


__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(unsigned long long)(const __attribute__((address_space(3))) void*)p;
}
// 16-byte LDS read the compiler does not track (the caller places the s_waitcnt).
template <class V>
__device__ __forceinline__ void lds_read_frag(V& dst, unsigned addr, int offset_bytes) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(offset_bytes));
}

template <int KS>
__global__ __launch_bounds__(WG_THREADS, 2) void match_tile_kernel(
    const FrameDev* __restrict__ frames, const int2* __restrict__ pairs, int wgs_per_pair, int col_chunks,
    uint4* __restrict__ rowres, uint2* __restrict__ colpart, int wb_stride, int row_stride) {
    constexpr int NSUB = MATCH_NSUB;
    constexpr int TILE_V4 = KS * 64;          // int4 per B tile
    constexpr int ROWS_WAVE = 32 * NSUB;      // query rows a wave keeps in registers
    constexpr int ROWS_WG = WAVES * ROWS_WAVE;
    static_assert(ROWS_WAVE <= (1 << KEY_SHIFT), "the local row must fit the key's code field");
    __shared__ v4i sB[3][TILE_V4];
    // One LDS region, two lives: during the sweep it buffers the column partials of the 4 waves for
    // bursts of BURST tiles (double-buffered), after the sweep it is the row-transposition slab.
    constexpr int BURST = 8;
    struct ColBuf { uint2 e[2][BURST][2][WAVES][32]; };  // [buffer][tile % BURST][row-parity group][wave][column]
    struct RowSlab { uint2 e[WAVES][32 * 33]; };
    __shared__ union { ColBuf c; RowSlab r; } sU;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cl = lane & 31, h = lane >> 5;
    // workgroup (pair p, row block rb, column chunk cc): frames with more than 4096 rows are swept in
    // chunks of CHUNK_TILES column tiles because a key has 7 bits for the tile index; K2 merges the
    // per-chunk row results (ascending chunks keep the lower column on ties).
    const int cc = blockIdx.x % col_chunks;
    const int rb = (blockIdx.x / col_chunks) % wgs_per_pair;
    const int p = blockIdx.x / (col_chunks * wgs_per_pair);
    const int2 pr = pairs[p];
    const FrameDev A = frames[pr.x], B = frames[pr.y];
    const int tbeg = cc * CHUNK_TILES;
    const int A_even = ((gint_t)A.meta)[0], A_tiles = ((gint_t)A.meta)[1];  // tiles of the even class / in use
    const int B_even = ((gint_t)B.meta)[0], B_tiles = ((gint_t)B.meta)[1];
    if (rb * (ROWS_WG / 32) >= A_tiles || tbeg >= B_tiles) return;  // workgroup-uniform
    const int wb = rb * WAVES + wave;                  // wave-block (ROWS_WAVE rows) of frame A
    const bool active = NSUB * wb < A_tiles;           // wave-uniform (tiles in use are a multiple of NSUB)
    const int T = min(B_tiles - tbeg, CHUNK_TILES);    // tiles of this chunk, t below is chunk-local
    const gfrag_t Afrag = (gfrag_t)A.frag, Bfrag = (gfrag_t)B.frag + (size_t)tbeg * TILE_V4;
    const gint_t Aca = (gint_t)A.norm, Bhb = (gint_t)B.normb + 32 * tbeg;

    v4i a[NSUB][KS];
    v16i cinit[NSUB];                 // floor(|a|^2/2) of this lane's 16 rows per sub-tile: the MFMA C-init
    unsigned rm1[NSUB][16], rm2[NSUB][16];
    const int wbc = active ? wb : 0;  // inactive waves load a valid block and never use it
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a[s][ks] = ~Afrag[((size_t)(NSUB * wbc + s) * KS + ks) * 64 + lane];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int lrow = 32 * s + (r & 3) + 8 * (r >> 2) + 4 * h;  // C/D layout of the 32x32 MFMA
            cinit[s][r] = Aca[ROWS_WAVE * wbc + lrow];
            rm1[s][r] = 0xffffffffu;
            rm2[s][r] = 0xffffffffu;
        }
    }

    // Software pipeline (no extra registers): the NSUB accumulators of a wave are staggered by one
    // sub-tile. The MFMA chains are issued in the order (t,0) (t,1) .. (t,NSUB-1) (t+1,0) ..., and
    // while chain c+1 is being issued the VALU runs the epilogue of chain c — an MFMA chain
    // (8 x 32 cycles) always hides under ~100 VALU ops (4 cycles each). Waves issue in order, hence
    // the source interleaves one MFMA with two epilogue elements and pins that order with
    // sched_barrier. B fragments are read from LDS just in time through a 3-deep register ring (a tile
    // is read once per accumulator) instead of holding a whole tile in VGPRs.
    // LDS ring of 3 tiles: sB[t % 3] holds tile t. Tile t+2 is DMA-ed into sB[(t+2) % 3] from the
    // top of iteration t (that slot held tile t-1, last read in iteration t-1, i.e. before the
    // previous barrier); the barrier at the end of the iteration (vmcnt(0) + s_barrier) publishes it.
    // Staging is LDS-DMA (global_load_lds_dwordx4): a wave-instruction moves 1 KiB = one k-step of
    // the fragment-major tile straight into LDS (destination = wave-uniform base + lane*16, which
    // is exactly the linear tile image), no VGPR round trip and no ds_write pass.
    static_assert(TILE_V4 % 64 == 0, "a tile is a whole number of 1 KiB pieces");
    constexpr int PIECES = TILE_V4 / 64;                 // 1 KiB pieces per tile (= KS)
    constexpr int PPW = (PIECES + WAVES - 1) / WAVES;    // pieces per wave
    auto stage_tile = [&](int tile, int slot) {
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int piece = wave + i * WAVES;
            if (piece < PIECES)
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void*)(Bfrag + (size_t)tile * TILE_V4 + piece * 64 + lane),
                    (__attribute__((address_space(3))) void*)(&sB[slot][piece * 64]), 16, 0, 0);
        }
    };
    if (T > 0) {
        stage_tile(0, 0);
        stage_tile(min(1, T - 1), 1);
    }
    int hb_cur = T > 0 ? Bhb[cl] : 0;
    __builtin_amdgcn_s_waitcnt(0);  // every prologue load has landed (keeps vmcnt(0) out of the loop)
    __syncthreads();

    const v16i zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    v16i acc[NSUB];
#pragma unroll
    for (int s = 0; s < NSUB; ++s) acc[s] = zero16;
    v4i bq[3];  // fragment ring: step i of the (phase, ks) sequence lives in bq[i % 3]
    if (T > 0 && active) {
        v4i b0[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) b0[ks] = sB[0][ks * 64 + lane];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[0][ks], b0[ks], ks ? acc[0] : cinit[0], 0, 0, 0);
        bq[0] = sB[0][lane];       // steps 0 and 1 of iteration 0 (chain (0,1) re-reads tile 0)
        bq[1] = sB[0][64 + lane];
    }

    // Column partials leave the workgroup merged over its 4 wave-blocks (a quarter of the traffic of
    // per-wave partials). Rows of different parity must not be merged, so a workgroup owns the slots
    // rb (its even rows) and rb + 1 (its odd rows); only the one workgroup of a frame that straddles
    // the even/odd boundary fills both, every other workgroup fills the one of its parity. K2 knows
    // from A_even which slots are in use: slot k holds even rows iff 8k < A_even.
    const int wg_tile0 = rb * (ROWS_WG / 32);
    const bool split = wg_tile0 < A_even && wg_tile0 + ROWS_WG / 32 > A_even;  // workgroup-uniform
    const int slot0 = rb + ((!split && wg_tile0 >= A_even) ? 1 : 0);
    // The workgroup's part of the partial array as a SCALAR base (two s-registers) + a 32-bit per-lane index: hoisted as a
    // per-lane 64-bit address it cost two VGPRs across the whole sweep on a kernel that sits at the 256-register limit of two
    // waves per SIMD (and was the value the compiler spilled).
    uint2* colpart_wg;
    {
        const unsigned long long u = (unsigned long long)(colpart + ((size_t)p * wb_stride + slot0) * row_stride + 32 * (size_t)tbeg);
        colpart_wg = (uint2*)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(u >> 32)) << 32) |
                              (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)u));
    }
    // Burst merge of the published tiles [t0, t0 + BURST) by the whole workgroup: thread -> (tile, column).
    auto merge_burst = [&](int t0) {
        const int tt = t0 + 2 * wave + h;  // tid >> 5
        if (tt < T) {
            for (int g = 0; g < (split ? 2 : 1); ++g) {
                const uint2(*src)[32] = sU.c.e[(t0 / BURST) & 1][tt % BURST][g];
                uint2 m = src[0][cl];
#pragma unroll
                for (int w = 1; w < WAVES; ++w) {
                    const uint2 e = src[w][cl];
                    m.y = umin(umin(umax(m.x, e.x), m.y), e.y);
                    m.x = umin(m.x, e.x);
                }
                colpart_wg[(unsigned)(g * row_stride + 32 * tt + cl)] = m;
            }
        }
    };
    constexpr int EPK = 16 / KS;         // epilogue elements interleaved per MFMA (KS = 8 -> 2)
    constexpr int NSTEP = NSUB * KS;     // (phase, ks) steps per tile
    // One tile of the sweep. The LDS slot ring (tile t lives in slot t % 3) and the fragment register ring (step i of the
    // (phase, ks) sequence lives in bq[(i + PH) % 3]; a tile advances it by NSTEP % 3) both have period 3 in t: the body
    // is instantiated for the three residues and the loop below runs three tiles per trip, so every ring index is a
    // compile-time constant and no register is moved to rotate a ring (8 v_mov per wave-tile before, 4 % of its VALU
    // instructions, on a kernel bound by its issue port).
    auto tile = [&](auto PHc, auto SLc, const int t) {
        constexpr int PH = decltype(PHc)::value, SL = decltype(SLc)::value;
        constexpr int slot_cur = SL, slot_nxt = (SL + 1) % 3, slot_new = (SL + 2) % 3;
        // per-column part of this tile's keys: (hb << 8) | pb << 7 | t  (pb is wave-uniform per tile)
        const unsigned lowc = ((unsigned)hb_cur << (KEY_SHIFT + 1)) | (unsigned)((tbeg + t >= B_even ? (1 << KEY_SHIFT) : 0) | t);
        const int t1 = min(t + 1, T - 1), t2 = min(t + 2, T - 1);
        hb_cur = Bhb[32 * t1 + cl];
        if (t > 0 && t % BURST == 0) merge_burst(t - BURST);  // tiles t-8 .. t-1 are published; their buffer is rewritten from tile t+8 on
        stage_tile(t2, slot_new);  // lands during this iteration; the barrier below publishes it
        unsigned cm1[NSUB], cm2[NSUB], pend[3] = {0, 0, 0};  // column top-2 per sub-tile (a sub-tile has one parity)
        if (active) {
            // LDS byte addresses of this lane's 16 bytes in the two live slots. The fragment reads
            // are inline asm with hand-placed s_waitcnt lgkmcnt(1): hipcc waits with lgkmcnt(0)
            // before every second MFMA, i.e. also for the read it issued one step earlier
            // (~50 cycles ago, well short of the LDS latency). Nothing else in the loop uses lgkmcnt.
            const unsigned curB = lds_addr(&sB[slot_cur][lane]);
            const unsigned nxtB = lds_addr(&sB[slot_nxt][lane]);
            // The ring phase advances by NSTEP % 3 per iteration, so the loop body is written for a
            // fixed phase and the ring is rotated at the end (register moves) to keep every index a
            // compile-time constant.
#pragma unroll
            for (int i = 0; i < NSTEP; ++i) {
                const int ph = i / KS, ks = i % KS;  // phase ph: epilogue of acc[ph], MFMAs of the next chain
                // prefetch the fragment of step i+2. Phase q < NSUB-1 issues chain (t, q+1): tile t;
                // phase NSUB-1 issues chain (t+1, 0) and phase 0 of the next iteration chain (t+1, 1):
                // tile t+1.
                const int j = i + 2;
                asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(bq[(i + PH) % 3]));  // step i landed (i+1 may be in flight)
                lds_read_frag(bq[(j + PH) % 3], (j / KS < NSUB - 1) ? curB : nxtB, (j % KS) * 1024);
                const int q = (ph + 1) % NSUB;       // accumulator of the chain being issued
                // (the last iteration recomputes tile T-1 into acc[0]; it is never read)
                acc[q] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[q][ks], bq[(i + PH) % 3], ks ? acc[q] : cinit[q], 0, 0, 0);
#pragma unroll
                for (int e = 0; e < EPK; ++e) {
                    const int r = ks * EPK + e;
                    const unsigned key = ((unsigned)acc[ph][r] << (KEY_SHIFT + 1)) + lowc;  // one v_lshl_add_u32
                    rm2[ph][r] = vmed3(rm1[ph][r], rm2[ph][r], key);
                    rm1[ph][r] = umin(rm1[ph][r], key);
                    // Column direction: the 16 keys of a sub-tile belong to this lane's column, so they
                    // are taken three at a time — {min3, med3} of a triple (2 ops) then one sorted-pair
                    // insert (3 ops) = 5 ops per 3 keys instead of 6 (and the first triple needs no insert).
                    const int eg = ks * EPK + e;  // 0..15 within the sub-tile, compile-time after unrolling
                    pend[eg % 3] = key;
                    if (eg % 3 == 2) {
                        const unsigned s1 = umin(umin(pend[0], pend[1]), pend[2]);
                        const unsigned s2 = vmed3(pend[0], pend[1], pend[2]);
                        if (eg == 2) {
                            cm1[ph] = s1;
                            cm2[ph] = s2;
                        } else {
                            cm2[ph] = umin(umin(umax(cm1[ph], s1), cm2[ph]), s2);
                            cm1[ph] = umin(cm1[ph], s1);
                        }
                    } else if (eg == 15) {  // 16 = 5 triples + 1
                        cm2[ph] = vmed3(cm1[ph], cm2[ph], key);
                        cm1[ph] = umin(cm1[ph], key);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // steps NSTEP and NSTEP + 1 (= steps 0, 1 of the next tile, whose ring phase is PH + NSTEP) are in flight:
            // they have landed before the barrier below lets anybody overwrite their slot
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bq[0]), "+v"(bq[1]), "+v"(bq[2]));
            // Merge the sub-tiles that share a parity: all of them, except in the workgroup that
            // straddles the even/odd boundary of frame A, which keeps the two parities apart.
            unsigned g1[2] = {0xffffffffu, 0xffffffffu}, g2[2] = {0xffffffffu, 0xffffffffu};
#pragma unroll
            for (int s = 0; s < NSUB; ++s) {
                const int g = (split && NSUB * wb + s >= A_even) ? 1 : 0;  // wave-uniform
                if (g == 0) {
                    g2[0] = umin(umin(umax(g1[0], cm1[s]), g2[0]), cm2[s]);
                    g1[0] = umin(g1[0], cm1[s]);
                } else {
                    g2[1] = umin(umin(umax(g1[1], cm1[s]), g2[1]), cm2[s]);
                    g1[1] = umin(g1[1], cm1[s]);
                }
            }
            // lanes l and l+32 hold the same column, rows 4h.. of each 8-row group: merge halves
            // (v_permlane32_swap: lanes 0-31 of the 2nd operand <-> lanes 32-63 of the 1st, pure VALU)
            {
                auto w1 = __builtin_amdgcn_permlane32_swap(g1[0], g1[0], false, false);
                auto w2 = __builtin_amdgcn_permlane32_swap(g2[0], g2[0], false, false);
                const unsigned n1 = umin(w1[0], w1[1]);
                const unsigned n2 = umin(umax(w1[0], w1[1]), umin(w2[0], w2[1]));
                if (h == 0) sU.c.e[(t / BURST) & 1][t % BURST][0][wave][cl] = make_uint2(n1, n2);
            }
            if (split) {
                auto w1 = __builtin_amdgcn_permlane32_swap(g1[1], g1[1], false, false);
                auto w2 = __builtin_amdgcn_permlane32_swap(g2[1], g2[1], false, false);
                const unsigned n1 = umin(w1[0], w1[1]);
                const unsigned n2 = umin(umax(w1[0], w1[1]), umin(w2[0], w2[1]));
                if (h == 0) sU.c.e[(t / BURST) & 1][t % BURST][1][wave][cl] = make_uint2(n1, n2);
            }
        } else {  // a wave beyond the frame's rows contributes nothing
            if (h == 0) sU.c.e[(t / BURST) & 1][t % BURST][0][wave][cl] = make_uint2(0xffffffffu, 0xffffffffu);
            if (split && h == 0) sU.c.e[(t / BURST) & 1][t % BURST][1][wave][cl] = make_uint2(0xffffffffu, 0xffffffffu);
        }
        __syncthreads();
    };
    {
        constexpr int ADV = NSTEP % 3;  // ring advance per tile
        using P0 = std::integral_constant<int, 0>;
        using P1 = std::integral_constant<int, ADV % 3>;
        using P2 = std::integral_constant<int, (2 * ADV) % 3>;
        using S1 = std::integral_constant<int, 1>;
        using S2 = std::integral_constant<int, 2>;
        int t = 0;
        for (; t + 3 <= T; t += 3) {
            tile(P0{}, P0{}, t);
            tile(P1{}, S1{}, t + 1);
            tile(P2{}, S2{}, t + 2);
        }
        if (t < T) {
            tile(P0{}, P0{}, t);
            if (t + 1 < T) tile(P1{}, S1{}, t + 1);
        }
    }
    if (T > 0) merge_burst((T - 1) / BURST * BURST);  // the last 1..8 tiles, published by the loop's last barrier
    __syncthreads();                                  // the region becomes the row slab
    if (!active) return;

    // Row direction: every lane holds, per row, its top-2 over the columns {32t + cl}. Transpose
    // through this wave's private LDS slab (rows padded to 33 entries: conflict-free) so that lane
    // (row, half) scans 16 of the 32 lane-partials of its row in ASCENDING lane-column order with a
    // strict '<': equal keys (same rank, same tile) then keep the lower column, which makes plain
    // 32-bit key compares exact — (key, lane-column) lexicographic == (rank, column) lexicographic.
    uint2* slab = sU.r.e[wave];
    uint4* rr = rowres + ((size_t)p * col_chunks + cc) * row_stride + ROWS_WAVE * wb;
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            slab[row * 33 + cl] = make_uint2(rm1[s][r], rm2[s][r]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        unsigned b1 = 0xffffffffu, b2 = 0xffffffffu;
        int c1 = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int cidx = 16 * h + j;
            const uint2 e = slab[cl * 33 + cidx];
            const bool lt = e.x < b1;
            b2 = lt ? b1 : umin(b2, e.x);
            c1 = lt ? cidx : c1;
            b1 = umin(b1, e.x);
            b2 = umin(b2, e.y);  // e.y >= e.x: it can only be a runner-up
        }
        const unsigned o1 = __shfl_xor(b1, 32), o2 = __shfl_xor(b2, 32);
        const int oc = __shfl_xor(c1, 32);
        if (h == 0) {  // the other half holds the higher columns: it wins only with a strictly smaller key
            const bool lt = o1 < b1;
            const unsigned key1 = lt ? o1 : b1, key2 = lt ? umin(b1, o2) : umin(b2, o1);
            const unsigned col1 = 32 * (tbeg + (key1 & KEY_MASK)) + (lt ? oc : c1);
            rr[32 * s + cl] = make_uint4(key1 >> KEY_SHIFT, col1, key2 >> KEY_SHIFT, 0);  // key >> 7 = 2H + pb
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// ------------------------------------------------------------------------------------------------
// K1r: the ROW sweep with the MFMA operands swapped (round 4) — the sweep of the candidate-only pipeline.
//
// match_tile_kernel keeps its query rows as the A operand: a lane then holds one train COLUMN of the tile, its 16 accumulators are 16
// different query rows, and every distance needs a key of its own — one VALU op to add the column's constant and tag the tile, two
// for the running top-2 of its row: 3 ops per distance on a kernel bound by the VALU issue port. Swapped — the train tile as the A
// operand, the wave's 64 query rows as the B operand — a lane IS a query row, its 16 accumulators are 16 train rows against it, and
// the per-train-row constant hb is the accumulator's C-init (read from LDS next to the tile: no VALU op), the per-query constant
// is added once after the sweep. The row's top-2 VALUES then run on the raw accumulators three at a time — {min3, med3} of a
// triple, a sorted-pair merge: 27 ops per 16 distances — and what a key used to carry is recovered elsewhere:
//   * the parity of the train row's norm: frames are stored parity-sorted, so the sweep passes all even tiles, then all odd ones;
//     the running state is set aside ONCE at the boundary and the two classes are joined when 2H + pb is formed;
//   * the column of the minimum: only the TILE of the first strict improvement is tracked (a compare + select per 16 distances);
//     the row inside it is found afterwards for the rows that pass the ratio test only (match_argmin_kernel: one 32 x 32 MFMA
//     group per (train tile, <= 32 passing rows)), lowest train index on ties as the reference's scan.
// 31 VALU ops per 16 distances instead of 48, and no 7-bit tile field: frames of any size in one sweep (no column chunks).
// Pipeline, LDS-DMA ring, just-in-time fragment ring and the three-tiles-per-trip loop are match_tile_kernel's.
// out   rowres[p][j] = {v1, tile1, v2, 0}: v = 2H + pb = d2 - pa_j + 2 of stored query row j, tile1 = first tile holding the minimum
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int imed3(int a, int b, int c) {
    int d;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
// sorted pair (s1 <= s2) merged into the running top-2 (m1 <= m2): 3 ops
__device__ __forceinline__ void top2_merge(int& m1, int& m2, int s1, int s2) {
    m2 = imin(imin(imax(m1, s1), m2), s2);
    m1 = imin(m1, s1);
}

//
// BOUND = true (round 5, the default of the lean form): the sweep keeps NO second-smallest value and no tile. Per sub-tile a lane
// runs FOUR minima, one per four of its sixteen accumulators (two v_min3 per group and tile: 8 VALU operations per 16 distances
// instead of 31), over the train rows of four disjoint subsets; with the partner lane and the two parity classes a query row ends
// with 16 partial minima over 16 DISJOINT subsets of the train frame. Their smallest is the row's minimum v1, and their second
// smallest u is an UPPER BOUND of the row's true second-smallest value (the runner-up is either the minimum of another subset, or
// hides behind v1 in v1's own subset and is then even smaller). The ratio test is monotone in the second value, so a row that
// fails it against u fails it against the truth: such rows are finished. The others — the rows that pass (a few per cent) and the
// few whose runner-up shared the minimum's subset — are candidates: match_rowpick_kernel lists them and match_colverify_kernel<KS, true>
// computes their exact {v1, tile, v2} against the whole train frame (the candidate-only pass of the columns with the frames' roles
// swapped), overwriting their rowres entries before match_rows2_kernel reads them. out: rowres[p][j] = {v1, 0, u, 0}.
//
// GATHER (KS = 8, exact): the exact pass behind the screen sweep. The workgroup is an item of the list the screen sweep's tail wrote
// (the comment above match_openprep_kernel): {segment head h, k} = candidates 256 k .. of the segment's region cands[h row_stride ..]
// ({pair index within the launch, stored query row}), min(256, segcount[h] - 256 k) of them and all onto one train frame (the
// first candidate's pair names it): wave w takes candidates 64 w .. 64 w + 63, a lane gathers ITS row's fragments from the
// candidate's own query frame (the addressing of match_colverify_kernel's gather), and the tail writes {v1, t1, v2, 0} to
// rowres[pair][row] from the h == 0 lanes of real candidates. A wave without candidates still stages; a lane past the count computes
// on the item's first candidate and writes nothing. Everything between prologue and tail is the sweep as it stands. The items are
// dense in [0, *n_items), in the order they were created; the workgroup is item blockIdx.x of a grid that bounds the list from above.
template <bool GATHER>
struct GatherList {};   // (no argument without the gather)
template <>
struct GatherList<true> {
    const uint2* cands;
    const int* segcount;
    const int2* items;
    const int* n_items;
};
constexpr int GATHER_WIDTH = 256;   // candidates per item: 64 per wave
template <int KS, bool BOUND = false, bool GATHER = false>
__global__ __launch_bounds__(WG_THREADS, KS >= 4 ? 3 : 4) void match_sweep_kernel(const FrameDev* __restrict__ frames, const int2* __restrict__ pairs,
                                                                   int wgs_per_pair, uint4* __restrict__ rowres, int row_stride,
                                                                   GatherList<GATHER> gl = {}) {
    constexpr int NSUB = 2;
    constexpr int TILE_V4 = KS * 64;
    constexpr int ROWS_WAVE = 32 * NSUB, ROWS_WG = WAVES * ROWS_WAVE;
    constexpr int BIG = 0x7fffffff;
    __shared__ v4i sB[3][TILE_V4];
    __shared__ __attribute__((aligned(16))) int sHb[3][32];  // hb of the tile in the same ring slot: the C-init of its MFMA chains
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cl = lane & 31, h = lane >> 5;
    int2 item = make_int2(0, 0);
    const uint2* pk = nullptr;            // GATHER: the item's candidates, item.y of them
    if constexpr (GATHER) {
        if ((int)blockIdx.x >= *gl.n_items) return;   // workgroup-uniform: the grid is an upper bound of the list
        item = gl.items[blockIdx.x];      // {segment head, k}: the sweep that counted the segment has ended, its count is final
        pk = gl.cands + (size_t)item.x * row_stride + GATHER_WIDTH * item.y;
        item.y = min(GATHER_WIDTH, gl.segcount[item.x] - GATHER_WIDTH * item.y);
    }
    const int rb = GATHER ? 0 : blockIdx.x % wgs_per_pair;
    const int p = GATHER ? (int)pk[0].x : blockIdx.x / wgs_per_pair;
    const int2 pr = pairs[p];
    const FrameDev A = frames[pr.x], B = frames[pr.y];
    const int A_tiles = ((gint_t)A.meta)[1];
    const int B_even = ((gint_t)B.meta)[0], T = ((gint_t)B.meta)[1];
    if (!GATHER && rb * (ROWS_WG / 32) >= A_tiles) return;  // workgroup-uniform
    const int wb = rb * WAVES + wave;
    const bool active = GATHER ? ROWS_WAVE * wave < item.y : NSUB * wb < A_tiles;
    const gfrag_t Afrag = (gfrag_t)A.frag, Bfrag = (gfrag_t)B.frag;
    const gint_t Aca = (gint_t)A.norm, Bhb = (gint_t)B.normb;
    const int wbc = active ? wb : 0;

    v4i a[NSUB][KS];   // this wave's 64 query rows, complemented: the B operand (a lane = a query row of the sub-tile)
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
        if constexpr (GATHER) {
            const int i = ROWS_WAVE * wave + 32 * s + cl;
            const uint2 c = pk[i < item.y ? i : 0];
            const gfrag_t Qfrag = (gfrag_t)frames[pairs[c.x].x].frag;   // the candidate's own query frame
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) a[s][ks] = ~Qfrag[((size_t)(c.y >> 5) * KS + ks) * 64 + 32 * h + (c.y & 31)];
        } else {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) a[s][ks] = ~Afrag[((size_t)(NSUB * wbc + s) * KS + ks) * 64 + lane];
        }
    }
    // running top-2 values and the tile of the minimum, per sub-tile; the even class is set aside at the parity boundary
    // (set aside in LDS, each lane its own words: six registers less through the sweep)
    constexpr int NG = 4;                    // BOUND: running minima per sub-tile (eight: 14 registers spilled at 256-D)
    constexpr int NSTATE = BOUND ? NG : 3;   // words of running state per sub-tile
    __shared__ int sEven[NSTATE * NSUB][WG_THREADS];
    int x1[NSUB], x2[NSUB], xt[NSUB];
    int xm[NSUB][NG];  // BOUND: the minimum over accumulators 4 g .. 4 g + 3 of every tile of the class
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
        x1[s] = x2[s] = BIG, xt[s] = 0;
#pragma unroll
        for (int g = 0; g < NG; ++g) xm[s][g] = BIG;
    }

    static_assert(TILE_V4 % 64 == 0, "a tile is a whole number of 1 KiB pieces");
    constexpr int PIECES = TILE_V4 / 64;
    constexpr int PPW = (PIECES + WAVES - 1) / WAVES;
    // (a wave stages PPW consecutive 1 KiB pieces: a scalar base, ONE 32-bit lane offset and immediate offsets — no 64-bit
    // per-lane addresses held through the sweep)
    const unsigned stage_off = (unsigned)(wave * PPW * 64 + lane) * 16u;
    auto stage_tile = [&](int tile, int slot) {
        const __attribute__((address_space(1))) char* base = (const __attribute__((address_space(1))) char*)(Bfrag + (size_t)tile * TILE_V4);
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int piece = wave * PPW + i;
            if (piece < PIECES)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + stage_off + i * 1024),
                                                 (__attribute__((address_space(3))) void*)(&sB[slot][piece * 64]), 16, 0, 0);
        }
    };
    if (T > 0) {
        stage_tile(0, 0);
        stage_tile(min(1, T - 1), 1);
        stage_tile(min(2, T - 1), 2);
        if (tid < 96) sHb[tid >> 5][tid & 31] = Bhb[32 * min(tid >> 5, T - 1) + (tid & 31)];
    }
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();

    // C-init of a chain on the tile in ring slot `slot`: accumulator r is train row (r & 3) + 8 (r >> 2) + 4 h
    auto cinit_of = [&](int slot) {
        v16i c;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const v4i q = *reinterpret_cast<const v4i*>(&sHb[slot][8 * g + 4 * h]);
#pragma unroll
            for (int k = 0; k < 4; ++k) c[4 * g + k] = q[k];
        }
        return c;
    };
    // Software pipeline: the MFMAs of tile t + 1 (both sub-tiles: every fragment is read from LDS ONCE and feeds two independent
    // chains) are issued interleaved with the epilogue of tile t, so the accumulators are double-buffered (tile parity). With one
    // LDS read per fragment and accumulator — the first form of this kernel, and match_tile_kernel's — the CU's LDS port is as busy as
    // its matrix pipes (16 KiB per wave-tile at 128 B / cycle = the 1024 cycles the MFMAs of two resident waves take) and the 256-D
    // sweep stayed where the VALU-bound kernel was; read once, the port is at half of that.
    // The chains' C-init (hb of the tile) is read from LDS straight into the accumulators that will take the chain: the ones whose
    // epilogue has just finished (a separate register set for it cost 16 VGPRs and, by the allocator's choice, a copy of a live chain).
    static_assert(KS >= 2, "the epilogue of a tile is spread over the first KS - 1 steps of the next tile's MFMAs");
    v16i accA[NSUB], accB[NSUB];
    const v16i zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < NSUB; ++s) accA[s] = zero16, accB[s] = zero16;
    v4i bq[3];  // fragment ring: step i of the ks sequence lives in bq[i % 3]
    constexpr int DIST = KS >= 2 ? 2 : 1;   // fragments are read DIST steps ahead of their MFMAs (a 32-D tile is a single step)
    if (T > 0 && active) {
        const v16i c0 = cinit_of(0);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const v4i b0 = sB[0][ks * 64 + lane];
#pragma unroll
            for (int s = 0; s < NSUB; ++s) accA[s] = __builtin_amdgcn_mfma_i32_32x32x32_i8(b0, a[s][ks], ks ? accA[s] : c0, 0, 0, 0);
        }
        bq[0] = sB[1][lane];   // the first fragments of tile 1 (the ring holds tile T - 1 again past the end: recomputed, never read)
        if constexpr (DIST == 2) bq[1] = sB[1][64 + lane];
#pragma unroll
        for (int s = 0; s < NSUB; ++s) accB[s] = cinit_of(1);
    }
    __syncthreads();   // slot 0 is staged into again by the first call below
    // keys of tile t handled by step ks of tile t + 1's MFMAs: all 32 within the first KS - 1 steps, so that the accumulators are
    // free for tile t + 2's constants a step before the call's drain
    auto key_lo = [](int ks) constexpr { return ks >= KS - 1 ? 32 : (32 * ks + KS - 2) / (KS - 1); };
    // One call: epilogue of tile t (held in `cur`), MFMAs of tile t + 1 into `nxt`, tile t + 3 staged into tile t's ring slot (its
    // fragments were consumed a call ago), the first fragments and the constants of tile t + 2 fetched at the end (published by the
    // previous call's barrier) and drained before this call's: nothing is in flight across a call. The LDS slot ring (period 3), the
    // fragment register ring (advance KS % 3 per call) and the accumulator parity (period 2) are compile-time: six instantiations.
    // key idx (sub-tile idx / 16, accumulator idx % 16) of tile t into the running state: triples through {min3, med3} + a sorted-pair
    // merge, the sixteenth key alone; the tile is recorded when the sub-tile has improved the class minimum strictly
    auto consume = [&](const v16i(&cur)[NSUB], const int idx, const int t, int(&pend)[3], int& before) {
        const int ph = idx / 16, eg = idx % 16;
        if constexpr (BOUND) {
            if (eg & 1) {   // accumulators 4 g .. 4 g + 3 -> xm[g], two at a time
                int d;
                asm("v_min3_i32 %0, %1, %2, %3" : "=v"(d) : "v"(xm[ph][eg >> 2]), "v"(cur[ph][eg - 1]), "v"(cur[ph][eg]));
                xm[ph][eg >> 2] = d;
            }
            return;
        }
        const int key = cur[ph][eg];
        if (eg == 0) before = x1[ph];  // the class minimum this sub-tile meets
        pend[eg % 3] = key;
        if (eg % 3 == 2) {
            const int s1 = imin(imin(pend[0], pend[1]), pend[2]);
            const int s2 = imed3(pend[0], pend[1], pend[2]);
            top2_merge(x1[ph], x2[ph], s1, s2);
        } else if (eg == 15) {
            x2[ph] = imed3(x1[ph], x2[ph], key);
            x1[ph] = imin(x1[ph], key);
            xt[ph] = x1[ph] < before ? t : xt[ph];  // a strict improvement somewhere in this tile: it is the minimum's tile now
        }
    };
    auto set_aside_even = [&]() {
#pragma unroll
        for (int s = 0; s < NSUB; ++s) {
            if constexpr (BOUND) {
#pragma unroll
                for (int g = 0; g < NG; ++g) sEven[NG * s + g][tid] = xm[s][g], xm[s][g] = BIG;
            } else {
                sEven[3 * s][tid] = x1[s], sEven[3 * s + 1][tid] = x2[s], sEven[3 * s + 2][tid] = xt[s];
                x1[s] = x2[s] = BIG;
            }
        }
    };
    auto tile = [&](auto PHc, auto SLc, auto PARc, const int t) {
        constexpr int PH = decltype(PHc)::value, SL = decltype(SLc)::value, PAR = decltype(PARc)::value;
        constexpr int slot_nxt = (SL + 1) % 3, slot_nn = (SL + 2) % 3;
        v16i(&cur)[NSUB] = PAR ? accB : accA;
        v16i(&nxt)[NSUB] = PAR ? accA : accB;
        const int t3 = min(t + 3, T - 1);
        const int hb_new = (tid < 32) ? *reinterpret_cast<const __attribute__((address_space(1))) int*>(reinterpret_cast<const __attribute__((address_space(1))) char*>(Bhb + 32 * t3) + (unsigned)tid * 4u) : 0;   // lands during this call; stored to the ring before the barrier
        stage_tile(t3, SL);
        if (t == B_even) set_aside_even();  // (workgroup-uniform, once per sweep) the even tiles are done: start the odd class
        if (active) {
            const unsigned nxtB = lds_addr(&sB[slot_nxt][lane]);
            const unsigned nnB = lds_addr(&sB[slot_nn][lane]);
            int pend[3] = {0, 0, 0}, before = 0;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if constexpr (DIST == 2) asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(bq[(ks + PH) % 3]));
                else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bq[(ks + PH) % 3]));
                const int j = ks + DIST;
                lds_read_frag(bq[(j + PH) % 3], j < KS ? nxtB : nnB, (j % KS) * 1024);
#pragma unroll
                for (int s = 0; s < NSUB; ++s)
                    nxt[s] = __builtin_amdgcn_mfma_i32_32x32x32_i8(bq[(ks + PH) % 3], a[s][ks], nxt[s], 0, 0, 0);
#pragma unroll
                for (int idx = key_lo(ks); idx < key_lo(ks + 1); ++idx) {
                    consume(cur, idx, t, pend, before);
                    if (idx % 16 == 15) cur[idx / 16] = cinit_of(slot_nn);   // done with these accumulators: tile t + 2's constants, for the next call's chains
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bq[0]), "+v"(bq[1]), "+v"(bq[2]));
        }
        if (tid < 32) sHb[SL][tid] = hb_new;
        __syncthreads();
    };
    // the last tile has nothing to issue and nothing to stage: its epilogue alone (which accumulators hold it is its parity)
    auto last = [&](auto PARc, const int t) {
        constexpr int PAR = decltype(PARc)::value;
        v16i(&cur)[NSUB] = PAR ? accB : accA;
        if (t == B_even) set_aside_even();
        if (active) {
            int pend[3] = {0, 0, 0}, before = 0;
#pragma unroll
            for (int idx = 0; idx < 32; ++idx) consume(cur, idx, t, pend, before);
        }
    };
    if (T > 0) {
        // tile(t) consumes tile t's accumulators and issues tile t + 1's, for t < T - 1
        constexpr int ADV = KS % 3;
        const int TM = T - 1;
        int t = 0;
        auto run = [&](auto K6c, int tt) {
            constexpr int K6 = decltype(K6c)::value;
            tile(std::integral_constant<int, (K6 * ADV) % 3>{}, std::integral_constant<int, K6 % 3>{}, std::integral_constant<int, K6 % 2>{}, tt);
        };
        for (; t + 6 <= TM; t += 6) {
            run(std::integral_constant<int, 0>{}, t);
            run(std::integral_constant<int, 1>{}, t + 1);
            run(std::integral_constant<int, 2>{}, t + 2);
            run(std::integral_constant<int, 3>{}, t + 3);
            run(std::integral_constant<int, 4>{}, t + 4);
            run(std::integral_constant<int, 5>{}, t + 5);
        }
        if (t < TM) run(std::integral_constant<int, 0>{}, t);
        if (t + 1 < TM) run(std::integral_constant<int, 1>{}, t + 1);
        if (t + 2 < TM) run(std::integral_constant<int, 2>{}, t + 2);
        if (t + 3 < TM) run(std::integral_constant<int, 3>{}, t + 3);
        if (t + 4 < TM) run(std::integral_constant<int, 4>{}, t + 4);
        if (TM & 1) last(std::integral_constant<int, 1>{}, TM);
        else last(std::integral_constant<int, 0>{}, TM);
    }
    if (!active) return;
    if constexpr (BOUND) {
        uint4* rr = rowres + (size_t)p * row_stride + ROWS_WAVE * wb;
#pragma unroll
        for (int s = 0; s < NSUB; ++s) {
            const int ca = Aca[ROWS_WAVE * wb + 32 * s + cl];
            unsigned v1 = 0xffffffffu, v2 = 0xffffffffu;   // the two smallest of the 16 partial minima (4 groups x 2 lanes x 2 classes)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    // a frame without odd rows never met the boundary: what ran is the even class
                    const int mine = c == 0 ? (B_even >= T ? xm[s][g] : sEven[NG * s + g][tid]) : (B_even >= T ? BIG : xm[s][g]);
                    const int other = __shfl_xor(mine, 32);
                    const unsigned w0 = mine == BIG ? 0xffffffffu : (unsigned)(2 * (mine + ca) + c);
                    const unsigned w1 = other == BIG ? 0xffffffffu : (unsigned)(2 * (other + ca) + c);
                    v2 = umin(v2, umax(v1, w0)), v1 = umin(v1, w0);
                    v2 = umin(v2, umax(v1, w1)), v1 = umin(v1, w1);
                }
            if (h == 0) rr[32 * s + cl] = make_uint4(v1, 0u, v2, 0u);
        }
        return;
    }
    int e1[NSUB], e2[NSUB], et[NSUB];
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
        if (B_even >= T) {  // a frame without odd rows never met the boundary: what ran is the even class
            e1[s] = x1[s], e2[s] = x2[s], et[s] = xt[s], x1[s] = x2[s] = BIG;
        } else {
            e1[s] = sEven[3 * s][tid], e2[s] = sEven[3 * s + 1][tid], et[s] = sEven[3 * s + 2][tid];
        }
    }
    uint4* rr = rowres + (size_t)p * row_stride + ROWS_WAVE * wb;
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
        // lanes l and l + 32 hold the same query row against complementary train rows of every tile: join them (equal minima:
        // the earlier tile), then the two parity classes as v = 2 (m + ca) + pb (never equal across classes)
        const int gi = ROWS_WAVE * wave + 32 * s + cl;                 // GATHER: this lane's candidate
        const uint2 gc = GATHER ? pk[gi < item.y ? gi : 0] : make_uint2(0u, 0u);
        const int ca = GATHER ? ((gint_t)frames[pairs[gc.x].x].norm)[gc.y] : Aca[ROWS_WAVE * wb + 32 * s + cl];
        int cls1[2] = {e1[s], x1[s]}, cls2[2] = {e2[s], x2[s]}, clst[2] = {et[s], xt[s]};
        unsigned v1 = 0xffffffffu, v2 = 0xffffffffu, t1 = 0;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int o1 = __shfl_xor(cls1[c], 32), o2 = __shfl_xor(cls2[c], 32), ot = __shfl_xor(clst[c], 32);
            const int tt = o1 < cls1[c] ? ot : (o1 == cls1[c] ? imin(ot, clst[c]) : clst[c]);
            int m1 = cls1[c], m2 = cls2[c];
            top2_merge(m1, m2, o1, o2);
            const unsigned w1 = m1 == BIG ? 0xffffffffu : (unsigned)(2 * (m1 + ca) + c);
            const unsigned w2 = m2 == BIG ? 0xffffffffu : (unsigned)(2 * (m2 + ca) + c);
            // (w1 <= w2) into (v1 <= v2)
            t1 = w1 < v1 ? (unsigned)tt : t1;
            v2 = umin(umin(umax(v1, w1), v2), w2);
            v1 = umin(v1, w1);
        }
        if constexpr (GATHER) {
            if (h == 0 && gi < item.y) rowres[(size_t)gc.x * row_stride + gc.y] = make_uint4(v1, t1, v2, 0);
        } else {
            if (h == 0) rr[32 * s + cl] = make_uint4(v1, t1, v2, 0);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// K1s: the SCREEN form of the row sweep above 128-D — match_sweep_kernel<8, true> on the FP6 image of the frames (match_screen.hpp).
//
// At 256-D the int8 sweep is bound by the matrix pipe (16 v_mfma_i32_32x32x32_i8 per wave-tile). The block-scaled f8f6f4 instructions
// with e2m3 operands take twice the K in the same cycles: half the matrix cycles per wave-tile over the quantised rows. They run in
// the 16x16x128 shape (v_mfma_scale_f32_16x16x128_f8f6f4, 16 of four passes per wave-tile where the 32x32x64 shape took 8 of eight:
// the same matrix cycles, under which the chip holds 1.61 GHz where it held 1.48; profiles/screen_shape16.txt). The stored
// image is the 32x32x64 operand's; which of its fragments a lane reads is screen::frag16_src. The train tile is the A operand,
// the wave's 128 query rows (eight sub-tiles of 16) the B operand with their sign bits flipped; both scale operands are 2^3 (one register), so a product is the
// integer -M_a M_b and, with |M_b|^2 / 2 as the C-init, an accumulator holds |M_b|^2 / 2 - M_a.M_b: every partial sum is a multiple of
// 1/2 below 2^22, exact in f32 in any order. |M_a|^2 / 2 is added once after the sweep: n = |M_a - M_b|^2 is twice the sum.
// The epilogue is the bound form's: running minima per chain (two v_min3_f32 per group of four train rows and tile). Nothing here
// depends on the parity of a norm, so there is no class boundary; the sixteen disjoint subsets of a query row are (tile parity, group
// of four stored train rows of the tile): a lane's four accumulators of a chain are one group (screen::acc16_row), the eight groups
// of a tile lie in the four lanes of the query row's column, two row halves each. Their smallest is n1, their second smallest u bounds the runner-up from above, and the tail turns them
// into L1 <= the true minimum and U2 >= the true runner-up (screen::lower_d2 / upper_d2 with the row's s and the train frame's E).
// out: rowres[p][j] = {L1 - pa + 2, 0, U2 - pa + 2, n1}: the bound form's slot and encoding ((e.x + pa) - 2 decodes to L1), so
// the rows that do not fail the ratio test on (L1, U2) are listed (match_rowpick_kernel's predicate), the gathered exact sweep
// (match_sweep_kernel<8, false, true>) overwrites them with exact {v1, tile, v2}, and match_rows2_kernel fails the others on the same two numbers (L1 is a valid lower bound for its L(p)).
// A row without a real minimum, or whose minima fill one subset only, carries the bound form's padding values. The fourth word
// (n1, ~0 without one) is read by eacham_match_debug_screen_pair only.
// openmask (null: none, the debug entry): openmask[p][wb] = one bit per row of wave-block wb, set where match_rowpick_kernel's
// predicate holds on the two words the tail is storing — one ballot, every lane owning the row of its number, stored from one lane (256 B per pair
// where its rowres is 32 KB: match_rows2_kernel<.., true> counts a pair's open rows from them). With the same word the tail
// reserves room in the candidate list of the pair's segment — one returning add per wave-block with an open row — and writes its
// candidates and, where its range holds a multiple of 256, the item that starts there (OpenList, match_openprep_kernel).
// LDS-DMA ring and just-in-time fragment ring are match_sweep_kernel's; a fragment is 24 bytes, two LDS reads, and feeds eight MFMAs.
// A wave owns 128 query rows — two wave-blocks of 64, the unit of the tail, of openmask and of the candidate list — at two waves per
// SIMD, with ONE set of accumulators (a second does not fit): per MFMA half the LDS reads, staged bytes, barriers and waits of the
// 64-row form (profiles/screen_rows128.txt). A workgroup is 512 query rows; the host launches ceil(wgs_per_pair / 2) per pair.
// The call structure is its own: a call covers TWO train tiles between
// two barriers (six ring slots of 6 KiB, three calls per trip), the four waves stage three pieces each spread over the call, and
// every wait inside a call is a counted one (see the call below; profiles/screen_two_tiles.txt).
// The sweep covers the train frame's meta[2] tiles, those that hold a real row. The tile that rounds meta[1] up to whole wave-blocks
// (the query side's unit) is padding alone: its distances are SCREEN_PAD in every subset, which the tail takes for no value, as it
// takes the BIGF of a subset that met no tile. Left out, every word of rowres stays what it was, and a frame of 63 real tiles ends
// on last() with no idle chains. An even count is made odd at the front: tile 0 is swept whole in the prologue (t0 = 1), into the
// minima of the even tiles, and the calls start at tile 1 — the sixteen subsets are the same sets of train rows either way, so
// every word of rowres stays what it was here too (profiles/screen_real_tiles.txt).
// ------------------------------------------------------------------------------------------------
typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v6i __attribute__((ext_vector_type(6)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void lds_read_frag64(v2i& dst, unsigned addr, int offset_bytes) {
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(offset_bytes));
}
__device__ __forceinline__ float fmin3(float a, float b, float c) {
    float d;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
// the ratio test of the finalize kernels (defined with them below): the screen kernel's tail lists its open rows with it
template <int METRIC>
__device__ __forceinline__ bool ratio_pass(int d2_best, int d2_second, double ratio);
// the candidate list of a launch as the tail writes it (the comment above match_openprep_kernel); unused where openmask is null
struct OpenList {
    const int* seghead;   // [pair of the launch] its segment's head, a pair index within the launch
    int* segcount;        // [pair of the launch] at a head: candidates of the segment so far
    uint2* cands;         // segment of head h: cands[h * row_stride ..]
    int2* items;          // {head, k}: candidates 256 k .. of that segment
    int* n_items;         // of the launch
};
struct ScreenFrag { v4i lo; v2i hi; };   // a lane's 32 codes of one K = 64 step
__device__ __forceinline__ v8i screen_operand(const ScreenFrag& f) { return v8i{f.lo[0], f.lo[1], f.lo[2], f.lo[3], f.hi[0], f.hi[1], 0, 0}; }

template <int METRIC>   // of the ratio test in the tail (binary frames of 129..256 bits carry the FP6 image too)
__global__ __launch_bounds__(WG_THREADS, 2) void match_screen_kernel(const FrameDev* __restrict__ frames, const int2* __restrict__ pairs,
                                                                     int wgs_per_pair, uint4* __restrict__ rowres, int row_stride, double ratio,
                                                                     unsigned long long* __restrict__ openmask, int mask_stride,
                                                                     OpenList ol) {
    constexpr int WBS = 2, WB_TILES = 2;      // a wave owns two wave-blocks of 64 query rows (the tail's unit), two stored tiles each
    constexpr int NSUB = WBS * WB_TILES;      // stored (32-row) query tiles of a wave
    constexpr int NQ = screen::QUERY_SUBTILES, NU = 2, NS = 2;   // per train tile: query sub-tiles of 16 rows x row halves u of the tile x K = 128 steps S
    static_assert(NQ == 2 * NSUB && screen::query16_block(NQ - 1) == WBS - 1, "match_screen.hpp maps the wave's eight sub-tiles");
    constexpr int KS = NU * NS;               // fragments of a tile = steps of a half, in the order f = u + NU S (see the call)
    static_assert(KS == SCREEN_KS && 2 * NS == SCREEN_KS && screen::STEP_BYTES == SCREEN_STEP_BYTES, "match_screen.hpp maps this stored tile");
    constexpr int TILE_V4 = SCREEN_TILE_BYTES / 16;
    constexpr int ROWS_WAVE = 32 * NSUB, ROWS_WG = WAVES * ROWS_WAVE;
    constexpr float BIGF = 3.0e38f;
    constexpr int SCALE = (int)0x82828282u;   // E8M0 2^3 in every byte, both operands: e2m3 numbers become the integers M, products -M_a M_b
    constexpr int NT = SCREEN_CALL_TILES, RING = 3 * NT;   // tile v of the train frame lives in ring slot v % RING
    static_assert(NT == 2 && KS == 4 && NT * 32 == 64, "the waits of a call are counted for two tiles of four steps; wave 0 carries the constants of a call");
    __shared__ v4i sB[RING][TILE_V4];
    __shared__ __attribute__((aligned(16))) float sHb[RING][32];  // |M_b|^2 / 2 of the tile in the same ring slot: the C-init of its chains
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rb = blockIdx.x % wgs_per_pair;
    const int p = blockIdx.x / wgs_per_pair;
    const int2 pr = pairs[p];
    const FrameDev A = frames[pr.x], B = frames[pr.y];
    const int A_even = ((gint_t)A.meta)[0], A_tiles = ((gint_t)A.meta)[1];
    const int T = ((gint_t)B.meta)[2];   // the train tiles that hold a real row (finish_screen_kernel): not the tile that rounds meta[1] up
    if (rb * (ROWS_WG / 32) >= A_tiles) return;  // workgroup-uniform
    const int wv = rb * WAVES + wave;            // this wave's 128 query rows: wave-blocks WBS wv and WBS wv + 1
    const bool active = NSUB * wv < A_tiles;     // (A_tiles counts whole wave-blocks: the second may lie past the frame)
    typedef const __attribute__((address_space(1))) char* gbytes_t;
    typedef const float __attribute__((address_space(1)))* gfloat_t;
    const gbytes_t Aimg = (gbytes_t)A.screen, Bimg = (gbytes_t)B.screen;
    const gfloat_t Am2 = (gfloat_t)(Aimg + (size_t)A.ntiles * SCREEN_TILE_BYTES), Bm2 = (gfloat_t)(Bimg + (size_t)B.ntiles * SCREEN_TILE_BYTES);

    // this wave's 128 query rows, sign bits flipped: the B operand (a lane = query row lane & 15 of the sub-tile, K block kg of the
    // step: the stored fragment that screen::query16_src names, the train side's assignment of kg)
    v6i a[NQ][NS];
#pragma unroll
    for (int s = 0; s < NQ; ++s)
#pragma unroll
        for (int S = 0; S < NS; ++S) {
            const screen::FragSrc src = screen::query16_src(s, S, lane);
            const int qt = NSUB * wv + screen::query16_tile(s);   // (a tile past the frame: tile 0 in its place, its minima are never read)
            const gbytes_t tb = Aimg + (size_t)(qt < A_tiles ? qt : 0) * SCREEN_TILE_BYTES;
            const v4i lo = *(const v4i __attribute__((address_space(1)))*)(tb + screen::frag_lo_offset(src));
            const v2i hi = *(const v2i __attribute__((address_space(1)))*)(tb + screen::frag_hi_offset(src));
            // the sign bit of code e is bit 6 e + 5: a pattern of period three words
            a[s][S] = v6i{lo[0] ^ 0x20820820, lo[1] ^ 0x08208208, lo[2] ^ (int)0x82082082u, lo[3] ^ 0x20820820, hi[0] ^ 0x08208208, hi[1] ^ (int)0x82082082u};
        }
    // [tile parity][sub-tile][row half]: the minimum over the lane's four accumulators of that chain (train rows 16 u + 4 kg .. + 3:
    // one group of four stored rows) over the tiles of that parity
    float xm[2][NQ][NU];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int s = 0; s < NQ; ++s)
#pragma unroll
            for (int u = 0; u < NU; ++u) xm[q][s][u] = BIGF;

    static_assert(TILE_V4 % 64 == 0, "a tile is a whole number of 1 KiB pieces");
    constexpr int PIECES = TILE_V4 / 64;
    static_assert((NT * PIECES) % WAVES == 0, "every wave stages the same number of pieces per call");
    constexpr int PPW = NT * PIECES / WAVES;   // 3: piece i of a wave is piece wave + WAVES i of the call's NT tiles, the earlier tile first
    const int TM = T - 1;
    // (the lane offsets of the staging and of the constants' load are kept opaque: added to the frame's base ahead of the loop they
    // would be held as 64-bit per-lane addresses through the sweep)
    unsigned stage_off = (unsigned)lane * 16u, hb_off = (unsigned)(lane & 31) * 4u;
    // one 1 KiB piece of train tile `tile` (clamped: tile T - 1 again past the end) into ring slot `slot`; all three are wave-uniform
    auto stage_piece = [&](int tile, int slot, int piece) {
        const gbytes_t base = Bimg + (size_t)min(tile, TM) * SCREEN_TILE_BYTES + piece * 1024;
        asm volatile("" : "+v"(stage_off));
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + stage_off),
                                         (__attribute__((address_space(3))) void*)(&sB[slot][piece * 64]), 16, 0, 0);
    };
    // the constants of tile `tile` + (lane / 32), clamped, one per lane of wave 0: loaded a call before they are stored to the ring
    auto load_hb = [&](int tile) {
        asm volatile("" : "+v"(hb_off));
        // (lane / 32 from the staging offset the sweep keeps: the lane itself would be one register more through the sweep, spilled)
        const gbytes_t row = reinterpret_cast<gbytes_t>(Bm2) + (size_t)128 * min(tile + (int)(stage_off >> 9), TM);
        return *reinterpret_cast<gfloat_t>(row + hb_off);
    };
    // An even tile count is peeled at the front, where nothing is in flight: t0 = 1, tile 0 is swept whole ahead of the calls and
    // tile v lives in ring slot (v - t0) mod RING, so that what the calls cover is an odd number of tiles and ends on last() (cut
    // at the back, the even count's last half call ran its chains on a tile that does not exist).
    const int t0 = T > 0 && !(T & 1) ? 1 : 0;   // wave-uniform
    float hb_new = 0.0f;
    if (T > 0) {
        // tiles 0 .. 2 NT + t0: the first call stages the next two into the slot of tile t0 and the one still empty (t0 = 1: tile 0's)
#pragma unroll
        for (int i = 0; i < ((2 * NT + 2) * PIECES + WAVES - 1) / WAVES; ++i) {
            const int idx = wave + WAVES * i, v = idx / PIECES;
            if (v < 2 * NT + 1 + t0) stage_piece(v, v < t0 ? RING - 1 : v - t0, idx % PIECES);
        }
        if (tid < 32 * (NT + 2 + t0)) {
            const int v = tid >> 5;
            sHb[v < t0 ? RING - 1 : v - t0][tid & 31] = Bm2[32 * min(v, TM) + (tid & 31)];
        }
        if (wave == 0) hb_new = load_hb(NT + 2 + t0);   // stored at the head of the first call
    }
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();

    // C-init of the chains of row half u on the tile in ring slot `slot`: accumulator r is train row 16 u + 4 kg + r (screen::acc16_row)
    // (the lane's address in slot 0 is one opaque register, slot and half immediate offsets: derived from the lane at every use it
    // kept the lane alive through the sweep, spilled)
    typedef const v4f __attribute__((address_space(3)))* lds_v4f_t;
    lds_v4f_t hb_lane = (lds_v4f_t)(const __attribute__((address_space(3))) void*)&sHb[0][screen::acc16_row(0, lane, 0)];
    asm volatile("" : "+v"(hb_lane));
    auto cinit_of = [&](int slot, int u) { return hb_lane[8 * slot + 4 * u]; };
    // (the scale is held in one register through the sweep: set up again inside a call it took the register of wave 0's load of the
    // constants, and the compiler put a vmcnt(0) in front of it that drained every wave's staging)
    int scale = SCALE;
    asm volatile("" : "+v"(scale));
    auto mfma = [&](const ScreenFrag& b, const v6i& q, const v4f& c) {
        const v8i q8 = __builtin_shufflevector(q, q, 0, 1, 2, 3, 4, 5, -1, -1);
        return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(screen_operand(b), q8, c, 2, 2, 0, scale, 0, scale);
    };
    v4f acc[NU][NQ];   // a chain = (row half, query sub-tile): two MFMAs, one per step S. ONE set: a second does not fit beside 128 rows
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int s = 0; s < NQ; ++s) acc[u][s] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    ScreenFrag bq[3];  // fragment ring: fragment i of the sequence lives in bq[i % 3]
    const char* sBb = reinterpret_cast<const char*>(&sB[0][0]);
    // the whole tile in ring slot `slot` into acc with reads the compiler tracks (ahead of the calls)
    auto tile_plain = [&](int slot) {
#pragma unroll
        for (int S = 0; S < NS; ++S)
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const screen::FragSrc src = screen::frag16_src(u, S, lane);
                ScreenFrag f;
                f.lo = *reinterpret_cast<const v4i*>(sBb + slot * SCREEN_TILE_BYTES + screen::frag_lo_offset(src));
                f.hi = *reinterpret_cast<const v2i*>(sBb + slot * SCREEN_TILE_BYTES + screen::frag_hi_offset(src));
                const v4f c0 = cinit_of(slot, u);
#pragma unroll
                for (int s = 0; s < NQ; ++s) acc[u][s] = mfma(f, a[s][S], S ? acc[u][s] : c0);
            }
    };
    // the chains of row half u into the minima m, plain (no v_min3_f32 in an asm string, where nothing pads the wait states between
    // the last MFMA and a reader of its accumulators): ahead of the calls and behind them
    auto consume_plain = [&](float(&m)[NQ][NU], int u) {
#pragma unroll
        for (int s = 0; s < NQ; ++s) m[s][u] = fminf(m[s][u], fminf(fminf(acc[u][s][0], acc[u][s][1]), fminf(acc[u][s][2], acc[u][s][3])));
    };
#pragma unroll
    for (int i = 0; i < 3; ++i) bq[i].lo = v4i{0, 0, 0, 0}, bq[i].hi = v2i{0, 0};
    // this lane's bytes in the two planes of slot 0, fragment (0, 0): slot and fragment are immediate offsets of the reads
    unsigned lds16 = lds_addr(sBb) + (unsigned)screen::frag_lo_offset(screen::frag16_src(0, 0, lane));
    unsigned lds8 = lds_addr(sBb) + (unsigned)(screen::frag_hi_offset(screen::frag16_src(0, 0, lane)) - screen::HI_PLANE);
    asm volatile("" : "+v"(lds16), "+v"(lds8));
    // fragment f = u + NU S of the tile in ring slot `slot`: the immediates of its two reads
    auto frag_lo_imm = [](int slot, int f) constexpr { return slot * SCREEN_TILE_BYTES + screen::frag_lo_offset(screen::frag16_src(f % NU, f / NU, 0)); };
    auto frag_hi_imm = [](int slot, int f) constexpr { return slot * SCREEN_TILE_BYTES + screen::frag_hi_offset(screen::frag16_src(f % NU, f / NU, 0)); };
    // Inside the sweep every LDS operation is one the compiler does not track, so that every wait is a counted one placed here: the
    // fragments, the C-init of the chains after next (ci: read into registers of the accumulators just consumed, handed to the first
    // MFMAs as their C operand behind the wait of the half that issues its chains) and wave 0's store of the constants.
    unsigned hb_rd = lds_addr(&sHb[0][screen::acc16_row(0, lane, 0)]), hb_wr = lds_addr(&sHb[0][0]) + 4u * lane;
    asm volatile("" : "+v"(hb_rd), "+v"(hb_wr));
    // A lane's four constants of a row half depend on the tile, the half and kg only, so ONE set serves the four query sub-tiles: it
    // is the C operand of the first step of all four chains, which write accumulators of their own (D != C; the last may go on in
    // ci's registers).
    v4f ci[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) ci[u] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    auto cinit_issue = [&](int slot) {
#pragma unroll
        for (int u = 0; u < NU; ++u) lds_read_frag(ci[u], hb_rd, 128 * slot + 64 * u);
    };
    // lgkmcnt(0) on everything the sweep may have in flight (ahead of the first call, and behind the last)
    auto drain_lds = [&]() {
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(bq[0].lo), "+v"(bq[0].hi), "+v"(bq[1].lo), "+v"(bq[1].hi), "+v"(bq[2].lo), "+v"(bq[2].hi), "+v"(ci[0]), "+v"(ci[1]));
    };
    if (T > 0 && active) {
        if (t0) {
            // the peeled tile 0, whole: its chains, then its epilogue into the minima of the even tiles (the second half's: the calls
            // start at tile 1, so xm[0] takes the odd tiles)
            tile_plain(RING - 1);
            consume_plain(xm[1], 0), consume_plain(xm[1], 1);
        }
        // tile t0: the chains of its row half 0 are consumed here, those of half 1 under the first step of the first call (or by last())
        tile_plain(0);
        consume_plain(xm[0], 0);
        // the constants and the first fragments of tile 1 (the ring holds tile T - 1 again past the end: recomputed, never consumed)
        cinit_issue(1);
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            lds_read_frag(bq[f].lo, lds16, frag_lo_imm(1, f));
            lds_read_frag64(bq[f].hi, lds8, frag_hi_imm(1, f));
        }
        drain_lds();
    }
    __syncthreads();   // slot 0 is staged into again by the first call below
    // the four accumulators of chain (u, s) -> its running minimum of tile parity q: two v_min3_f32
    auto consume = [&](float(&m)[NQ][NU], const int u, const int s) {
        m[s][u] = fmin3(m[s][u], acc[u][s][0], acc[u][s][1]);
        m[s][u] = fmin3(m[s][u], acc[u][s][2], acc[u][s][3]);
    };
    // One call covers NT = 2 train tiles between two barriers (t = t0 + 2 k; K3 = call mod 3 gives the ring slots and the phase of
    // the fragment ring, which advances NT KS = 8 steps per call). Half HH runs the chains of tile t + 1 + HH. A tile is 32 MFMAs of
    // the 16x16x128 shape: its four fragments f = u + 2 S (row half u of the tile, K = 128 step S; screen::frag16_src) in the order
    // (0,0) (1,0) (0,1) (1,1), each the A operand of EIGHT MFMAs, one per query sub-tile of 16 rows: a step. The sixteen chains
    // (u, sub-tile) of a tile are two MFMAs long, and the second comes two steps = sixteen MFMAs behind the first.
    // There is one set of accumulators, and each row half's has one step in which it is consumed:
    //     step 0 (0,0)  writes acc[0] from ci[0]          consumes acc[1] of the tile BEFORE (ended in its step 3)  -> xm[HH]
    //     step 1 (1,0)  writes acc[1] from ci[1]
    //     step 2 (0,1)  ends the chains of acc[0]         issues the C-init of the next tile (ci is free from step 1 on)
    //     step 3 (1,1)  ends the chains of acc[1]         consumes acc[0] of THIS tile (ended in step 2)            -> xm[1 - HH]
    // (tile t + HH has parity HH behind t0, tile t + 1 + HH the other). A step goes in four groups of two MFMAs with a scheduling
    // barrier behind each; group g consumes sub-tiles 2 g and 2 g + 1, whose chains ended with MFMAs 2 g and 2 g + 1 of the step
    // before: at least 6 MFMAs lie between the MFMA that finished an accumulator and the v_min3_f32 that reads it, wherever the
    // compiler puts the four inside their group. Ahead of the first call and behind the last there is no step to hide under:
    // consume_plain().
    // Step i of the eight waits for fragment i, issues fragment i + 2 (the last two are the first of tile t + 3) and, once per half,
    // the C-init of the next tile into ci: two ds_read_b128 (one per row half: the constants of train rows 16 u + 4 kg .. + 3) at
    // step 2. One set of constants starts the eight chains of a row half at step u of the half.
    // The LDS queue of a wave is in order and every operation in it is issued here, so every wait is counted. A half issues
    //     step 0: F2    step 1: F3    step 2: F4, C    step 3: F5          (F_k: the two reads of the fragment of step k, F4 / F5 the
    //                                                                       next half's steps 0 / 1; C: the two reads of the C-init)
    // so that behind the fragment of step ks were issued
    //     ks 0   the C-init (2, needed too: the chains start on it), the fragment of step 1 (2)   lgkmcnt(2)
    //     ks 1   the fragment of step 2 (2)                                                        lgkmcnt(2)
    //     ks 2   the fragment of step 3 (2)                                                        lgkmcnt(2)
    //     ks 3   the fragment of the next step 0 (2), the C-init (2)                               lgkmcnt(4)
    // (the issue order of a half is what it was with four MFMAs to a step, so the counts are; wave 0's store of the constants at
    // the head of the call is one more operation behind some of them: a wait that asks for more than it needs). Nothing is drained
    // at the barrier: the two fragments and the C-init in flight read slots that the next call does not stage into.
    // Staging: the call stages tiles t + 2 NT + 1 and t + 2 NT + 2 into the slots of tiles t - 1 and t (read for the last time
    // ahead of the previous barrier), three pieces per wave behind steps 0, 2 and 4, the earlier tile's first. The earlier tile is
    // read from step 6 of the NEXT call on, the later one a call after that: before the barrier a wave waits for all but the last
    // piece it issued (vmcnt(1): every wave's last piece belongs to the later tile), so a piece has between half a call and a call
    // and a half to land. Wave 0 loads the constants of tiles t + 2 NT + 2 / + 3 first (the oldest entry of its counter), stores
    // them at the head of the next call, and they are read from the call after that on.
    auto call = [&](auto K3c, const int t) {
        constexpr int K3 = decltype(K3c)::value;
        constexpr int BASE = NT * K3;                 // ring slot of tile t
        constexpr int PH = (K3 * ((NT * KS) % 3)) % 3;
        auto stage = [&](int i) {
            const int idx = wave + WAVES * i, later = idx >= PIECES ? 1 : 0;
            stage_piece(t + 2 * NT + 1 + later, later ? (BASE + 2 * NT + 2) % RING : (BASE + 2 * NT + 1) % RING, idx - PIECES * later);
        };
        if (wave == 0) {
            asm volatile("ds_write_b32 %0, %1 offset:%2" : : "v"(hb_wr), "v"(hb_new), "n"(((BASE + NT + 2) % RING) * 128) : "memory");
            hb_new = load_hb(t + 2 * NT + 2);
        }
        auto half = [&](auto HHc) {
            constexpr int HH = decltype(HHc)::value;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int i = HH * KS + ks, j = i + 2;
                ScreenFrag& f = bq[(i + PH) % 3];
                const int u = ks % NU, S = ks / NU;   // the fragment of this step
                if (ks == 0) {
                    // the fragment of this step and, behind it, the C-init were issued at step 2 of the half before: younger is the fragment of step 1
                    asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(f.lo), "+v"(f.hi), "+v"(ci[0]), "+v"(ci[1]));
                } else if (ks < KS - 1) {
                    asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(f.lo), "+v"(f.hi));   // issued two steps ago; younger: the fragment of the next step
                } else {
                    // issued at step 1; younger: the fragment of the next step 0 (2) and the C-init (2), both issued at step 2
                    asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(f.lo), "+v"(f.hi));
                }
                lds_read_frag(bq[(j + PH) % 3].lo, lds16, frag_lo_imm((BASE + 1 + j / KS) % RING, j % KS));
                lds_read_frag64(bq[(j + PH) % 3].hi, lds8, frag_hi_imm((BASE + 1 + j / KS) % RING, j % KS));
                // eight MFMAs on eight chains, in groups of two: the second step of a chain comes NU steps = sixteen MFMAs behind its
                // first. The eight chains of a row half start on its one set of constants
#pragma unroll
                for (int g = 0; g < NQ / 2; ++g) {
#pragma unroll
                    for (int s = 2 * g; s < 2 * g + 2; ++s) acc[u][s] = mfma(f, a[s][S], S ? acc[u][s] : ci[u]);
#pragma unroll
                    for (int s = 2 * g; s < 2 * g + 2; ++s) {
                        if (ks == 0) consume(xm[HH], 1, s);           // the tile before, row half 1
                        if (ks == KS - 1) consume(xm[1 - HH], 0, s);  // this tile, row half 0
                    }
                    if (g < NQ / 2 - 1) __builtin_amdgcn_sched_barrier(0);
                }
                if (ks == 2) cinit_issue((BASE + HH + 2) % RING);   // the constants of the next tile: ci[1] was last read by step 1's MFMAs
                if (i % 2 == 0 && i / 2 < PPW) stage(i / 2);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        if (active) {
            half(std::integral_constant<int, 0>{});
            half(std::integral_constant<int, 1>{});
        } else {
#pragma unroll
            for (int i = 0; i < PPW; ++i) stage(i);
        }
        asm volatile("s_waitcnt vmcnt(1)" : : : "memory");
        __builtin_amdgcn_s_barrier();
    };
    // the last tile (an even number of tiles behind t0) has nothing to issue and nothing to stage: the epilogue of its row half 1 alone
    // (plain minima, as for the peeled tile: those chains ended with the last MFMAs of the last call)
    auto last = [&]() {
        if (active) consume_plain(xm[0], 1);
    };
    if (T > 0) {
        // tiles t0 + 1 .. TM have their chains inside a call, tiles t0 .. TM - 1 their epilogue: TM - t0 of each, an even number (the
        // front peel), so (TM - t0) / 2 calls and tile TM is left to last()
        const int NC = (TM - t0) / 2;
        int c = 0;
        for (; c + 3 <= NC; c += 3) {
            call(std::integral_constant<int, 0>{}, t0 + NT * c);
            call(std::integral_constant<int, 1>{}, t0 + NT * (c + 1));
            call(std::integral_constant<int, 2>{}, t0 + NT * (c + 2));
        }
        if (c < NC) call(std::integral_constant<int, 0>{}, t0 + NT * c);
        if (c + 1 < NC) call(std::integral_constant<int, 1>{}, t0 + NT * (c + 1));
        // nothing may land in a register or in this workgroup's LDS once the sweep is over
        asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
        drain_lds();
        last();
    }
    if (!active) return;
    // The tail runs per wave-block of 64 rows, the wave's two one after the other (the second only where it has a tile of the frame).
    // A query row's sixteen subset minima lie in the four lanes of its column (lane & 15 of its sub-tile, one per kg), four each
    // (tile parity x row half): the two smallest of the four, joined across the lanes (xor 16, xor 32) as pairs. All four lanes end
    // with the same two numbers, so lane 16 s + i keeps those of sub-tile s of the wave-block: every lane owns the row of the
    // wave-block of its number, and the bounds are computed once for the 64 rows.
    constexpr int ROWS_WB = 32 * WB_TILES;
    const gint_t Asr = (gint_t)(Am2 + 32 * (size_t)A.ntiles);
    const int e_b = T > 0 ? ((gint_t)(Bm2 + 64 * (size_t)B.ntiles))[0] : 0;
    const int lane_t = (int)((hb_wr - lds_addr(&sHb[0][0])) >> 2);   // (the lane, from what the sweep kept)
    constexpr unsigned PAD_V = 2u * PADH;
    auto tail = [&](auto Hc) {
        constexpr int H = decltype(Hc)::value;
        const int wb = WBS * wv + H;
        if (WB_TILES * wb >= A_tiles) return;   // wave-uniform
        uint4* rr = rowres + (size_t)p * row_stride + ROWS_WB * wb;
        float v1 = BIGF, v2 = BIGF;
#pragma unroll
        for (int s = 0; s < NQ / WBS; ++s) {
            static_assert(screen::query16_block(NQ / WBS * H) == H, "the sub-tiles of wave-block H");
            float m1 = BIGF, m2 = BIGF;
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const float mine = xm[q][NQ / WBS * H + s][u];
                    m2 = fminf(m2, fmaxf(m1, mine)), m1 = fminf(m1, mine);
                }
#pragma unroll
            for (int x = 16; x <= 32; x *= 2) {
                const float o1 = __shfl_xor(m1, x), o2 = __shfl_xor(m2, x);   // two sorted pairs: min of the firsts, then the next
                m2 = fminf(fmaxf(m1, o1), fminf(m2, o2)), m1 = fminf(m1, o1);
            }
            if ((lane_t >> 4) == s) v1 = m1, v2 = m2;
        }
        unsigned long long open_rows = 0;   // bit = row of the wave-block: that row goes to the exact pass
        {
            const int s = lane_t >> 5;      // the stored query tile of the row
            const int j = ROWS_WB * wb + lane_t;
            const float ma = Am2[j];
            // a padding train row holds SCREEN_PAD or more, a subset that met no tile BIGF; real values stay below 2^21
            const bool real_row = ma < 0.5f * SCREEN_PAD;
            const bool real1 = real_row && v1 < 0.5f * SCREEN_PAD, real2 = real_row && v2 < 0.5f * SCREEN_PAD;
            const unsigned pa = WB_TILES * wb + s >= A_even ? 1u : 0u;
            const int s_a = Asr[j];
            const unsigned n1 = real1 ? (unsigned)(2.0f * (v1 + ma)) : 0u, u = real2 ? (unsigned)(2.0f * (v2 + ma)) : 0u;
            const unsigned w1 = real1 ? (unsigned)screen::lower_d2(n1, s_a, e_b) - pa + 2u : 0xffffffffu;
            const unsigned w2 = real2 ? (unsigned)screen::upper_d2(u, s_a, e_b) - pa + 2u : 0xffffffffu;
            rr[lane_t] = make_uint4(w1, 0u, w2, real1 ? n1 : 0xffffffffu);
            // match_rowpick_kernel's predicate on the two words just stored (a padding row carries 0xffffffff in the first)
            const bool open = WB_TILES * wb + s < A_tiles && w1 < PAD_V && (w2 >= PAD_V || ratio_pass<METRIC>((int)(w1 + pa) - 2, (int)(w2 + pa) - 2, ratio));
            open_rows = __ballot(open);
        }
        if (!openmask) return;   // (the debug entry: no list)
        if (lane_t == 0) openmask[(size_t)p * mask_stride + wb] = open_rows;
        // the wave-block's open rows go into its segment's region of the candidate list (the comment above match_openprep_kernel)
        const int c = __popcll(open_rows);
        if (c == 0) return;      // wave-uniform: open_rows is a ballot
        const int head = ol.seghead[p];
        int pos = 0;
        if (lane_t == 0) pos = atomicAdd(&ol.segcount[head], c);
        pos = __shfl(pos, 0);
        if ((open_rows >> lane_t) & 1)
            ol.cands[(size_t)head * row_stride + pos + __popcll(open_rows & ((1ull << lane_t) - 1))] = make_uint2((unsigned)p, (unsigned)(ROWS_WB * wb + lane_t));
        const int k = (pos + GATHER_WIDTH - 1) / GATHER_WIDTH;   // c <= 64: at most one multiple of the width in [pos, pos + c)
        if (lane_t == 0 && GATHER_WIDTH * k < pos + c) ol.items[atomicAdd(ol.n_items, 1)] = make_int2(head, k);
    };
    tail(std::integral_constant<int, 0>{});
    tail(std::integral_constant<int, 1>{});
}

// ------------------------------------------------------------------------------------------------
// K2: merge column partials, ratio test, mutual check, thresholds, ordered compaction
// ------------------------------------------------------------------------------------------------

// FeatureMatcherFlann.cpp:23 — `m[0].distance / m[1].distance < 0.8`: distances are
// sqrtf(squared L2) in fp32, fp32 quotient, compared as double. d2 values are exact integers.
//
// metric = METRIC_HAMMING (binary frames, matcher_ham.hip): a bit is stored as 0 / 255, so d2 = 65025 h exactly, and
// cv::BFMatcher(NORM_HAMMING) hands the same test the quotient (float)h0 / (float)h1 with no square root. h and 65025 h are
// both exact in fp32, hence fdiv(d2_0, d2_1) is bit for bit fdiv(h0, h1): the Hamming test on the integers the kernels hold,
// the bounds (no multiples of 65025) included. Like the L2 form it is monotone in both arguments, false on 0/0 and false
// on a negative argument (the "no real minimum" values: sqrtf gives NaN there, the Hamming form says so).
constexpr int METRIC_L2 = 0, METRIC_HAMMING = 1;
// The kernels that test the ratio take the metric as a template argument: their L2 instantiations are the code they were before.
template <int METRIC>
__device__ __forceinline__ bool ratio_pass(int d2_best, int d2_second, double ratio) {
    if (METRIC == METRIC_HAMMING) return d2_best >= 0 && d2_second >= 0 && (double)__fdiv_rn((float)d2_best, (float)d2_second) < ratio;
    float q = __fdiv_rn(__fsqrt_rn((float)d2_best), __fsqrt_rn((float)d2_second));
    return (double)q < ratio;  // 0/0 = NaN -> false
}

// mode 0: mutual matches + thresholds (apps/sfm/main.cpp:111-146); mode 1: directed list m12.
// out_matches[p][k] = {q, t} sorted by q; counts[p]; stats[p] = {|m12|, |m21|, |mutual|, edge}.
// Rows/columns are addressed by stored position inside; q and t leave in the caller's numbering.
template <int METRIC>
__global__ __launch_bounds__(FIN_THREADS) void match_finalize_kernel(
    const FrameDev* __restrict__ frames, const int2* __restrict__ pairs,
    const uint4* __restrict__ rowres, const uint2* __restrict__ colpart, int col_chunks, int wb_stride,
    int row_stride, double ratio, int min_dir, int min_mutual, int mode,
    uint2* __restrict__ out_matches, int* __restrict__ counts, int4* __restrict__ stats) {
    extern __shared__ int smem[];
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    const int2 pr = pairs[p];
    const FrameDev A = frames[pr.x], B = frames[pr.y];
    const int A_even = A.meta[0], A_tiles = A.meta[1], B_even = B.meta[0], B_tiles = B.meta[1];
    int* keepcol = smem;           // [row_stride] by stored row: stored column of the kept match or -1
    int* bwd = smem + row_stride;  // [row_stride] by stored column: d2 of the column's best if it passes the ratio test, else -1
    __shared__ int s_cnt[3];
    if (tid < 3) s_cnt[tid] = 0;
    __syncthreads();
    constexpr unsigned PAD_V = 2u * PADH;  // v = 2H + parity of anything involving a padding row/column

    // columns first: top-2 VALUES of every stored column over the wave-blocks of A
    int c12 = 0, c21 = 0;
    constexpr int WG_TILES = ROWS_PER_WG / 32;
    const int nslots = (A_tiles + WG_TILES - 1) / WG_TILES + 1;  // workgroup rb fills slot rb (even rows) and/or rb + 1 (odd rows)
    const int first_odd = A_even / WG_TILES + 1;
    for (int c = tid; c < 32 * B_tiles; c += FIN_THREADS) {
        int d = -1;
        if (B.orig[c] >= 0) {
            unsigned v1 = 0xffffffffu, v2 = 0xffffffffu;
            const uint2* cp = colpart + (size_t)p * wb_stride * row_stride + c;
            for (int k = 0; k < nslots; ++k) {
                const bool even = WG_TILES * k < A_even;
                if (!even && k < first_odd) continue;                     // the slot between the classes when A_even % 8 == 0
                const uint2 e = cp[(size_t)k * row_stride];
                const unsigned pa = even ? 0u : 1u;                        // one parity per slot
                const unsigned va = ((e.x >> (KEY_SHIFT + 1)) << 1) | pa, vb = ((e.y >> (KEY_SHIFT + 1)) << 1) | pa;
                v2 = umin(umin(umax(v1, va), v2), vb);  // (va <= vb) merged into (v1 <= v2)
                v1 = umin(v1, va);
            }
            const unsigned pb = (c >> 5) >= B_even ? 1u : 0u;
            const bool ok = v2 < PAD_V && ratio_pass<METRIC>((int)(v1 + pb) - 2, (int)(v2 + pb) - 2, ratio);  // pad second => < 2 query rows
            d = ok ? (int)(v1 + pb) - 2 : -1;
            c21 += ok;
        }
        bwd[c] = d;
    }
    __syncthreads();
    const int nchunks = (B_tiles + CHUNK_TILES - 1) / CHUNK_TILES;
    for (int j = tid; j < 32 * A_tiles; j += FIN_THREADS) {
        int keep = -1;
        if (A.orig[j] >= 0) {
            unsigned v1 = 0xffffffffu, v2 = 0xffffffffu, col = 0;
            for (int ch = 0; ch < nchunks; ++ch) {  // ascending columns; strict '<' keeps the lower column on ties
                const uint4 e = rowres[((size_t)p * col_chunks + ch) * row_stride + j];
                if (e.x < v1) {
                    v2 = umin(v1, e.z);
                    v1 = e.x;
                    col = e.y;
                } else {
                    v2 = umin(v2, e.x);
                }
            }
            const unsigned pa = (j >> 5) >= A_even ? 1u : 0u;
            const bool ok = v2 < PAD_V && ratio_pass<METRIC>((int)(v1 + pa) - 2, (int)(v2 + pa) - 2, ratio);  // pad second => < 2 train rows
            c12 += ok;
            // main.cpp:133-140: q is kept iff t's own best match is q, i.e. iff t passes the ratio
            // test (unique minimum for any ratio <= 1) and its minimum is d2(q, t)
            if (ok && (mode == 1 || bwd[col] == (int)(v1 + pa) - 2)) keep = (int)col;
        }
        keepcol[j] = keep;
    }
    atomicAdd(&s_cnt[0], c12);
    atomicAdd(&s_cnt[1], c21);
    __syncthreads();

    // (by stored position inside, the caller's numbering out)
    const int base = compact_kept_rows(
        A.n, tid, out_matches + (size_t)p * row_stride, [&](int q) { return keepcol[A.pos[q]]; }, [&](int t) { return B.orig[t]; });
    if (tid == 0) write_pair_result(p, mode, s_cnt[0], s_cnt[1], base, min_dir, min_mutual, counts, stats);
}

// ------------------------------------------------------------------------------------------------
// The candidate-only column pass (round 4). The tile sweep is bound by the VALU issue port and its column direction is
// 1.67 of the 4.67 operations it spends per distance (profiles/r04_coltop_knockout.txt: the sweep alone is 26 % / 39 %
// faster at 256-D / 128-D). But the pair loop of apps/sfm/main.cpp:111,133-142 only ever looks at column t = m12[q] of a
// row q that passed the ratio test: with |mutual| > min_mutual >= min_dir - 1 the two direction thresholds are implied
// (every mutual match is in m12 and in m21), so a pair with no more than min_mutual passing rows is dead, and for the
// others the column top-2 is needed for the passing rows' best columns only. Small kernels replace K2:
//   R  match_rows2_kernel      per pair: ratio test, ordered list of the passing rows (candidates); match_argmin_kernel finds
//                              their columns and settles what it can, match_colpick_kernel lists the rest, 64 per work item
//   V  match_colverify_kernel  per item: d2 of 64 candidate columns against ALL rows of the query frame on the int8 MFMA
//                              with the operands swapped (candidates = B operand, one per lane), top-2 VALUES per column
//   F  match_finalize2_kernel  per pair: keep candidate (q, t) iff column t passes the ratio test with minimum d2(q, t);
//                              ordered compaction in the caller's row order, threshold
// ------------------------------------------------------------------------------------------------

constexpr int VER_GROUPS = 2;                 // 32-candidate groups per wave: one fetched A fragment feeds two MFMA chains
constexpr int VER_CANDS = 32 * VER_GROUPS;    // candidates per work item

// Behind the BOUND form of the sweep (match_sweep_kernel<KS, true>): rowres[p][j] = {v1, 0, u, 0} with u an upper bound of the row's
// second-smallest value. A row that fails the ratio test against u fails it against the truth and stays as it is (match_rows2_kernel
// will fail it on the same two numbers); every other row with a real minimum is a candidate of the exact pass — also a row whose bound
// is a padding value (its runner-up, if it has one, shares the minimum's subset: a train frame of two adjacent rows). Lists the
// candidates of the pair (candlist, state[p].x = their number) and appends one item per 64 of them for match_colverify_kernel<KS, true>.
template <int METRIC>
__global__ __launch_bounds__(FIN_THREADS) void match_rowpick_kernel(
    const FrameDev* __restrict__ frames, const int2* __restrict__ pairs, const uint4* __restrict__ rowres, int row_stride, double ratio,
    int* __restrict__ candlist, int4* __restrict__ state, int2* __restrict__ items, int* __restrict__ n_items,
    unsigned long long* __restrict__ tally = nullptr) {
    __shared__ int s_wave[FIN_THREADS / 64];
    __shared__ int s_item0;
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    const int2 pr = pairs[p];
    const FrameDev A = frames[pr.x];
    const int A_even = A.meta[0], A_tiles = A.meta[1];
    constexpr unsigned PAD_V = 2u * PADH;
    int* cl = candlist + (size_t)p * row_stride;
    int base = 0;
    if (tally && tid == 0) atomicAdd(&tally[0], (unsigned long long)A.n);   // behind the screen sweep: {real query rows, rows left open} of the call
    for (int j0 = 0; j0 < 32 * A_tiles; j0 += FIN_THREADS) {
        const int j = j0 + tid;
        bool ok = false;
        if (j < 32 * A_tiles && A.orig[j] >= 0) {
            const uint4 e = rowres[(size_t)p * row_stride + j];
            const unsigned pa = (j >> 5) >= A_even ? 1u : 0u;
            ok = e.x < PAD_V && (e.z >= PAD_V || ratio_pass<METRIC>((int)(e.x + pa) - 2, (int)(e.z + pa) - 2, ratio));
        }
        int total;
        const int rank = block_rank(ok, tid, s_wave, total);
        if (ok) cl[base + rank] = j;
        base += total;
    }
    const int groups = (base + VER_CANDS - 1) / VER_CANDS;
    if (tid == 0) {
        state[p] = make_int4(base, 0, 0, 0);
        s_item0 = groups ? atomicAdd(n_items, groups) : 0;
        if (tally) atomicAdd(&tally[1], (unsigned long long)base);
    }
    __syncthreads();
    for (int g = tid; g < groups; g += FIN_THREADS) items[s_item0 + g] = make_int2(p, g);
}

// Behind the SCREEN form of the sweep (match_screen_kernel): the rows its tail left open (openmask[p][wb]: one bit per row of
// wave-block wb, match_rowpick_kernel's predicate) become ONE candidate list per launch, cut into items per train-frame run.
// At the headline nine pairs in ten have an open row but the typical pair has two or three (the bound's slack), and an item streams
// the whole train frame whatever it holds: per-pair items of 64 ran about half empty (38 103 items for 1.39 M open rows of an S200
// step). Only the streamed frame has to be common to an item — the exact pass gathers its query rows per lane — so the candidates of
// consecutive pairs onto one train frame share items (shard.order_pairs sorts a job by train frame): 5 537 items of 256.
//   segment    a maximal run of consecutive pairs of the launch with one train frame (pairs[p].y); any pair order is legal and
//              only gives shorter segments. Its head is its first pair
//   cands      {pair index within the launch, stored query row}. The segment of head h owns cands[h * row_stride ..] of the
//              slot's rowcand area: room for row_stride candidates per pair of the segment, never less than its open rows, so no
//              prefix sum places it. Inside the region the candidates stand in the order the sweep's waves reserved their room
//              (one returning add of the wave's open rows to segcount[h]): no output depends on it, a candidate is a lane of the
//              exact pass
//   items      {h, k}: candidates 256 k .. 256 k + 255 of the segment of head h, as far as segcount[h] goes (width GATHER_WIDTH =
//              256, a workgroup of the gathered sweep). The wave whose reservation holds candidate 256 k creates the item (one
//              add to the launch's counter), so a segment of n open rows has ceil(n / 256) items and a launch with no open row
//              none; their order in the list is that of the adds
// seghead, segcount and the item counters are arrays of the CALL, outside the workspace slots: match_openprep_kernel sets them up
// for every launch ahead of the first sweep (the launches are a function of the pair's index: LaunchCut, match_plan.hpp), and nothing of the list
// runs between a sweep and its exact pass. The debug tallies: the real query rows here (they depend on the pairs only), open rows
// and items by match_opentally_kernel on the second stream behind the exact pass — one add per workgroup, never one per pair.
constexpr int PREP_THREADS = 256;
__global__ __launch_bounds__(PREP_THREADS) void match_openprep_kernel(const FrameDev* __restrict__ frames, const int2* __restrict__ pairs, int npairs,
                                                                      LaunchCut cut, int* __restrict__ seghead, int* __restrict__ segcount,
                                                                      int* __restrict__ launch_items, unsigned long long* __restrict__ tally) {
    __shared__ unsigned long long s_rows[PREP_THREADS / 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * PREP_THREADS + threadIdx.x;
    const bool live = i < npairs;
    int start = 0, y = 0, v = -1;   // v: the last segment head at or before pair i, as far as this wave sees
    unsigned long long rows = 0;
    if (live) {
        const int2 pr = pairs[i];
        const int b = launch_of(cut, i, &start);
        y = pr.y;
        rows = (unsigned long long)frames[pr.x].n;
        if (i == start || pairs[i - 1].y != y) v = i;
        segcount[i] = 0;
        if (i == start) launch_items[b] = 0;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d);
        if (lane >= d) v = max(v, u);
    }
    // lanes without a head up to them continue the segment of the wave's first pair (a launch starts a segment, so they are of its
    // launch): the wave looks for its head 64 pairs at a time, back to the start of the launch
    const bool need = live && v < 0;
    if (__ballot(need)) {   // wave-uniform; lane 0 is one of them
        const int w0 = blockIdx.x * PREP_THREADS + 64 * wave, s0 = __shfl(start, 0), y0 = __shfl(y, 0);
        int hd = s0;
        for (int base = w0 - 1; base >= s0; base -= 64) {
            const int j = base - lane;
            const unsigned long long m = __ballot(j >= s0 && pairs[j].y != y0);
            if (m) {   // the nearest pair onto another frame: the segment starts behind it
                hd = base - (__ffsll((long long)m) - 1) + 1;
                break;
            }
        }
        if (need) v = hd;
    }
    if (live) seghead[i] = v - start;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) rows += __shfl_xor(rows, d);
    if (lane == 0) s_rows[wave] = rows;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long r = 0;
        for (int k = 0; k < PREP_THREADS / 64; ++k) r += s_rows[k];
        atomicAdd(&tally[0], r);   // {real query rows} of the call
    }
}

// {rows left open, items of the exact pass} of a launch into the call's tally, once the launch's sweep has ended
constexpr int TALLY_THREADS = 1024;
__global__ __launch_bounds__(TALLY_THREADS) void match_opentally_kernel(const int* __restrict__ seghead, const int* __restrict__ segcount, int npairs,
                                                                        const int* __restrict__ n_items, unsigned long long* __restrict__ tally) {
    __shared__ unsigned long long s_open[TALLY_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x * TALLY_THREADS + threadIdx.x;
    unsigned long long open = p < npairs && seghead[p] == p ? (unsigned long long)segcount[p] : 0ull;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) open += __shfl_xor(open, d);
    if (lane == 0) s_open[wave] = open;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long o = 0;
        for (int k = 0; k < TALLY_THREADS / 64; ++k) o += s_open[k];
        atomicAdd(&tally[1], o);
        if (blockIdx.x == 0) atomicAdd(&tally[2], (unsigned long long)*n_items);
    }
}

// The rows kernel of the operand-swapped sweep (match_sweep_kernel): rowres carries the TILE of a row's minimum, not its column.
// rowcand[p][j] = {tile of row j's best, d2} if stored row j passes the ratio test, else {~0, 0}; candlist[p][i] = stored row of the
// i-th passing row (ascending j); state[p] = {passing rows, live, L(p), 0}. The passing rows of a pair that goes on are grouped by
// that tile (bytile[p][..], a counting sort in LDS) and one argmin item is appended per (tile, <= 32 rows) — match_argmin_kernel
// turns the tile into the column.
// state[p].z = L(p), a lower bound of d2(q', t) for every real row q' and every column t that is not q''s own best column: the
// smallest of d2_1 over the rows that are no candidates (their minimum bounds ALL their distances; under the bound form of the sweep
// their third word is no runner-up, so only the first is used) and of d2_2 over the candidates (exact {v1, tile, v2} in both forms:
// every column but the best one is at least the runner-up). match_argmin_kernel settles candidate columns with it.
constexpr int MAX_TILES = MAX_ROWS / 32;
constexpr int AITEM_SHARED = 1 << 16;   // aitems[..].y: the tile, plus this flag when the pair has more than one item of that tile
// OPEN = true (mode 0 behind the SCREEN form of the sweep only): every candidate is a row the screen left open, and their number is
// the popcount of the pair's mask words (openmask[p][..], 256 B where its rowres is 32 KB; every wave counts them all, so no
// barrier). A pair with no more than min_mutual open rows is dead
// whatever its rows hold (nine pairs in ten of S200), so it gets a dead pair's state — not live, no arg-min item, which is all that
// match_colpick_kernel and match_finalize2_kernel read of it (count 0) — without one byte of its rowres; its rowcand,
// candlist and L(p) are left out, nothing reads them for a dead pair.
template <int METRIC, bool OPEN = false>
__global__ __launch_bounds__(FIN_THREADS) void match_rows2_kernel(
    const FrameDev* __restrict__ frames, const int2* __restrict__ pairs, const uint4* __restrict__ rowres, int row_stride, double ratio,
    int min_dir, int min_mutual, int mode, uint2* __restrict__ rowcand, int* __restrict__ candlist, int* __restrict__ bytile,
    int4* __restrict__ state, int4* __restrict__ aitems, int* __restrict__ n_aitems,
    const unsigned long long* __restrict__ openmask = nullptr, int mask_stride = 0) {   // (OPEN only)
    __shared__ int s_wave[FIN_THREADS / 64];
    __shared__ int s_cnt[MAX_TILES], s_pos[MAX_TILES], s_grp[MAX_TILES];
    __shared__ int s_scan[FIN_THREADS], s_scan2[FIN_THREADS];
    __shared__ int s_aitem0, s_low;
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    if constexpr (OPEN) {
        const int nwords = (frames[pairs[p].x].meta[1] + 1) / 2;   // the words the sweep wrote: one per wave-block with a real tile
        int open = 0;
        for (int w = tid & 63; w < nwords; w += 64) open += __popcll(openmask[(size_t)p * mask_stride + w]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) open += __shfl_xor(open, d);
        if (open <= min_mutual) {   // workgroup-uniform: every wave has counted all the words
            if (tid == 0) state[p] = make_int4(open, 0, 0x7fffffff, 0);
            return;
        }
    }
    const int2 pr = pairs[p];
    const FrameDev A = frames[pr.x], B = frames[pr.y];
    const int A_even = A.meta[0], A_tiles = A.meta[1], B_tiles = B.meta[1];
    constexpr unsigned PAD_V = 2u * PADH;
    uint2* rc = rowcand + (size_t)p * row_stride;
    int* cl = candlist + (size_t)p * row_stride;
    for (int t = tid; t < MAX_TILES; t += FIN_THREADS) s_cnt[t] = 0;
    if (tid == 0) s_low = 0x7fffffff;
    __syncthreads();
    int base = 0, low = 0x7fffffff;
    for (int j0 = 0; j0 < 32 * A_tiles; j0 += FIN_THREADS) {
        const int j = j0 + tid;
        bool ok = false;
        unsigned tile = 0;
        int d2 = 0;
        if (j < 32 * A_tiles && A.orig[j] >= 0) {
            const uint4 e = rowres[(size_t)p * row_stride + j];
            const unsigned pa = (j >> 5) >= A_even ? 1u : 0u;
            tile = e.y;
            d2 = (int)(e.x + pa) - 2;
            ok = e.z < PAD_V && ratio_pass<METRIC>(d2, (int)(e.z + pa) - 2, ratio);  // pad second => < 2 train rows
            low = imin(low, ok ? (int)(e.z + pa) - 2 : d2);   // (a row without a real minimum gives a negative value: nothing is settled then)
        }
        if (j < 32 * A_tiles) rc[j] = ok ? make_uint2(tile, (unsigned)d2) : make_uint2(0xffffffffu, 0u);
        if (ok) atomicAdd(&s_cnt[tile], 1);
        int total;
        const int rank = block_rank(ok, tid, s_wave, total);
        if (ok) cl[base + rank] = j;
        base += total;
    }
    // main.cpp:111,142: an edge needs |m12| >= min_dir and |mutual| > min_mutual, and mutual is a subset of m12
    const bool live = mode == 0 && base >= min_dir && base > min_mutual;
    const bool want_col = live || (mode == 1 && base > 0);   // directed lists need the column of every passing row
    atomicMin(&s_low, low);
    __syncthreads();
    if (want_col) {  // workgroup-uniform
        // exclusive prefix of the per-tile counts (positions in bytile) and of the per-tile item counts, two tiles per thread
        static_assert(MAX_TILES == 2 * FIN_THREADS, "two tiles per thread");
        const int c0 = 2 * tid < B_tiles ? s_cnt[2 * tid] : 0, c1 = 2 * tid + 1 < B_tiles ? s_cnt[2 * tid + 1] : 0;
        const int g0 = (c0 + 31) / 32, g1 = (c1 + 31) / 32;
        s_scan[tid] = c0 + c1;
        s_scan2[tid] = g0 + g1;
        __syncthreads();
        for (int off = 1; off < FIN_THREADS; off <<= 1) {
            const int u = tid >= off ? s_scan[tid - off] : 0, v = tid >= off ? s_scan2[tid - off] : 0;
            __syncthreads();
            s_scan[tid] += u;
            s_scan2[tid] += v;
            __syncthreads();
        }
        const int pos0 = s_scan[tid] - (c0 + c1), grp0 = s_scan2[tid] - (g0 + g1), n_groups = s_scan2[FIN_THREADS - 1];
        s_pos[2 * tid] = pos0;
        s_pos[2 * tid + 1] = pos0 + c0;
        s_grp[2 * tid] = grp0;
        s_grp[2 * tid + 1] = grp0 + g0;
        if (tid == 0) s_aitem0 = atomicAdd(n_aitems, n_groups);
        __syncthreads();
        for (int t = tid; t < B_tiles; t += FIN_THREADS) {  // the items of tile t: rows [pos, pos + cnt) of bytile in groups of 32
            const int cnt = s_cnt[t], pos = s_pos[t];
            for (int g = 0; g < (cnt + 31) / 32; ++g)
                aitems[s_aitem0 + s_grp[t] + g] = make_int4(p, t | (cnt > 32 ? AITEM_SHARED : 0), pos + 32 * g, min(32, cnt - 32 * g));
        }
        __syncthreads();
        int* bt = bytile + (size_t)p * row_stride;
        for (int i = tid; i < base; i += FIN_THREADS) {
            const int j = cl[i];
            bt[atomicAdd(&s_pos[rc[j].x], 1)] = j;   // (any order inside a tile: every row is resolved on its own)
        }
    }
    if (tid == 0) state[p] = make_int4(base, live ? 1 : 0, s_low, 0);   // .w: match_colpick_kernel's count
}

// rowcand[p][j].x: the tile of row j's minimum -> its column. One wave per item (train tile T of the pair, <= 32 passing rows whose
// minimum lies in T): the 32 x 32 distance block on the MFMA with the operands of match_sweep_kernel (the tile as A, the gathered
// query rows as B, hb as C-init), then every lane scans its 16 train rows in ascending order with a strict '<', the two halves
// of a query row are joined lower-index-first: the lowest train row of the minimum, the reference's tie rule.
//
// colres != nullptr (mode 0): the wave also SETTLES candidate columns from what the row sweep left behind, so that
// match_colverify_kernel streams the query frame for the others only. Candidate (q, t) with v = d2(q, t) survives the mutual check
// of match_finalize2_kernel iff ratio_pass(v, m), m = the smallest d2(q', t) over the OTHER rows q' (ratio_pass is monotone in its
// second argument and false for m <= v at any ratio <= 1: the unique minimum and the column's ratio test in one condition). Every
// other row is bounded from below:
//   * a row that is no candidate, or a candidate whose best column is not t:  d2(q', t) >= L(p)   (state[p].z, match_rows2_kernel);
//   * a candidate whose best column IS t has its minimum in t's tile: it is a row of this item when the tile has one item only,
//     and then d2(q', t) is in this wave's accumulators, exactly (put in LDS: a candidate walks its column over the item's rows).
// So with lo = min(L(p), the exact values of the item's other rows): m >= lo, and ratio_pass(v, lo) implies ratio_pass(v, m) — the
// candidate is kept, and colres[p][j] = {v, lo} (encoded as match_colverify_kernel encodes them) makes match_finalize2_kernel keep it.
// A tile with more than 32 candidates (a second item, whose rows this wave does not hold), a query frame with fewer than two rows
// (the reference needs two neighbours) and every candidate with !ratio_pass(v, lo) stay unresolved: colres[p][j].x = COL_OPEN,
// match_colpick_kernel lists them for match_colverify_kernel, which decides them as before. settle = 0: every candidate unresolved.
constexpr unsigned COL_OPEN = 0xffffffffu;
template <int KS, int METRIC>
__global__ __launch_bounds__(64) void match_argmin_kernel(const FrameDev* __restrict__ frames, const int2* __restrict__ pairs,
                                                          uint2* __restrict__ rowcand, const int* __restrict__ bytile,
                                                          const int4* __restrict__ aitems, const int* __restrict__ n_aitems, int row_stride,
                                                          uint2* __restrict__ colres, const int4* __restrict__ state, double ratio, int settle) {
    __shared__ int sD[32 * 33];   // d2 of the item's block: [query row of the item][train row of the tile], rows padded to 33 words
    constexpr unsigned PAD_V = 2u * PADH;
    const int lane = threadIdx.x & 63, cl = lane & 31, h = lane >> 5;
    const int n = *n_aitems;
    for (int w = blockIdx.x; w < n; w += gridDim.x) {
        const int4 it = aitems[w];
        const int p = it.x, tile = it.y & (AITEM_SHARED - 1);
        const int2 pr = pairs[p];
        const FrameDev A = frames[pr.x], B = frames[pr.y];
        const gfrag_t Afrag = (gfrag_t)A.frag, Bfrag = (gfrag_t)B.frag;
        const gint_t Bhb = (gint_t)B.normb;
        const int j = bytile[(size_t)p * row_stride + it.z + (cl < it.w ? cl : 0)];
        v16i acc;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const v4i q = *(const v4i __attribute__((address_space(1)))*)(Bhb + 32 * tile + 8 * g + 4 * h);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[4 * g + k] = q[k];
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const v4i t = Bfrag[((size_t)tile * KS + ks) * 64 + lane];
            const v4i q = ~Afrag[((size_t)(j >> 5) * KS + ks) * 64 + 32 * h + (j & 31)];
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(t, q, acc, 0, 0, 0);
        }
        int best = 0x7fffffff, bi = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;   // ascending in r
            if (acc[r] < best) best = acc[r], bi = row;
        }
        const int o = __shfl_xor(best, 32), oi = __shfl_xor(bi, 32);
        if (o < best || (o == best && oi < bi)) bi = oi;   // (both lanes of a query row end with the same train row)
        if (h == 0 && cl < it.w) rowcand[(size_t)p * row_stride + j].x = (unsigned)(32 * tile + bi);
        if (colres == nullptr) continue;   // directed lists: no column direction
        const int low = state[p].z;
        const int v = (int)rowcand[(size_t)p * row_stride + j].y;
        // (a pair whose L(p) cannot settle even this item's smallest candidate skips the walk)
        const bool open = settle && !(it.y & AITEM_SHARED) && A.n >= 2 && cl < it.w && ratio_pass<METRIC>(v, low, ratio);
        uint2 res = make_uint2(COL_OPEN, 0u);
        if (__ballot(open)) {   // wave-uniform
            const int pb = tile >= B.meta[0] ? 1 : 0;
            const int add = 2 * ((gint_t)A.norm)[j] + ((j >> 5) >= A.meta[0] ? 1 : 0) + pb - 2;   // d2 = 2 (acc + ca) + pa + pb - 2, as the sweep's epilogue forms it
#pragma unroll
            for (int r = 0; r < 16; ++r) sD[33 * cl + (r & 3) + 8 * (r >> 2) + 4 * h] = 2 * acc[r] + add;
            __syncthreads();
            int lo = low;
            for (int k = 0; k < 16; ++k) {   // each lane of a candidate walks half of the item's rows
                const int q = 16 * h + k;
                if (q < it.w && q != cl) lo = imin(lo, sD[33 * q + bi]);
            }
            lo = imin(lo, __shfl_xor(lo, 32));
            __syncthreads();
            const unsigned second = (unsigned)(lo - pb + 2);
            if (open && ratio_pass<METRIC>(v, lo, ratio) && second < PAD_V) res = make_uint2((unsigned)(v - pb + 2), second);
        }
        if (h == 0 && cl < it.w) colres[(size_t)p * row_stride + j] = res;
    }
}

// Behind match_argmin_kernel: openlist[p][i] = stored row of the i-th candidate of live pair p that is still unresolved (ascending,
// as candlist), state[p].w = their number, one match_colverify_kernel item per 64 of them. totals (optional): {settled, verified}
// candidates of the call, one atomic add per pair each.
__global__ __launch_bounds__(FIN_THREADS) void match_colpick_kernel(const int* __restrict__ candlist, const uint2* __restrict__ colres,
                                                                    int4* __restrict__ state, int row_stride, int* __restrict__ openlist,
                                                                    int2* __restrict__ vitems, int* __restrict__ n_vitems,
                                                                    unsigned long long* __restrict__ totals) {
    __shared__ int s_wave[FIN_THREADS / 64];
    __shared__ int s_item0;
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    const int4 st = state[p];
    if (!st.y) return;   // workgroup-uniform: the pair cannot reach the thresholds
    const int* cl = candlist + (size_t)p * row_stride;
    const uint2* cr = colres + (size_t)p * row_stride;
    int* ol = openlist + (size_t)p * row_stride;
    int base = 0;
    for (int i0 = 0; i0 < st.x; i0 += FIN_THREADS) {
        const int i = i0 + tid;
        const int j = i < st.x ? cl[i] : 0;
        const bool open = i < st.x && cr[j].x == COL_OPEN;
        int total;
        const int rank = block_rank(open, tid, s_wave, total);
        if (open) ol[base + rank] = j;
        base += total;
    }
    const int groups = (base + VER_CANDS - 1) / VER_CANDS;
    if (tid == 0) {
        state[p].w = base;
        s_item0 = groups ? atomicAdd(n_vitems, groups) : 0;
        if (totals) {
            atomicAdd(&totals[0], (unsigned long long)(st.x - base));
            atomicAdd(&totals[1], (unsigned long long)base);
        }
    }
    __syncthreads();
    for (int g = tid; g < groups; g += FIN_THREADS) vitems[s_item0 + g] = make_int2(p, g);
}

// colres[p][j] = {v1, v2}: the two smallest 2H + pa over ALL stored rows of frame A against column rowcand[p][j].x of
// frame B (d2 = v + pb - 2), for the candidates of live pairs. Persistent workgroups over the item list.
//
// The MFMA of the sweep with its operands swapped: the 64 candidate columns of an item are the B operand (gathered once,
// two 32-column groups held in registers: a candidate is a LANE), the query frame's tiles stream as the A operand straight
// from L2, each fetched fragment feeding both groups' chains. Because a lane's 16 accumulators are 16 rows against ITS
// column, the column's constant hb is added once at the very end and the top-2 runs on the raw accumulators, three at a
// time: 27 VALU operations per 16 distances (the sweep needs 48) under 8 MFMAs — the kernel is bound by the matrix pipe,
// which the sweep (bound by the VALU port) leaves idle more than half of the time. Rows of the two parity classes are kept
// apart (a tile has one parity) and joined when 2H + pa is formed. candlist is the pair's list of stored rows, state[p] word
// count_word its length: every passing row (match_rows2_kernel), or the ones match_argmin_kernel left unresolved (match_colpick_kernel).
// ROWS = true: the same pass with the frames' roles swapped — the candidates are stored ROWS of the query frame (candlist holds them
// directly), the train frame's tiles stream — for the rows the bound form of the sweep (match_sweep_kernel<KS, true>) could not
// finish: their exact {v1 = 2H + pb minimum, first tile holding it, v2} go to rowres[p][j], what match_rows2_kernel reads. A wave
// meets its tiles in ascending order and takes a tile only on a STRICT improvement; equal minima of two waves / the two lanes of
// a candidate keep the lower tile: the first tile of the minimum, as the exact sweep records it.
template <int KS, bool ROWS = false>
__global__ __launch_bounds__(WG_THREADS) void match_colverify_kernel(
    const FrameDev* __restrict__ frames, const int2* __restrict__ pairs, const uint2* __restrict__ rowcand,
    const int* __restrict__ candlist, const int4* __restrict__ state, const int2* __restrict__ items,
    const int* __restrict__ n_items, int row_stride, int count_word, uint2* __restrict__ colres, uint4* __restrict__ rowres_out = nullptr) {
    __shared__ int4 sM[WAVES][VER_GROUPS][32];  // per wave, group, column: {m1 even, m2 even, m1 odd, m2 odd}
    __shared__ int2 sT[WAVES][VER_GROUPS][32];  // ROWS: {tile of m1 even, tile of m1 odd}
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cl = lane & 31, h = lane >> 5;
    const int n = *n_items;
    constexpr int BIG = 0x7fffffff;
    for (int w = blockIdx.x; w < n; w += gridDim.x) {
        const int2 it = items[w];
        const int p = it.x;
        const int2 pr = pairs[p];
        const FrameDev A = frames[ROWS ? pr.y : pr.x], B = frames[ROWS ? pr.x : pr.y];   // A: the frame whose tiles stream, B: the candidates'
        const int A_even = ((gint_t)A.meta)[0], A_tiles = ((gint_t)A.meta)[1];
        const int ncand = ((const int*)&state[p])[count_word];   // length of the pair's list: .x of candlist, .w of match_colpick_kernel's
        const gfrag_t Afrag = (gfrag_t)A.frag, Bfrag = (gfrag_t)B.frag;
        const gint_t Aca = (gint_t)A.norm;
        const int* cand = candlist + (size_t)p * row_stride;
        const uint2* rc = rowcand + (size_t)p * row_stride;
        v4i b[VER_GROUPS][KS];
        int jg[VER_GROUPS];  // stored row of this lane's candidate per group (-1: past the list)
#pragma unroll
        for (int g = 0; g < VER_GROUPS; ++g) {
            const int i = VER_CANDS * it.y + 32 * g + cl;
            const int j = cand[i < ncand ? i : VER_CANDS * it.y];  // (an item has at least one candidate)
            jg[g] = i < ncand ? j : -1;
            const unsigned col = ROWS ? (unsigned)j : rc[j].x;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) b[g][ks] = Bfrag[((size_t)(col >> 5) * KS + ks) * 64 + 32 * h + (col & 31)];
        }
        int m1[VER_GROUPS][2], m2[VER_GROUPS][2];  // [group][row parity]
        int mt[VER_GROUPS][2];                      // ROWS: the tile of m1
#pragma unroll
        for (int g = 0; g < VER_GROUPS; ++g) m1[g][0] = m1[g][1] = m2[g][0] = m2[g][1] = BIG, mt[g][0] = mt[g][1] = 0;
        // this wave's tiles: wave, wave + 4, ...; the next tile's fragments and C-init are in flight under the current chains
        v4i a_nxt[KS];
        v4i c_nxt[4];
        auto fetch = [&](int t) {
            const int tc = min(t, A_tiles - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) a_nxt[ks] = Afrag[((size_t)tc * KS + ks) * 64 + lane];
#pragma unroll
            for (int q = 0; q < 4; ++q) c_nxt[q] = *(const v4i __attribute__((address_space(1)))*)(Aca + 32 * tc + 8 * q + 4 * h);  // rows 8q + 4h .. + 3: registers 4q .. 4q + 3
        };
        fetch(wave);
        for (int t = wave; t < A_tiles; t += WAVES) {
            v4i a[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) a[ks] = ~a_nxt[ks];
            v16i c0;
#pragma unroll
            for (int r = 0; r < 16; ++r) c0[r] = c_nxt[r >> 2][r & 3];
            fetch(t + WAVES);
            v16i acc[VER_GROUPS];
#pragma unroll
            for (int g = 0; g < VER_GROUPS; ++g) {
                acc[g] = c0;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) acc[g] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[ks], b[g][ks], acc[g], 0, 0, 0);
            }
            const bool odd = t >= A_even;  // wave-uniform
#pragma unroll
            for (int g = 0; g < VER_GROUPS; ++g) {
                int x1 = odd ? m1[g][1] : m1[g][0], x2 = odd ? m2[g][1] : m2[g][0];
#pragma unroll
                for (int k = 0; k < 15; k += 3) {  // five triples: {min3, med3} + a sorted-pair merge
                    const int s1 = imin(imin(acc[g][k], acc[g][k + 1]), acc[g][k + 2]);
                    const int s2 = imed3(acc[g][k], acc[g][k + 1], acc[g][k + 2]);
                    top2_merge(x1, x2, s1, s2);
                }
                x2 = imed3(x1, x2, acc[g][15]);
                x1 = imin(x1, acc[g][15]);
                if constexpr (ROWS) {
                    const int before = odd ? m1[g][1] : m1[g][0];
                    if (odd) mt[g][1] = x1 < before ? t : mt[g][1];
                    else mt[g][0] = x1 < before ? t : mt[g][0];
                }
                if (odd) m1[g][1] = x1, m2[g][1] = x2;
                else m1[g][0] = x1, m2[g][0] = x2;
            }
        }
#pragma unroll
        for (int g = 0; g < VER_GROUPS; ++g) {  // lanes l and l + 32 hold the same column, different rows
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int o1 = __shfl_xor(m1[g][e], 32), o2 = __shfl_xor(m2[g][e], 32);
                if constexpr (ROWS) {
                    const int ot = __shfl_xor(mt[g][e], 32);
                    mt[g][e] = o1 < m1[g][e] ? ot : (o1 == m1[g][e] ? imin(ot, mt[g][e]) : mt[g][e]);
                }
                top2_merge(m1[g][e], m2[g][e], o1, o2);
            }
            if (h == 0) sM[wave][g][cl] = make_int4(m1[g][0], m2[g][0], m1[g][1], m2[g][1]);
            if (ROWS && h == 0) sT[wave][g][cl] = make_int2(mt[g][0], mt[g][1]);
        }
        __syncthreads();
        if (tid < 32 * VER_GROUPS) {
            const int g = tid >> 5, c = tid & 31;
            int4 m = sM[0][g][c];
            int2 mtile = ROWS ? sT[0][g][c] : make_int2(0, 0);
#pragma unroll
            for (int k = 1; k < WAVES; ++k) {
                const int4 e = sM[k][g][c];
                if constexpr (ROWS) {
                    const int2 et = sT[k][g][c];
                    mtile.x = e.x < m.x ? et.x : (e.x == m.x ? imin(et.x, mtile.x) : mtile.x);
                    mtile.y = e.z < m.z ? et.y : (e.z == m.z ? imin(et.y, mtile.y) : mtile.y);
                }
                top2_merge(m.x, m.y, e.x, e.y);
                top2_merge(m.z, m.w, e.z, e.w);
            }
            // H = acc + hb; v = 2 H + pa. A class without rows stays at BIG (never the minimum of a frame with rows)
            const int i = VER_CANDS * it.y + tid;
            if (i < ncand) {
                const int j = cand[i];
                const long long hb2 = 2ll * ((gint_t)B.normb)[ROWS ? (unsigned)j : rc[j].x];
                auto val = [&](int m, int pa) { return m == BIG ? 0xffffffffull : (unsigned long long)(2ll * m + hb2 + pa); };
                unsigned long long e1 = val(m.x, 0), e2 = val(m.y, 0), o1 = val(m.z, 1), o2 = val(m.w, 1);
                const unsigned long long v1 = e1 < o1 ? e1 : o1;
                const unsigned long long hi = e1 < o1 ? o1 : e1, lo2 = e2 < o2 ? e2 : o2;
                const unsigned long long v2 = hi < lo2 ? hi : lo2;
                if constexpr (ROWS) rowres_out[(size_t)p * row_stride + j] = make_uint4((unsigned)v1, (unsigned)(e1 < o1 ? mtile.x : mtile.y), (unsigned)v2, 0u);
                else colres[(size_t)p * row_stride + j] = make_uint2((unsigned)v1, (unsigned)v2);
            }
        }
        __syncthreads();
        (void)jg;
    }
}

// out_matches[p][k] = {q, t} sorted by q; counts[p] (mode 0: |mutual| if it exceeds min_mutual, else 0; mode 1: |m12|)
template <int METRIC>
__global__ __launch_bounds__(FIN_THREADS) void match_finalize2_kernel(
    const FrameDev* __restrict__ frames, const int2* __restrict__ pairs, const uint2* __restrict__ rowcand,
    const uint2* __restrict__ colres, const int4* __restrict__ state, int row_stride, double ratio, int min_mutual, int mode,
    uint2* __restrict__ out_matches, int* __restrict__ counts) {
    extern __shared__ int smem[];
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    const int4 st = state[p];
    if (st.x == 0 || (mode == 0 && !st.y)) {  // workgroup-uniform: no passing row, or a pair that cannot reach the thresholds
        if (tid == 0) counts[p] = 0;
        return;
    }
    const int2 pr = pairs[p];
    const FrameDev A = frames[pr.x], B = frames[pr.y];
    const int A_tiles = A.meta[1], B_even = B.meta[0];
    constexpr unsigned PAD_V = 2u * PADH;
    int* keepcol = smem;  // [row_stride] by stored row: stored column of the kept match or -1
    const uint2* rc = rowcand + (size_t)p * row_stride;
    const uint2* cr = colres + (size_t)p * row_stride;
    for (int j = tid; j < 32 * A_tiles; j += FIN_THREADS) {
        const uint2 c = rc[j];
        int keep = -1;
        if (c.x != 0xffffffffu) {
            if (mode == 1) {
                keep = (int)c.x;
            } else {
                // main.cpp:133-140: q is kept iff t's own best match is q, i.e. iff column t passes the ratio test (a unique
                // minimum for any ratio <= 1) and its minimum is d2(q, t)
                const uint2 v = cr[j];
                const unsigned pb = (c.x >> 5) >= (unsigned)B_even ? 1u : 0u;
                const int d1 = (int)(v.x + pb) - 2;
                if (d1 == (int)c.y && v.y < PAD_V && ratio_pass<METRIC>(d1, (int)(v.y + pb) - 2, ratio)) keep = (int)c.x;
            }
        }
        keepcol[j] = keep;
    }
    __syncthreads();
    // (by stored position inside, the caller's numbering out)
    const int base = compact_kept_rows(
        A.n, tid, out_matches + (size_t)p * row_stride, [&](int q) { return keepcol[A.pos[q]]; }, [&](int t) { return B.orig[t]; });
    if (tid == 0) counts[p] = mode == 1 ? base : (base > min_mutual ? base : 0);  // main.cpp:142
}

// offsets[first + i] = running total; single workgroup, sequential over chunks (npairs is small)
__global__ __launch_bounds__(1024) void scan_counts_kernel(const int* __restrict__ counts, int n,
                                                           long long* __restrict__ offsets,
                                                           long long* __restrict__ total,
                                                           int first, int is_last) {
    __shared__ long long s[1024];
    __shared__ long long carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = first == 0 ? 0 : *total;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 1024) {
        int i = i0 + tid;
        long long v = i < n ? counts[i] : 0;
        s[tid] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            long long u = tid >= off ? s[tid - off] : 0;
            __syncthreads();
            s[tid] += u;
            __syncthreads();
        }
        if (i < n) offsets[first + i] = carry + s[tid] - v;
        __syncthreads();
        if (tid == 0) carry += s[1023];
        __syncthreads();
    }
    if (tid == 0) {
        *total = carry;
        if (is_last) offsets[first + n] = carry;
    }
}

__global__ void compact_edges_kernel(const uint2* __restrict__ matches, const int* __restrict__ counts,
                                     const long long* __restrict__ offsets, int row_stride,
                                     uint2* __restrict__ edges, long long edge_cap) {
    const int p = blockIdx.x;
    const int n = counts[p];
    const long long off = offsets[p];
    for (int k = threadIdx.x; k < n; k += blockDim.x)
        if (off + k < edge_cap) edges[off + k] = matches[(size_t)p * row_stride + k];
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------

// (up to 128-D a multiple of 16; above, any dimension: the upload kernels pad a row with centred zeros to the 256 of the class)
static int ks_for_dim(int dim) {
    if (dim <= 0 || dim > 256) return 0;
    if (dim > 128) return 8;
    if (dim % 16) return 0;
    return dim <= 64 ? 2 : 4;
}

// f(std::integral_constant<int, KS>) for the KS of the resident frames (ks_for_dim: 2, 4 or 8)
template <class F>
static void with_ks(int ks, F&& f) {
    if (ks == 2) f(std::integral_constant<int, 2>{});
    else if (ks == 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 8>{});
}

// FRAME_INT8: the caller's integer rows; FRAME_BITS: rows of 0 / 255 expanded from packed bits, which get 8 words per row
// behind the per-row arrays for their packed copy (FrameHost::bits, filled by the caller)
static int upload_frame(eacham_ctx* ctx, int frame_id, const float* src_dev, int n, int dim, FrameKind kind = FRAME_INT8) {
    const int ks = ks_for_dim(dim);
    FrameHost* slot = nullptr;
    if (int rc = open_frame_slot(ctx, frame_id, kind, n, MAX_ROWS, ks, 0, &slot)) return rc;
    FrameHost& f = *slot;
    // each parity class is padded to whole tiles (at most one extra tile), the total to whole wave-blocks
    const int group_rows = 32 * GROUP_TILES;
    const int ntiles = n > 0 ? ((n + 31) / 32 + 1 + GROUP_TILES - 1) / GROUP_TILES * GROUP_TILES : 0;
    const int npad = ntiles * 32;
    {
        // norm (ca) | normb (hb) | orig | pos | s2 | s1 | meta[8] (partition_kernel: two words; above 128-D finish_screen_kernel: the
        // third; the rest unused, 32-byte alignment); binary frames only: | the packed rows, 8 words each
        const size_t ints = (size_t)6 * npad + 8 + (kind == FRAME_BITS ? (size_t)8 * n : 0);
        EACHAM_HIP_TRY(ctx, hipMalloc((void**)&f.norm, ints * sizeof(int)));
        EACHAM_HIP_TRY(ctx, hipMemsetAsync(f.norm, 0, ints * sizeof(int), ctx->stream));
        f.normb = f.norm + npad;
        f.orig = f.norm + 2 * (size_t)npad;
        f.pos = f.norm + 3 * (size_t)npad;
        int* s2 = f.norm + 4 * (size_t)npad;
        int* s1 = f.norm + 5 * (size_t)npad;
        f.meta = f.norm + 6 * (size_t)npad;
        if (kind == FRAME_BITS) f.bits = (unsigned*)(f.norm + 6 * (size_t)npad + 8);   // 32-byte aligned: npad is a multiple of 32
        if (npad > 0) {
            // above 128-D the FP6 image of the screen sweep follows the int8 fragments: image | |M|^2 | s_r | {E} (quantize_screen_kernel)
            const size_t frag_bytes = (size_t)ntiles * ks * 64 * sizeof(int4);
            const size_t screen_bytes = ks == 8 ? (size_t)ntiles * SCREEN_TILE_BYTES + (size_t)npad * 8 + 16 : 0;
            EACHAM_HIP_TRY(ctx, hipMalloc((void**)&f.frag, frag_bytes + screen_bytes));
            const long long sums = (long long)n * ((dim + 15) / 16);
            rowsum_kernel<<<(unsigned)((sums + 255) / 256), 256, 0, ctx->stream>>>(src_dev, n, dim, s2, s1, &ctx->flag_dev->not_integer);
            partition_kernel<<<1, 1024, 0, ctx->stream>>>(s2, s1, n, npad, group_rows, f.norm, f.normb, f.orig, f.pos, f.meta);
            const long long work = (long long)npad * ks * 2;
            quantize_kernel<<<(unsigned)((work + 255) / 256), 256, 0, ctx->stream>>>(src_dev, dim, ks, npad, f.orig, (v4i*)f.frag);
            if (screen_bytes) {
                char* img = (char*)f.frag + frag_bytes;
                int* msq = (int*)(img + (size_t)ntiles * SCREEN_TILE_BYTES);   // becomes hm, floats
                int* sr = msq + npad;
                EACHAM_HIP_TRY(ctx, hipMemsetAsync(msq, 0, (size_t)npad * 8 + 16, ctx->stream));
                quantize_screen_kernel<<<(npad * 2 * SCREEN_KS + 255) / 256, 256, 0, ctx->stream>>>(src_dev, dim, npad, f.orig, img, msq, sr);
                finish_screen_kernel<<<(npad + 255) / 256, 256, 0, ctx->stream>>>(npad, f.orig, msq, sr, sr + npad, f.meta);
                f.screen = (int4*)img;
            }
            EACHAM_HIP_TRY(ctx, hipGetLastError());
        }
    }
    commit_frame(ctx, f, kind, n, dim, ks, ntiles, 0);
    return EACHAM_OK;
}

int check_integer_flag(eacham_ctx* ctx) {
    if (ctx->kind_common == FRAME_F32) return EACHAM_OK;  // fp32 frames take any value
    int flag = 0;
    EACHAM_HIP_TRY(ctx, hipMemcpyAsync(&flag, &ctx->flag_dev->not_integer, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (flag) {
        EACHAM_HIP_TRY(ctx, hipMemsetAsync(&ctx->flag_dev->not_integer, 0, sizeof(int), ctx->stream));
        return ctx->fail(EACHAM_ERR_NOT_INTEGER,
                         "descriptors must be integer-valued in [0,255] for the exact int8 path");
    }
    return EACHAM_OK;
}

// {settled, verified}: the candidate columns of the last matching call that match_argmin_kernel settled / that went to match_colverify_kernel
static unsigned long long* colprune_totals(eacham_ctx* ctx) { return ctx->flag_dev->colprune; }
// {real query rows, rows left open, items}: what the screen sweeps of the last matching call met / handed to the exact pass / in how many items
static unsigned long long* screen_tally(eacham_ctx* ctx) { return ctx->flag_dev->screen; }
// every resident frame with rows carries the FP6 image (all frames share one dim class, so this is ks_common == 8)
static bool frames_have_screen(const eacham_ctx* ctx) {
    if (ctx->kind_common == FRAME_F32 || ctx->ks_common != SCREEN_EXACT_KS) return false;
    for (const auto& f : ctx->frames)
        if (f.n > 0 && !f.screen) return false;
    return true;
}

// The plan of a job (match_plan.hpp) for the resident frames
static MatchPlan make_plan(const eacham_ctx* ctx, int npairs, bool full_cols) {
    int max_tiles = std::max(4, GROUP_TILES);
    for (const auto& f : ctx->frames)
        if (f.n >= 0) max_tiles = std::max(max_tiles, f.tiles_used);
    // (match_no_overlap: diagnostic switch, read once at eacham_ctx_create)
    return make_plan(MatchPlanIn{max_tiles, npairs, (size_t)ctx->match_budget_mb << 20, full_cols, ctx->match_no_overlap});
}

// A matching call of the int8 kinds as its launches see it, and one launch: pairs [first, first + nb) of the call, its launch b, in
// workspace slot s. The four sequences a launch consists of follow; run_match_metric orders them on the two streams.
struct MatchCall {
    eacham_ctx* ctx;
    MatchPlan pl;
    CallArrays call;
    hipStream_t st1, st2;
    double ratio;
    int min_dir, min_mutual, mode;
    size_t fin_smem;
    bool screen_sweep, bound_sweep;
};
struct MatchLaunch {
    Slot s;
    const int2* pb;
    int nb, first, b;
    int* cnt;
    bool sweep_beside;   // the tail runs on the second stream beside the next launch's sweep
};

// The row sweep, on st1. The full-column form sweeps with match_tile_kernel, the lean form with match_sweep_kernel: up to 128-D its
// BOUND form (the sweep is bound by its epilogue's VALU work there) + an exact pass over the rows it could not finish; above, where
// the matrix pipe binds, the rows are screened on the FP6 matrix cores (match_screen_kernel), the same exact pass behind
// a workgroup of match_screen_kernel owns 512 query rows where the plan counts workgroups of 256
static int screen_wgs_per_pair(const MatchPlan& pl) { return (pl.wgs_per_pair + 1) / 2; }
template <int METRIC>
static void launch_sweep(const MatchCall& c, const MatchLaunch& l) {
    const MatchPlan& pl = c.pl;
    const FrameDev* frames = c.ctx->frame_table_dev;
    with_ks(c.ctx->ks_common, [&](auto ks) {
        constexpr int KS = decltype(ks)::value;
        if (c.screen_sweep)
            match_screen_kernel<METRIC><<<l.nb * screen_wgs_per_pair(pl), WG_THREADS, 0, c.st1>>>(
                frames, l.pb, screen_wgs_per_pair(pl), l.s.rowres, pl.row_stride, c.ratio, l.s.openmask, pl.mask_stride,
                OpenList{c.call.seghead + l.first, c.call.segcount + l.first, l.s.rowcand, l.s.items, c.call.launch_items + l.b});
        else if (pl.full_cols)
            match_tile_kernel<KS><<<l.nb * pl.wgs_per_pair * pl.col_chunks, WG_THREADS, 0, c.st1>>>(
                frames, l.pb, pl.wgs_per_pair, pl.col_chunks, l.s.rowres, l.s.colpart, pl.wb_stride, pl.row_stride);
        else if (c.bound_sweep)
            match_sweep_kernel<KS, true><<<l.nb * pl.wgs_per_pair, WG_THREADS, 0, c.st1>>>(frames, l.pb, pl.wgs_per_pair, l.s.rowres, pl.row_stride);
        else
            match_sweep_kernel<KS, false><<<l.nb * pl.wgs_per_pair, WG_THREADS, 0, c.st1>>>(frames, l.pb, pl.wgs_per_pair, l.s.rowres, pl.row_stride);
    });
}

// The exact pass over the rows the screen left open, on the sweep's stream directly behind it and ahead of ev_tile (beside the next
// sweep it got in only as sweep workgroups retired and held the slot the sweep after next waits for: DESIGN.md 3.3,
// profiles/screen_exact_behind_sweep.txt): the exact sweep itself with gathered query rows, over the candidate list the sweep's tail
// wrote (the comment above match_openprep_kernel). The list lives in the slot's rowcand area ({pair, row} is a uint2, one per stored
// row per pair at the most), which match_rows2_kernel first writes on the second stream behind ev_tile; {head, k} items: at most
// row_stride / 256 + 1 per pair, the items area holds row_stride / 32. The slot-free wait covers rowcand and items of this slot.
static void launch_open_rows_exact(const MatchCall& c, const MatchLaunch& l) {
    // a workgroup per item, the grid an upper bound of the dense list: workgroups past it leave at once
    const int ggrid = l.nb * ((c.pl.row_stride + GATHER_WIDTH - 1) / GATHER_WIDTH + 1);
    match_sweep_kernel<SCREEN_EXACT_KS, false, true><<<ggrid, WG_THREADS, 0, c.st1>>>(
        c.ctx->frame_table_dev, l.pb, 0, l.s.rowres, c.pl.row_stride,
        GatherList<true>{l.s.rowcand, c.call.segcount + l.first, l.s.items, c.call.launch_items + l.b});
}

// The tail of the full-column form, on st2: every column's top-2 came out of the sweep
template <int METRIC>
static void launch_full_cols_tail(const MatchCall& c, const MatchLaunch& l, int4* stats) {
    match_finalize_kernel<METRIC><<<l.nb, FIN_THREADS, c.fin_smem, c.st2>>>(c.ctx->frame_table_dev, l.pb, l.s.rowres, l.s.colpart, c.pl.col_chunks, c.pl.wb_stride,
                                                                     c.pl.row_stride, c.ratio, c.min_dir, c.min_mutual, c.mode, l.s.matches, l.cnt, stats);
}

// The tail of the lean form, on st2: (the bound form's open rows) -> passing rows and their candidate columns -> arg-min over the
// candidates' tiles -> the columns it could not settle -> matches
template <int METRIC>
static int launch_lean_tail(const MatchCall& c, const MatchLaunch& l) {
    eacham_ctx* ctx = c.ctx;
    const MatchPlan& pl = c.pl;
    const Slot& s = l.s;
    const FrameDev* frames = ctx->frame_table_dev;
    hipStream_t st2 = c.st2;
    const int nb = l.nb, mode = c.mode;
    int *n_items = &s.counters->n_items, *n_pre = &s.counters->n_pre, *n_aitems = &s.counters->n_aitems;
    // persistent workgroups over an item list (its length is only known on the device): one round of the chip
    const int vgrid = std::min(std::max(nb * pl.wgs_per_pair, 1), 512);
    // one wave per item, persistent over the list: a round of the chip, half a round beside a screen sweep (argmin_grid, match_plan.hpp;
    // the bound and exact forms keep the full round beside their sweeps: their lines are no faster with half, profiles/tail_placement.txt)
    const int agrid = argmin_grid(nb, pl.wgs_per_pair, ctx->cus, c.screen_sweep && l.sweep_beside);
    EACHAM_HIP_TRY(ctx, hipMemsetAsync(s.counters, 0, sizeof(SlotCounters), st2));
    if (c.screen_sweep)   // the launch's open rows and items into the debug tally: off the sweeps' chain
        match_opentally_kernel<<<(nb + TALLY_THREADS - 1) / TALLY_THREADS, TALLY_THREADS, 0, st2>>>(c.call.seghead + l.first, c.call.segcount + l.first, nb,
                                                                                               c.call.launch_items + l.b, screen_tally(ctx));
    with_ks(ctx->ks_common, [&](auto ks) {
        constexpr int KS = decltype(ks)::value;
        if (c.bound_sweep) {   // the rows the bound form left open: exact {v1, tile, v2} into rowres, before the rows kernel reads it (the screen form's ran behind its sweep)
            match_rowpick_kernel<METRIC><<<nb, FIN_THREADS, 0, st2>>>(frames, l.pb, s.rowres, pl.row_stride, c.ratio, s.candlist, s.state, s.items, n_pre);
            match_colverify_kernel<KS, true><<<vgrid, WG_THREADS, 0, st2>>>(frames, l.pb, nullptr, s.candlist, s.state, s.items, n_pre, pl.row_stride, 0, nullptr, s.rowres);
        }
        // (mutual matching behind the screen sweep: a pair its open count already fails leaves before it reads a row; L2 only)
        if (METRIC == METRIC_L2 && c.screen_sweep && mode == 0)
            match_rows2_kernel<METRIC_L2, true><<<nb, FIN_THREADS, 0, st2>>>(frames, l.pb, s.rowres, pl.row_stride, c.ratio, c.min_dir, c.min_mutual, mode, s.rowcand,
                                                                      s.candlist, s.bytile, s.state, s.aitems, n_aitems, s.openmask, pl.mask_stride);
        else
            match_rows2_kernel<METRIC><<<nb, FIN_THREADS, 0, st2>>>(frames, l.pb, s.rowres, pl.row_stride, c.ratio, c.min_dir, c.min_mutual, mode, s.rowcand,
                                                            s.candlist, s.bytile, s.state, s.aitems, n_aitems);
        match_argmin_kernel<KS, METRIC><<<agrid, 64, 0, st2>>>(frames, l.pb, s.rowcand, s.bytile, s.aitems, n_aitems, pl.row_stride, mode == 0 ? s.colres : nullptr,
                                                       s.state, c.ratio, ctx->match_colprune ? 1 : 0);
        if (mode == 0) {   // the candidates the arg-min pass could not settle (state[p].w of them): listed, then the column pass
            match_colpick_kernel<<<nb, FIN_THREADS, 0, st2>>>(s.candlist, s.colres, s.state, pl.row_stride, s.openlist, s.items, n_items, colprune_totals(ctx));
            match_colverify_kernel<KS><<<vgrid, WG_THREADS, 0, st2>>>(frames, l.pb, s.rowcand, s.openlist, s.state, s.items, n_items, pl.row_stride, 3, s.colres);
        }
    });
    match_finalize2_kernel<METRIC><<<nb, FIN_THREADS, c.fin_smem, st2>>>(frames, l.pb, s.rowcand, s.colres, s.state, pl.row_stride, c.ratio, c.min_mutual, mode,
                                                                  s.matches, l.cnt);
    return EACHAM_OK;
}

// Core driver, CSR over the pairs out. mode 0 = mutual + thresholds, mode 1 = directed lists.
template <int METRIC>
static int run_match_metric(eacham_ctx* ctx, const int2* pairs_dev, int npairs, double ratio, int min_dir,
                            int min_mutual, int mode, int* counts_dev, long long* offsets_dev,
                            uint2* edges_dev, long long edge_cap, long long* total_dev, int4* stats_dev, const int2** pairs_used) {
    int rc = sync_frame_table(ctx);
    if (rc) return rc;
    if (npairs <= 0) return EACHAM_OK;
    if (mode == 0 && !(ratio <= 1.0))  // the mutual check relies on a passing column having a unique minimum
        return ctx->fail(EACHAM_ERR_INVALID, "ratio %g: mutual matching supports 0 < ratio <= 1 (the reference uses 0.8)", ratio);
    rc = sanitize_pairs(ctx, pairs_dev, npairs, &pairs_dev);  // a bad frame id in a device-side list must not reach the kernels
    if (rc) return rc;
    if (pairs_used) *pairs_used = pairs_dev;   // the list the kernels ran on (what the Hamming distance kernel indexes the frames with)
    const bool binary = ctx->kind_common == FRAME_BITS || ctx->kind_common == FRAME_BITS_WIDE;
    if (METRIC != (binary ? METRIC_HAMMING : METRIC_L2))
        return ctx->fail(EACHAM_ERR_UNSUPPORTED, binary ? "the resident frames are binary: use the _hamming entry points"
                                                        : "Hamming matching needs binary frames (eacham_upload_descriptors_bits)");
    if (ctx->kind_common == FRAME_BITS_WIDE)   // (run_match hands wide frames to run_match_ham_wide before they get here)
        return ctx->fail(EACHAM_ERR_UNSUPPORTED, "the resident frames are wide binary frames: the int8 kernels do not take them");
    if (ctx->kind_common == FRAME_F32)
        return run_match_f32(ctx, pairs_dev, npairs, ratio, min_dir, min_mutual, mode, counts_dev, offsets_dev, edges_dev,
                             edge_cap, total_dev, stats_dev);
    // Which form of the column direction: the reference's thresholds (30 / 30, main.cpp:111,142) make the direction counts
    // redundant once |mutual| > min_mutual >= min_dir - 1, so only the columns that are some passing row's best are ever
    // looked at (candidate-only pass); directed lists need no column at all. Callers that ask for the per-pair statistics
    // (|m12|, |m21|) or use other thresholds get every column's top-2 from the sweep itself, as before.
    const bool full_cols = mode == 0 && (stats_dev != nullptr || (long long)min_mutual < (long long)min_dir - 1);
    const MatchPlan pl = make_plan(ctx, npairs, full_cols);
    // The row sweep of the lean form. EACHAM_MATCH_SWEEP_FORM forces the exact (1) or the bound form (2) at every dimension; screen (3)
    // and the default (0) run the screen sweep where the frames have the FP6 image (above 128-D) and the bound form up to 128-D.
    const int form = ctx->match_sweep_form;
    const bool screen_sweep = !full_cols && (form == 0 || form == 3) && frames_have_screen(ctx);
    const bool bound_sweep = !full_cols && !screen_sweep && (form == 2 || ((form == 0 || form == 3) && ctx->ks_common <= 4));
    // the arrays of the call behind the slots (under the screen sweep only), one item counter per launch: the launches are counted
    // and the cut as match_openprep_kernel sees it is checked against them
    const LaunchCut cut = launch_cut(pl);
    int launches = 0;
    for (int first = 0; screen_sweep && first < npairs; ++launches) {
        int start = 0;
        if (launch_of(cut, first, &start) != launches || start != first)
            return ctx->fail(EACHAM_ERR_INVALID, "internal: launch %d at pair %d is not where the cut has it", launches, first);
        first += next_batch(pl, launches, first, npairs);
    }
    rc = ensure_workspace(ctx, pl.total + (screen_sweep ? call_bytes(npairs, launches) : 0));
    if (rc) return rc;
    const size_t fin_smem = (size_t)(full_cols ? 2 : 1) * pl.row_stride * sizeof(int);
    if (fin_smem > 48 * 1024) {
        if (full_cols) EACHAM_HIP_TRY(ctx, hipFuncSetAttribute((const void*)match_finalize_kernel<METRIC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fin_smem));
        else EACHAM_HIP_TRY(ctx, hipFuncSetAttribute((const void*)match_finalize2_kernel<METRIC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fin_smem));
    }
    // Two streams: the sweeps (and the screen form's exact pass) run back to back on the context stream; the tail, scan and
    // compaction of a launch run on stream2 beside the next launch's sweep, each launch in its own workspace slot.
    hipStream_t st1 = ctx->stream, st2 = pl.slots == 2 || npairs <= pl.batch ? ctx->stream2 : ctx->stream;
    const MatchCall c{ctx, pl, call_arrays(ctx->ws, pl, npairs, launches), st1, st2, ratio, min_dir, min_mutual, mode, fin_smem, screen_sweep, bound_sweep};
    EACHAM_HIP_TRY(ctx, hipEventRecord(ctx->ev_join, st1));        // inputs queued on the context stream
    EACHAM_HIP_TRY(ctx, hipStreamWaitEvent(st2, ctx->ev_join, 0));
    EACHAM_HIP_TRY(ctx, hipMemsetAsync(colprune_totals(ctx), 0, 2 * sizeof(unsigned long long), st2));
    EACHAM_HIP_TRY(ctx, hipMemsetAsync(screen_tally(ctx), 0, 3 * sizeof(unsigned long long), screen_sweep ? st1 : st2));   // on the stream that adds to it first
    if (screen_sweep)   // segment heads, zeroed counters and the rows of the tally for every launch of the call: nothing of the list sits between two sweeps
        match_openprep_kernel<<<(npairs + PREP_THREADS - 1) / PREP_THREADS, PREP_THREADS, 0, st1>>>(ctx->frame_table_dev, pairs_dev, npairs, cut, c.call.seghead,
                                                                                                    c.call.segcount, c.call.launch_items, screen_tally(ctx));
    // The work behind a batch's sweep (rows / candidate columns / finalize / compaction) runs on the second stream beside the NEXT
    // batch's sweep — except the last batch's, which nothing hides: the job is cut into equal full batches and a short last one
    // (an eighth of a full one at the most; make_plan), so the exposed lists, exact pass and tail are those of ~1 200 pairs instead
    // of ~10 000. S200 under the 1 GiB budget: 9 344 + 9 344 + 1 212 pairs.
    int b = 0;
    for (int first = 0, nb = 0; first < npairs; first += nb, ++b) {
        nb = next_batch(pl, b, first, npairs);
        const int slot = b % pl.slots;
        const MatchLaunch l{pl.slot(ctx->ws, slot), pairs_dev + first, nb, first, b, counts_dev + first, st2 != st1 && first + nb < npairs};
        if (b >= pl.slots) EACHAM_HIP_TRY(ctx, hipStreamWaitEvent(st1, ctx->ev_fin[slot], 0));  // slot free again
        {
            ProfileScope ps(ctx, EACHAM_KERNEL_MATCH_TILE, st1);
            launch_sweep<METRIC>(c, l);
        }
        if (screen_sweep) {
            ProfileScope ps(ctx, EACHAM_KERNEL_MATCH_FINALIZE, st1);
            launch_open_rows_exact(c, l);
        }
        EACHAM_HIP_TRY(ctx, hipEventRecord(ctx->ev_tile[slot], st1));
        EACHAM_HIP_TRY(ctx, hipStreamWaitEvent(st2, ctx->ev_tile[slot], 0));
        {
            ProfileScope ps(ctx, EACHAM_KERNEL_MATCH_FINALIZE, st2);
            if (full_cols) launch_full_cols_tail<METRIC>(c, l, stats_dev ? stats_dev + first : nullptr);
            else if ((rc = launch_lean_tail<METRIC>(c, l))) return rc;
            scan_counts_kernel<<<1, 1024, 0, st2>>>(l.cnt, nb, offsets_dev, total_dev, first, first + nb == npairs);
            compact_edges_kernel<<<nb, 256, 0, st2>>>(l.s.matches, l.cnt, offsets_dev + first, pl.row_stride, edges_dev, edge_cap);
        }
        EACHAM_HIP_TRY(ctx, hipEventRecord(ctx->ev_fin[slot], st2));
        EACHAM_HIP_TRY(ctx, hipGetLastError());
    }
    EACHAM_HIP_TRY(ctx, hipEventRecord(ctx->ev_join, st2));         // later work on the context stream sees the results
    EACHAM_HIP_TRY(ctx, hipStreamWaitEvent(st1, ctx->ev_join, 0));
    return EACHAM_OK;
}

static int run_match(eacham_ctx* ctx, const int2* pairs_dev, int npairs, double ratio, int metric, int min_dir, int min_mutual, int mode,
                     int* counts_dev, long long* offsets_dev, uint2* edges_dev, long long edge_cap, long long* total_dev, int4* stats_dev,
                     const int2** pairs_used = nullptr, const int32_t* pairs_host = nullptr) {
    if (metric == METRIC_HAMMING && ctx->kind_common == FRAME_BITS_WIDE)   // the Hamming form on a sweep of its own (matcher_ham_wide.hip)
        return run_match_ham_wide(ctx, pairs_dev, npairs, ratio, min_dir, min_mutual, mode, counts_dev, offsets_dev, edges_dev, edge_cap,
                                  total_dev, stats_dev, pairs_host, pairs_used);
    return metric == METRIC_HAMMING
               ? run_match_metric<METRIC_HAMMING>(ctx, pairs_dev, npairs, ratio, min_dir, min_mutual, mode, counts_dev, offsets_dev, edges_dev,
                                                  edge_cap, total_dev, stats_dev, pairs_used)
               : run_match_metric<METRIC_L2>(ctx, pairs_dev, npairs, ratio, min_dir, min_mutual, mode, counts_dev, offsets_dev, edges_dev,
                                             edge_cap, total_dev, stats_dev, pairs_used);
}

void launch_scan_counts(eacham_ctx* ctx, const int* counts, int n, long long* offsets, long long* total, int first, int is_last) {
    scan_counts_kernel<<<1, 1024, 0, ctx->stream>>>(counts, n, offsets, total, first, is_last);
}
void launch_compact_edges(eacham_ctx* ctx, int nb, const uint2* matches, const int* counts, const long long* offsets,
                          int row_stride, uint2* edges, long long edge_cap) {
    compact_edges_kernel<<<nb, 256, 0, ctx->stream>>>(matches, counts, offsets, row_stride, edges, edge_cap);
}

static int check_pairs_host(eacham_ctx* ctx, const int32_t* pairs, int npairs) {
    for (int i = 0; i < 2 * npairs; ++i) {
        int f = pairs[i];
        if (f < 0 || (size_t)f >= ctx->frames.size() || ctx->frames[f].n < 0)
            return ctx->fail(EACHAM_ERR_INVALID, "pair %d references frame %d which is not resident", i / 2, f);
    }
    return EACHAM_OK;
}

// Every host-pointer matching call runs its body through this: null context, the context's lock, its device, and nothing thrown
// (std::vector on an absurd capacity) leaves extern "C".
template <class Body>
static int match_entry(eacham_ctx* ctx, Body body) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    try {
        return body();
    } catch (const std::exception& e) {
        return ctx->fail(EACHAM_ERR_INVALID, "matcher: %s", e.what());
    } catch (...) {
        return ctx->fail(EACHAM_ERR_INVALID, "matcher: unknown exception");
    }
}

// What a host-pointer call runs: the L2 ratio test on the resident frames (int8 or float), the dot-product form on float
// frames (matcher_dot.hip), or that form behind the fp16 screen (matcher_dot16.hip; mutual only).
enum MatchForm { MATCH_L2, MATCH_DOT, MATCH_DOT_SCREENED, MATCH_HAMMING };

// Host pointers in, CSR over the pairs out: mode 0 = mutual + thresholds, mode 1 = directed lists. `thresh` is the ratio of the
// L2 and Hamming forms or the minimum score of the dot forms. out_val: one 4-byte value per match, the float score of the dot forms,
// the int32 Hamming distance of the Hamming form (may be null), nothing in the L2 form.
static int match_pairs_host(eacham_ctx* ctx, MatchForm form, const int32_t* pairs, int npairs, double thresh, int min_dir,
                            int min_mutual, int mode, int32_t* counts, int64_t* offsets, uint32_t* out_q, uint32_t* out_t,
                            void* out_val, int64_t cap, int64_t* out_total, int32_t* stats) {
    const bool dot = form == MATCH_DOT || form == MATCH_DOT_SCREENED, ham = form == MATCH_HAMMING;
    if (npairs < 0 || (npairs > 0 && (!pairs || !counts || !offsets)) || !out_total || cap < 0 || (cap > 0 && (!out_q || !out_t)))
        return ctx->fail(EACHAM_ERR_INVALID, dot ? "bad arguments to the dot-product matcher" : "bad arguments to match_all_pairs");
    int rc = check_pairs_host(ctx, pairs, npairs);
    if (rc) return rc;
    const bool wide = ctx->kind_common == FRAME_BITS_WIDE;
    if (npairs > 0 && !dot && ham != (ctx->kind_common == FRAME_BITS || wide))
        return ctx->fail(EACHAM_ERR_UNSUPPORTED, ham ? "Hamming matching needs binary frames (eacham_upload_descriptors_bits)"
                                                     : "the resident frames are binary: use the _hamming entry points");
    if (!dot) {
        rc = wide ? EACHAM_OK : check_integer_flag(ctx);   // (no upload kernel of the wide kind raises the flag)
        if (rc) return rc;
    } else if (npairs > 0 && ctx->kind_common != FRAME_F32) {
        return ctx->fail(EACHAM_ERR_UNSUPPORTED, "dot-product matching needs float frames (eacham_upload_descriptors_f32); the resident frames are %s",
                         ctx->kind_common == FRAME_INT8 ? "int8" : "binary");
    }
    *out_total = 0;
    if (npairs == 0) {
        if (offsets) offsets[0] = 0;
        return EACHAM_OK;
    }
    if (dot) {
        rc = sync_frame_table(ctx);
        if (rc) return rc;
    }
    std::vector<int32_t> pairs_fb;   // the screened form's second pair list
    int n_fallback = 0;
    if (form == MATCH_DOT_SCREENED) {
        pairs_fb.resize((size_t)npairs * 2);
        rc = prepare_match_dot_screened(ctx, pairs, npairs, pairs_fb.data(), &n_fallback);
        if (rc) return rc;
    }
    long long total = 0;
    IoStage io(ctx, ctx->stream);
    const auto h_pairs = io.in<int2>(pairs, (size_t)npairs), h_fb = io.in<int2>(pairs_fb.data(), pairs_fb.size() / 2);
    const auto h_counts = io.out<int>(counts, (size_t)npairs);
    const auto h_offsets = io.out<long long>(offsets, (size_t)npairs + 1), h_total = io.out<long long>(&total, 1);
    IoArray<int4> h_stats{0};
    if (stats) h_stats = io.out<int4>(stats, (size_t)npairs);
    // device-only: as results they would pin cap elements and come back whole, where only `total` of them are wanted
    const auto h_edges = io.scratch<uint2>((size_t)cap);
    const auto h_vals = io.scratch<uint32_t>(dot || (ham && out_val) ? (size_t)cap : 0);   // 4 bytes per match: float scores or int32 distances
    IoDev d;
    rc = io.upload(d);
    if (rc) return rc;
    int4* stats_dev = stats ? d(h_stats) : nullptr;   // null selects the lean form in run_match
    const int2* pairs_used = nullptr;   // the sanitised list run_match ran on
    if (form == MATCH_DOT_SCREENED)
        rc = run_match_dot_screened(ctx, d(h_pairs), d(h_fb), pairs_fb.data(), npairs, n_fallback, (float)thresh, min_dir, min_mutual,
                                    d(h_counts), d(h_offsets), d(h_edges), (float*)d(h_vals), cap, d(h_total), stats_dev);
    else if (form == MATCH_DOT)
        rc = run_match_dot(ctx, d(h_pairs), npairs, (float)thresh, min_dir, min_mutual, mode, d(h_counts), d(h_offsets), d(h_edges),
                           (float*)d(h_vals), cap, d(h_total), stats_dev);
    else
        rc = run_match(ctx, d(h_pairs), npairs, thresh, ham ? METRIC_HAMMING : METRIC_L2, min_dir, min_mutual, mode, d(h_counts),
                       d(h_offsets), d(h_edges), cap, d(h_total), stats_dev, &pairs_used, pairs);
    if (rc) return rc;
    if (ham && out_val) {
        rc = hamming_distances(ctx, pairs_used, npairs, d(h_offsets), d(h_total), d(h_edges), cap, (int*)d(h_vals));
        if (rc) return rc;
    }
    rc = io.finish();
    if (rc) return rc;
    *out_total = total;
    if (total > cap) return ctx->fail(EACHAM_ERR_CAPACITY, "%lld matches but capacity %lld", total, (long long)cap);
    if (total > 0) {
        // The one direct copy beside IoStage: how many edges there are is known only now, and exactly that many come back.
        std::vector<uint2> tmp((size_t)total);
        EACHAM_HIP_TRY(ctx, hipMemcpy(tmp.data(), d(h_edges), sizeof(uint2) * (size_t)total, hipMemcpyDeviceToHost));
        for (long long k = 0; k < total; ++k) {
            out_q[k] = tmp[k].x;
            out_t[k] = tmp[k].y;
        }
        if (out_val && (dot || ham)) EACHAM_HIP_TRY(ctx, hipMemcpy(out_val, d(h_vals), sizeof(uint32_t) * (size_t)total, hipMemcpyDeviceToHost));
    }
    return EACHAM_OK;
}

}  // namespace eacham

using namespace eacham;

extern "C" {


int eacham_upload_descriptors_dev(eacham_ctx* ctx, int frame_id, const float* rowmajor_dev, int n, int dim) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    if (n > 0 && !rowmajor_dev) return ctx->fail(EACHAM_ERR_INVALID, "null descriptor pointer");
    return upload_frame(ctx, frame_id, rowmajor_dev, n, dim);
}

int eacham_upload_descriptors(eacham_ctx* ctx, int frame_id, const float* rowmajor, int n, int dim) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    if (n > 0 && !rowmajor) return ctx->fail(EACHAM_ERR_INVALID, "null descriptor pointer");
    if (n < 0 || dim <= 0) return ctx->fail(EACHAM_ERR_INVALID, "bad descriptor shape %d x %d", n, dim);
    size_t bytes = (size_t)n * dim * sizeof(float);
    int rc = ensure_io(ctx, std::max<size_t>(bytes, 256));
    if (rc) return rc;
    if (bytes) {
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(ctx->io, rowmajor, bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    rc = upload_frame(ctx, frame_id, (const float*)ctx->io, n, dim);
    if (rc) return rc;
    return check_integer_flag(ctx);  // also orders reuse of the staging buffer
}

int eacham_frame_rows(eacham_ctx* ctx, int frame_id) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (frame_id < 0 || (size_t)frame_id >= ctx->frames.size() || ctx->frames[frame_id].n < 0)
        return ctx->fail(EACHAM_ERR_INVALID, "frame %d is not resident", frame_id);
    return ctx->frames[frame_id].n;
}

int eacham_match_all_pairs_dev(eacham_ctx* ctx, const int32_t* pairs_dev, int npairs, double ratio,
                               int min_dir, int min_mutual, int32_t* counts_dev, int64_t* offsets_dev,
                               uint32_t* edges_dev, int64_t edge_cap, int64_t* total_dev,
                               int32_t* stats_dev) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    if (npairs < 0 || (npairs > 0 && (!pairs_dev || !counts_dev || !offsets_dev || !total_dev)) ||
        edge_cap < 0 || (edge_cap > 0 && !edges_dev))
        return ctx->fail(EACHAM_ERR_INVALID, "bad arguments to match_all_pairs_dev");
    return run_match(ctx, (const int2*)pairs_dev, npairs, ratio, METRIC_L2, min_dir, min_mutual, 0, counts_dev,
                     (long long*)offsets_dev, (uint2*)edges_dev, edge_cap, (long long*)total_dev,
                     (int4*)stats_dev);
}

int eacham_match_pair(eacham_ctx* ctx, int f1, int f2, double ratio, uint32_t* out_q, uint32_t* out_t,
                      int cap, int* out_count) {
    return match_entry(ctx, [&]() -> int {
        if (!out_count || cap < 0 || (cap > 0 && (!out_q || !out_t))) return ctx->fail(EACHAM_ERR_INVALID, "null output");
        const int32_t pr[2] = {f1, f2};
        int32_t count = 0;
        int64_t offsets[2] = {0, 0}, total = 0;
        const int rc = match_pairs_host(ctx, MATCH_L2, pr, 1, ratio, 0, 0, 1, &count, offsets, out_q, out_t, nullptr, cap, &total, nullptr);
        if (rc == EACHAM_OK || rc == EACHAM_ERR_CAPACITY) *out_count = (int)total;
        return rc;
    });
}

int eacham_match_all_pairs(eacham_ctx* ctx, const int32_t* pairs, int npairs, double ratio, int min_dir,
                           int min_mutual, int32_t* counts, int64_t* offsets, uint32_t* out_q,
                           uint32_t* out_t, int64_t cap, int64_t* out_total, int32_t* stats) {
    return match_entry(ctx, [&]() -> int {
        return match_pairs_host(ctx, MATCH_L2, pairs, npairs, ratio, min_dir, min_mutual, 0, counts, offsets, out_q, out_t, nullptr, cap,
                                out_total, stats);
    });
}

int eacham_match_debug_batches(eacham_ctx* ctx, int npairs, int with_stats, int32_t* starts, int cap, int* n_batches, int* n_slots) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (npairs < 0 || !n_batches || cap < 0 || (cap > 0 && !starts)) return ctx->fail(EACHAM_ERR_INVALID, "bad arguments to match_debug_batches");
    if (ctx->kind_common == FRAME_F32) return ctx->fail(EACHAM_ERR_UNSUPPORTED, "the fp32 path plans its batches on its own");
    const bool full_cols = with_stats != 0;
    MatchPlan pl = make_plan(ctx, std::max(npairs, 1), full_cols);
    int b = 0;
    for (int first = 0, nb = 0; first < npairs; first += nb, ++b) {
        nb = next_batch(pl, b, first, npairs);
        if (b < cap) starts[b] = first;
    }
    *n_batches = b;
    if (n_slots) *n_slots = pl.slots;
    return EACHAM_OK;
}

int eacham_match_debug_plan(eacham_ctx* ctx, int npairs, int with_stats, int* batch, int* round_pairs, int* tail_pairs) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (npairs < 0 || !batch || !round_pairs || !tail_pairs) return ctx->fail(EACHAM_ERR_INVALID, "bad arguments to match_debug_plan");
    if (ctx->kind_common == FRAME_F32) return ctx->fail(EACHAM_ERR_UNSUPPORTED, "the fp32 path plans its batches on its own");
    const MatchPlan pl = make_plan(ctx, std::max(npairs, 1), with_stats != 0);
    *batch = pl.batch;
    *round_pairs = pl.round_pairs;
    *tail_pairs = pl.tail_pairs;
    return EACHAM_OK;
}

int eacham_match_debug_colprune(eacham_ctx* ctx, int64_t* settled, int64_t* verified) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    if (!settled || !verified) return ctx->fail(EACHAM_ERR_INVALID, "null output");
    unsigned long long tot[2] = {0, 0};
    EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    EACHAM_HIP_TRY(ctx, hipMemcpy(tot, colprune_totals(ctx), sizeof(tot), hipMemcpyDeviceToHost));
    *settled = (int64_t)tot[0];
    *verified = (int64_t)tot[1];
    return EACHAM_OK;
}

int eacham_match_debug_screen(eacham_ctx* ctx, int64_t* rows, int64_t* open) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    if (!rows || !open) return ctx->fail(EACHAM_ERR_INVALID, "null output");
    unsigned long long tot[2] = {0, 0};
    EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    EACHAM_HIP_TRY(ctx, hipMemcpy(tot, screen_tally(ctx), sizeof(tot), hipMemcpyDeviceToHost));
    *rows = (int64_t)tot[0];
    *open = (int64_t)tot[1];
    return EACHAM_OK;
}

int eacham_match_debug_screen_items(eacham_ctx* ctx, int64_t* items) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    if (!items) return ctx->fail(EACHAM_ERR_INVALID, "null output");
    unsigned long long n = 0;
    EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    EACHAM_HIP_TRY(ctx, hipMemcpy(&n, screen_tally(ctx) + 2, sizeof(n), hipMemcpyDeviceToHost));
    *items = (int64_t)n;
    return EACHAM_OK;
}

int eacham_match_debug_screen_pair(eacham_ctx* ctx, int f1, int f2, uint32_t* n1, int32_t* l1, int32_t* u2, int cap) {
    return match_entry(ctx, [&]() -> int {
        if (!n1 || !l1 || !u2 || cap < 0) return ctx->fail(EACHAM_ERR_INVALID, "null output");
        const int32_t pr[2] = {f1, f2};
        int rc = check_pairs_host(ctx, pr, 1);
        if (rc) return rc;
        rc = check_integer_flag(ctx);
        if (rc) return rc;
        rc = sync_frame_table(ctx);
        if (rc) return rc;
        if (!frames_have_screen(ctx)) return ctx->fail(EACHAM_ERR_UNSUPPORTED, "the screen sweep needs int8 frames above 128-D");
        const FrameHost& A = ctx->frames[f1];
        if (cap < A.n) return ctx->fail(EACHAM_ERR_CAPACITY, "%d rows but capacity %d", A.n, cap);
        if (A.n == 0) return EACHAM_OK;
        const MatchPlan pl = make_plan(ctx, 1, false);
        rc = ensure_workspace(ctx, pl.total);
        if (rc) return rc;
        uint4* const rowres = pl.slot(ctx->ws, 0).rowres;
        IoStage io(ctx, ctx->stream);
        const auto h_pair = io.in<int2>(pr, 1);
        IoDev d;
        rc = io.upload(d);
        if (rc) return rc;
        match_screen_kernel<METRIC_L2><<<screen_wgs_per_pair(pl), WG_THREADS, 0, ctx->stream>>>(ctx->frame_table_dev, d(h_pair), screen_wgs_per_pair(pl), rowres, pl.row_stride, 0.0, nullptr, 0,
                                                                                        OpenList{});
        EACHAM_HIP_TRY(ctx, hipGetLastError());
        rc = io.finish();
        if (rc) return rc;
        // the slots as the sweep wrote them, by stored row: back to the caller's rows
        const int rows = 32 * A.tiles_used;
        std::vector<uint4> res((size_t)rows);
        std::vector<int> pos((size_t)A.n), meta(2);
        EACHAM_HIP_TRY(ctx, hipMemcpy(res.data(), rowres, sizeof(uint4) * res.size(), hipMemcpyDeviceToHost));
        EACHAM_HIP_TRY(ctx, hipMemcpy(pos.data(), A.pos, sizeof(int) * pos.size(), hipMemcpyDeviceToHost));
        EACHAM_HIP_TRY(ctx, hipMemcpy(meta.data(), A.meta, sizeof(int) * 2, hipMemcpyDeviceToHost));
        for (int q = 0; q < A.n; ++q) {
            const int j = pos[q];
            const uint4 e = res[j];
            const unsigned pa = (j >> 5) >= meta[0] ? 1u : 0u;
            n1[q] = e.w;
            l1[q] = e.x == 0xffffffffu ? -1 : (int32_t)(e.x + pa) - 2;   // -1: no real minimum / no bound (the bound form's padding values)
            u2[q] = e.z == 0xffffffffu ? -1 : (int32_t)(e.z + pa) - 2;
        }
        return EACHAM_OK;
    });
}

int eacham_match_pairs_directed(eacham_ctx* ctx, const int32_t* pairs, int npairs, double ratio, int32_t* counts,
                                int64_t* offsets, uint32_t* out_q, uint32_t* out_t, int64_t cap, int64_t* out_total) {
    return match_entry(ctx, [&]() -> int {
        return match_pairs_host(ctx, MATCH_L2, pairs, npairs, ratio, 0, 0, 1, counts, offsets, out_q, out_t, nullptr, cap, out_total, nullptr);
    });
}

// ---- dot-product form (matcher_dot.hip): CSR over the pairs + scores out ----
int eacham_match_pair_dot(eacham_ctx* ctx, int f1, int f2, float min_score, uint32_t* out_q, uint32_t* out_t, float* out_score,
                          int cap, int* out_count) {
    return match_entry(ctx, [&]() -> int {
        if (!out_count) return ctx->fail(EACHAM_ERR_INVALID, "null output");
        const int32_t pr[2] = {f1, f2};
        int32_t count = 0;
        int64_t offsets[2] = {0, 0}, total = 0;
        const int rc = match_pairs_host(ctx, MATCH_DOT, pr, 1, min_score, 0, 0, 1, &count, offsets, out_q, out_t, out_score, cap, &total, nullptr);
        if (rc == EACHAM_OK || rc == EACHAM_ERR_CAPACITY) *out_count = (int)total;
        return rc;
    });
}

int eacham_match_pairs_directed_dot(eacham_ctx* ctx, const int32_t* pairs, int npairs, float min_score, int32_t* counts,
                                    int64_t* offsets, uint32_t* out_q, uint32_t* out_t, float* out_score, int64_t cap,
                                    int64_t* out_total) {
    return match_entry(ctx, [&]() -> int {
        return match_pairs_host(ctx, MATCH_DOT, pairs, npairs, min_score, 0, 0, 1, counts, offsets, out_q, out_t, out_score, cap, out_total, nullptr);
    });
}

int eacham_match_all_pairs_dot(eacham_ctx* ctx, const int32_t* pairs, int npairs, float min_score, int min_dir, int min_mutual,
                               int32_t* counts, int64_t* offsets, uint32_t* out_q, uint32_t* out_t, float* out_score, int64_t cap,
                               int64_t* out_total, int32_t* stats) {
    return match_entry(ctx, [&]() -> int {
        return match_pairs_host(ctx, MATCH_DOT, pairs, npairs, min_score, min_dir, min_mutual, 0, counts, offsets, out_q, out_t, out_score, cap,
                                out_total, stats);
    });
}

int eacham_match_all_pairs_dot_screened(eacham_ctx* ctx, const int32_t* pairs, int npairs, float min_score, int min_dir, int min_mutual,
                                        int32_t* counts, int64_t* offsets, uint32_t* out_q, uint32_t* out_t, float* out_score,
                                        int64_t cap, int64_t* out_total, int32_t* stats) {
    return match_entry(ctx, [&]() -> int {
        return match_pairs_host(ctx, MATCH_DOT_SCREENED, pairs, npairs, min_score, min_dir, min_mutual, 0, counts, offsets, out_q, out_t, out_score,
                                cap, out_total, stats);
    });
}

// ---- binary descriptors under Hamming distance (matcher_ham.hip): CSR over the pairs + distances out ----
// The packed rows (device pointer) become a resident binary frame: expanded to 0 / 255 floats in the staging buffer for the int8
// upload kernels, padded with zero bits to the next legal dimension, and kept packed beside the frame for the distance kernel.
static int upload_frame_bits(eacham_ctx* ctx, int frame_id, const unsigned char* packed_dev, int n, int bytes_per_row, size_t stage_off) {
    const int dim = bytes_per_row <= 16 ? (8 * bytes_per_row + 15) / 16 * 16 : 8 * bytes_per_row;
    if (n > 0) launch_bits_expand(ctx, packed_dev, n, bytes_per_row, dim, (float*)((char*)ctx->io + stage_off));
    int rc = upload_frame(ctx, frame_id, (const float*)((char*)ctx->io + stage_off), n, dim, FRAME_BITS);
    if (rc) return rc;
    if (n > 0) launch_bits_store(ctx, packed_dev, n, bytes_per_row, 8, ctx->frames[frame_id].bits);
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // orders reuse of the staging buffer (and of the caller's rows)
    return EACHAM_OK;
}
static int check_bits_shape(eacham_ctx* ctx, const void* rows, int n, int bytes_per_row) {
    if (n < 0 || bytes_per_row <= 0) return ctx->fail(EACHAM_ERR_INVALID, "bad descriptor shape %d x %d bytes", n, bytes_per_row);
    if (n > 0 && !rows) return ctx->fail(EACHAM_ERR_INVALID, "null descriptor pointer");
    if (bytes_per_row > 32) return ctx->fail(EACHAM_ERR_UNSUPPORTED, "binary descriptors of %d bytes: this build supports <= 32 (256 bits)", bytes_per_row);
    if (n > MAX_ROWS) return ctx->fail(EACHAM_ERR_UNSUPPORTED, "frame has %d rows; this build supports <= %d", n, MAX_ROWS);
    return EACHAM_OK;
}
static size_t bits_stage_bytes(int n, int bytes_per_row) {   // the expanded rows (a padded dimension is at most 8 bits per byte + 8)
    return ((size_t)n * (8 * bytes_per_row + 8) * sizeof(float) + 255) & ~(size_t)255;
}

int eacham_upload_descriptors_bits_dev(eacham_ctx* ctx, int frame_id, const uint8_t* rowmajor_dev, int n, int bytes_per_row) {
    return match_entry(ctx, [&]() -> int {
        int rc = check_bits_shape(ctx, rowmajor_dev, n, bytes_per_row);
        if (rc) return rc;
        rc = ensure_io(ctx, std::max<size_t>(bits_stage_bytes(n, bytes_per_row), 256));
        if (rc) return rc;
        return upload_frame_bits(ctx, frame_id, rowmajor_dev, n, bytes_per_row, 0);
    });
}

int eacham_upload_descriptors_bits(eacham_ctx* ctx, int frame_id, const uint8_t* rowmajor, int n, int bytes_per_row) {
    return match_entry(ctx, [&]() -> int {
        int rc = check_bits_shape(ctx, rowmajor, n, bytes_per_row);
        if (rc) return rc;
        // staging: the packed rows as they came (the only host-to-device copy), then the expanded rows
        const size_t packed = ((size_t)n * bytes_per_row + 255) & ~(size_t)255;
        rc = ensure_io(ctx, std::max<size_t>(packed + bits_stage_bytes(n, bytes_per_row), 256));
        if (rc) return rc;
        if (n > 0) EACHAM_HIP_TRY(ctx, hipMemcpyAsync(ctx->io, rowmajor, (size_t)n * bytes_per_row, hipMemcpyHostToDevice, ctx->stream));
        return upload_frame_bits(ctx, frame_id, (const unsigned char*)ctx->io, n, bytes_per_row, packed);
    });
}

int eacham_match_pair_hamming(eacham_ctx* ctx, int f1, int f2, double ratio, uint32_t* out_q, uint32_t* out_t, int32_t* out_dist,
                              int cap, int* out_count) {
    return match_entry(ctx, [&]() -> int {
        if (!out_count) return ctx->fail(EACHAM_ERR_INVALID, "null output");
        const int32_t pr[2] = {f1, f2};
        int32_t count = 0;
        int64_t offsets[2] = {0, 0}, total = 0;
        const int rc = match_pairs_host(ctx, MATCH_HAMMING, pr, 1, ratio, 0, 0, 1, &count, offsets, out_q, out_t, out_dist, cap, &total, nullptr);
        if (rc == EACHAM_OK || rc == EACHAM_ERR_CAPACITY) *out_count = (int)total;
        return rc;
    });
}

int eacham_match_pairs_directed_hamming(eacham_ctx* ctx, const int32_t* pairs, int npairs, double ratio, int32_t* counts,
                                        int64_t* offsets, uint32_t* out_q, uint32_t* out_t, int32_t* out_dist, int64_t cap,
                                        int64_t* out_total) {
    return match_entry(ctx, [&]() -> int {
        return match_pairs_host(ctx, MATCH_HAMMING, pairs, npairs, ratio, 0, 0, 1, counts, offsets, out_q, out_t, out_dist, cap, out_total, nullptr);
    });
}

int eacham_match_all_pairs_hamming(eacham_ctx* ctx, const int32_t* pairs, int npairs, double ratio, int min_dir, int min_mutual,
                                   int32_t* counts, int64_t* offsets, uint32_t* out_q, uint32_t* out_t, int32_t* out_dist, int64_t cap,
                                   int64_t* out_total, int32_t* stats) {
    return match_entry(ctx, [&]() -> int {
        return match_pairs_host(ctx, MATCH_HAMMING, pairs, npairs, ratio, min_dir, min_mutual, 0, counts, offsets, out_q, out_t, out_dist, cap,
                                out_total, stats);
    });
}

int eacham_match_all_pairs_hamming_dev(eacham_ctx* ctx, const int32_t* pairs_dev, int npairs, double ratio, int min_dir, int min_mutual,
                                       int32_t* counts_dev, int64_t* offsets_dev, uint32_t* edges_dev, int64_t edge_cap,
                                       int64_t* total_dev, int32_t* stats_dev, int32_t* dist_dev) {
    return match_entry(ctx, [&]() -> int {
        if (npairs < 0 || (npairs > 0 && (!pairs_dev || !counts_dev || !offsets_dev || !total_dev)) || edge_cap < 0 ||
            (edge_cap > 0 && !edges_dev))
            return ctx->fail(EACHAM_ERR_INVALID, "bad arguments to match_all_pairs_hamming_dev");
        const int2* pairs_used = nullptr;
        int rc = run_match(ctx, (const int2*)pairs_dev, npairs, ratio, METRIC_HAMMING, min_dir, min_mutual, 0, counts_dev, (long long*)offsets_dev,
                           (uint2*)edges_dev, edge_cap, (long long*)total_dev, (int4*)stats_dev, &pairs_used);
        if (rc || !dist_dev || npairs <= 0) return rc;
        return hamming_distances(ctx, pairs_used, npairs, (const long long*)offsets_dev, (const long long*)total_dev, (const uint2*)edges_dev,
                                 edge_cap, dist_dev);
    });
}

// ---- wide binary descriptors (matcher_ham_wide.hip): up to 64 bytes per row, a kind of their own behind the _hamming calls above ----
int eacham_upload_descriptors_bits_wide_dev(eacham_ctx* ctx, int frame_id, const uint8_t* rowmajor_dev, int n, int bytes_per_row) {
    return match_entry(ctx, [&]() -> int { return upload_frame_bits_wide(ctx, frame_id, rowmajor_dev, n, bytes_per_row); });
}

int eacham_upload_descriptors_bits_wide(eacham_ctx* ctx, int frame_id, const uint8_t* rowmajor, int n, int bytes_per_row) {
    return match_entry(ctx, [&]() -> int {
        // staging: the packed rows as they came, the only host-to-device copy. Nothing is copied for a shape upload_frame_bits_wide refuses
        // (it tells which way; the pointer it is handed is then never read)
        const bool copy = n > 0 && n <= MAX_ROWS && bytes_per_row > 0 && bytes_per_row <= 64 && rowmajor;
        if (copy) {
            const int rc = ensure_io(ctx, std::max<size_t>((size_t)n * bytes_per_row, 256));
            if (rc) return rc;
            EACHAM_HIP_TRY(ctx, hipMemcpyAsync(ctx->io, rowmajor, (size_t)n * bytes_per_row, hipMemcpyHostToDevice, ctx->stream));
        }
        return upload_frame_bits_wide(ctx, frame_id, (const unsigned char*)(copy ? ctx->io : (const void*)rowmajor), n, bytes_per_row);
    });
}

int eacham_match_debug_hamming_wide_pair(eacham_ctx* ctx, int f1, int f2, int32_t* best, int32_t* h0, int32_t* h1, int cap) {
    return match_entry(ctx, [&]() -> int {
        const int32_t pr[2] = {f1, f2};
        const int rc = check_pairs_host(ctx, pr, 1);
        if (rc) return rc;
        return ham_wide_debug_pair(ctx, f1, f2, best, h0, h1, cap);
    });
}

int eacham_match_debug_hamming_wide(eacham_ctx* ctx, int64_t out[4]) {
    return match_entry(ctx, [&]() -> int {
        if (!out) return ctx->fail(EACHAM_ERR_INVALID, "null output");
        for (int i = 0; i < 4; ++i) out[i] = ctx->wide_debug[i];
        return EACHAM_OK;
    });
}

}  // extern "C"
