// match_guided.hip — guided matching for gfx950 (MI355X): the pairs of a verified match graph matched again, with only the
// candidates that agree with the pair's two-view model admitted (COLMAP's guided_matching, OpenCV's masked knnMatch).
// eacham_match_guided (pairs, models and keypoints from the caller) and eacham_graph_match_guided (those a resident graph
// holds) run the same three kernels; include/eacham_hip.h states the semantics, DESIGN §3.8 the kernel.
//
// guided_sweep_kernel   one workgroup = 4 waves = 4 x 32 query rows of one (pair, direction), swept over the whole train frame.
//     The resident int8 fragments (FrameDev::frag) are MFMA operands for either role: the TRAIN tile is the A operand (rows of the
//     32 x 32 accumulator), the QUERY tile the B operand (columns), so a lane owns ONE query row (column lane % 32) and meets 16
//     train rows per tile (row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5), ascending in i); the two lanes of a query row are merged
//     once, behind the sweep.   d2 = |a|^2 + |b|^2 - 2 a.b   with a.b from the int32 accumulator and the full squared norms from
//     what the upload stored: |c|^2 = 2 (norm[pos] - 1) + (pos >= 32 meta[0]).
//     The gate is score_one<KIND> (score_dev.hpp) cut at the point where its operations start to depend on both points: what
//     depends on the f1 point alone (F: l2 = F x1 and l2[0]^2 + l2[1]^2; E: the normalised point's E x1 and Ex1[0]^2 + Ex1[1]^2;
//     H: the projected point) and on the f2 point alone (F: the point and l1[0]^2 + l1[1]^2; E: the normalised point and the two
//     squares of E' x2; H: the point as floats) is computed once per row — the query's by its lane before the sweep, the train
//     rows' by 128 threads per 128-row chunk into LDS — and only the operations on both run per element, in score_one's order
//     with score_one's intrinsics (no contraction: csrc/Makefile), so err has score_one's bits. A NaN error is not admissible.
//     The admissible set is ONE bipartite mask: in direction 1 (f2's rows as queries) the gate's arguments keep their f1 / f2
//     places.
//     Top-2 under the mask, per query row, as two 64-bit keys (d2 << 16 | stored train position): indices travel with the
//     values, since under a mask the uniqueness of the minimum no longer identifies the partner.
//     TIES: d2(q,t) = |a|^2 + |b|^2 - 2 a.b has the parity of |a|^2 + |b|^2, so two train rows at equal d2 from one query have
//     centred squared norms of equal parity: they lie in ONE parity class of the stored frame, where the upload's stable
//     partition keeps the caller's order. "Lower stored position" is therefore "lower caller index" wherever it decides.
//     Padding positions (orig < 0) are never admissible.
// guided_tail_kernel    one workgroup per pair: ratio test / single candidate / max_d2 per direction, the cross-check, and the
//     pair's matches compacted in ascending q (devprim.hpp's block scan) into the pair's slab; counts and stats.
// launch_scan_counts (matcher.hip) + guided_compact_kernel    CSR offsets over the pairs, the slabs packed into q / t / d2.
//
// Many pairs per launch: the sweep's grid is (pairs x directions, 128-row blocks of the largest query frame), nothing loops over
// pairs on the host. No scratch memory (checked at build time from the compiler's resource remarks).
#include "context.hpp"
#include "devprim.hpp"
#include "score_dev.hpp"

#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

namespace eacham {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef const v4i __attribute__((address_space(1)))* gfrag_t;

constexpr int GM_THREADS = 256;
constexpr int GM_WAVES = GM_THREADS / 64;      // query tiles of a workgroup
constexpr int GM_CHUNK_TILES = 4;              // train tiles whose per-row gate terms are staged in LDS at once
constexpr int GM_CHUNK = 32 * GM_CHUNK_TILES;
constexpr int GM_POS_BITS = 16;                // stored positions: at most 16384 rows + padding of two parity classes and a wave-block
constexpr unsigned long long GM_NONE = ~0ull;
static_assert(GM_CHUNK <= GM_THREADS && prim::SCAN_THREADS == GM_THREADS, "one thread per staged train row; the tail scans with devprim's block");

// What of score_one<KIND> depends on one point alone. first = the point is the pair's f1 point (score_one's `a`).
template <int KIND>
__device__ __forceinline__ double4 gate_terms(bool first, double2 p, const double* __restrict__ M, const double* __restrict__ K, bool normalise) {
    if (KIND == EACHAM_SCORE_FUNDAMENTAL) {
        if (first) {
            double l2[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) l2[r] = dadd(dadd(dmul(M[3 * r], p.x), dmul(M[3 * r + 1], p.y)), M[3 * r + 2]);
            return make_double4(l2[0], l2[1], l2[2], dadd(dmul(l2[0], l2[0]), dmul(l2[1], l2[1])));
        }
        const double l10 = dadd(dadd(dmul(M[0], p.x), dmul(M[3], p.y)), M[6]);
        const double l11 = dadd(dadd(dmul(M[1], p.x), dmul(M[4], p.y)), M[7]);
        return make_double4(p.x, p.y, dadd(dmul(l10, l10), dmul(l11, l11)), 0.0);
    } else if (KIND == EACHAM_SCORE_ESSENTIAL) {
        double x[3] = {p.x, p.y, 1.0};
        if (normalise) {
            x[0] = __ddiv_rn(dadd(p.x, -K[2]), K[0]);
            x[1] = __ddiv_rn(dadd(p.y, -K[3]), K[1]);
        }
        if (first) {
            double Ex1[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) Ex1[r] = dadd(dadd(dmul(M[3 * r], x[0]), dmul(M[3 * r + 1], x[1])), dmul(M[3 * r + 2], x[2]));
            return make_double4(Ex1[0], Ex1[1], Ex1[2], dadd(dmul(Ex1[0], Ex1[0]), dmul(Ex1[1], Ex1[1])));
        }
        const double Et0 = dadd(dadd(dmul(M[0], x[0]), dmul(M[3], x[1])), dmul(M[6], x[2]));
        const double Et1 = dadd(dadd(dmul(M[1], x[0]), dmul(M[4], x[1])), dmul(M[7], x[2]));
        return make_double4(x[0], x[1], dmul(Et0, Et0), dmul(Et1, Et1));
    } else {
        const float x = (float)p.x, y = (float)p.y;
        if (first) {
            const float H0 = (float)M[0], H1 = (float)M[1], H2 = (float)M[2], H3 = (float)M[3], H4 = (float)M[4], H5 = (float)M[5],
                        H6 = (float)M[6], H7 = (float)M[7];
            const float ww = __fdiv_rn(1.f, fadd(fadd(fmul(H6, x), fmul(H7, y)), 1.f));
            const float px = fmul(fadd(fadd(fmul(H0, x), fmul(H1, y)), H2), ww);
            const float py = fmul(fadd(fadd(fmul(H3, x), fmul(H4, y)), H5), ww);
            return make_double4((double)px, (double)py, 0.0, 0.0);   // (floats widened: exact both ways)
        }
        return make_double4((double)x, (double)y, 0.0, 0.0);
    }
}

// The rest of score_one<KIND>: A = the f1 point's terms, B = the f2 point's.
// In front of the divisions of the F and E kinds stands a division-free SCREEN that never rejects an admissible element (DESIGN §3.8
// has the proof). With T = max_error, U = the next float above T and c = RN(U (1 + 2^-50)) >= U (1 + 2^-51) (host, fp64; c = 0:
// screen off; T = +inf or FLT_MAX: c = +inf, nothing is ever rejected): for a denominator n > 0 and p = RN(c n) in the normal range,
//     num > p  =>  num > U n  =>  num / n > U  =>  RN(num / n) >= U  =>  (float)RN(num / n) >= U > T,
// and score_one's max(e1, e2) is >= U or NaN as soon as one of e1, e2 is >= U: the element is not admissible: NaN is returned for it, which no max_error admits.
// NaN operands fail every comparison below and reach the exact lines; so do n = 0, n = inf and a p below the normal range.
constexpr double GM_SCREEN_MIN = 1e-300;   // p at or above this is normal: |RN(c n) - c n| <= 2^-53 c n
template <int KIND>
__device__ __forceinline__ float gate_error(const double4& A, const double4& B, double c) {
    if (KIND == EACHAM_SCORE_FUNDAMENTAL) {
        const double d = dadd(dadd(dmul(B.x, A.x), dmul(B.y, A.y)), A.z);
        const double d2 = dmul(d, d);
        const double pa = dmul(c, A.w), pb = dmul(c, B.z);
        if ((pa >= GM_SCREEN_MIN && d2 > pa) || (pb >= GM_SCREEN_MIN && d2 > pb)) return __builtin_nanf("");
        const double e1 = __ddiv_rn(d2, B.z);
        const double e2 = __ddiv_rn(d2, A.w);
        return (float)(e1 < e2 ? e2 : e1);
    } else if (KIND == EACHAM_SCORE_ESSENTIAL) {
        const double x2tEx1 = dadd(dadd(dmul(B.x, A.x), dmul(B.y, A.y)), dmul(1.0, A.z));
        const double d = dadd(dadd(A.w, B.z), B.w);
        const double num = dmul(x2tEx1, x2tEx1), p = dmul(c, d);
        if (p >= GM_SCREEN_MIN && num > p) return __builtin_nanf("");
        return (float)__ddiv_rn(num, d);
    } else {
        const float dx = fadd((float)A.x, -(float)B.x), dy = fadd((float)A.y, -(float)B.y);
        return fadd(fmul(dx, dx), fmul(dy, dy));
    }
}

struct GuidedDev {
    const FrameDev* frames;
    const int2* pairs;
    const double* models;            // npairs x 9
    const double* K;                 // 4 doubles (read only when normalise)
    const long long* kp_offsets;     // first keypoint of a frame in xy
    const double2* xy;
    const long long* best_off;       // [npairs x 2] first row of an item (pair, direction) in `best`
    ulonglong2* best;                // per stored query row: the two smallest keys under the mask (GM_NONE: none)
    int ndir;                        // 2 with the cross-check, else 1
    int normalise;
    float max_error;
    double screen_c;                 // RN(U (1 + 2^-50)), U = the float above max_error; 0 = no screen (gate_error)
};

__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int m) {
    const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
    return ((unsigned long long)hi << 32) | lo;
}

template <int KS, int KIND>
__global__ __launch_bounds__(GM_THREADS) void guided_sweep_kernel(const GuidedDev g) {
    __shared__ double4 s_terms[GM_CHUNK];
    __shared__ int s_norm[GM_CHUNK];   // the train row's full squared norm, -1 = padding (never admissible)
    const int item = blockIdx.x, p = item / g.ndir, dir = item - p * g.ndir;
    const int2 pr = g.pairs[p];
    const int fq = dir ? pr.y : pr.x, ft = dir ? pr.x : pr.y;
    const FrameDev Q = g.frames[fq], T = g.frames[ft];
    const int qtiles = Q.n > 0 ? Q.meta[1] : 0;
    const int qt0 = blockIdx.y * GM_WAVES;
    if (qt0 >= qtiles) return;   // (the whole workgroup)
    const double* __restrict__ M = g.models + 9 * (size_t)p;
    bool none = true;            // the estimators' "none" record: no candidate is admissible, by rule
#pragma unroll
    for (int k = 0; k < 9; ++k) none = none && M[k] == 0.0;
    const int ttiles = (T.n > 0 && !none) ? T.meta[1] : 0;
    const bool q_first = dir == 0;   // the query rows are the pair's f1 points

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, cl = lane & 31, h = lane >> 5;
    const int qtile = qt0 + wave;
    const bool active = qtile < qtiles;
    const int qpos = 32 * qtile + cl;
    const int qorig = active ? Q.orig[qpos] : -1;
    v4i a[KS];
    int nq = 0;
    double4 qterms = make_double4(0.0, 0.0, 0.0, 0.0);
    if (active) {
        const gfrag_t Qfrag = (gfrag_t)Q.frag;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a[ks] = Qfrag[((size_t)qtile * KS + ks) * 64 + lane];
        if (qorig >= 0) {
            nq = 2 * (Q.norm[qpos] - 1) + (qtile >= Q.meta[0] ? 1 : 0);
            qterms = gate_terms<KIND>(q_first, g.xy[g.kp_offsets[fq] + qorig], M, g.K, g.normalise != 0);
        }
    } else {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a[ks] = v4i{0, 0, 0, 0};
    }
    unsigned long long k0 = GM_NONE, k1 = GM_NONE;
    const gfrag_t Tfrag = (gfrag_t)T.frag;
    const int teven = ttiles > 0 ? T.meta[0] : 0;
    for (int c0 = 0; c0 < ttiles; c0 += GM_CHUNK_TILES) {
        __syncthreads();   // (the chunk before has been read)
        if (tid < GM_CHUNK) {
            const int tpos = 32 * c0 + tid;
            int nt = -1;
            if (tpos < 32 * ttiles) {
                const int torig = T.orig[tpos];
                if (torig >= 0) {
                    nt = 2 * (T.norm[tpos] - 1) + ((tpos >> 5) >= teven ? 1 : 0);
                    s_terms[tid] = gate_terms<KIND>(!q_first, g.xy[g.kp_offsets[ft] + torig], M, g.K, g.normalise != 0);
                }
            }
            s_norm[tid] = nt;
        }
        __syncthreads();
        if (!active) continue;   // (a wave without a query tile still meets the barriers)
        const int cend = ttiles - c0 < GM_CHUNK_TILES ? ttiles - c0 : GM_CHUNK_TILES;
        for (int tt = 0; tt < cend; ++tt) {
            const int tile = c0 + tt;
            v16i acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(Tfrag[((size_t)tile * KS + ks) * 64 + lane], a[ks], acc, 0, 0, 0);
            if (qorig < 0) continue;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r = (i & 3) + 8 * (i >> 2) + 4 * h;   // ascending in i
                const int nt = s_norm[32 * tt + r];
                if (nt < 0) continue;
                const double4 tterms = s_terms[32 * tt + r];
                const float err = q_first ? gate_error<KIND>(qterms, tterms, g.screen_c) : gate_error<KIND>(tterms, qterms, g.screen_c);
                if (!(err <= g.max_error)) continue;   // (NaN: not admissible)
                const unsigned d2 = (unsigned)(nq + nt - 2 * acc[i]);
                const unsigned long long key = ((unsigned long long)d2 << GM_POS_BITS) | (unsigned)(32 * tile + r);
                if (key < k0) k1 = k0, k0 = key;
                else if (key < k1) k1 = key;
            }
        }
    }
    if (!active) return;
    // the two lanes of a query row: keys are distinct (the position is part of them), so the merge is a plain 2-of-4
    const unsigned long long o0 = shfl_xor64(k0, 32), o1 = shfl_xor64(k1, 32);
    const unsigned long long lo = k0 < o0 ? k0 : o0, hi = k0 < o0 ? o0 : k0, s = k1 < o1 ? k1 : o1;
    if (h == 0) g.best[g.best_off[item] + qpos] = make_ulonglong2(lo, hi < s ? hi : s);
}

// eacham_match_pair's predicate on the top-2 under the mask (include/eacham_hip.h: the table of the directed match)
__device__ __forceinline__ bool guided_pass(const ulonglong2 k, double ratio, unsigned max_d2) {
    if (k.x == GM_NONE) return false;                                    // no admissible candidate
    const unsigned d0 = (unsigned)(k.x >> GM_POS_BITS);
    if (max_d2 != 0 && d0 > max_d2) return false;
    if (k.y == GM_NONE) return true;                                     // exactly one: the runner-up counts as +inf
    const unsigned d1 = (unsigned)(k.y >> GM_POS_BITS);
    const float quot = __fdiv_rn(__fsqrt_rn((float)d0), __fsqrt_rn((float)d1));
    return (double)quot < ratio;                                         // 0 / 0 = NaN: rejected
}

__global__ __launch_bounds__(GM_THREADS) void guided_tail_kernel(const GuidedDev g, double ratio, unsigned max_d2, const long long* __restrict__ slab_off,
                                                                 unsigned* __restrict__ slab_q, unsigned* __restrict__ slab_t, unsigned* __restrict__ slab_d2,
                                                                 int* __restrict__ counts, int* __restrict__ stats) {
    __shared__ int lds[prim::SCAN_THREADS];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int2 pr = g.pairs[p];
    const FrameDev A = g.frames[pr.x], B = g.frames[pr.y];
    const bool cross = g.ndir == 2;
    const ulonglong2* bestA = g.best + g.best_off[(size_t)p * g.ndir];
    const ulonglong2* bestB = cross ? g.best + g.best_off[(size_t)p * g.ndir + 1] : nullptr;
    const long long so = slab_off[p];
    int base = 0, m12 = 0, m21 = 0;
    for (int q0 = 0; q0 < A.n; q0 += GM_THREADS) {
        const int q = q0 + tid;
        bool ok = false, keep = false;
        unsigned tpos = 0, d2 = 0;
        if (q < A.n) {
            const int pos = A.pos[q];
            const ulonglong2 k = bestA[pos];
            ok = keep = guided_pass(k, ratio, max_d2);
            tpos = (unsigned)(k.x & ((1u << GM_POS_BITS) - 1)), d2 = (unsigned)(k.x >> GM_POS_BITS);
            if (ok && cross) {
                const ulonglong2 kb = bestB[tpos];
                keep = guided_pass(kb, ratio, max_d2) && (int)(kb.x & ((1u << GM_POS_BITS) - 1)) == pos;
            }
        }
        m12 += __syncthreads_count(ok);
        int tot = 0;
        const int at = prim::block_exclusive<int>(keep ? 1 : 0, lds, &tot);
        if (keep) {
            slab_q[so + base + at] = (unsigned)q;
            slab_t[so + base + at] = (unsigned)B.orig[tpos];
            slab_d2[so + base + at] = d2;
        }
        base += tot;
    }
    if (cross)
        for (int t0 = 0; t0 < B.n; t0 += GM_THREADS) {
            const int t = t0 + tid;
            m21 += __syncthreads_count(t < B.n && guided_pass(bestB[B.pos[t < B.n ? t : 0]], ratio, max_d2));
        }
    if (tid == 0) {
        counts[p] = base;
        stats[3 * (size_t)p] = m12, stats[3 * (size_t)p + 1] = m21, stats[3 * (size_t)p + 2] = base;
    }
}

__global__ __launch_bounds__(GM_THREADS) void guided_compact_kernel(const int* __restrict__ counts, const long long* __restrict__ offsets,
                                                                    const long long* __restrict__ slab_off, const unsigned* __restrict__ slab_q,
                                                                    const unsigned* __restrict__ slab_t, const unsigned* __restrict__ slab_d2,
                                                                    unsigned* __restrict__ out_q, unsigned* __restrict__ out_t,
                                                                    unsigned* __restrict__ out_d2, long long cap) {
    const int p = blockIdx.x, n = counts[p];
    const long long off = offsets[p], so = slab_off[p];
    for (int k = threadIdx.x; k < n; k += GM_THREADS)
        if (off + k < cap) out_q[off + k] = slab_q[so + k], out_t[off + k] = slab_t[so + k], out_d2[off + k] = slab_d2[so + k];
}

template <int KS>
void launch_sweep(hipStream_t st, dim3 grid, int kind, const GuidedDev& g) {
    if (kind == EACHAM_SCORE_FUNDAMENTAL) guided_sweep_kernel<KS, EACHAM_SCORE_FUNDAMENTAL><<<grid, GM_THREADS, 0, st>>>(g);
    else if (kind == EACHAM_SCORE_ESSENTIAL) guided_sweep_kernel<KS, EACHAM_SCORE_ESSENTIAL><<<grid, GM_THREADS, 0, st>>>(g);
    else guided_sweep_kernel<KS, EACHAM_SCORE_HOMOGRAPHY><<<grid, GM_THREADS, 0, st>>>(g);
}

// One call of either form. The keypoints are the caller's (kp_offsets_h / xy_h: the layout of eacham_graph_create, read for the
// frames the pairs name) or, xy_h == null and graph != null, the resident graph's.
struct GuidedCall {
    const char* what;
    int kind;
    const int32_t* pairs;
    int npairs;
    const double* models;
    const double* K;
    const int64_t* kp_offsets_h;
    const double* xy_h;
    const eacham_graph* graph;
    float max_error;
    double ratio;
    uint32_t max_d2;
    int cross_check;
    int32_t* counts;
    int64_t* offsets;
    uint32_t *out_q, *out_t, *out_d2;
    int64_t cap;
    int64_t* out_total;
    int32_t* stats;
};

int run_guided(eacham_ctx* ctx, const GuidedCall& c) {
    const char* what = c.what;
    const int P = c.npairs;
    // ---- every check, before anything is launched or written
    if (P < 0 || c.cap < 0) return ctx->fail(EACHAM_ERR_INVALID, "%s: negative size", what);
    if (!c.out_total || !c.offsets || (P > 0 && (!c.pairs || !c.models || !c.counts)) || (c.cap > 0 && (!c.out_q || !c.out_t)))
        return ctx->fail(EACHAM_ERR_INVALID, "%s: null required pointer", what);
    if (c.kind != EACHAM_SCORE_ESSENTIAL && c.kind != EACHAM_SCORE_HOMOGRAPHY && c.kind != EACHAM_SCORE_FUNDAMENTAL)
        return ctx->fail(EACHAM_ERR_INVALID, "%s: unknown kind %d", what, c.kind);
    if (!(c.max_error >= 0.f)) return ctx->fail(EACHAM_ERR_INVALID, "%s: max_error is negative or not a number", what);
    if (std::isnan(c.ratio)) return ctx->fail(EACHAM_ERR_INVALID, "%s: the ratio is not a number", what);
    if (c.cross_check && !(c.ratio > 0.0 && c.ratio <= 1.0)) return ctx->fail(EACHAM_ERR_INVALID, "%s: the cross-check needs a ratio in (0, 1]", what);
    if (c.graph && !c.graph->has_xy) return ctx->fail(EACHAM_ERR_INVALID, "%s: the graph has no keypoint coordinates (eacham_graph_set_keypoints)", what);
    if (!c.graph && P > 0 && !c.kp_offsets_h) return ctx->fail(EACHAM_ERR_INVALID, "%s: null kp_offsets", what);
    int max_frame = -1;
    for (int i = 0; i < 2 * P; ++i) {
        const int f = c.pairs[i];
        if (f < 0 || (size_t)f >= ctx->frames.size() || ctx->frames[f].n < 0)
            return ctx->fail(EACHAM_ERR_INVALID, "%s: pair %d names frame %d, which is not resident", what, i / 2, f);
        max_frame = std::max(max_frame, f);
    }
    if (P > 0 && ctx->kind_common != FRAME_INT8)
        return ctx->fail(EACHAM_ERR_UNSUPPORTED, "%s: the resident frames are not int8 frames (eacham_upload_descriptors)", what);
    const int64_t* kpo = c.graph ? (const int64_t*)c.graph->kp_offsets_h.data() : c.kp_offsets_h;
    long long n_xy = 0;   // rows of xy the pairs' frames reach (list form: what is uploaded)
    for (int i = 0; i < 2 * P; ++i) {
        const int f = c.pairs[i];
        if (c.graph && f >= c.graph->n_frames) return ctx->fail(EACHAM_ERR_INVALID, "%s: frame %d is not a frame of the graph", what, f);
        const long long nk = kpo[f + 1] - kpo[f];
        if (kpo[f] < 0 || nk != ctx->frames[f].n)
            return ctx->fail(EACHAM_ERR_INVALID, "%s: frame %d has %lld keypoints and %d resident rows", what, f, nk, ctx->frames[f].n);
        n_xy = std::max<long long>(n_xy, kpo[f + 1]);
    }
    if (!c.graph && n_xy > 0 && !c.xy_h) return ctx->fail(EACHAM_ERR_INVALID, "%s: null xy", what);
    if (P == 0) {
        c.offsets[0] = 0, *c.out_total = 0;
        return EACHAM_OK;
    }
    if (int rc = check_integer_flag(ctx)) return rc;
    if (int rc = sync_frame_table(ctx)) return rc;

    // ---- the plan: where each (pair, direction) keeps its rows' top-2, where each pair's slab of matches lies
    const int ndir = c.cross_check ? 2 : 1;
    std::vector<long long> best_off((size_t)P * ndir), slab_off((size_t)P + 1, 0);
    long long rows = 0;
    int max_qtiles = 0;
    for (int p = 0; p < P; ++p) {
        const FrameHost &A = ctx->frames[c.pairs[2 * p]], &B = ctx->frames[c.pairs[2 * p + 1]];
        best_off[(size_t)p * ndir] = rows, rows += 32LL * A.ntiles;
        max_qtiles = std::max(max_qtiles, A.ntiles);
        if (ndir == 2) best_off[(size_t)p * ndir + 1] = rows, rows += 32LL * B.ntiles, max_qtiles = std::max(max_qtiles, B.ntiles);
        slab_off[p + 1] = slab_off[p] + A.n;
    }
    const long long slab = slab_off[P];
    if ((long long)P * ndir > INT_MAX) return ctx->fail(EACHAM_ERR_CAPACITY, "%s: %d pairs in one call", what, P);
    const size_t o_best = 0, o_sq = align256(o_best + sizeof(ulonglong2) * (size_t)rows), o_st = align256(o_sq + 4 * (size_t)slab),
                 o_sd = align256(o_st + 4 * (size_t)slab), ws_bytes = align256(o_sd + 4 * (size_t)slab);
    if (int rc = ensure_workspace(ctx, std::max<size_t>(ws_bytes, 256))) return rc;
    char* ws = (char*)ctx->ws;

    hipStream_t st = ctx->stream;
    std::vector<int32_t> h_counts_v((size_t)P), h_stats_v(3 * (size_t)P);
    std::vector<long long> h_offsets_v((size_t)P + 1);
    long long total = 0;
    IoStage io(ctx, st);
    const auto h_counts = io.out<int>(h_counts_v.data(), (size_t)P);
    const auto h_offsets = io.out<long long>(h_offsets_v.data(), (size_t)P + 1), h_total = io.out<long long>(&total, 1);
    const auto h_stats = io.out<int>(h_stats_v.data(), 3 * (size_t)P);
    const auto h_pairs = io.in<int2>(c.pairs, (size_t)P);
    const auto h_models = io.in<double>(c.models, 9 * (size_t)P);
    const auto h_K = io.in<double>(c.K, 4);
    const auto h_boff = io.in<long long>(best_off.data(), best_off.size()), h_soff = io.in<long long>(slab_off.data(), slab_off.size());
    const auto h_kpo = io.in<long long>(c.graph ? nullptr : kpo, c.graph ? 0 : (size_t)max_frame + 2);
    const auto h_xy = io.in<double2>(c.graph ? nullptr : c.xy_h, c.graph ? 0 : (size_t)n_xy);
    // device-only: the capacity comes back as `total` entries, not whole
    const auto h_q = io.scratch<unsigned>((size_t)c.cap), h_t = io.scratch<unsigned>((size_t)c.cap), h_d2 = io.scratch<unsigned>((size_t)c.cap);
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    GuidedDev g;
    g.frames = ctx->frame_table_dev, g.pairs = d(h_pairs), g.models = d(h_models), g.K = d(h_K);
    g.kp_offsets = c.graph ? c.graph->kp_offsets : d(h_kpo);
    g.xy = c.graph ? (const double2*)c.graph->xy : d(h_xy);
    g.best_off = d(h_boff), g.best = (ulonglong2*)(ws + o_best);
    g.ndir = ndir, g.normalise = c.K != nullptr, g.max_error = c.max_error;
    g.screen_c = ctx->guided_screen ? (double)std::nextafterf(c.max_error, INFINITY) * (1.0 + 0x1p-50) : 0.0;   // (inf stays inf)
    {
        ProfileScope scope(ctx, EACHAM_KERNEL_MATCH_GUIDED);
        if (max_qtiles > 0) {
            const dim3 grid((unsigned)(P * ndir), (unsigned)((max_qtiles + GM_WAVES - 1) / GM_WAVES));
            if (ctx->ks_common == 2) launch_sweep<2>(st, grid, c.kind, g);
            else if (ctx->ks_common == 4) launch_sweep<4>(st, grid, c.kind, g);
            else launch_sweep<8>(st, grid, c.kind, g);
        }
        guided_tail_kernel<<<P, GM_THREADS, 0, st>>>(g, c.ratio, c.max_d2, d(h_soff), (unsigned*)(ws + o_sq), (unsigned*)(ws + o_st), (unsigned*)(ws + o_sd),
                                                    d(h_counts), d(h_stats));
        launch_scan_counts(ctx, d(h_counts), P, d(h_offsets), d(h_total), 0, 1);
        guided_compact_kernel<<<P, GM_THREADS, 0, st>>>(d(h_counts), d(h_offsets), d(h_soff), (const unsigned*)(ws + o_sq), (const unsigned*)(ws + o_st),
                                                       (const unsigned*)(ws + o_sd), d(h_q), d(h_t), d(h_d2), (long long)c.cap);
    }
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    if (int rc = io.finish()) return rc;
    *c.out_total = total;
    if (total > c.cap) return ctx->fail(EACHAM_ERR_CAPACITY, "%s: %lld matches but capacity %lld", what, total, (long long)c.cap);
    memcpy(c.counts, h_counts_v.data(), sizeof(int32_t) * (size_t)P);
    memcpy(c.offsets, h_offsets_v.data(), sizeof(int64_t) * ((size_t)P + 1));
    if (c.stats) memcpy(c.stats, h_stats_v.data(), sizeof(int32_t) * 3 * (size_t)P);
    if (total > 0) {   // exactly the matches there are come back (as the other matching calls do it)
        EACHAM_HIP_TRY(ctx, hipMemcpy(c.out_q, d(h_q), 4 * (size_t)total, hipMemcpyDeviceToHost));
        EACHAM_HIP_TRY(ctx, hipMemcpy(c.out_t, d(h_t), 4 * (size_t)total, hipMemcpyDeviceToHost));
        if (c.out_d2) EACHAM_HIP_TRY(ctx, hipMemcpy(c.out_d2, d(h_d2), 4 * (size_t)total, hipMemcpyDeviceToHost));
    }
    return EACHAM_OK;
}

template <class Body>
int guided_entry(eacham_ctx* ctx, const char* what, Body body) {   // nothing may leave extern "C"
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
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

extern "C" int eacham_match_guided(eacham_ctx* ctx, int kind, const int32_t* pairs, int npairs, const double* models, const double* K,
                                   const int64_t* kp_offsets, const double* xy, float max_error, double ratio, uint32_t max_d2,
                                   int cross_check, int32_t* counts, int64_t* offsets, uint32_t* out_q, uint32_t* out_t, uint32_t* out_d2,
                                   int64_t cap, int64_t* out_total, int32_t* stats) {
    if (!ctx) return EACHAM_ERR_INVALID;
    return guided_entry(ctx, "match_guided", [&]() -> int {
        return run_guided(ctx, GuidedCall{"match_guided", kind, pairs, npairs, models, K, kp_offsets, xy, nullptr, max_error, ratio, max_d2, cross_check,
                                          counts, offsets, out_q, out_t, out_d2, cap, out_total, stats});
    });
}

extern "C" int eacham_graph_match_guided(eacham_graph* graph, int kind, const double* models, const double* K, float max_error, double ratio,
                                         uint32_t max_d2, int cross_check, int32_t* counts, int64_t* offsets, uint32_t* out_q,
                                         uint32_t* out_t, uint32_t* out_d2, int64_t cap, int64_t* out_total, int32_t* stats) {
    if (!graph) return EACHAM_ERR_INVALID;
    eacham_ctx* ctx = graph->ctx;
    return guided_entry(ctx, "graph_match_guided", [&]() -> int {
        return run_guided(ctx, GuidedCall{"graph_match_guided", kind, graph->pairs_h.data(), graph->npairs, models, K, nullptr, nullptr, graph, max_error,
                                          ratio, max_d2, cross_check, counts, offsets, out_q, out_t, out_d2, cap, out_total, stats});
    });
}
