// tracks.hip — multi-view tracks from the CSR match graph: the stage between the pairwise matches (and their LMedS inlier masks)
// and eacham_triangulate_tracks / eacham_ba_solve. The reference forms a star around ONE frame's keypoints with hash maps, one
// frame at a time (modules/sfm/reconstruction/Triangulator.cpp:202-241); here the whole graph is settled at once.
//
// A node is a keypoint (global id kp_offsets[f] + k), an edge a kept match, a track a connected component with at least min_len
// nodes, labelled by its SMALLEST node id — so the answer is a pure function of the input, whatever order the hardware runs
// things in. No numeric work: integers only, and the only atomic is an integer atomicMin whose fixed point is order-free.
//
//   tracks_init / tracks_edges      parent[i] = root[i] = i; per packed match its two node ids (or NONE if not kept), touched flags
//   prim::exclusive_scan(touched)   -> the compacted position of every touched node, their number T
//   rounds, ONE LAUNCH PER STEP (no workgroup ever waits for another inside a kernel):
//     tracks_hook      over matches: the two ends' roots are read from the SNAPSHOT `root` (every entry a root of the round's
//                      start), atomicMin(parent[larger root], smaller root); a hook raises changed[round]
//     tracks_compress  over nodes: follow parent to the root, write it to parent and to the snapshot (full compression)
//   compaction of the touched nodes (ascending), prim::radix_sort_pairs by label (stable: inside a track nodes stay ascending =
//   frame-major, then keypoint; tracks come out by smallest node id), runs of equal labels -> lengths, conflict flags (two
//   adjacent observations of one frame), the min_len / conflict filter as one scan of (kept, kept length) + one emitting kernel.
//
// ROUND CAP. Look at one component with k >= 2 trees at a round's start; all parents are roots, so the round is synchronous:
// afterwards parent[t] = min(t, smallest root among t's neighbour trees). A root survives iff it is a local minimum among
// its neighbour trees. Every neighbour t of a survivor s was hooked below some root <= s, so after the compression root(t) <= s:
// either (a) all of s's neighbours now hang under s — s's tree holds at least two of the old trees — or (b) some neighbour
// tree has a root < s, and s is hooked in the NEXT round. After two rounds only trees of kind (a) can be left, and those are
// disjoint unions of >= 2 old trees: k halves at least every TWO rounds (one round alone does not: a star whose centre carries
// the largest id keeps k - 1 of k trees). From k <= T_max = min(nodes, 2 x matches) single nodes a component is one tree after
// 2 * ceil(log2 T_max) rounds, and one more round sees nothing to hook: cap = 2 * ceil(log2 T_max) + 1. Past the cap the call
// returns an error; nothing loops unbounded.
//
// READ-BACKS. changed[] has one word per round; a hook kernel whose predecessor's word is 0 returns at once, so rounds are
// enqueued ROUND_BATCH at a time and the words are read back (with T, through the pinned mirror of the staging buffer) once
// per batch; one more read-back brings the totals after the emitting kernel.
#include "context.hpp"
#include "devprim.hpp"

#include <climits>
#include <exception>
#include <vector>

namespace eacham {
namespace {

constexpr int TT = 256;
constexpr unsigned NONE = 0xffffffffu;
constexpr int ROUND_BATCH = 4;
// status words at the head of the staging buffer (the first result array: offset 0 of the pinned mirror)
constexpr int W_TOUCHED = 0, W_RUNS = 1, W_TOTALS = 2 /* I3: tracks, observations, - */, W_CHANGED = 8, N_WORDS = W_CHANGED + 64;

__device__ __forceinline__ long long gid() { return (long long)blockIdx.x * TT + threadIdx.x; }

__global__ __launch_bounds__(TT) void tracks_init_kernel(int n, unsigned* __restrict__ parent, unsigned* __restrict__ root,
                                                         int* __restrict__ touched, int* __restrict__ node_track) {
    const long long i = gid();
    if (i >= n) return;
    parent[i] = root[i] = (unsigned)i;
    touched[i] = 0;
    node_track[i] = -1;
}

// packed match m belongs to the pair p with poff[p] <= m < poff[p] + counts[p] (pairs without matches share their successor's start
// and are never the LAST entry that is <= m, unless they trail — then no m reaches them)
__global__ __launch_bounds__(TT) void tracks_edges_kernel(int m_total, const int2* __restrict__ pairs, int npairs,
                                                          const long long* __restrict__ poff, const long long* __restrict__ src_off,
                                                          const long long* __restrict__ keep_off, const unsigned* __restrict__ q,
                                                          const unsigned* __restrict__ t, const unsigned char* __restrict__ keep,
                                                          const long long* __restrict__ kp_offsets, unsigned* __restrict__ eu,
                                                          unsigned* __restrict__ ev, int* __restrict__ touched) {
    const long long m = gid();
    if (m >= m_total) return;
    const int p = prim::segment_of(poff, npairs, m);
    const long long k = m - poff[p];
    unsigned u = NONE, v = NONE;
    if (!keep || keep[keep_off[p] + k]) {
        const int2 pr = pairs[p];
        const unsigned a = (unsigned)(kp_offsets[pr.x] + q[src_off[p] + k]), b = (unsigned)(kp_offsets[pr.y] + t[src_off[p] + k]);
        u = a < b ? a : b;
        v = a < b ? b : a;
        touched[u] = 1;
        touched[v] = 1;
    }
    eu[m] = u;
    ev[m] = v;
}

__global__ __launch_bounds__(TT) void tracks_hook_kernel(int m_total, const unsigned* __restrict__ eu, const unsigned* __restrict__ ev,
                                                         const unsigned* __restrict__ root, unsigned* parent, int* changed, int round) {
    if (round > 0 && changed[round - 1] == 0) return;   // settled: the rest of the batch is empty launches
    const long long m = gid();
    if (m >= m_total) return;
    const unsigned u = eu[m];
    if (u == NONE) return;
    const unsigned ru = root[u], rv = root[ev[m]];
    if (ru == rv) return;
    atomicMin(&parent[ru > rv ? ru : rv], ru > rv ? rv : ru);
    changed[round] = 1;
}

// parent[x] <= x always, a root's own entry does not change here, and an entry another thread has already compressed leads to the
// same root: the walk ends at the root whatever it reads on the way
__global__ __launch_bounds__(TT) void tracks_compress_kernel(int n, const int* __restrict__ touched, unsigned* parent, unsigned* __restrict__ root,
                                                             const int* __restrict__ changed, int round) {
    if (changed[round] == 0) return;
    const long long i = gid();
    if (i >= n || !touched[i]) return;
    unsigned p = __atomic_load_n(&parent[i], __ATOMIC_RELAXED);
    for (;;) {
        const unsigned pp = __atomic_load_n(&parent[p], __ATOMIC_RELAXED);
        if (pp == p) break;
        p = pp;
    }
    __atomic_store_n(&parent[i], p, __ATOMIC_RELAXED);
    root[i] = p;
}

__global__ __launch_bounds__(TT) void tracks_compact_kernel(int n, const int* __restrict__ touched, const int* __restrict__ pos,
                                                            const unsigned* __restrict__ root, uint32_t* __restrict__ keys,
                                                            uint32_t* __restrict__ vals) {
    const long long i = gid();
    if (i >= n || !touched[i]) return;
    keys[pos[i]] = root[i];
    vals[pos[i]] = (uint32_t)i;
}

__global__ __launch_bounds__(TT) void tracks_heads_kernel(int T, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                          const long long* __restrict__ kp_offsets, int n_frames, int* __restrict__ head,
                                                          unsigned* __restrict__ frame) {
    const long long j = gid();
    if (j >= T) return;
    head[j] = (j == 0 || keys[j] != keys[j - 1]) ? 1 : 0;
    frame[j] = (unsigned)prim::segment_of(kp_offsets, n_frames, (long long)vals[j]);   // (frames without keypoints own no id)
}

// hx = exclusive scan of the heads: the run of j is hx[j] + head(j) - 1
__global__ __launch_bounds__(TT) void tracks_runs_kernel(int T, const uint32_t* __restrict__ keys, const int* __restrict__ hx,
                                                         const unsigned* __restrict__ frame, const int* __restrict__ words,
                                                         int* __restrict__ run_start, int* __restrict__ run_conf) {
    const long long j = gid();
    if (j >= T) return;
    const int h = (j == 0 || keys[j] != keys[j - 1]) ? 1 : 0;
    const int r = hx[j] + h - 1;
    if (h) run_start[r] = (int)j;
    else if (frame[j] == frame[j - 1]) run_conf[r] = 1;   // sorted by node id inside the run: one frame's keypoints are adjacent
    if (j == 0) run_start[words[W_RUNS]] = T;
}

__global__ __launch_bounds__(TT) void tracks_select_kernel(int T, const int* __restrict__ words, const int* __restrict__ run_start,
                                                           const int* __restrict__ run_conf, int min_len, int policy,
                                                           prim::I3* __restrict__ sel) {
    const long long r = gid();
    if (r >= T) return;
    prim::I3 s{0, 0, 0};
    if (r < words[W_RUNS]) {
        const int len = run_start[r + 1] - run_start[r];
        if (len >= min_len && !(policy == 1 && run_conf[r])) s = prim::I3{1, len, 0};
    }
    sel[r] = s;
}

__global__ __launch_bounds__(TT) void tracks_emit_kernel(int T, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                         const int* __restrict__ hx, const unsigned* __restrict__ frame,
                                                         const int* __restrict__ run_start, const int* __restrict__ run_conf,
                                                         const prim::I3* __restrict__ sel, const prim::I3* __restrict__ selx,
                                                         const long long* __restrict__ kp_offsets, const int* __restrict__ words,
                                                         long long* __restrict__ track_ptr, unsigned* __restrict__ obs_frame,
                                                         unsigned* __restrict__ obs_kp, unsigned char* __restrict__ track_flags,
                                                         int* __restrict__ node_track) {
    const long long j = gid();
    if (j >= T) return;
    if (j == 0) track_ptr[words[W_TOTALS]] = words[W_TOTALS + 1];
    const int h = (j == 0 || keys[j] != keys[j - 1]) ? 1 : 0;
    const int r = hx[j] + h - 1;
    if (!sel[r].a) return;
    const int tix = selx[r].a, base = selx[r].b;
    const long long o = base + (j - run_start[r]);
    const unsigned f = frame[j], node = vals[j];
    obs_frame[o] = f;
    obs_kp[o] = (unsigned)(node - kp_offsets[f]);
    node_track[node] = tix;
    if (h) {
        track_ptr[tix] = base;
        track_flags[tix] = run_conf[r] ? 1 : 0;
    }
}

inline int ceil_log2(long long x) {
    int b = 0;
    while ((1ll << b) < x) ++b;
    return b;
}

// where the temporaries and the device-side results lie in the call's one scratch array
struct TracksPlan {
    long long tmax = 0;   // bound of the touched nodes = of the observations
    int key_bits = 1, round_cap = 1;
    size_t parent, root, touched, pos, eu, ev, ka, kb, va, vb, head, frame, run_start, run_conf, sel, selx, sort_ws, scan_ws, scan_ws3;
    size_t o_ptr, o_frame, o_kp, o_flags, total = 0;
    TracksPlan(long long n, long long m) {
        tmax = std::min<long long>(n, 2 * m);
        key_bits = std::max(1, ceil_log2(n));
        round_cap = 2 * ceil_log2(tmax) + 1;
        auto take = [&](size_t bytes) { size_t o = total; total = align256(total + bytes); return o; };
        const size_t N = (size_t)n, M = (size_t)m, T = (size_t)tmax;
        parent = take(4 * N), root = take(4 * N), touched = take(4 * N), pos = take(4 * N);
        eu = take(4 * M), ev = take(4 * M);
        ka = take(4 * T), kb = take(4 * T), va = take(4 * T), vb = take(4 * T);
        head = take(4 * T), frame = take(4 * T), run_start = take(4 * (T + 1)), run_conf = take(4 * T);
        sel = take(sizeof(prim::I3) * T), selx = take(sizeof(prim::I3) * T);
        sort_ws = take(sizeof(int) * prim::radix_ws_ints((int)T));
        scan_ws = take(sizeof(int) * prim::scan_ws_elems(std::max(N, T)));
        scan_ws3 = take(sizeof(prim::I3) * prim::scan_ws_elems(T));
        o_ptr = take(8 * (T / 2 + 2)), o_frame = take(4 * T), o_kp = take(4 * T), o_flags = take(T / 2 + 2);
    }
};

struct TracksGraphDev {   // the graph as the kernels see it
    int n_frames, npairs;
    long long n_nodes, n_matches;   // nodes; packed matches
    const int2* pairs;
    const long long *poff, *src_off, *keep_off, *kp_offsets;
    const unsigned *q, *t;
    const unsigned char* keep;
};
struct TracksOut {
    int64_t cap_obs;
    int32_t cap_tracks;
    int32_t* n_tracks;
    int64_t* n_obs;
    int64_t* track_ptr;
    uint32_t *obs_frame, *obs_kp;
    uint8_t* track_flags;
};

inline unsigned nblk(long long n) { return (unsigned)((n + TT - 1) / TT); }

// everything after the upload: `words` / `node_track` / `scratch` are the call's staged arrays, words_off where the words lie in the mirror
int tracks_run(eacham_ctx* ctx, IoStage& io, const TracksPlan& pl, const TracksGraphDev& g, int* words, size_t words_off, int* node_track,
               char* sc, int min_len, int policy, const TracksOut& out) {
    hipStream_t st = ctx->stream;
    const int n = (int)g.n_nodes, m = (int)g.n_matches;
    unsigned *parent = (unsigned*)(sc + pl.parent), *root = (unsigned*)(sc + pl.root), *eu = (unsigned*)(sc + pl.eu), *ev = (unsigned*)(sc + pl.ev);
    int *touched = (int*)(sc + pl.touched), *pos = (int*)(sc + pl.pos), *changed = words + W_CHANGED;
    volatile const int* pin = (volatile const int*)((char*)ctx->io_host + words_off);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ctx->profile) {
        EACHAM_HIP_TRY(ctx, hipEventCreate(&e0));
        EACHAM_HIP_TRY(ctx, hipEventCreate(&e1));
        EACHAM_HIP_TRY(ctx, hipEventRecord(e0, st));
    }
    struct Ev { hipEvent_t &a, &b; ~Ev() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev_guard{e0, e1};
    auto readback = [&]() -> int {
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync((char*)ctx->io_host + words_off, words, sizeof(int) * N_WORDS, hipMemcpyDeviceToHost, st));
        EACHAM_HIP_TRY(ctx, hipStreamSynchronize(st));
        ++ctx->tracks_readbacks;
        return EACHAM_OK;
    };
    EACHAM_HIP_TRY(ctx, hipMemsetAsync(words, 0, sizeof(int) * N_WORDS, st));
    tracks_init_kernel<<<nblk(n), TT, 0, st>>>(n, parent, root, touched, node_track);
    tracks_edges_kernel<<<nblk(m), TT, 0, st>>>(m, g.pairs, g.npairs, g.poff, g.src_off, g.keep_off, g.q, g.t, g.keep, g.kp_offsets, eu, ev, touched);
    prim::exclusive_scan<int>(st, touched, pos, n, (int*)(sc + pl.scan_ws), words + W_TOUCHED);
    int used = -1;
    for (int r = 0; used < 0;) {
        if (r >= pl.round_cap)
            return ctx->fail(EACHAM_ERR_HIP, "tracks: the components have not settled after %d rounds (cap for %lld touched nodes)", r, pl.tmax);
        const int nb = std::min(ROUND_BATCH, pl.round_cap - r);
        for (int b = 0; b < nb; ++b) {
            tracks_hook_kernel<<<nblk(m), TT, 0, st>>>(m, eu, ev, root, parent, changed, r + b);
            tracks_compress_kernel<<<nblk(n), TT, 0, st>>>(n, touched, parent, root, changed, r + b);
        }
        EACHAM_HIP_TRY(ctx, hipGetLastError());
        if (int rc = readback()) return rc;
        for (int b = 0; b < nb && used < 0; ++b)
            if (pin[W_CHANGED + r + b] == 0) used = r + b + 1;
        r += nb;
    }
    ctx->tracks_rounds = used;
    const int T = pin[W_TOUCHED];
    long long n_tracks = 0, n_obs = 0;
    if (T > 0) {
        uint32_t *ka = (uint32_t*)(sc + pl.ka), *kb = (uint32_t*)(sc + pl.kb), *va = (uint32_t*)(sc + pl.va), *vb = (uint32_t*)(sc + pl.vb);
        tracks_compact_kernel<<<nblk(n), TT, 0, st>>>(n, touched, pos, root, ka, va);
        if (prim::radix_sort_pairs<uint32_t>(st, ka, va, kb, vb, T, pl.key_bits, (int*)(sc + pl.sort_ws))) std::swap(ka, kb), std::swap(va, vb);
        int *head = (int*)(sc + pl.head), *run_start = (int*)(sc + pl.run_start), *run_conf = (int*)(sc + pl.run_conf);
        unsigned* frame = (unsigned*)(sc + pl.frame);
        prim::I3 *sel = (prim::I3*)(sc + pl.sel), *selx = (prim::I3*)(sc + pl.selx);
        tracks_heads_kernel<<<nblk(T), TT, 0, st>>>(T, ka, va, g.kp_offsets, g.n_frames, head, frame);
        prim::exclusive_scan<int>(st, head, head, T, (int*)(sc + pl.scan_ws), words + W_RUNS);
        EACHAM_HIP_TRY(ctx, hipMemsetAsync(run_conf, 0, sizeof(int) * (size_t)T, st));
        tracks_runs_kernel<<<nblk(T), TT, 0, st>>>(T, ka, head, frame, words, run_start, run_conf);
        tracks_select_kernel<<<nblk(T), TT, 0, st>>>(T, words, run_start, run_conf, min_len, policy, sel);
        prim::exclusive_scan<prim::I3>(st, sel, selx, T, (prim::I3*)(sc + pl.scan_ws3), (prim::I3*)(words + W_TOTALS));
        tracks_emit_kernel<<<nblk(T), TT, 0, st>>>(T, ka, va, head, frame, run_start, run_conf, sel, selx, g.kp_offsets, words,
                                                   (long long*)(sc + pl.o_ptr), (unsigned*)(sc + pl.o_frame), (unsigned*)(sc + pl.o_kp),
                                                   (unsigned char*)(sc + pl.o_flags), node_track);
        EACHAM_HIP_TRY(ctx, hipGetLastError());
        if (e1) EACHAM_HIP_TRY(ctx, hipEventRecord(e1, st));
        if (int rc = readback()) return rc;
        n_tracks = pin[W_TOTALS], n_obs = pin[W_TOTALS + 1];
    } else if (e1) {
        EACHAM_HIP_TRY(ctx, hipEventRecord(e1, st));
        EACHAM_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    if (e1) EACHAM_HIP_TRY(ctx, hipEventElapsedTime(&ctx->tracks_ms, e0, e1));
    *out.n_tracks = (int32_t)n_tracks;
    *out.n_obs = n_obs;
    if (n_obs > out.cap_obs || n_tracks > out.cap_tracks)
        return ctx->fail(EACHAM_ERR_CAPACITY, "tracks: %lld tracks with %lld observations, room for %d and %lld", n_tracks, n_obs,
                         (int)out.cap_tracks, (long long)out.cap_obs);
    if (n_tracks > 0) {
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(out.track_ptr, sc + pl.o_ptr, 8 * (size_t)(n_tracks + 1), hipMemcpyDeviceToHost, st));
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(out.obs_frame, sc + pl.o_frame, 4 * (size_t)n_obs, hipMemcpyDeviceToHost, st));
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(out.obs_kp, sc + pl.o_kp, 4 * (size_t)n_obs, hipMemcpyDeviceToHost, st));
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(out.track_flags, sc + pl.o_flags, (size_t)n_tracks, hipMemcpyDeviceToHost, st));
    }
    if (int rc = io.finish()) return rc;   // node_track, and the stream's synchronisation
    if (n_tracks == 0) out.track_ptr[0] = 0;
    return EACHAM_OK;
}

// what both entry points check of the arguments they share
int tracks_check_common(eacham_ctx* ctx, int min_len, int policy, int64_t cap_obs, int32_t cap_tracks, const TracksOut& o) {
    if (!o.n_tracks || !o.n_obs || !o.track_ptr) return ctx->fail(EACHAM_ERR_INVALID, "tracks: null n_tracks, n_obs or track_ptr");
    if (cap_obs < 0 || cap_tracks < 0) return ctx->fail(EACHAM_ERR_INVALID, "tracks: negative capacity");
    if ((cap_obs > 0 && (!o.obs_frame || !o.obs_kp)) || (cap_tracks > 0 && !o.track_flags))
        return ctx->fail(EACHAM_ERR_INVALID, "tracks: null observation or flag array with a capacity above 0");
    if (min_len < 2) return ctx->fail(EACHAM_ERR_INVALID, "tracks: min_len %d, a track has at least 2 observations", min_len);
    if (policy != 0 && policy != 1) return ctx->fail(EACHAM_ERR_INVALID, "tracks: unknown conflict_policy %d (0 = flag, 1 = drop)", policy);
    return EACHAM_OK;
}

// prim::radix_sort_pairs scans (segments x 2^10) histogram entries with int indices: 2^30 elements at most
int tracks_check_sort(eacham_ctx* ctx, long long n_nodes, long long m) {
    if (std::min<long long>(n_nodes, 2 * m) > (1ll << 30))
        return ctx->fail(EACHAM_ERR_CAPACITY, "tracks: %lld nodes and %lld matches can touch more than 2^30 nodes", n_nodes, m);
    return EACHAM_OK;
}

// a graph without a match: no device work
int tracks_empty(eacham_ctx* ctx, long long n_nodes, const TracksOut& o, int32_t* node_track) {
    ctx->tracks_rounds = 0;
    *o.n_tracks = 0;
    *o.n_obs = 0;
    o.track_ptr[0] = 0;
    if (node_track) std::fill(node_track, node_track + n_nodes, -1);
    return EACHAM_OK;
}

template <class Body>
int tracks_entry(eacham_ctx* ctx, Body body) {   // nothing may leave extern "C" (std::vector throws on an absurd size)
    std::lock_guard<std::mutex> lock(ctx->mu);
    try {
        ctx->tracks_rounds = ctx->tracks_round_cap = ctx->tracks_readbacks = 0;
        ctx->tracks_ms = -1.f;
        return body();
    } catch (const std::exception& e) {
        return ctx->fail(EACHAM_ERR_INVALID, "tracks: %s", e.what());
    } catch (...) {
        return ctx->fail(EACHAM_ERR_INVALID, "tracks: unknown exception");
    }
}

}  // namespace
}  // namespace eacham

using namespace eacham;

extern "C" int eacham_tracks_build(eacham_ctx* ctx, int n_frames, const int32_t* pairs, int npairs, const int32_t* counts,
                                   const int64_t* offsets, const uint32_t* q, const uint32_t* t, const int64_t* kp_offsets,
                                   const uint8_t* keep, int min_len, int conflict_policy, int64_t cap_obs, int32_t cap_tracks,
                                   int32_t* n_tracks, int64_t* n_obs, int64_t* track_ptr, uint32_t* obs_frame, uint32_t* obs_kp,
                                   uint8_t* track_flags, int32_t* node_track) {
    if (!ctx) return EACHAM_ERR_INVALID;
    return tracks_entry(ctx, [&]() -> int {
        const TracksOut out{cap_obs, cap_tracks, n_tracks, n_obs, track_ptr, obs_frame, obs_kp, track_flags};
        if (n_frames < 0 || npairs < 0 || !kp_offsets || (npairs > 0 && (!pairs || !counts || !offsets)))
            return ctx->fail(EACHAM_ERR_INVALID, "tracks_build: null graph array or negative size");
        if (int rc = tracks_check_common(ctx, min_len, conflict_policy, cap_obs, cap_tracks, out)) return rc;
        if (kp_offsets[0] != 0) return ctx->fail(EACHAM_ERR_INVALID, "tracks_build: kp_offsets[0] is %lld, not 0", (long long)kp_offsets[0]);
        for (int f = 0; f < n_frames; ++f)
            if (kp_offsets[f + 1] < kp_offsets[f]) return ctx->fail(EACHAM_ERR_INVALID, "tracks_build: kp_offsets decreases at frame %d", f);
        if (npairs > 0 && offsets[0] != 0) return ctx->fail(EACHAM_ERR_INVALID, "tracks_build: offsets[0] is %lld, not 0", (long long)offsets[0]);
        std::vector<long long> poff((size_t)npairs);   // the pairs' match lists one behind the other: what a flat launch over matches indexes
        long long m_packed = 0, m_src = 0;
        for (int p = 0; p < npairs; ++p) {
            const int f1 = pairs[2 * p], f2 = pairs[2 * p + 1];
            if (p > 0 && offsets[p] < offsets[p - 1]) return ctx->fail(EACHAM_ERR_INVALID, "tracks_build: offsets decreases at pair %d", p);
            if (counts[p] < 0) return ctx->fail(EACHAM_ERR_INVALID, "tracks_build: negative count at pair %d", p);
            if (f1 < 0 || f2 < 0 || f1 >= n_frames || f2 >= n_frames)
                return ctx->fail(EACHAM_ERR_INVALID, "tracks_build: pair %d names frame %d/%d of %d", p, f1, f2, n_frames);
            if (counts[p] > 0 && (!q || !t)) return ctx->fail(EACHAM_ERR_INVALID, "tracks_build: null match arrays");
            const long long n1 = kp_offsets[f1 + 1] - kp_offsets[f1], n2 = kp_offsets[f2 + 1] - kp_offsets[f2];
            for (long long k = offsets[p]; k < offsets[p] + counts[p]; ++k)
                if (q[k] >= n1 || t[k] >= n2) return ctx->fail(EACHAM_ERR_INVALID, "tracks_build: match %lld of pair %d is beyond its frame's keypoints", k, p);
            poff[p] = m_packed;
            m_packed += counts[p];
            m_src = std::max<long long>(m_src, offsets[p] + counts[p]);
        }
        const long long n_nodes = kp_offsets[n_frames];
        if (n_nodes > INT_MAX || m_packed > INT_MAX)
            return ctx->fail(EACHAM_ERR_CAPACITY, "tracks_build: %lld nodes and %lld matches, at most 2^31 - 1 of each in one call", n_nodes, m_packed);
        if (m_packed == 0 || n_nodes == 0) return tracks_empty(ctx, n_nodes, out, node_track);
        if (int rc = tracks_check_sort(ctx, n_nodes, m_packed)) return rc;
        EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
        const TracksPlan pl(n_nodes, m_packed);
        ctx->tracks_round_cap = pl.round_cap;
        IoStage io(ctx, ctx->stream);
        const auto h_words = io.out<int>(nullptr, N_WORDS);   // first: offset 0, always inside the pinned mirror
        const auto h_nt = io.out<int>(node_track, (size_t)n_nodes);
        const auto h_pairs = io.in<int2>(pairs, (size_t)npairs);
        const auto h_poff = io.in<long long>(poff.data(), (size_t)npairs), h_off = io.in<long long>(offsets, (size_t)npairs);
        const auto h_q = io.in<unsigned>(q, (size_t)m_src), h_t = io.in<unsigned>(t, (size_t)m_src);
        const auto h_kpo = io.in<long long>(kp_offsets, (size_t)n_frames + 1);
        const auto h_keep = io.in<unsigned char>(keep, keep ? (size_t)m_src : 0);
        const auto h_sc = io.scratch<char>(pl.total);
        IoDev d;
        if (int rc = io.upload(d)) return rc;
        const TracksGraphDev g{n_frames, npairs, n_nodes, m_packed, d(h_pairs), d(h_poff), d(h_off), d(h_off), d(h_kpo), d(h_q), d(h_t),
                               keep ? d(h_keep) : nullptr};
        return tracks_run(ctx, io, pl, g, d(h_words), io.lay.off[h_words.k], d(h_nt), d(h_sc), min_len, conflict_policy, out);
    });
}

// eacham_graph_tracks / eacham_graph_tracks_verified: `keep_dev` is a mask already on the device (the one a verify call retained), else
// `keep` is the caller's host array or null
static int graph_tracks_run(eacham_graph* gr, const uint8_t* keep, const unsigned char* keep_dev, int min_len, int conflict_policy, int64_t cap_obs,
                            int32_t cap_tracks, int32_t* n_tracks, int64_t* n_obs, int64_t* track_ptr, uint32_t* obs_frame, uint32_t* obs_kp,
                            uint8_t* track_flags, int32_t* node_track) {
    eacham_ctx* ctx = gr->ctx;
    const TracksOut out{cap_obs, cap_tracks, n_tracks, n_obs, track_ptr, obs_frame, obs_kp, track_flags};
    if (int rc = tracks_check_common(ctx, min_len, conflict_policy, cap_obs, cap_tracks, out)) return rc;
    if (gr->n_kp > INT_MAX || gr->n_matches > INT_MAX)
        return ctx->fail(EACHAM_ERR_CAPACITY, "graph_tracks: %lld nodes and %lld matches, at most 2^31 - 1 of each in one call", gr->n_kp, gr->n_matches);
    if (gr->n_matches == 0 || gr->n_kp == 0) return tracks_empty(ctx, gr->n_kp, out, node_track);
    if (int rc = tracks_check_sort(ctx, gr->n_kp, gr->n_matches)) return rc;
    EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const TracksPlan pl(gr->n_kp, gr->n_matches);
    ctx->tracks_round_cap = pl.round_cap;
    IoStage io(ctx, ctx->stream);
    const auto h_words = io.out<int>(nullptr, N_WORDS);
    const auto h_nt = io.out<int>(node_track, (size_t)gr->n_kp);
    const auto h_keep = io.in<unsigned char>(keep, keep && !keep_dev ? (size_t)gr->n_src : 0);
    const auto h_sc = io.scratch<char>(pl.total);
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    // the resident match lists are packed in edge order (offsets); src_offsets says where each began in the arrays `keep` indexes
    const TracksGraphDev g{gr->n_frames, gr->n_edges, gr->n_kp, gr->n_matches, gr->pairs, gr->offsets, gr->offsets, gr->src_offsets,
                           gr->kp_offsets, gr->q, gr->t, keep_dev ? keep_dev : keep ? d(h_keep) : nullptr};
    return tracks_run(ctx, io, pl, g, d(h_words), io.lay.off[h_words.k], d(h_nt), d(h_sc), min_len, conflict_policy, out);
}

extern "C" int eacham_graph_tracks(eacham_graph* gr, const uint8_t* keep, int min_len, int conflict_policy, int64_t cap_obs,
                                   int32_t cap_tracks, int32_t* n_tracks, int64_t* n_obs, int64_t* track_ptr, uint32_t* obs_frame,
                                   uint32_t* obs_kp, uint8_t* track_flags, int32_t* node_track) {
    if (!gr) return EACHAM_ERR_INVALID;
    return tracks_entry(gr->ctx, [&]() -> int {
        return graph_tracks_run(gr, keep, nullptr, min_len, conflict_policy, cap_obs, cap_tracks, n_tracks, n_obs, track_ptr, obs_frame, obs_kp,
                                track_flags, node_track);
    });
}

extern "C" int eacham_graph_tracks_verified(eacham_graph* gr, int min_len, int conflict_policy, int64_t cap_obs, int32_t cap_tracks,
                                            int32_t* n_tracks, int64_t* n_obs, int64_t* track_ptr, uint32_t* obs_frame, uint32_t* obs_kp,
                                            uint8_t* track_flags, int32_t* node_track) {
    if (!gr) return EACHAM_ERR_INVALID;
    return tracks_entry(gr->ctx, [&]() -> int {
        if (!gr->has_keep) return gr->ctx->fail(EACHAM_ERR_INVALID, "graph_tracks_verified: no verify call has retained a mask in this graph");
        return graph_tracks_run(gr, nullptr, gr->keep_mask, min_len, conflict_policy, cap_obs, cap_tracks, n_tracks, n_obs, track_ptr, obs_frame,
                                obs_kp, track_flags, node_track);
    });
}

extern "C" int eacham_tracks_debug_last(eacham_ctx* ctx, int32_t* rounds, int32_t* round_cap, int32_t* readbacks, float* kernel_ms) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (rounds) *rounds = ctx->tracks_rounds;
    if (round_cap) *round_cap = ctx->tracks_round_cap;
    if (readbacks) *readbacks = ctx->tracks_readbacks;
    if (kernel_ms) *kernel_ms = ctx->tracks_ms;
    return EACHAM_OK;
}
