// context.hpp — per-device context shared by the matcher and the bundle adjuster.
// One context = one HIP device + one stream; the C-ABI in include/eacham_hip.h serialises calls on
// a context with `mu` so the reference's concurrent Match() pattern (apps/sfm/main.cpp:98-109)
// stays legal.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstring>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/eacham_hip.h"
#include "io_layout.hpp"

namespace eacham {

// What the resident frames hold. All frames of a context are of one kind (eacham_ctx::kind_common) and one k-step class.
enum FrameKind {
    FRAME_INT8 = 0,       // int8 fragments (matcher.hip)
    FRAME_F32 = 1,        // fp32 fragments (matcher_f32.hip)
    FRAME_BITS = 2,       // binary rows as int8 fragments of 0 / 255 (matcher_ham.hip): the int8 kernels under the Hamming predicate
    FRAME_BITS_WIDE = 3,  // wide binary rows as FP4 fragments of +-1 (matcher_ham_wide.hip): a Hamming sweep of their own
};

// The context's small block of device words (eacham_ctx::flag_dev), zeroed at create. Kernels receive plain pointers to its members.
struct FlagBlock {
    int not_integer;                  // a non-integer descriptor was seen by an int8 upload
    int bad_pair;                     // a device-side pair list named a frame that is not resident
    int pad0[6];
    int standin_meta[8];              // meta of the empty stand-in frame (zeros)
    int standin_rows[16];             // its orig / pos (zeros, never indexed: the frame has no row)
    unsigned long long colprune[2];   // {settled, verified} candidate columns of the last matching call (eacham_match_debug_colprune)
    int pad1[4];
    unsigned long long dot16[6];      // the tally of the screened dot-product form
    unsigned long long screen[3];     // {real query rows, rows left open} of the last call's screen sweeps (eacham_match_debug_screen),
                                      // {items the exact pass took them in} (eacham_match_debug_screen_items)
    int pad2[6];
};
static_assert(offsetof(FlagBlock, bad_pair) == 1 * sizeof(int) && offsetof(FlagBlock, standin_meta) == 8 * sizeof(int) &&
                  offsetof(FlagBlock, standin_rows) == 16 * sizeof(int) && offsetof(FlagBlock, colprune) == 32 * sizeof(int) &&
                  offsetof(FlagBlock, dot16) == 40 * sizeof(int) && offsetof(FlagBlock, screen) == 52 * sizeof(int) &&
                  sizeof(FlagBlock) == 64 * sizeof(int),
              "the block's words stay where the kernels and the debug calls have always found them");

// Descriptor of one resident frame as the kernels see it (device-side table entry).
// int8 frames are stored PARITY-SORTED: rows whose centred squared norm is even come first (stable),
// padded to whole 32-row tiles, then the odd ones; `orig`/`pos` translate between stored position
// and the caller's row index (see matcher.hip). fp32 frames keep the caller's order (orig = pos = null).
struct FrameDev {
    const int4* frag;  // [ntiles][KS][64] 16-byte MFMA operand fragments (int8, centred by -128)
    const int* norm;   // int8: floor(|c|^2 / 2) per stored position (query role, MFMA C-init); fp32: |x|^2 as float bits
    const int* normb;  // int8: floor(|c|^2 / 2) + sum(c) per stored position (train role)
    const int* orig;   // int8: stored position -> caller's row (-1 = padding)
    const int* pos;    // int8: caller's row -> stored position
    const int* meta;   // int8: {tiles of the even class, tiles in use, above 128-D: tiles that hold a real row}; written by the upload kernels
    const int4* screen;  // int8 frames above 128-D: the FP6 image of the screen sweep (matcher.hip, match_screen.hpp), at the same stored
                         // positions and tiles: [ntiles][4 k-steps]{64 x 16 B | 64 x 8 B} | |M|^2 / 2 as float [32 ntiles] | s_r [32 ntiles] | {E}; else null
    int n;             // real rows
    int ntiles;        // allocated 32-row tiles (upper bound of meta[1] for int8 frames)
    int resident;      // 0: no descriptors uploaded under this id (device-side pair lists naming it are neutralised)
};

struct FrameHost {
    int4* frag = nullptr;
    int* norm = nullptr;   // one allocation: norm | normb | orig | pos | scratch (int8 path)
    int* normb = nullptr;
    int* orig = nullptr;
    int* pos = nullptr;
    int* meta = nullptr;
    int4* screen = nullptr;  // the FP6 image of a frame above 128-D: the tail of frag's allocation
    unsigned* bits = nullptr;  // binary frames: the packed rows in the caller's order, zero-padded to 8 words per row (matcher_ham.hip: the
                               // tail of norm's allocation) or 16 (matcher_ham_wide.hip: the tail of frag's). The kernels reach it through
                               // a table of its own (eacham_ctx::bits_table_dev), not through FrameDev
    int n = -1;  // -1 = not resident
    int dim = 0;
    int ks = 0;
    int ntiles = 0;      // allocated tiles
    int tiles_used = 0;  // tiles in use (<= ntiles), known after sync_frame_table
    // fp16 image of an fp32 frame (matcher_dot16.hip): one allocation, fragments | norm bounds | {max bound, flag}; built on the
    // frame's first screened call, freed with frag (release_frame)
    void* img16 = nullptr;
    bool img16_ready = false;   // built (or nothing to build: an empty frame)
    bool img16_bad = false;     // holds a value that is not finite or beyond the fp16 range: its pairs run the fp32 tile kernel
    float img16_maxn = 0.0f;    // max of the per-row norm bounds
};

// One arena of the bundle adjuster: every device array of a prepared problem is carved out of ONE allocation, and the
// arena (with its block of pinned host scalars) goes back to the context's pool when the problem is released. The
// reference calls RefineBA for a new local window after every frame (apps/sfm/main.cpp:207): ~60 hipMalloc + hipFree +
// a pinned allocation per call were 0.8 ms of a 1.9 ms window.
struct BaBlock {
    void* dev = nullptr;
    size_t bytes = 0;
    double* pinned = nullptr;
    bool busy = false;
};

// Scratch of the device-side problem construction (temporaries of its sorts and scans): kept with the context, grown on demand.
struct BaScratch {
    void* dev = nullptr;
    size_t bytes = 0;
};

struct ProfileSlot {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t used = 0;
    int64_t launches = 0;
    double total_ms = 0.0;
};

}  // namespace eacham

struct eacham_ctx {
    int device = 0;
    int cus = 256;   // compute units of the device (read at create): sizes the persistent grids that are a share of the chip
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;   // finalize/compaction of batch i runs here beside the tile kernel of batch i+1
    hipEvent_t ev_tile[2] = {nullptr, nullptr}, ev_fin[2] = {nullptr, nullptr}, ev_join = nullptr;
    std::mutex mu;
    std::string err;

    // descriptor store
    std::vector<eacham::FrameHost> frames;
    eacham::FrameDev* frame_table_dev = nullptr;
    int frame_table_cap = 0;
    bool frame_table_dirty = true;
    eacham::FlagBlock* flag_dev = nullptr;   // the flags, the stand-in frame's arrays and the tallies of the debug calls
    int ks_common = 0;        // k-step class shared by all resident frames (0 = none yet)
    eacham::FrameKind kind_common = eacham::FRAME_INT8;   // their kind (meaningful while ks_common != 0)
    const unsigned** bits_table_dev = nullptr;  // [frames + 1] the frames' packed rows (FrameHost::bits; null: none), rebuilt when dirty
    int bits_table_cap = 0;
    bool bits_table_dirty = true;
    // wide binary frames (matcher_ham_wide.hip): FrameHost::frag is the FP4 image with the packed rows (FrameHost::bits, 16 words per
    // row) behind it; every per-row array of FrameDev is null. ks_common is their k-step count (1..8)
    int wide_bytes_common = 0;           // bytes per row shared by the resident wide frames (0: the frames are of another kind)
    size_t wide_budget_bytes = 0;        // EACHAM_MATCH_BUDGET_MB as this path reads it: any positive value, fractions included (0: match_budget_mb)
    long long wide_debug[4] = {0, 0, 0, 0};  // {batches, pairs per batch, sweep launches, query rows swept} of the last wide matching call
    void* table16_dev = nullptr;   // device table of the frames' fp16 images (matcher_dot16.hip), rebuilt by every screened call
    int table16_cap = 0;
    long long dot16_fallback_pairs = 0;  // pairs of the last screened call that ran the fp32 tile kernel (eacham_match_debug_dot_screen)

    // matcher workspace (grown on demand, never inside a timed launch sequence after warm-up)
    void* ws = nullptr;
    size_t ws_bytes = 0;
    int2* pairs_safe = nullptr;  // sanitised copy of the caller's device-side pair list
    int pairs_safe_cap = 0;
    void* io = nullptr;  // staging for the host-pointer entry points
    size_t io_bytes = 0;
    void* io_host = nullptr;  // pinned mirror of the head of `io`: the small arrays of a call travel as ONE copy each way (IoStage)
    size_t io_host_bytes = 0;

    std::vector<eacham::BaBlock> ba_pool;  // arenas of released BA problems, reused by the next eacham_ba_prepare
    eacham::BaScratch ba_scratch[4];
    int ba_prepare_mode = 0;  // EACHAM_BA_PREPARE=host|device (diagnostic / tests: force one form of the structure construction;
                              // default: device for >= 65536 observations), read at create
    int stream2_attempt = -1;        // which candidate of the second-stream search was kept (0..4; 4 = the last, kept unprobed; -1 = no search)
    float stream2_lead_ms = -1.f;    // how long before the spin's end the probe on it finished (> 0.010: a hardware queue of its own)
    bool io_busy = false;            // an IoStage call has not reached its finish(): copies out of the pinned mirror may be in flight
    bool ba_groups_lds_set = false;  // ba_schur_groups has been granted its dynamic LDS size on this context's device
    int ba_group_rows = 0;    // EACHAM_BA_GROUP_ROWS=<n> (diagnostic): rows per landmark group instead of ba_groups.hpp's choice
    int ba_schur_mode = 0;    // EACHAM_BA_SCHUR=groups|pairs (diagnostic / tests). 0 = by problem size: the landmark groups of ba_groups.hpp for the
                              // problems eacham_ba_prepare builds on the device, the pair lists of rounds 1-4 (ba_schur_pairs) for the
                              // small ones it builds with host loops (a local window: building the group structure on the host costs
                              // more than the 13 us per LM iteration it saves there); 1 = groups whenever they apply, 2 = always pairs.
                              // Any other value means 0: the retired =dense (docs/HISTORY.md) now gives a local window its default, the pair lists
    int ba_ordering = 0;  // EACHAM_BA_ORDERING=natural|rcm|nd read ONCE at eacham_ctx_create (diagnostic override of
                          // eacham_ba_problem.ordering == AUTO); nothing on the solve path reads the environment
    int match_sweep_form = 0;         // EACHAM_MATCH_SWEEP_FORM=exact|bound|screen (diagnostic A/B, tests): the lean form's row sweep keeps every row's exact top-2 (1),
                                      // runs its bound form + the exact pass over the rows left open (2), or screens the rows on the FP6 image where the frames
                                      // have one, with the same exact pass (3); 0 = by descriptor dimension (bound up to 128-D, screen above)
    bool guided_screen = true;        // EACHAM_GUIDED_SCREEN=0 (A/B, tests): match_guided.hip's exact gate runs its divisions for every element, no screen in front
    bool match_colprune = true;       // EACHAM_MATCH_COLPRUNE=0 (A/B, tests): no candidate column is settled from the sweep's row minima, all go to match_colverify_kernel
    int match_budget_mb = 1024;     // EACHAM_MATCH_BUDGET_MB (diagnostic: workspace budget of one batch of pairs), read at create
    bool match_no_overlap = false;  // EACHAM_NO_OVERLAP (diagnostic: finalize on the tile kernel's stream), read at create

    // the last track-building call (tracks.hip; eacham_tracks_debug_last): hook-and-compress rounds it ran until one changed nothing,
    // its cap, the read-backs of device words it made, and (profiling on) the device time between its upload and its copies back
    int tracks_rounds = 0, tracks_round_cap = 0, tracks_readbacks = 0;
    float tracks_ms = -1.f;
    // the last threshold-RANSAC call (ransac_batch.hip; eacham_ransac_debug_last): the samples it solved over both passes and the host
    // milliseconds it spent building the budget rows
    long long ransac_solved = 0;
    double ransac_table_ms = 0.0;

    // profiling
    bool profile = false;
    eacham::ProfileSlot prof[EACHAM_KERNEL_COUNT];

    int fail(int code, const char* fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
};

// The resident CSR match graph (graph.hip builds and queries it, tracks.hip forms tracks on it): the edges are the pairs with
// matches, compacted, their match lists packed in pair order.
struct eacham_graph {
    eacham_ctx* ctx = nullptr;
    int n_frames = 0, n_edges = 0;       // edges = pairs with matches
    long long n_matches = 0, n_kp = 0;
    long long n_src = 0;                 // matches the caller's arrays spanned (max offsets + counts): the length of a `keep` mask
    char* dev = nullptr;
    int2* pairs = nullptr;
    int* counts = nullptr;
    long long* offsets = nullptr;
    unsigned *q = nullptr, *t = nullptr, *edge_counts = nullptr, *best = nullptr;
    unsigned char *valid = nullptr, *excluded = nullptr, *has3d = nullptr;
    long long* kp_offsets = nullptr;
    long long* src_offsets = nullptr;    // per edge: where its match list began in the caller's arrays
    std::vector<long long> kp_offsets_h;
    // what the geometric verification adds (graph_verify.hip: a PROBLEM is a caller pair, in the caller's order)
    int npairs = 0;                      // caller pairs, those without matches included
    std::vector<int> pair_counts_h;      // [npairs] the caller's counts
    std::vector<int> pairs_h;            // [npairs x 2] the caller's pairs, those without matches included (match_guided.hip)
    long long* pair_ptr = nullptr;       // [npairs + 1] where each caller pair's matches begin in the packed lists (a pair without matches owns none)
    double* xy = nullptr;                // [n_kp x 2] pixel coordinates (eacham_graph_set_keypoints), an allocation of its own
    bool has_xy = false;
    unsigned char* keep_mask = nullptr;  // [n_src] the inlier mask a verify call retained, an allocation of its own
    bool has_keep = false;
};

#define EACHAM_HIP_TRY(ctx, expr)                                                              \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return (ctx)->fail(EACHAM_ERR_HIP, "%s failed: %s (%s:%d)", #expr,                 \
                               hipGetErrorString(e_), __FILE__, __LINE__);                     \
    } while (0)

namespace eacham {

int ensure_workspace(eacham_ctx* ctx, size_t bytes);
int ensure_io(eacham_ctx* ctx, size_t bytes);
int ensure_io_host(eacham_ctx* ctx, size_t bytes);

// The host-pointer entry points of the estimators, the triangulation and the graph query are called once or more per frame of
// the incremental loop with a handful of small arrays each way (points, a few models, counts): as separate copies from pageable
// memory every one of them is a submission and a wait of ~10 us (25 copies per solvePnPRansac of the loop). IoStage is how such a
// call stages its arrays through ctx->io. Each array is declared ONCE — element type, element count, role — and yields a typed
// handle; io_layout.hpp places them. upload() sizes the staging buffer and its pinned mirror (which covers everything before the
// device-only group), lays the inputs that are small into the mirror at the SAME offsets and moves them in one copy (the bytes
// between two packed arrays travel along); arrays above PACK_MAX keep their own direct copy. It hands back the IoDev that turns
// a handle into its device pointer — not before, since growing ctx->io moves it. finish() brings the results back the same way.
template <class T>
struct IoArray { int k; };
struct IoDev {
    char* base = nullptr;
    const size_t* off = nullptr;
    template <class T>
    T* operator()(IoArray<T> h) const { return (T*)(base + off[h.k]); }
};
struct IoStage {
    static constexpr size_t PACK_MAX = 256 * 1024;
    eacham_ctx* ctx;
    hipStream_t st;
    IoLayout lay;
    void* host[IoLayout::MAX_ARRAYS];   // the caller's array: source of an input, destination of a result; null = not copied
    char* dev = nullptr;
    size_t in_lo = ~(size_t)0, in_hi = 0, out_lo = ~(size_t)0, out_hi = 0;
    size_t direct_lo = ~(size_t)0, direct_hi = 0;  // what has been copied directly so far: a packed span must not cover it
    int packed[IoLayout::MAX_ARRAYS], n_packed = 0;   // the arrays of the packed span being gathered
    IoStage(eacham_ctx* c, hipStream_t s) : ctx(c), st(s) {}

    // A null input still owns its bytes (the kernels' optional K, in_mask); a null result is not brought back.
    template <class T>
    IoArray<T> in(const void* src, size_t count) { return add<T>(IO_IN, const_cast<void*>(src), count); }
    template <class T>
    IoArray<T> out(void* dst, size_t count) { return add<T>(IO_OUT, dst, count); }
    template <class T>
    IoArray<T> scratch(size_t count) { return add<T>(IO_DEV, nullptr, count); }   // never leaves the device

    int upload(IoDev& d) {
        if (lay.overflow) return ctx->fail(EACHAM_ERR_CAPACITY, "more than %d staged arrays in one call", IoLayout::MAX_ARRAYS);
        lay.place();
        if (int rc = ensure_io(ctx, lay.total)) return rc;
        if (int rc = ensure_io_host(ctx, lay.cut)) return rc;
        dev = (char*)ctx->io;
        // a call that returned on an error may have left a copy out of the mirror in flight: wait before writing into it again
        if (ctx->io_busy) (void)hipStreamSynchronize(st);
        ctx->io_busy = true;
        for (int k = 0; k < lay.n; ++k) {
            const size_t off = lay.off[k], bytes = lay.bytes[k];
            if (lay.role[k] != IO_IN || !host[k] || bytes == 0) continue;
            if (bytes <= PACK_MAX && off + bytes <= ctx->io_host_bytes) {
                memcpy((char*)ctx->io_host + off, host[k], bytes);
                in_lo = std::min(in_lo, off), in_hi = std::max(in_hi, off + bytes);
                packed[n_packed++] = k;
                continue;
            }
            // (what has been packed so far goes first; the direct copy is remembered: a later packed span that would cover it — the
            // gaps of the mirror hold stale bytes — is sent piece by piece instead)
            if (int rc = flush_in()) return rc;
            EACHAM_HIP_TRY(ctx, hipMemcpyAsync(dev + off, host[k], bytes, hipMemcpyHostToDevice, st));
            direct_lo = std::min(direct_lo, off), direct_hi = std::max(direct_hi, off + bytes);
        }
        if (int rc = flush_in()) return rc;
        d.base = dev, d.off = lay.off;
        return EACHAM_OK;
    }
    int finish() {   // one copy back, the stream's synchronisation, the hand-over to the caller's arrays
        n_packed = 0;
        for (int k = 0; k < lay.n; ++k) {
            const size_t off = lay.off[k], bytes = lay.bytes[k];
            if (lay.role[k] != IO_OUT || !host[k] || bytes == 0) continue;
            if (bytes <= PACK_MAX && off + bytes <= ctx->io_host_bytes) {
                packed[n_packed++] = k;
                out_lo = std::min(out_lo, off), out_hi = std::max(out_hi, off + bytes);
            } else {
                EACHAM_HIP_TRY(ctx, hipMemcpyAsync(host[k], dev + off, bytes, hipMemcpyDeviceToHost, st));
            }
        }
        if (out_hi > out_lo) EACHAM_HIP_TRY(ctx, hipMemcpyAsync((char*)ctx->io_host + out_lo, dev + out_lo, out_hi - out_lo, hipMemcpyDeviceToHost, st));
        EACHAM_HIP_TRY(ctx, hipStreamSynchronize(st));
        for (int j = 0; j < n_packed; ++j) memcpy(host[packed[j]], (char*)ctx->io_host + lay.off[packed[j]], lay.bytes[packed[j]]);
        ctx->io_busy = false;  // (an early error return leaves it set: the next upload() waits for the stream first)
        return EACHAM_OK;
    }

private:
    template <class T>
    IoArray<T> add(int role, void* p, size_t count) {
        const int k = lay.add(role, sizeof(T) * count);
        host[k] = p;
        return IoArray<T>{k};
    }
    int flush_in() {
        if (in_hi > in_lo) {
            if (in_lo < direct_hi && direct_lo < in_hi) {
                for (int j = 0; j < n_packed; ++j)
                    EACHAM_HIP_TRY(ctx, hipMemcpyAsync(dev + lay.off[packed[j]], (char*)ctx->io_host + lay.off[packed[j]], lay.bytes[packed[j]], hipMemcpyHostToDevice, st));
            } else {
                EACHAM_HIP_TRY(ctx, hipMemcpyAsync(dev + in_lo, (char*)ctx->io_host + in_lo, in_hi - in_lo, hipMemcpyHostToDevice, st));
            }
        }
        in_lo = ~(size_t)0, in_hi = 0, n_packed = 0;
        return EACHAM_OK;
    }
};
int sync_frame_table(eacham_ctx* ctx);
// copies `pairs` into the workspace tail with every pair that names a missing frame redirected to the empty
// stand-in entry frames[n_frames] (and flags it); returns the sanitised device pointer in *out
int sanitize_pairs(eacham_ctx* ctx, const int2* pairs_dev, int npairs, const int2** out);

// The life of a frame slot (context.hip), the same under every kind's upload.
// open_frame_slot: what every upload checks before it allocates, in the order the error codes have always had — the id and the row
// count (INVALID), then what this build does not take (UNSUPPORTED): ks == 0 says the uploader found no class for the row size,
// n > max_rows, a kind, class or (wide frames) bytes per row other than the resident frames'. Then the table grows to hold the id
// and whatever the slot held is released behind a synchronisation. *slot is the empty slot; nothing changed if the call fails.
int open_frame_slot(eacham_ctx* ctx, int frame_id, FrameKind kind, int n, int max_rows, int ks, int wide_bytes, FrameHost** slot);
// the only place that frees a frame's allocations (frag, norm and what shares them, the fp16 image); the caller has synchronised
void release_frame(FrameHost& f);
// hands the finished frame over: its shape, the context's common kind / class / wide row bytes, both device tables marked stale
void commit_frame(eacham_ctx* ctx, FrameHost& f, FrameKind kind, int n, int dim, int ks, int ntiles, int wide_bytes);

// matcher_f32.hip
int upload_frame_f32(eacham_ctx* ctx, int frame_id, const float* src_dev, int n, int dim);
int run_match_f32(eacham_ctx* ctx, const int2* pairs_dev, int npairs, double ratio, int min_dir, int min_mutual, int mode,
                  int* counts_dev, long long* offsets_dev, uint2* edges_dev, long long edge_cap, long long* total_dev,
                  int4* stats_dev);
// How the float path cuts a job into launches and lays one launch's arrays into the workspace (both of its forms, L2 and dot
// product): match_plan.hpp, here for the resident frames
struct MatchPlanF32;
struct F32Arrays;
MatchPlanF32 plan_match_f32(const eacham_ctx* ctx, int npairs);
// matcher_dot.hip
int run_match_dot(eacham_ctx* ctx, const int2* pairs_dev, int npairs, float min_score, int min_dir, int min_mutual, int mode,
                  int* counts_dev, long long* offsets_dev, uint2* edges_dev, float* scores_dev, long long edge_cap,
                  long long* total_dev, int4* stats_dev);
// the launches of run_match_dot, shared with the screened form: the fp32 tile kernel over nb pairs, and finalize + scan + compaction
void launch_match_tile_dot(eacham_ctx* ctx, const int2* pb, int nb, const MatchPlanF32& pl, int2* rr, int2* cp);
int launch_match_dot_tail(eacham_ctx* ctx, const MatchPlanF32& pl, const F32Arrays& a, const int2* pb, int nb, int first, bool is_last,
                          float min_score, int min_dir, int min_mutual, int mode, int* counts_dev, long long* offsets_dev,
                          uint2* edges_dev, float* scores_dev, long long edge_cap, long long* total_dev, int4* stats_dev);
// matcher_dot16.hip
void free_frame_image16(FrameHost& f);
int prepare_match_dot_screened(eacham_ctx* ctx, const int32_t* pairs, int npairs, int32_t* pairs_fb, int* n_fallback);
int run_match_dot_screened(eacham_ctx* ctx, const int2* pairs_dev, const int2* pairs_fb_dev, const int32_t* pairs_fb_host, int npairs,
                           int n_fallback, float min_score, int min_dir, int min_mutual, int* counts_dev, long long* offsets_dev,
                           uint2* edges_dev, float* scores_dev, long long edge_cap, long long* total_dev, int4* stats_dev);
// matcher_ham.hip: binary descriptors. The packed rows are expanded on the device to the 0 / 255 rows the int8 upload takes, kept
// packed beside the frame (both binary kinds: 8 or 16 words per row), and give every emitted match its Hamming distance (popcount
// of the XOR, independent of the sweep): hamming_distances is the one place that computes it, for the frames of either kind.
void launch_bits_expand(eacham_ctx* ctx, const unsigned char* packed_dev, int n, int bytes_per_row, int dim, float* dst_dev);
void launch_bits_store(eacham_ctx* ctx, const unsigned char* packed_dev, int n, int bytes_per_row, int words_per_row, unsigned* bits_dev);
int hamming_distances(eacham_ctx* ctx, const int2* pairs_dev, int npairs, const long long* offsets_dev, const long long* total_dev,
                      const uint2* edges_dev, long long edge_cap, int* dist_dev);
// matcher_ham_wide.hip: binary rows of up to 64 bytes as a kind of their own, swept on the FP4 matrix cores. *pairs_used: the
// sanitised list the kernels ran on (what hamming_distances indexes the frames with)
int upload_frame_bits_wide(eacham_ctx* ctx, int frame_id, const unsigned char* packed_dev, int n, int bytes_per_row);
int run_match_ham_wide(eacham_ctx* ctx, const int2* pairs_dev, int npairs, double ratio, int min_dir, int min_mutual, int mode,
                       int* counts_dev, long long* offsets_dev, uint2* edges_dev, long long edge_cap, long long* total_dev,
                       int4* stats_dev, const int32_t* pairs_host, const int2** pairs_used);
int ham_wide_debug_pair(eacham_ctx* ctx, int f1, int f2, int32_t* best, int32_t* h0, int32_t* h1, int cap);
// matcher.hip
int check_integer_flag(eacham_ctx* ctx);   // the sticky "a descriptor was not an integer" flag of the int8 uploads, read and cleared
void launch_scan_counts(eacham_ctx* ctx, const int* counts, int n, long long* offsets, long long* total, int first, int is_last);
void launch_compact_edges(eacham_ctx* ctx, int nb, const uint2* matches, const int* counts, const long long* offsets,
                          int row_stride, uint2* edges, long long edge_cap);

// RAII: records a start/stop HIP event pair around a launch sequence when profiling is on.
struct ProfileScope {
    eacham_ctx* ctx;
    int id;
    hipEvent_t stop = nullptr;
    hipStream_t stream;
    bool range = false;  // a ROCTx range is open (EACHAM_ROCTX=1)
    ProfileScope(eacham_ctx* c, int kernel_id, hipStream_t on = nullptr);
    ~ProfileScope();
};

}  // namespace eacham
