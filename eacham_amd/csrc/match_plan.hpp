// How the matching drivers cut a job into launches and lay a launch's arrays into the device workspace. Host-only arithmetic on
// plain numbers (no eacham_ctx, no HIP header): compiled alone with g++ and executed by tests/test_match_plan.py through
// tests/cpp/match_plan_driver.cpp. Every layout is ONE walk of a carver (ws_carve.hpp) over its arrays: with a null base it gives
// the bytes, with the workspace the typed pointers the launches take.
#pragma once

#include "ws_carve.hpp"

#include <algorithm>
#include <cstddef>

#if defined(__HIPCC__)
#define EACHAM_PLAN_HD __host__ __device__
#else
#define EACHAM_PLAN_HD
// the vector types of the device arrays, as far as a layout needs them: their sizes
struct alignas(8) int2 { int x, y; };       struct alignas(8) uint2 { unsigned x, y; };       struct alignas(8) float2 { float x, y; };
struct alignas(16) int4 { int x, y, z, w; };  struct alignas(16) uint4 { unsigned x, y, z, w; };
#endif

namespace eacham {

// 32-row tiles of a frame that one workgroup sweeps (the kernels' files assert them against their own constants)
constexpr int PLAN_WG_TILES = 8;        // matcher.hip: ROWS_PER_WG / 32
constexpr int PLAN_CHUNK_TILES = 128;   // matcher.hip: column tiles one sweep can tag in a key
constexpr int PLAN_F32_WG_TILES = 4;    // matcher_f32.hip, matcher_dot.hip: one per wave
constexpr int PLAN_HW_WG_TILES = 8;     // matcher_ham_wide.hip

// ---- the int8 kinds (run_match_metric) --------------------------------------------------------------------------------------
struct MatchPlanIn {
    int max_tiles;     // 32-row tiles of the largest resident frame
    int npairs;
    size_t budget;     // bytes of one workspace slot
    bool full_cols;    // every column's top-2 from the sweep (per-pair statistics, other thresholds) / the candidate-only column pass
    bool no_overlap;   // diagnostic switch: one slot
};

struct SlotCounters {   // a slot's 256-byte block of device counters, zeroed by one memset ahead of a launch's tail
    int n_items, pad0[7];    // items of the candidate column pass
    int n_pre, pad1[7];      // items of the exact pass over the open rows of the bound form
    int n_aitems, pad2[15];  // items of the arg-min pass
};
static_assert(sizeof(SlotCounters) == 32 * sizeof(int), "the kernels' counters lie at ints 0, 8 and 16 of 32");

struct Slot {   // the arrays of one launch in its workspace slot; an array its form does not have is null
    uint4* rowres;
    uint2* colpart;
    uint2* matches;
    // the candidate-only column pass
    uint2* rowcand;
    int* candlist;
    uint2* colres;
    int4* state;
    int2* items;
    SlotCounters* counters;
    int* bytile;
    int4* aitems;
    int* openlist;
    unsigned long long* openmask;   // the screen sweep's open-row masks
};

struct MatchPlan {
    int max_tiles;
    bool full_cols;
    int batch;       // pairs per launch
    int round_pairs; // pairs of one round of 512 workgroups (launches are sized in whole rounds)
    int tail_pairs;  // the job's short last launch holds this many pairs at the most
    int full_launches, full_rounds, long_launches;   // the cut of a job through two slots (make_plan, next_batch)
    int wb_stride;   // wave-blocks per frame (max over resident frames)
    int row_stride;  // padded rows per frame (max)
    int wgs_per_pair;
    int col_chunks;  // sweeps of <= 4096 train rows per pair
    int mask_stride; // 64-bit words per pair of the screen sweep's open-row masks: one per wave-block
    int slots;       // workspace copies: batch i+1's tile kernel overlaps batch i's finalize
    size_t per_pair, slot_bytes, total;
    inline Slot slot(void* ws, int k) const;
};

// The arrays of a slot, declared once and in their order in memory, as elements per pair. One walk carves them (a null base: sizes
// only) and sums the bytes per pair that size a launch (batch = budget / per_pair): the open-row masks came after the launches were
// cut and stay out of that sum (1/128 of rowres), the counter block is one per slot.
struct SlotWalk {
    Bump b;
    size_t batch, per_pair = 0;
    template <class T>
    T* pair(size_t n, bool budgeted = true) {
        per_pair += budgeted ? n * sizeof(T) : 0;
        return n && batch ? b.take<T>(n * batch) : nullptr;   // (an array the form does not have takes no bytes)
    }
};
inline Slot slot_arrays(const MatchPlan& pl, SlotWalk& w) {
    const size_t rs = (size_t)pl.row_stride, mt = (size_t)pl.max_tiles;
    const size_t full = pl.full_cols ? 1 : 0, lean = 1 - full;   // the candidate arrays exist in the other form only
    Slot s;
    s.rowres = w.pair<uint4>(pl.col_chunks * rs);
    s.colpart = w.pair<uint2>(full * pl.wb_stride * rs);
    s.matches = w.pair<uint2>(rs);
    s.rowcand = w.pair<uint2>(lean * rs);
    s.candlist = w.pair<int>(lean * rs);
    s.colres = w.pair<uint2>(lean * rs);
    s.state = w.pair<int4>(lean);
    s.items = w.pair<int2>(lean * mt);
    s.counters = w.b.take<SlotCounters>(1);
    s.bytile = w.pair<int>(lean * rs);
    s.aitems = w.pair<int4>(lean * 2 * mt);
    s.openlist = w.pair<int>(lean * rs);
    s.openmask = w.pair<unsigned long long>(lean * pl.mask_stride, false);
    return s;
}
inline Slot MatchPlan::slot(void* ws, int k) const {
    SlotWalk w{Bump(ws ? (char*)ws + (size_t)k * slot_bytes : nullptr), (size_t)batch};
    return slot_arrays(*this, w);
}

inline MatchPlan make_plan(const MatchPlanIn& in) {
    const int max_tiles = in.max_tiles, npairs = in.npairs;
    MatchPlan pl;
    pl.max_tiles = max_tiles, pl.full_cols = in.full_cols;
    pl.row_stride = max_tiles * 32;
    pl.wb_stride = (max_tiles + PLAN_WG_TILES - 1) / PLAN_WG_TILES + 1;  // column-partial slots per pair: one per workgroup + 1
    pl.wgs_per_pair = (max_tiles + PLAN_WG_TILES - 1) / PLAN_WG_TILES;
    pl.col_chunks = (max_tiles + PLAN_CHUNK_TILES - 1) / PLAN_CHUNK_TILES;
    pl.mask_stride = (pl.row_stride + 63) / 64;
    // per pair: row results + match list, and EITHER the column partials of the full sweep OR the arrays of the candidate pass
    SlotWalk pp{Bump(nullptr), 0};
    slot_arrays(pl, pp);
    pl.per_pair = pp.per_pair;
    // bound a slot near 1 GiB so the column partials of one batch stay cache-friendly
    int batch = (int)std::min<size_t>(std::max<size_t>(in.budget / pl.per_pair, 1), (size_t)npairs);
    // whole rounds of workgroups (2 per CU x 256 CUs) keep the tail of a launch short
    const int wgs = pl.wgs_per_pair * pl.col_chunks;
    int round_pairs = 512;
    for (int g = 512; g >= 1; g >>= 1)
        if (wgs % g == 0) { round_pairs = 512 / g; break; }
    if (batch < npairs && batch > round_pairs) batch -= batch % round_pairs;
    // a job that fits one launch (a shard of a multi-GPU run) is still cut in two, so that the finalize
    // of its first half runs beside the tile kernel of the second
    if (batch >= npairs && npairs >= 8 * round_pairs) batch = ((npairs + 1) / 2 + round_pairs - 1) / round_pairs * round_pairs;
    pl.batch = std::max(batch, 1);
    pl.round_pairs = pl.batch % round_pairs == 0 ? round_pairs : 1;   // (a budget below one round: launches are sized in pairs)
    pl.slots = (pl.batch < npairs && !in.no_overlap) ? 2 : 1;
    // The cut of the whole job, two slots in use: n full launches and ONE short last launch, the only one whose exact pass and
    // candidate tail nothing hides. The short launch is planned first — the last tail_pairs of the job at the most (an eighth of
    // a full launch in whole rounds), less whatever fills the full launches up to whole rounds — and the rest is dealt out over as
    // few launches as the budget allows, equal to a round. So the last launch is never the budget's remnant: full launches with only the
    // last one shortened had cut S200 into 9 792 + 9 792 + 316 and cut 2 x batch + 1 pairs into batch + batch + 1 (profiles/launch_cut.txt).
    pl.tail_pairs = std::max(pl.round_pairs, pl.batch / 8 / pl.round_pairs * pl.round_pairs);
    pl.full_launches = pl.full_rounds = pl.long_launches = 0;
    if (pl.slots == 2) {
        const int rp = pl.round_pairs, last_max = std::min(pl.tail_pairs, pl.batch);   // last launch: (last_max - rp, last_max] pairs
        const int rounds = (npairs - last_max + rp - 1) / rp;                          // of all full launches; >= 1: npairs > batch
        pl.full_launches = (int)(((long long)rounds * rp + pl.batch - 1) / pl.batch);
        pl.full_rounds = rounds / pl.full_launches;
        pl.long_launches = rounds % pl.full_launches;   // the first so many take one round more (then full_rounds * rp < batch)
    }
    SlotWalk sizes{Bump(nullptr), (size_t)pl.batch};
    slot_arrays(pl, sizes);
    pl.slot_bytes = sizes.b.off;
    pl.total = pl.slot_bytes * pl.slots;
    return pl;
}

// Pairs of launch b, which starts at `first`: the cut make_plan planned for the npairs it was given when two workspace slots are in
// use (equal full launches, then the short one), else full batches and what is left. One definition for run_match and for
// eacham_match_debug_batches.
inline int next_batch(const MatchPlan& pl, int b, int first, int npairs) {
    if (pl.slots == 2 && b < pl.full_launches) return (pl.full_rounds + (b < pl.long_launches ? 1 : 0)) * pl.round_pairs;
    return std::min(pl.batch, npairs - first);
}
// ... and the same launches as a function of the pair's index, for match_openprep_kernel (run_match_metric checks one against the other)
struct LaunchCut {   // [0, n1) in launches of len1, [n1, n2) of len2, then len3
    int n1, len1, n2, len2, len3;
};
inline LaunchCut launch_cut(const MatchPlan& pl) {
    LaunchCut c{0, 1, 0, 1, pl.batch};
    if (pl.slots == 2) {
        c.len1 = (pl.full_rounds + 1) * pl.round_pairs, c.n1 = pl.long_launches * c.len1;
        c.len2 = pl.full_rounds * pl.round_pairs, c.n2 = c.n1 + (pl.full_launches - pl.long_launches) * c.len2;
    }
    return c;
}
EACHAM_PLAN_HD inline int launch_of(const LaunchCut& c, int i, int* start) {
    if (i < c.n1) { const int b = i / c.len1; *start = b * c.len1; return b; }
    if (i < c.n2) { const int b = (i - c.n1) / c.len2; *start = c.n1 + b * c.len2; return c.n1 / c.len1 + b; }
    const int b = (i - c.n2) / c.len3;
    *start = c.n2 + b * c.len3;
    return c.n1 / c.len1 + (c.n2 - c.n1) / c.len2 + b;
}

// Workgroups of match_argmin_kernel (one wave each, persistent over an item list whose length only the device knows) for a launch of
// nb pairs on a chip of `cus` CUs. 100 VGPRs: four of its waves fit a SIMD, sixteen a CU, and that round of the chip is what a launch
// with the chip to itself gets (the job's last launch, a job of one launch, one stream). Beside the next launch's screen sweep it gets
// half a round: its waves enter where a sweep workgroup retired (254 VGPRs on each of the CU's four SIMDs, room for eight of them)
// and hold that slot until the list is done, so a full round can displace every sweep workgroup of the chip while the kernel, which
// waits on gathered loads, is hardly faster for it: alone 323 us with sixteen waves per CU, 399 us with four (profiles/tail_placement.txt).
inline int argmin_grid(int nb, int wgs_per_pair, int cus, bool beside_screen_sweep) {
    const long long bound = std::max<long long>((long long)nb * wgs_per_pair, 1);
    const long long cap = (long long)std::max(cus, 1) * (beside_screen_sweep ? 8 : 16);
    return (int)std::min(bound, cap);
}

// Behind the slots, under the screen sweep: the arrays of the CALL that its candidate list needs (seghead | segcount | one item
// counter per launch). Carved as ONE block of ints and indexed inside it: call_pairs is a multiple of 64 ints, so the three lie
// where a carve each would put them, but the block ends with its last counter, not on the next 256 bytes (call_bytes).
struct CallArrays {
    int *seghead, *segcount, *launch_items;
};
inline size_t call_pairs(int npairs) { return ((size_t)npairs + 63) & ~(size_t)63; }
inline size_t call_bytes(int npairs, int launches) { return (2 * call_pairs(npairs) + (size_t)launches) * sizeof(int); }
inline CallArrays call_arrays(void* ws, const MatchPlan& pl, int npairs, int launches) {
    Bump b(ws);
    b.take<char>(pl.total);   // the slots
    int* const block = b.take<int>(call_bytes(npairs, launches) / sizeof(int));
    return {block, block + call_pairs(npairs), block + 2 * call_pairs(npairs)};
}

// ---- the float kind (L2 and dot product: run_match_f32, run_match_dot, run_match_dot_screened) --------------------------------
struct F32Arrays {
    int4 *rowres, *colpart;
    uint2* matches;
    int2 *rowres_dot, *colpart_dot;   // the dot-product form's {bits, index} entries in the same arrays, half used: one plan for both forms
    // behind them, the screened dot-product form only (else null): the sweep's top-2 arrays and the lists of the open
    int4 *rr16, *cp16;
    int* open_idx;
    int2* open_cnt;
};
struct MatchPlanF32 {
    int row_stride, wb_stride, wgs_per_pair;  // padded rows per frame (max over the resident frames), its 32-row tiles, workgroups per pair
    int batch;                                // pairs per launch
    size_t total, total_screened;
    F32Arrays carve(void* ws, bool screened = false, size_t* bytes = nullptr) const {
        Bump b(ws);
        const size_t n = (size_t)batch * row_stride;
        F32Arrays a{};
        a.rowres = b.take<int4>(n), a.colpart = b.take<int4>(n * wb_stride), a.matches = b.take<uint2>(n);
        a.rowres_dot = (int2*)a.rowres, a.colpart_dot = (int2*)a.colpart;
        if (screened) a.rr16 = b.take<int4>(n), a.cp16 = b.take<int4>(n * wb_stride), a.open_idx = b.take<int>(2 * n), a.open_cnt = b.take<int2>((size_t)batch);
        if (bytes) *bytes = b.off;
        return a;
    }
};
inline MatchPlanF32 plan_match_f32(int max_tiles, int npairs) {
    MatchPlanF32 pl;
    pl.row_stride = max_tiles * 32, pl.wb_stride = max_tiles;
    pl.wgs_per_pair = (max_tiles + PLAN_F32_WG_TILES - 1) / PLAN_F32_WG_TILES;
    const size_t per_pair = (size_t)pl.row_stride * sizeof(int4) + (size_t)pl.wb_stride * pl.row_stride * sizeof(int4) +
                            (size_t)pl.row_stride * sizeof(uint2) + sizeof(int);
    pl.batch = (int)std::max<size_t>(1, std::min<size_t>(((size_t)1 << 30) / per_pair, (size_t)npairs));
    pl.carve(nullptr, false, &pl.total), pl.carve(nullptr, true, &pl.total_screened);
    return pl;
}

// ---- wide binary frames (run_match_ham_wide) ---------------------------------------------------------------------------------
struct HamWideArrays {
    float2* rowres;   // two directions of row results
    uint2* matches;
};
struct HamWidePlan {
    int row_stride, wgs_per_pair, batch;
    size_t total;
    HamWideArrays carve(void* ws, size_t* bytes = nullptr) const {
        Bump b(ws);
        const size_t n = (size_t)batch * row_stride;
        HamWideArrays a{b.take<float2>(2 * n), b.take<uint2>(n)};
        if (bytes) *bytes = b.off;
        return a;
    }
};
// per pair: two directions of row results and the match list. Where a batch ends decides nothing: every pair's arrays are its own.
inline HamWidePlan plan_ham_wide(int max_tiles, int npairs, size_t budget) {
    HamWidePlan pl;
    pl.row_stride = 32 * max_tiles;
    pl.wgs_per_pair = (max_tiles + PLAN_HW_WG_TILES - 1) / PLAN_HW_WG_TILES;
    const size_t per_pair = (size_t)pl.row_stride * (2 * sizeof(float2) + sizeof(uint2));
    pl.batch = (int)std::min<size_t>(std::max<size_t>(budget / per_pair, 1), (size_t)std::max(npairs, 1));
    pl.carve(nullptr, &pl.total);
    return pl;
}

}  // namespace eacham
