// match_tail.hpp — the end of a pair, shared by the per-pair tail kernels of every descriptor kind (match_finalize_kernel and
// match_finalize2_kernel of matcher.hip, match_finalize_f32_kernel, match_finalize_dot_kernel, ham_wide_finalize_kernel): the
// ordered compaction of the kept query rows and what a pair's workgroup writes last. How a row result is decoded and which
// predicate passes is the kind's own and stays in its kernel.
#pragma once

#include <hip/hip_runtime.h>

namespace eacham {

constexpr int FIN_THREADS = 256;   // threads of a pair-tail workgroup (one workgroup per pair)

// exclusive rank of this thread's flag among the workgroup's flags (thread order) + the workgroup's total
__device__ __forceinline__ int block_rank(bool flag, int tid, int* s_wave /* [FIN_THREADS / 64] */, int& total) {
    const unsigned long long bal = __ballot(flag);
    const int lane = tid & 63, wave = tid >> 6;
    const int in_wave = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < FIN_THREADS / 64; ++w) {
        const int c = s_wave[w];
        before += w < wave ? c : 0;
        all += c;
    }
    __syncthreads();
    total = all;
    return before + in_wave;
}

struct SameTrainRow {
    __device__ int operator()(int t) const { return t; }
};

// Ordered compaction over the caller's query rows q = 0 .. n - 1: pick(q) is the train row of the match row q keeps, or -1;
// out[k] = {q, label(pick(q))} for the k-th kept row in ascending q. label turns the train row into the caller's numbering where
// the kind numbers its rows otherwise inside; it runs for kept rows only, behind the rank, so the ballot does not wait for what it
// loads. Returns the number of kept rows. Holds barriers: the whole workgroup calls it, on a workgroup-uniform n, after a barrier
// behind whatever pick reads.
template <class Pick, class Label = SameTrainRow>
__device__ __forceinline__ int compact_kept_rows(int n, int tid, uint2* __restrict__ out, Pick pick, Label label = Label()) {
    __shared__ int s_wave[FIN_THREADS / 64];
    int base = 0;
    for (int q0 = 0; q0 < n; q0 += FIN_THREADS) {
        const int q = q0 + tid;
        const int t = q < n ? pick(q) : -1;
        int total;
        const int rank = block_rank(t >= 0, tid, s_wave, total);
        if (t >= 0) out[base + rank] = make_uint2((unsigned)q, (unsigned)label(t));
        base += total;
    }
    return base;
}

// What one thread of the pair's workgroup does last: the edge rule of apps/sfm/main.cpp:111,142 on {|m12|, |m21|, |mutual|},
// counts[p] (mode 1: the directed list's length whatever the thresholds) and, where asked for, stats[p] = {|m12|, |m21|, |mutual|, edge}
__device__ __forceinline__ void write_pair_result(int p, int mode, int n12, int n21, int base, int min_dir, int min_mutual,
                                                  int* __restrict__ counts, int4* __restrict__ stats) {
    const bool edge = n12 >= min_dir && n21 >= min_dir && base > min_mutual;
    counts[p] = mode == 1 ? base : (edge ? base : 0);
    if (stats) stats[p] = make_int4(n12, n21, base, edge ? 1 : 0);
}

}  // namespace eacham
