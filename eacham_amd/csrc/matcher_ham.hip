// matcher_ham.hip — binary descriptors (ORB, BRIEF, AKAZE: up to 256 bits, packed) under Hamming distance.
//
// The reference's TUM, KITTI and Realsense configurations name ORB, matched by cv::BFMatcher(NORM_HAMMING) and the ratio test
// `m[0].distance / m[1].distance < 0.8` (FeatureMatcherFlann.cpp:23) on integer distances stored as float.
//
// Exact embedding: a bit b is the descriptor value 255 b, so the squared L2 distance of two rows is exactly 65025 h, at most
// 256 * 255^2 = screen::MAX_D2 < 2^24 < 2 PADH. Everything the int8 path of matcher.hip does is exact integer work on such rows:
// sweeps, screen, column pass, pruning, batch plan run unchanged, and the order of the distances (ties to the lower index
// included) is the order of h. The FP6 screen stays sharp: 0 reconstructs 0 and 255 reconstructs 256, so s_r is the popcount of
// a row and the slack sqrt(s_a) + sqrt(E_B) is at most 32 against distances of 255 sqrt(h). (Bits as 0 / 1 would share one FP6
// code and send every row to the exact pass.) The one arithmetic that differs is the predicate: ratio_pass(.., METRIC_HAMMING).
//
// What this file adds: the expansion of packed rows on the device (the host-to-device copy is the packed bytes), the resident
// packed copy (8 words per row, reached through a table of its own so that FrameDev and the sweeps' argument loads stay as they
// are), and the distance kernel: popcount of the XOR of the two packed rows of every emitted match, the DMatch.distance a
// caller expects and an arithmetic path independent of the sweep. The wide kind (matcher_ham_wide.hip, 16 words per row) stores
// its packed rows with the same kernel, enters the same table and gets its distances from the same place.
#include "context.hpp"
#include "devprim.hpp"

namespace eacham {

// thread per (row, byte of the padded row): eight floats 0 / 255, the most significant bit first (np.unpackbits' order);
// bytes at or beyond bytes_per_row are the zero bits of the padding
__global__ void bits_expand_kernel(const unsigned char* __restrict__ packed, int n, int bytes_per_row, int dim, float* __restrict__ dst) {
    const int row_bytes = dim / 8;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)n * row_bytes) return;
    const int row = (int)(idx / row_bytes), j = (int)(idx % row_bytes);
    const unsigned v = j < bytes_per_row ? packed[(size_t)row * bytes_per_row + j] : 0u;
    float* out = dst + (size_t)row * dim + 8 * j;
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = (v >> (7 - i)) & 1u ? 255.0f : 0.0f;
}

// thread per (row, word): the packed row as `words` words (8: up to 256 bits, 16: the wide kind), zero beyond bytes_per_row
__global__ void bits_store_kernel(const unsigned char* __restrict__ packed, int n, int bytes_per_row, int words, unsigned* __restrict__ bits) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * words) return;
    const int row = idx / words, w = idx % words;
    unsigned v = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int j = 4 * w + b;
        if (j < bytes_per_row) v |= (unsigned)packed[(size_t)row * bytes_per_row + j] << (8 * b);
    }
    bits[idx] = v;
}

// dist[k] = popcount(row q of frame pairs[p].x ^ row t of frame pairs[p].y) for edge k = {q, t} of pair p, the pair found by
// its offsets; k runs over the edges that were written (min(total, cap)). V4 = uint4s per packed row: 2 (8 words) or 4 (16, wide frames)
template <int V4>
__global__ void hamming_dist_kernel(const unsigned* const* __restrict__ table, const int2* __restrict__ pairs, int npairs,
                                    const long long* __restrict__ offsets, const long long* __restrict__ total,
                                    const uint2* __restrict__ edges, long long cap, int* __restrict__ dist) {
    const long long m = *total < cap ? *total : cap;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (long long)gridDim.x * blockDim.x) {
        const int p = prim::segment_of(offsets, npairs, k);
        const int2 pr = pairs[p];
        const uint2 e = edges[k];
        const uint4* a = reinterpret_cast<const uint4*>(table[pr.x]);
        const uint4* b = reinterpret_cast<const uint4*>(table[pr.y]);
        int h = -1;   // (a pair of the stand-in frame has no edge; nothing without packed rows is ever read)
        if (a && b) {
            h = 0;
#pragma unroll
            for (int w = 0; w < V4; ++w) {
                const uint4 x = a[V4 * (size_t)e.x + w], y = b[V4 * (size_t)e.y + w];
                h = h + __popc(x.x ^ y.x) + __popc(x.y ^ y.y) + __popc(x.z ^ y.z) + __popc(x.w ^ y.w);
            }
        }
        dist[k] = h;
    }
}

void launch_bits_expand(eacham_ctx* ctx, const unsigned char* packed_dev, int n, int bytes_per_row, int dim, float* dst_dev) {
    const long long work = (long long)n * (dim / 8);
    bits_expand_kernel<<<(unsigned)((work + 255) / 256), 256, 0, ctx->stream>>>(packed_dev, n, bytes_per_row, dim, dst_dev);
}

void launch_bits_store(eacham_ctx* ctx, const unsigned char* packed_dev, int n, int bytes_per_row, int words_per_row, unsigned* bits_dev) {
    bits_store_kernel<<<(n * words_per_row + 255) / 256, 256, 0, ctx->stream>>>(packed_dev, n, bytes_per_row, words_per_row, bits_dev);
}

// the table of the frames' packed rows, entry [frames] = the empty stand-in of sanitize_pairs
static int sync_bits_table(eacham_ctx* ctx) {
    if (!ctx->bits_table_dirty && ctx->bits_table_dev) return EACHAM_OK;
    const int need = (int)ctx->frames.size() + 1;
    if (need > ctx->bits_table_cap) {
        if (ctx->bits_table_dev) {
            EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            EACHAM_HIP_TRY(ctx, hipFree((void*)ctx->bits_table_dev));
            ctx->bits_table_dev = nullptr;
            ctx->bits_table_cap = 0;
        }
        const int cap = need < 64 ? 64 : need * 2;
        EACHAM_HIP_TRY(ctx, hipMalloc((void**)&ctx->bits_table_dev, sizeof(unsigned*) * cap));
        ctx->bits_table_cap = cap;
    }
    std::vector<const unsigned*> tab((size_t)need, nullptr);
    for (int i = 0; i + 1 < need; ++i) tab[i] = ctx->frames[i].n > 0 ? ctx->frames[i].bits : nullptr;
    // (pageable source: staged before the call returns)
    EACHAM_HIP_TRY(ctx, hipMemcpyAsync((void*)ctx->bits_table_dev, tab.data(), sizeof(unsigned*) * need, hipMemcpyHostToDevice, ctx->stream));
    EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->bits_table_dirty = false;
    return EACHAM_OK;
}

int hamming_distances(eacham_ctx* ctx, const int2* pairs_dev, int npairs, const long long* offsets_dev, const long long* total_dev,
                      const uint2* edges_dev, long long edge_cap, int* dist_dev) {
    if (npairs <= 0 || edge_cap <= 0) return EACHAM_OK;
    int rc = sync_bits_table(ctx);
    if (rc) return rc;
    const int grid = (int)std::min<long long>((edge_cap + 255) / 256, 2048);
    if (ctx->kind_common == FRAME_BITS_WIDE)
        hamming_dist_kernel<4><<<grid, 256, 0, ctx->stream>>>(ctx->bits_table_dev, pairs_dev, npairs, offsets_dev, total_dev, edges_dev, edge_cap, dist_dev);
    else
        hamming_dist_kernel<2><<<grid, 256, 0, ctx->stream>>>(ctx->bits_table_dev, pairs_dev, npairs, offsets_dev, total_dev, edges_dev, edge_cap, dist_dev);
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return EACHAM_OK;
}

}  // namespace eacham
