// groups_stats_driver.cpp — what eacham_amd/csrc/ba_groups.hpp's host statement (build_groups) holds for a GIVEN problem.
// Reads   nc nl no rows   then lm_ptr[nl + 1] and obs_cam[no] (landmark order) from stdin, builds the structure (rows = 0: the size
// the problem selects) and prints one JSON line: the lengths of the runs (entries of one camera block inside one group), of the
// segments (lanes folded into one partial) and of the blocks' partial lists. Test infrastructure (tests/ba_ragged_cases.py: the
// ragged cases assert that they reach short and long runs, short segments and long blocks); nothing here runs on the product path.
#include <cstdio>
#include <map>
#include <utility>
#include <vector>

#include "../../eacham_amd/csrc/ba_groups.hpp"

using namespace eacham;

int main() {
    int nc, nl, no, rows;
    if (scanf("%d %d %d %d", &nc, &nl, &no, &rows) != 4 || nc < 1 || nl < 0 || no < 0) return 2;
    std::vector<int> lm_ptr(nl + 1);
    std::vector<unsigned> obs_cam(no);
    for (int& v : lm_ptr)
        if (scanf("%d", &v) != 1) return 2;
    for (unsigned& v : obs_cam)
        if (scanf("%u", &v) != 1 || v >= (unsigned)nc) return 2;
    for (int j = 0; j < nl; ++j)
        if (lm_ptr[j] > lm_ptr[j + 1]) return 2;
    if (lm_ptr[0] != 0 || lm_ptr[nl] != no) return 2;
    std::vector<double> obs_uv(2 * (size_t)no, 0.0);
    BaGroups G;
    if (!build_groups(nc, nl, lm_ptr.data(), obs_cam.data(), obs_uv.data(), G, rows)) {
        printf("{\"built\": false}\n");
        return 0;
    }
    const size_t R = (size_t)G.rows;
    std::map<std::pair<int, long long>, int> runs;
    long long short_segments = 0, full_segments = 0, entries = 0;
    for (size_t g = 0; g < G.groups.size(); ++g) {
        const BaGroup& gr = G.groups[g];
        for (int c = gr.chunk0; c < gr.chunk0 + gr.nchunks; ++c) {
            const BaChunk ch = G.chunks[c];
            for (int l = 0; l < 64; ++l) {
                int len = 0;
                long long key = -1;
                for (int i = 0; i < 4 * ch.n4; ++i) {
                    const uint32_t e = G.ent[((size_t)ch.ent0 + i / 4) * 256 + 4 * l + i % 4];
                    const int r1 = (int)(e & 0xffffu), r2 = (int)(e >> 16);
                    if (r1 == G.rows) continue;
                    if (!len) key = (long long)G.rowinfo[g * R + r1].x * (nc + 1) + G.rowinfo[g * R + r2].x;
                    ++len;
                }
                if (len) runs[{(int)g, key}] += len, entries += len;
                const uint32_t info = G.laneinfo[64 * (size_t)c + l];
                if (info & 0x0fffffffu) ((int)(info >> 28) + 1 < GRP_SEG ? short_segments : full_segments)++;
            }
        }
    }
    long long short_runs = 0, long_runs = 0;
    int max_run = 0, max_partials = 0;
    for (const auto& kv : runs) short_runs += kv.second <= 4, long_runs += kv.second > GRP_SLICE, max_run = std::max(max_run, kv.second);
    for (const GrpI4& b : G.blk) max_partials = std::max(max_partials, b.w);
    printf("{\"built\": true, \"rows\": %d, \"groups\": %zu, \"short_runs\": %lld, \"long_runs\": %lld, \"max_run\": %d, \"short_segments\": %lld, "
           "\"full_segments\": %lld, \"long_blocks\": %zu, \"max_partials\": %d, \"entries_ok\": %s}\n",
           G.rows, G.groups.size(), short_runs, long_runs, max_run, short_segments, full_segments, G.longblk.size(), max_partials,
           entries == G.n_entries ? "true" : "false");
    return 0;
}
