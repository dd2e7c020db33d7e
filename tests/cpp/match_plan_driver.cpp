// Executes eacham_amd/csrc/match_plan.hpp on the CPU for tests/test_match_plan.py. One job per line of standard input, one JSON
// object per job on standard output (a JSON list in all):
//   plan <max_tiles> <npairs> <budget bytes> <full_cols> <no_overlap>   the cut, the launches, launch_of at every launch start, the
//                                                                      pair before it and the last pair, the slot and call layouts
//   f32 <max_tiles> <npairs>                                           the float plan with the screened dot-product form's arrays
//   wide <max_tiles> <npairs> <budget bytes>                           the wide-Hamming plan
// Offsets are pointers minus the workspace base (address space reserved, never touched); -1 is an array the form does not have.
#include "../../eacham_amd/csrc/match_plan.hpp"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <sys/mman.h>
#include <vector>

using namespace eacham;

static char* g_base = nullptr;
static long long off(const void* p) { return p ? (long long)((const char*)p - g_base) : -1; }

struct Reserve {   // address space for a workspace of `bytes`
    size_t bytes;
    explicit Reserve(size_t n) : bytes(n + 4096) {
        void* p = mmap(nullptr, bytes, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        g_base = p == MAP_FAILED ? nullptr : (char*)p;
    }
    ~Reserve() { if (g_base) munmap(g_base, bytes); g_base = nullptr; }
};

static void print_slot(const char* name, const Slot& s) {
    printf("\"%s\":{\"rowres\":%lld,\"colpart\":%lld,\"matches\":%lld,\"rowcand\":%lld,\"candlist\":%lld,\"colres\":%lld,\"state\":%lld,"
           "\"items\":%lld,\"counters\":%lld,\"bytile\":%lld,\"aitems\":%lld,\"openlist\":%lld,\"openmask\":%lld},",
           name, off(s.rowres), off(s.colpart), off(s.matches), off(s.rowcand), off(s.candlist), off(s.colres), off(s.state), off(s.items),
           off(s.counters), off(s.bytile), off(s.aitems), off(s.openlist), off(s.openmask));
}

static int job_plan(std::istringstream& in) {
    MatchPlanIn pin{};
    int full = 0, no_overlap = 0;
    if (!(in >> pin.max_tiles >> pin.npairs >> pin.budget >> full >> no_overlap)) return 1;
    pin.full_cols = full != 0, pin.no_overlap = no_overlap != 0;
    const MatchPlan pl = make_plan(pin);
    const int npairs = pin.npairs;
    std::vector<int> starts;
    for (int first = 0, b = 0; first < npairs; ++b) {
        starts.push_back(first);
        first += next_batch(pl, b, first, npairs);
    }
    const int launches = (int)starts.size();
    printf("{\"batch\":%d,\"round_pairs\":%d,\"tail_pairs\":%d,\"full_launches\":%d,\"full_rounds\":%d,\"long_launches\":%d,\"slots\":%d,"
           "\"wgs_per_pair\":%d,\"wb_stride\":%d,\"row_stride\":%d,\"col_chunks\":%d,\"mask_stride\":%d,\"per_pair\":%zu,\"slot_bytes\":%zu,"
           "\"total\":%zu,\"null_base_gives_null\":%d,",
           pl.batch, pl.round_pairs, pl.tail_pairs, pl.full_launches, pl.full_rounds, pl.long_launches, pl.slots, pl.wgs_per_pair,
           pl.wb_stride, pl.row_stride, pl.col_chunks, pl.mask_stride, pl.per_pair, pl.slot_bytes, pl.total,
           (int)(pl.slot(nullptr, 0).rowres == nullptr && pl.slot(nullptr, 0).matches == nullptr));
    printf("\"starts\":[");
    for (int b = 0; b < launches; ++b) printf("%s%d", b ? "," : "", starts[b]);
    // launch_of at every launch start, the pair before it and the last pair: [pair, launch, start]
    const LaunchCut cut = launch_cut(pl);
    printf("],\"cut\":[%d,%d,%d,%d,%d],\"launch_of\":[", cut.n1, cut.len1, cut.n2, cut.len2, cut.len3);
    bool any = false;
    for (int b = 0; b <= launches; ++b)
        for (int i : {(b < launches ? starts[b] : npairs) - 1, b < launches ? starts[b] : -1}) {
            if (i < 0) continue;
            int start = -1;
            const int l = launch_of(cut, i, &start);
            printf("%s[%d,%d,%d]", any ? "," : "", i, l, start);
            any = true;
        }
    printf("],");
    Reserve r(pl.total + call_bytes(npairs, launches));
    if (!g_base) return 2;
    print_slot("slot0", pl.slot(g_base, 0));
    print_slot("slot1", pl.slot(g_base, pl.slots - 1));
    const CallArrays c = call_arrays(g_base, pl, npairs, launches);
    printf("\"seghead\":%lld,\"segcount\":%lld,\"launch_items\":%lld,\"call_bytes\":%zu,\"counters\":[%zu,%zu,%zu,%zu]}", off(c.seghead),
           off(c.segcount), off(c.launch_items), call_bytes(npairs, launches), offsetof(SlotCounters, n_items), offsetof(SlotCounters, n_pre),
           offsetof(SlotCounters, n_aitems), sizeof(SlotCounters));
    return 0;
}

static int job_f32(std::istringstream& in) {
    int max_tiles = 0, npairs = 0;
    if (!(in >> max_tiles >> npairs)) return 1;
    const MatchPlanF32 pl = plan_match_f32(max_tiles, npairs);
    Reserve r(pl.total_screened);
    if (!g_base) return 2;
    size_t plain = 0, screened = 0;
    const F32Arrays a = pl.carve(g_base, false, &plain), s = pl.carve(g_base, true, &screened);
    if (a.rr16 || a.cp16 || a.open_idx || a.open_cnt || s.rowres != a.rowres || s.colpart != a.colpart || s.matches != a.matches) return 3;
    printf("{\"batch\":%d,\"row_stride\":%d,\"wb_stride\":%d,\"wgs_per_pair\":%d,\"total\":%zu,\"total_screened\":%zu,\"carved\":[%zu,%zu],"
           "\"rowres\":%lld,\"colpart\":%lld,\"matches\":%lld,\"rowres_dot\":%lld,\"colpart_dot\":%lld,\"rr16\":%lld,\"cp16\":%lld,"
           "\"open_idx\":%lld,\"open_cnt\":%lld}",
           pl.batch, pl.row_stride, pl.wb_stride, pl.wgs_per_pair, pl.total, pl.total_screened, plain, screened, off(a.rowres), off(a.colpart),
           off(a.matches), off(a.rowres_dot), off(a.colpart_dot), off(s.rr16), off(s.cp16), off(s.open_idx), off(s.open_cnt));
    return 0;
}

static int job_wide(std::istringstream& in) {
    int max_tiles = 0, npairs = 0;
    size_t budget = 0;
    if (!(in >> max_tiles >> npairs >> budget)) return 1;
    const HamWidePlan pl = plan_ham_wide(max_tiles, npairs, budget);
    Reserve r(pl.total);
    if (!g_base) return 2;
    const HamWideArrays a = pl.carve(g_base);
    printf("{\"batch\":%d,\"row_stride\":%d,\"wgs_per_pair\":%d,\"total\":%zu,\"rowres\":%lld,\"matches\":%lld}", pl.batch, pl.row_stride,
           pl.wgs_per_pair, pl.total, off(a.rowres), off(a.matches));
    return 0;
}

int main() {
    std::string line;
    bool first = true;
    printf("[");
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        printf("%s\n", first ? "" : ",");
        first = false;
        const int rc = kind == "plan" ? job_plan(in) : kind == "f32" ? job_f32(in) : kind == "wide" ? job_wide(in) : 1;
        if (rc) {
            fprintf(stderr, "bad job (%d): %s\n", rc, line.c_str());
            return rc;
        }
    }
    printf("\n]\n");
    return 0;
}
