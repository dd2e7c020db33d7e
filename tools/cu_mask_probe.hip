// Which CUs a stream made by hipExtStreamCreateWithCUMask runs on, per mask: every workgroup of a spinning grid records the XCD
// (HW_REG_XCC_ID) and the shader engine / array / CU (HW_REG_HW_ID) it ran on; the host prints the distinct places per mask.
//   hipcc --offload-arch=gfx950 -O2 tools/cu_mask_probe.hip -o tools/cu_mask_probe && tools/cu_mask_probe
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <set>
#include <vector>

#define CK(x)                                                                      \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                    \
            printf("%s: %s\n", #x, hipGetErrorString(e_));                         \
            return 1;                                                              \
        }                                                                          \
    } while (0)

__global__ void where_kernel(uint2* out, long long ticks) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) {}   // long enough for the grid to fill every CU it may use
    if (threadIdx.x == 0) {
        const unsigned xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);   // HW_REG_XCC_ID, all 32 bits
        const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_REG_HW_ID
        out[blockIdx.x] = make_uint2(xcc & 15u, hw);
    }
}

int main() {
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount, words = (cus + 31) / 32;
    printf("%s: %d CUs, %d mask words\n", prop.name, cus, words);
    const int grid = 4096;
    uint2* out = nullptr;
    CK(hipMalloc((void**)&out, grid * sizeof(uint2)));
    std::vector<uint2> host(grid);
    struct Case { const char* name; std::vector<int> bits; };
    std::vector<Case> cases;
    static char names[64][32];
    int nn = 0;
    for (int b : {0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 40, 64, 128, 255}) {
        if (b >= cus) continue;
        snprintf(names[nn], 32, "bit %d", b);
        cases.push_back({names[nn++], {b}});
    }
    for (int k : {8, 16, 32, 64}) {
        std::vector<int> low;
        for (int b = 0; b < k; ++b) low.push_back(b);
        snprintf(names[nn], 32, "low %d", k);
        cases.push_back({names[nn++], low});
    }
    for (const Case& c : cases) {
        std::vector<uint32_t> mask(words, 0u);
        for (int b : c.bits) mask[b / 32] |= 1u << (b % 32);
        hipStream_t s;
        CK(hipExtStreamCreateWithCUMask(&s, (uint32_t)words, mask.data()));
        CK(hipMemsetAsync(out, 0xff, grid * sizeof(uint2), s));
        where_kernel<<<grid, 64, 0, s>>>(out, 2000);   // 20 us of the 100 MHz clock per workgroup
        CK(hipGetLastError());
        CK(hipStreamSynchronize(s));
        CK(hipMemcpy(host.data(), out, grid * sizeof(uint2), hipMemcpyDeviceToHost));
        CK(hipStreamDestroy(s));
        std::map<unsigned, std::set<unsigned>> per_xcc;   // xcc -> {se, sh, cu}
        for (const uint2& v : host) per_xcc[v.x].insert(((v.y >> 13) & 7u) << 8 | ((v.y >> 12) & 1u) << 4 | ((v.y >> 8) & 15u));
        size_t n = 0;
        for (auto& kv : per_xcc) n += kv.second.size();
        printf("%-8s %3zu CUs:", c.name, n);
        for (auto& kv : per_xcc) {
            printf("  xcd %u [", kv.first);
            for (unsigned p : kv.second) printf(" se%u.sh%u.cu%u", p >> 8, (p >> 4) & 1u, p & 15u);
            printf(" ]");
        }
        printf("\n");
    }
    CK(hipFree(out));
    return 0;
}
