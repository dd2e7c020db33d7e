// devprim_driver.hip — the device primitives of eacham_amd/csrc/devprim.hpp called DIRECTLY, outside every product:
// prim::exclusive_scan<int | long long | I3>, prim::radix_sort_pairs<uint32_t | int2> and (through one kernel of this
// file) prim::segment_of<int | long long>, on cases read from ONE file, results written to ONE file; Python
// (tests/test_devprim_gpu.py) judges every byte. A stand-alone program: not an export of the product library.
//
// Every device buffer a primitive writes lies between two guards of GUARD bytes of GUARD_BYTE; the workspaces have exactly
// scan_ws_elems(n) elements / radix_ws_ints(n) ints between theirs. The guards are copied back with the results.
//
//   devprim_driver <cases> <results>       all cases, one process, one stream; non-zero exit at the first HIP error
//   devprim_driver --host-info n...        no HIP call: "n scan_ws_elems(n) radix_nseg(n) radix_ws_ints(n)" per line
//
// in : i32 ncases, then per case  i32 kind | i32 name length | name | body
//      kind 0 scan : i32 type (0 int, 1 long long, 2 I3) | i32 n | i32 nforms | i32 form[nforms] (bit 0: out == in,
//                    bit 1: total_dev given) | input
//      kind 1 sort : i32 V (0 uint32_t: value = index, 1 int2: value = (index, ~index)) | i32 n (as passed to the call) |
//                    i32 emit_all | i32 nkb | i32 key_bits[nkb] | keys (u32; its count sizes the four buffers, >= n)
//      kind 2 segof: i32 type (0 int, 1 long long) | ptr | v (i64)
//      arrays are framed  i64 count | i64 element size | bytes
// out: framed arrays in case order
//      scan, per form : out[n] | guards (out, ws, total: front then back, GUARD bytes each) | total[1] | input[n] if out != in
//      sort, per key_bits: for run 0 and run 1: rc (i32[1]) | keys, values of the pair rc names (with emit_all: ka, va, kb, vb);
//                     then guards (ka, va, kb, vb, ws) once, read after the second run
//      segof          : i32 result[count of v]
//      then the driver's own wall time over all cases in ms (f64[1])
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "devprim.hpp"

using namespace eacham;

static constexpr size_t GUARD = 256;
static constexpr int GUARD_BYTE = 0xC3;
static constexpr int FILL_BYTE = 0x5A;  // what a buffer the primitive is to write holds before the call

static std::string g_case = "(start)";

#define CK(expr)                                                                                                     \
    do {                                                                                                             \
        const hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) {                                                                                      \
            std::fprintf(stderr, "case %s: %s failed: %s (%s:%d)\n", g_case.c_str(), #expr, hipGetErrorString(e_), \
                         __FILE__, __LINE__);                                                                        \
            std::exit(1);                                                                                            \
        }                                                                                                            \
    } while (0)

static void die(const char* what) {
    std::fprintf(stderr, "case %s: %s\n", g_case.c_str(), what);
    std::exit(2);
}

// ---- files ---------------------------------------------------------------------------------------------------------
static void rd_raw(FILE* f, void* p, size_t bytes) {
    if (bytes && fread(p, 1, bytes, f) != bytes) die("short input");
}
static int32_t rd_i32(FILE* f) {
    int32_t v;
    rd_raw(f, &v, sizeof v);
    return v;
}
// a framed array of elements of `elsize` bytes; returns the count
static size_t rd_framed(FILE* f, size_t elsize, std::vector<char>& bytes) {
    int64_t head[2];
    rd_raw(f, head, sizeof head);
    if (head[0] < 0 || (size_t)head[1] != elsize) die("bad array header");
    bytes.resize((size_t)head[0] * elsize);
    rd_raw(f, bytes.data(), bytes.size());
    return (size_t)head[0];
}
static void wr_framed(FILE* f, const void* p, size_t count, size_t elsize) {
    const int64_t head[2] = {(int64_t)count, (int64_t)elsize};
    if (fwrite(head, sizeof(int64_t), 2, f) != 2) die("short output");
    if (count && fwrite(p, elsize, count, f) != count) die("short output");
}

// ---- guarded device buffers out of one arena -------------------------------------------------------------------------
struct Buf {
    char* base = nullptr;  // front guard | payload | back guard
    size_t bytes = 0;
    char* data() const { return base + GUARD; }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(base + GUARD); }
};

struct Arena {
    char* mem = nullptr;
    size_t cap = 0, used = 0;
    static size_t need(size_t bytes) { return ((bytes + 255) & ~(size_t)255) + 2 * GUARD; }
    void reserve(size_t total) {
        used = 0;
        if (total <= cap) return;
        if (mem) CK(hipFree(mem));
        mem = nullptr, cap = 0;
        CK(hipMalloc((void**)&mem, total));
        cap = total;
    }
    Buf take(hipStream_t st, size_t bytes) {
        if (used + need(bytes) > cap) die("arena too small");
        Buf b;
        b.base = mem + used, b.bytes = bytes;
        used += need(bytes);
        CK(hipMemsetAsync(b.base, GUARD_BYTE, GUARD, st));
        CK(hipMemsetAsync(b.base + GUARD + bytes, GUARD_BYTE, GUARD, st));
        return b;
    }
};

static void fill(hipStream_t st, const Buf& b, int byte) {
    if (b.bytes) CK(hipMemsetAsync(b.data(), byte, b.bytes, st));
}
static void upload(hipStream_t st, const Buf& b, const void* src) {
    if (b.bytes) CK(hipMemcpyAsync(b.data(), src, b.bytes, hipMemcpyHostToDevice, st));
}
// (the stream is idle when these run)
static void emit_payload(FILE* out, const Buf& b, size_t elsize, std::vector<char>& host) {
    host.resize(b.bytes);
    if (b.bytes) CK(hipMemcpy(host.data(), b.data(), b.bytes, hipMemcpyDeviceToHost));
    wr_framed(out, host.data(), b.bytes / elsize, elsize);
}
static void emit_guards(FILE* out, std::initializer_list<const Buf*> bufs) {
    std::vector<uint8_t> g(2 * GUARD * bufs.size());
    size_t k = 0;
    for (const Buf* b : bufs) {
        CK(hipMemcpy(g.data() + k, b->base, GUARD, hipMemcpyDeviceToHost));
        CK(hipMemcpy(g.data() + k + GUARD, b->base + GUARD + b->bytes, GUARD, hipMemcpyDeviceToHost));
        k += 2 * GUARD;
    }
    wr_framed(out, g.data(), g.size(), 1);
}

// ---- scan ------------------------------------------------------------------------------------------------------------
template <class T>
static void scan_case(FILE* in, FILE* out, hipStream_t st, Arena& arena, std::vector<char>& host) {
    const int n = rd_i32(in);
    const int nforms = rd_i32(in);
    std::vector<int32_t> forms((size_t)nforms);
    rd_raw(in, forms.data(), forms.size() * sizeof(int32_t));
    std::vector<char> input;
    if (n < 0 || rd_framed(in, sizeof(T), input) != (size_t)n) die("scan input size");
    const size_t wsn = prim::scan_ws_elems((size_t)n);
    for (const int form : forms) {
        const bool inplace = form & 1, has_total = form & 2;
        arena.reserve(2 * Arena::need(input.size()) + Arena::need(wsn * sizeof(T)) + Arena::need(sizeof(T)));
        const Buf bout = arena.take(st, input.size());
        const Buf bws = arena.take(st, wsn * sizeof(T));
        const Buf btot = arena.take(st, sizeof(T));
        Buf bin;
        if (!inplace) bin = arena.take(st, input.size());
        fill(st, bws, FILL_BYTE), fill(st, btot, FILL_BYTE);
        if (inplace) upload(st, bout, input.data());
        else fill(st, bout, FILL_BYTE), upload(st, bin, input.data());
        prim::exclusive_scan<T>(st, inplace ? bout.as<T>() : bin.as<T>(), bout.as<T>(), n, bws.as<T>(),
                                has_total ? btot.as<T>() : nullptr);
        CK(hipGetLastError());
        CK(hipStreamSynchronize(st));
        emit_payload(out, bout, sizeof(T), host);
        emit_guards(out, {&bout, &bws, &btot});
        emit_payload(out, btot, sizeof(T), host);
        if (!inplace) emit_payload(out, bin, sizeof(T), host);
    }
}

// ---- sort ------------------------------------------------------------------------------------------------------------
static void make_value(uint32_t& v, uint32_t i) { v = i; }
static void make_value(int2& v, uint32_t i) { v = int2{(int)i, (int)~i}; }

template <class V>
static void sort_case(FILE* in, FILE* out, hipStream_t st, Arena& arena, std::vector<char>& host) {
    const int n = rd_i32(in);
    const bool emit_all = rd_i32(in) != 0;
    const int nkb = rd_i32(in);
    std::vector<int32_t> kbs((size_t)nkb);
    rd_raw(in, kbs.data(), kbs.size() * sizeof(int32_t));
    std::vector<char> keys;
    const size_t cap = rd_framed(in, sizeof(uint32_t), keys);
    if ((long long)cap < (long long)n) die("sort input size");
    std::vector<V> vals(cap);
    for (size_t i = 0; i < cap; ++i) make_value(vals[i], (uint32_t)i);
    const size_t wsn = prim::radix_ws_ints(n > 0 ? n : 0);
    arena.reserve(2 * Arena::need(cap * sizeof(uint32_t)) + 2 * Arena::need(cap * sizeof(V)) + Arena::need(wsn * sizeof(int)));
    const Buf ka = arena.take(st, cap * sizeof(uint32_t)), va = arena.take(st, cap * sizeof(V));
    const Buf kb = arena.take(st, cap * sizeof(uint32_t)), vb = arena.take(st, cap * sizeof(V));
    const Buf ws = arena.take(st, wsn * sizeof(int));
    for (const int key_bits : kbs) {
        for (int run = 0; run < 2; ++run) {
            upload(st, ka, keys.data()), upload(st, va, vals.data());
            fill(st, kb, FILL_BYTE), fill(st, vb, FILL_BYTE), fill(st, ws, FILL_BYTE);
            const int32_t rc = prim::radix_sort_pairs<V>(st, ka.as<uint32_t>(), va.as<V>(), kb.as<uint32_t>(), vb.as<V>(), n,
                                                         key_bits, ws.as<int>());
            CK(hipGetLastError());
            CK(hipStreamSynchronize(st));
            wr_framed(out, &rc, 1, sizeof rc);
            if (rc != 0 && rc != 1) die("radix_sort_pairs returned neither 0 nor 1");
            if (emit_all || rc == 0) emit_payload(out, ka, sizeof(uint32_t), host), emit_payload(out, va, sizeof(V), host);
            if (emit_all || rc == 1) emit_payload(out, kb, sizeof(uint32_t), host), emit_payload(out, vb, sizeof(V), host);
        }
        emit_guards(out, {&ka, &va, &kb, &vb, &ws});
    }
}

// ---- segment_of --------------------------------------------------------------------------------------------------------
template <class T>
__global__ void segof_kernel(const T* __restrict__ ptr, int n, const long long* __restrict__ v, int nv, int* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nv) out[i] = prim::segment_of<T>(ptr, n, v[i]);
}

template <class T>
static void segof_case(FILE* in, FILE* out, hipStream_t st, Arena& arena, std::vector<char>& host) {
    std::vector<char> ptr, v;
    const size_t n = rd_framed(in, sizeof(T), ptr);
    const size_t nv = rd_framed(in, sizeof(long long), v);
    if (n < 1 || nv < 1) die("segof input size");
    arena.reserve(Arena::need(ptr.size()) + Arena::need(v.size()) + Arena::need(nv * sizeof(int)));
    const Buf bptr = arena.take(st, ptr.size()), bv = arena.take(st, v.size()), bout = arena.take(st, nv * sizeof(int));
    upload(st, bptr, ptr.data()), upload(st, bv, v.data()), fill(st, bout, FILL_BYTE);
    segof_kernel<T><<<(unsigned)((nv + 255) / 256), 256, 0, st>>>(bptr.as<T>(), (int)n, bv.as<long long>(), (int)nv, bout.as<int>());
    CK(hipGetLastError());
    CK(hipStreamSynchronize(st));
    emit_payload(out, bout, sizeof(int), host);
}

// ---- main ------------------------------------------------------------------------------------------------------------
static int host_info(int argc, char** argv) {
    for (int i = 2; i < argc; ++i) {
        const long long n = std::atoll(argv[i]);
        if (n < 0 || n > (1ll << 30)) return 2;
        std::printf("%lld %zu %d %zu\n", n, prim::scan_ws_elems((size_t)n), prim::radix_nseg((int)n), prim::radix_ws_ints((int)n));
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "--host-info") == 0) return host_info(argc, argv);
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <cases> <results> | --host-info n...\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) die("cannot open the case or the result file");
    hipStream_t st;
    CK(hipSetDevice(0));
    CK(hipStreamCreate(&st));
    Arena arena;
    std::vector<char> host;
    const auto t0 = std::chrono::steady_clock::now();
    const int ncases = rd_i32(in);
    for (int c = 0; c < ncases; ++c) {
        const int kind = rd_i32(in);
        const int len = rd_i32(in);
        if (len < 0 || len > 256) die("bad case name");
        std::string name((size_t)len, ' ');
        rd_raw(in, name.data(), (size_t)len);
        g_case = name;
        const int type = rd_i32(in);
        if (kind == 0 && type == 0) scan_case<int>(in, out, st, arena, host);
        else if (kind == 0 && type == 1) scan_case<long long>(in, out, st, arena, host);
        else if (kind == 0 && type == 2) scan_case<prim::I3>(in, out, st, arena, host);
        else if (kind == 1 && type == 0) sort_case<uint32_t>(in, out, st, arena, host);
        else if (kind == 1 && type == 1) sort_case<int2>(in, out, st, arena, host);
        else if (kind == 2 && type == 0) segof_case<int>(in, out, st, arena, host);
        else if (kind == 2 && type == 1) segof_case<long long>(in, out, st, arena, host);
        else die("unknown case kind");
    }
    g_case = "(end)";
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    wr_framed(out, &ms, 1, sizeof ms);
    if (arena.mem) CK(hipFree(arena.mem));
    CK(hipStreamDestroy(st));
    if (fclose(out) != 0) die("cannot close the result file");
    fclose(in);
    std::fprintf(stderr, "devprim_driver: %d cases, %.1f ms\n", ncases, ms);
    return 0;
}
