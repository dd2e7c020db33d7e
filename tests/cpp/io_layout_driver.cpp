// Runs the staging layout of the host-pointer entry points (eacham_amd/csrc/io_layout.hpp) on the CPU: reads one declaration per
// line from stdin, "<role> <element size> <element count>" with role 0 = result, 1 = input, 2 = device-only, and prints the
// placement as JSON. More than IoLayout::MAX_ARRAYS lines must set `overflow`.
#include <cstdio>

#include "../../eacham_amd/csrc/io_layout.hpp"

int main() {
    eacham::IoLayout lay;
    int role;
    unsigned long long elem, count;
    while (scanf("%d %llu %llu", &role, &elem, &count) == 3) lay.add(role, (size_t)elem * (size_t)count);
    lay.place();
    printf("{\"overflow\": %s, \"cut\": %zu, \"total\": %zu, \"arrays\": [", lay.overflow ? "true" : "false", lay.cut, lay.total);
    for (int k = 0; k < lay.n; ++k)
        printf("%s{\"role\": %d, \"bytes\": %zu, \"off\": %zu}", k ? ", " : "", lay.role[k], lay.bytes[k], lay.off[k]);
    printf("]}\n");
    return 0;
}
