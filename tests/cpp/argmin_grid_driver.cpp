// argmin_grid of eacham_amd/csrc/match_plan.hpp on plain numbers, for tests/test_argmin_grid_host.py: reads lines
// "<nb> <wgs_per_pair> <cus> <beside>" and prints one grid per line.
#include "../../eacham_amd/csrc/match_plan.hpp"

#include <cstdio>

int main() {
    int nb, wgs, cus, beside;
    while (std::scanf("%d %d %d %d", &nb, &wgs, &cus, &beside) == 4) std::printf("%d\n", eacham::argmin_grid(nb, wgs, cus, beside != 0));
    return 0;
}
