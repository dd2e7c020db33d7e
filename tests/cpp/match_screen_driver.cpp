// Executes eacham_amd/csrc/match_screen.hpp on the CPU (tests/test_match_screen_host.py): the FP6 grid of the screen sweep — nearest
// grid value, code round trip and sign symmetry, the dense 6-bit packing — and its bounds L1 <= d2 <= U2 on seeded random and
// extreme row pairs, with the row's own s and the frame maximum. Prints one JSON object; "bad" counts violated checks.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../eacham_amd/csrc/match_screen.hpp"

using namespace eacham::screen;

static int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad < 5) std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++bad; } } while (0)

struct Row { std::vector<int> x, m; int s = 0; };
static Row make_row(const std::vector<int>& x) {
    Row r;
    r.x = x;
    for (int v : x) {
        const int c = encode(v);
        r.m.push_back(decode(c));
        const int d = v - reconstruct(c);
        r.s += d * d;
    }
    return r;
}

static long long pairs = 0, l_zero = 0, clamped = 0;
static double worst_l = 0, worst_u = 0;   // the smallest margins d2 - L and U - d2 (must stay >= 0)
static void check_pair(const Row& a, const Row& b, int e_b) {
    long long d2 = 0, n = 0;
    for (size_t k = 0; k < a.x.size(); ++k) {
        d2 += (long long)(a.x[k] - b.x[k]) * (a.x[k] - b.x[k]);
        n += (long long)(a.m[k] - b.m[k]) * (a.m[k] - b.m[k]);
    }
    CHECK(n <= (1 << 20) * 4);
    CHECK(e_b >= b.s);
    for (int eb : {b.s, e_b}) {   // the row's own error, and the frame maximum the sweep uses
        const int L = lower_d2((unsigned)n, a.s, eb), U = upper_d2((unsigned)n, a.s, eb);
        CHECK(L >= 0 && L <= d2);
        CHECK(U >= d2 && U <= MAX_D2);
        if (L == 0) ++l_zero;
        if (U == MAX_D2) ++clamped;
        if (pairs == 0 || d2 - L < worst_l) worst_l = (double)(d2 - L);
        if (pairs == 0 || U - d2 < worst_u) worst_u = (double)(U - d2);
        ++pairs;
    }
}

int main() {
    // 1. all 256 values map to a nearest grid value, the smaller magnitude on a tie
    std::vector<int> grid;
    for (int c = 0; c < 64; ++c) grid.push_back(CENTRE + STEP * decode(c));
    int max_err = 0;
    for (int x = 0; x < 256; ++x) {
        const int c = encode(x), g = reconstruct(c);
        CHECK(c >= 0 && c < 64);
        int best = 1 << 30;
        for (int v : grid) best = std::min(best, std::abs(x - v));
        CHECK(std::abs(x - g) == best);
        for (int v : grid)
            if (std::abs(x - v) == best) CHECK(std::abs(g - CENTRE) <= std::abs(v - CENTRE));
        max_err = std::max(max_err, std::abs(x - g));
    }
    // 2. the 64 codes: value set, round trip, sign symmetry
    for (int c = 0; c < 32; ++c) {
        const int m = mag_value(c);
        CHECK(decode(c) == m && decode(c | 32) == -m);
        CHECK(m <= MAX_M && (m < 16 || (m < 32 ? m % 2 == 0 : m % 4 == 0)));
        if (c) CHECK(mag_value(c) > mag_value(c - 1));
        for (int sgn : {0, 32}) {
            const int x = CENTRE + STEP * decode(c | sgn);
            if (x >= 0 && x <= 255) CHECK(encode(x) == (c ? (c | sgn) : 0));
        }
    }
    for (int y = 1; y <= 64; ++y) CHECK(encode(CENTRE + y) == (encode(CENTRE - y) ^ 32) || encode(CENTRE + y) == 0);
    CHECK(encode(CENTRE) == 0 && encode(CENTRE + 2) == 0 && encode(CENTRE - 2) == 0);
    // the dense packing of a lane's 32 codes
    {
        std::mt19937 rng(7);
        for (int rep = 0; rep < 64; ++rep) {
            unsigned char codes[32];
            for (auto& c : codes) c = (unsigned char)(rng() & 63);
            uint32_t w[6];
            pack32(codes, w);
            for (int e = 0; e < 32; ++e) CHECK(unpack32(w, e) == codes[e]);
        }
    }
    // 3. L <= d2 <= U on row pairs: half-normal values and uniform 0..255, several dimensions, and the extremes
    std::mt19937 rng(12345);
    std::normal_distribution<double> nd(0.0, 40.0);
    for (int dim : {16, 129, 160, 255, 256}) {
        for (int kind = 0; kind < 2; ++kind) {
            std::vector<Row> frame;
            for (int r = 0; r < 24; ++r) {
                std::vector<int> x(dim);
                for (auto& v : x) v = kind == 0 ? std::min(255, (int)std::fabs(nd(rng))) : (int)(rng() % 256);
                frame.push_back(make_row(x));
            }
            // near neighbours: the rows that can pass a ratio test
            for (int r = 0; r < 8; ++r) {
                std::vector<int> x = frame[r].x;
                for (auto& v : x) v = std::min(255, std::max(0, v + (int)(rng() % 7) - 3));
                frame.push_back(make_row(x));
            }
            int e = 0;
            for (const Row& r : frame) e = std::max(e, r.s);
            for (const Row& a : frame)
                for (const Row& b : frame) check_pair(a, b, e);
        }
        // extremes: all 0, all 255, the centre, and values midway between grid points at every step size
        std::vector<Row> ext;
        for (int v : {0, 255, 64, 66, 62, 132, 196, 200, 2, 58, 191}) ext.push_back(make_row(std::vector<int>(dim, v)));
        {
            std::vector<int> x(dim);
            for (int k = 0; k < dim; ++k) x[k] = (k & 1) ? 255 : 0;
            ext.push_back(make_row(x));
            for (int k = 0; k < dim; ++k) x[k] = (k & 1) ? 0 : 255;
            ext.push_back(make_row(x));
        }
        int e = 0;
        for (const Row& r : ext) e = std::max(e, r.s);
        for (const Row& a : ext)
            for (const Row& b : ext) check_pair(a, b, e);
    }
    // 4. the clamp and the L1 = 0 case
    CHECK(upper_d2(1u << 20, 16384, 16384) == MAX_D2);
    CHECK(upper_d2(0, 0, 0) == 1);
    CHECK(lower_d2(0, 0, 0) == 0 && lower_d2(1, 16, 0) == 0 && lower_d2(100, 1000, 1000) == 0);
    CHECK(lower_d2(100, 0, 0) == 1599);                       // floor((4 * 10)^2) - 1
    CHECK(lower_d2(100, 16, 9) == 33 * 33 - 1);               // (40 - 4 - 3)^2 - 1
    CHECK(upper_d2(100, 16, 9) == 47 * 47 + 1);
    CHECK(lower_d2(1u << 20, 0, 0) <= MAX_D2);
    std::printf("{\"bad\": %d, \"pairs\": %lld, \"max_err\": %d, \"l_zero\": %lld, \"clamped\": %lld, \"worst_l\": %.1f, \"worst_u\": %.1f}\n", bad, pairs,
                max_err, l_zero, clamped, worst_l, worst_u);
    return bad ? 1 : 0;
}
