// match_screen.hpp — the FP6 (e2m3) grid of the 256-D screen sweep and its bound arithmetic, pure C++ usable from host and device
// (matcher.hip quantises and bounds with it; tests/cpp/match_screen_driver.cpp executes it on the CPU).
//
// What it serves: above 128-D the exact int8 row sweep is bound by the matrix pipe. v_mfma_scale_f32_32x32x64_f8f6f4 with e2m3
// operands runs twice the K per instruction in the same cycles, so a sweep over QUANTISED descriptors costs the pipe half — and the
// result only needs exact distances for the rows that can pass the ratio test. A row is finished by the quantised sweep where the
// bound below proves that it fails the test; every other row gets exact numbers from the int8 pass (match_colverify_kernel<KS, true>).
//
// Definition:
//  1. a descriptor value x in 0..255 gets a 6-bit code {sign, 5-bit magnitude code c}. The code's integer value M is 8 times the
//     e2m3 number: |M| = c for c < 16, 16 + 2 (c - 16) for c < 24, 32 + 4 (c - 24) beyond, so M lies in
//     +-{0..15, 16..30 step 2, 32..60 step 4};
//  2. reconstruction x~ = CENTRE + STEP M with CENTRE = 64, STEP = 4; the code of x is the grid value nearest x - 64, the one of
//     smaller magnitude on a tie (so codes are symmetric in sign about the centre, and zero has one code). x - 64 lies in -64..191
//     and the grid reaches +-240: nothing clips. Padded dimensions carry code 0 on both sides;
//  3. the centre cancels in a difference: d~2(a, b) = STEP^2 n, n = |M_a - M_b|^2, an integer of at most 2^20 (exact in f32);
//  4. per stored row r the exact integer s_r = sum (x - x~)^2, per frame E = the largest s_r over its real rows. By the triangle
//     inequality |d(a, b) - d~(a, b)| <= sqrt(s_a) + sqrt(E_B) for every row b of frame B;
//  5. with n1 the smallest n of a query row over the train frame and u an upper bound of the second smallest (the second smallest
//     of the minima over disjoint subsets of the train rows):
//         L1 = floor(max(0, STEP sqrt(n1) - sqrt(s_a) - sqrt(E_B))^2) - 1, clamped at 0       <= the row's true minimum d2
//         U2 = ceil((STEP sqrt(u) + sqrt(s_a) + sqrt(E_B))^2) + 1, clamped at 256 * 255^2      >= the row's true runner-up
//     in double, each rounded outward by one more integer, so that no rounding of a square root turns a bound into a lie. The
//     ratio test is monotone in both arguments: a row that fails it on (L1, U2) fails it on the true pair.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define EACHAM_SCREEN_HD __host__ __device__
#else
#define EACHAM_SCREEN_HD
#endif

namespace eacham {
namespace screen {

constexpr int CENTRE = 64;
constexpr int STEP = 4;
constexpr int MAX_D2 = 256 * 255 * 255;   // no squared distance of two 256-D rows of 0..255 is larger
constexpr int MAX_M = 60;

// |M| of a 5-bit magnitude code
EACHAM_SCREEN_HD inline int mag_value(int c) { return c < 16 ? c : (c < 24 ? 16 + 2 * (c - 16) : 32 + 4 * (c - 24)); }
// M of a 6-bit code (bit 5 = sign)
EACHAM_SCREEN_HD inline int decode(int code) {
    const int m = mag_value(code & 31);
    return (code & 32) ? -m : m;
}
// 6-bit code of a descriptor value x in 0..255: the grid value nearest x - CENTRE, the smaller magnitude on a tie
EACHAM_SCREEN_HD inline int encode(int x) {
    const int y = x - CENTRE;
    const int a = y < 0 ? -y : y;   // 0..191
    int c;
    if (a < 64) c = (a + 1) >> 2;                        // grid step 4: M = 0..16
    else if (a < 128) c = 16 + ((a - 64 + 3) >> 3);      // grid step 8: M = 16..32 (codes 16..24)
    else c = 24 + ((a - 128 + 7) >> 4);                  // grid step 16: M = 32..
    return (y < 0 && c != 0) ? (c | 32) : c;
}
// x~ of a code
EACHAM_SCREEN_HD inline int reconstruct(int code) { return CENTRE + STEP * decode(code); }

// A lane's 32 codes of one K = 64 step as the instruction reads them: 6 bits each, dense, element e at bits 6 e .. 6 e + 5.
EACHAM_SCREEN_HD inline void pack32(const unsigned char* codes, uint32_t out[6]) {
    for (int w = 0; w < 6; ++w) out[w] = 0u;
    for (int e = 0; e < 32; ++e) {
        const int bit = 6 * e, w = bit >> 5, sh = bit & 31;
        const uint32_t v = codes[e] & 63u;
        out[w] |= v << sh;
        if (sh > 26) out[w + 1] |= v >> (32 - sh);
    }
}
EACHAM_SCREEN_HD inline int unpack32(const uint32_t in[6], int e) {
    const int bit = 6 * e, w = bit >> 5, sh = bit & 31;
    uint32_t v = in[w] >> sh;
    if (sh > 26) v |= in[w + 1] << (32 - sh);
    return (int)(v & 63u);
}

// sqrt(s_a) + sqrt(E_B): how far a true distance can lie from the quantised one
EACHAM_SCREEN_HD inline double slack(int s_a, int e_b) { return sqrt((double)s_a) + sqrt((double)e_b); }

// L1: a lower bound of every true d2 of a row whose smallest quantised n is n1
EACHAM_SCREEN_HD inline int lower_d2(unsigned n1, int s_a, int e_b) {
    const double l = (double)STEP * sqrt((double)n1) - slack(s_a, e_b);
    if (!(l > 0.0)) return 0;
    const double f = floor(l * l) - 1.0;
    return f <= 0.0 ? 0 : (f >= (double)MAX_D2 ? MAX_D2 : (int)f);
}
// U2: an upper bound of the true d2 of every row whose quantised n is at most u
EACHAM_SCREEN_HD inline int upper_d2(unsigned u, int s_a, int e_b) {
    const double h = (double)STEP * sqrt((double)u) + slack(s_a, e_b);
    const double c = ceil(h * h) + 1.0;
    return c >= (double)MAX_D2 ? MAX_D2 : (int)c;
}

}  // namespace screen
}  // namespace eacham
