// match_screen.hpp — the FP6 (e2m3) grid of the 256-D screen sweep and its bound arithmetic, pure C++ usable from host and device
// (matcher.hip quantises and bounds with it; tests/cpp/match_screen_driver.cpp executes it on the CPU), and the lane map of the
// sweep's 16x16x128 chains over the stored tile (tests/cpp/screen_shape16_driver.cpp executes that).
//
// What it serves: above 128-D the exact int8 row sweep is bound by the matrix pipe. The block-scaled f8f6f4 MFMA with e2m3 operands
// (v_mfma_scale_f32_32x32x64 / 16x16x128) runs twice the K in the same cycles, so a sweep over QUANTISED descriptors costs the pipe half — and the
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

// ---- the stored tile and the lane map of the 16x16x128 chains (match_screen_kernel) ----
// A stored tile is 32 rows x 256 codes. Per K = 64 step ks, stored lane L = row + 32 h holds the 32 codes 64 ks + 32 h .. of `row`
// (K block 2 ks + h of the row's eight), packed as above: words 0..3 at ks * STEP_BYTES + 16 L, words 4..5 at ks * STEP_BYTES +
// HI_PLANE + 8 L. That is the operand image of v_mfma_scale_f32_32x32x64_f8f6f4, and the upload kernels write nothing else.
// v_mfma_scale_f32_16x16x128_f8f6f4 wants of operand lane l the row l & 15 and the K block kg = l >> 4 of a K = 128 step. The sweep
// cuts a tile into two row halves u and two steps S; the fragment of (u, S) gives lane l the stored fragment of row 16 u + (l & 15)
// at ks = 2 S + (kg >> 1), h = kg & 1 — the K blocks of step S in their natural order. Any assignment of kg to the four (ks, h) of
// the step would do as long as the query operand uses the same one (the sums are exact in any order), and none is better for the
// LDS: the four candidates of a row lie multiples of 256 bytes apart in both planes. The 16-byte reads are conflict-free under all of
// them (a group of 16 lanes covers the sixteen 16-byte slots of a bank row once); the 8-byte reads, served 32 lanes at a time, put
// lanes l and l + 16 — one row, two K blocks — on one bank pair under all of them: two-way, 4 array cycles where the 32x32 form's
// read took 2. A tile pays 4 x (4 + 4) + 2 x 4 (C-init) = 40 array cycles where it paid 4 x (4 + 2) + 4 x 4 = 40.
constexpr int STEP_BYTES = 1536, HI_PLANE = 1024, TILE_ROWS = 32;
struct FragSrc { int row, ks, h; };   // where a lane's fragment lies in the stored tile
// train side: fragment (u, S) of a tile as operand lane `lane` reads it
EACHAM_SCREEN_HD constexpr FragSrc frag16_src(int u, int S, int lane) { return FragSrc{16 * u + (lane & 15), 2 * S + (lane >> 5), (lane >> 4) & 1}; }
// query side: sub-tile s4 (16 of the wave's 64 query rows), step S. The rows are those of stored tile query16_tile(s4) of the
// wave-block, the K block of a lane the train side's
EACHAM_SCREEN_HD constexpr int query16_tile(int s4) { return s4 >> 1; }
EACHAM_SCREEN_HD constexpr FragSrc query16_src(int s4, int S, int lane) { return frag16_src(s4 & 1, S, lane); }
// A wave of the sweep owns QUERY_SUBTILES = 8 sub-tiles s8: two wave-blocks of 64 rows (the tail's unit: one openmask word, one row
// per lane), four stored tiles. The two functions above serve all eight: query16_tile(s8) counts the stored tiles from the wave's
// first, sub-tile s8 is sub-tile s8 & 3 of wave-block query16_block(s8) of the wave, and its 16 rows are the wave's rows 16 s8 ..
constexpr int QUERY_SUBTILES = 8;
EACHAM_SCREEN_HD constexpr int query16_block(int s8) { return s8 >> 2; }
EACHAM_SCREEN_HD constexpr int query16_wave_row(int s8, int lane) { return TILE_ROWS * query16_tile(s8) + query16_src(s8, 0, lane).row; }
constexpr bool query16_eight() {
    for (int s8 = 0; s8 < QUERY_SUBTILES; ++s8)
        for (int l = 0; l < 64; ++l) {
            if (query16_tile(s8) != 2 * query16_block(s8) + query16_tile(s8 & 3) || query16_tile(s8) >= QUERY_SUBTILES / 2) return false;
            if (query16_wave_row(s8, l) != 16 * s8 + (l & 15)) return false;
            for (int S = 0; S < 2; ++S) {
                const FragSrc f = query16_src(s8, S, l), g = query16_src(s8 & 3, S, l), t = frag16_src(0, S, l);
                if (f.row != g.row || f.ks != g.ks || f.h != g.h || f.ks != t.ks || f.h != t.h) return false;
            }
        }
    return true;
}
static_assert(query16_eight(), "eight sub-tiles = two wave-blocks of the four-sub-tile map, the train side's K blocks");
EACHAM_SCREEN_HD constexpr int frag_lo_offset(FragSrc f) { return f.ks * STEP_BYTES + 16 * (f.row + TILE_ROWS * f.h); }
EACHAM_SCREEN_HD constexpr int frag_hi_offset(FragSrc f) { return f.ks * STEP_BYTES + HI_PLANE + 8 * (f.row + TILE_ROWS * f.h); }
EACHAM_SCREEN_HD constexpr int frag_kblock(FragSrc f) { return 2 * f.ks + f.h; }   // of the row's eight blocks of 32 codes
// accumulator r (0..3) of the chain of row half u in output lane `lane`: the train row of the tile (the lane's query row is lane & 15
// of the sub-tile). A lane's four are one group of four stored rows, row >> 2 = 4 u + (lane >> 4): one of the tile's eight subsets
EACHAM_SCREEN_HD constexpr int acc16_row(int u, int lane, int r) { return 16 * u + 4 * (lane >> 4) + r; }
// the kernel adds a lane's offset in fragment (0, 0) and the fragment's offset in lane 0: the map is the sum of the two
EACHAM_SCREEN_HD constexpr bool frag16_separable() {
    for (int u = 0; u < 2; ++u)
        for (int S = 0; S < 2; ++S)
            for (int l = 0; l < 64; ++l) {
                if (frag_lo_offset(frag16_src(u, S, l)) != frag_lo_offset(frag16_src(0, 0, l)) + frag_lo_offset(frag16_src(u, S, 0))) return false;
                if (frag_hi_offset(frag16_src(u, S, l)) != frag_hi_offset(frag16_src(0, 0, l)) + frag_hi_offset(frag16_src(u, S, 0)) - HI_PLANE) return false;
            }
    return true;
}
static_assert(frag16_separable(), "lane offset + fragment offset");

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
