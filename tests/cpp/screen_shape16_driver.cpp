// CPU driver of the lane map of the screen sweep's 16x16x128 chains (eacham_amd/csrc/match_screen.hpp: frag16_src, query16_src,
// frag_lo_offset / frag_hi_offset, acc16_row), judged by tests/test_screen_shape16_host.py. It builds stored tiles the way
// quantize_screen_kernel does (per K = 64 step ks, lane 32 h + row: pack32 of the 32 codes 64 ks + 32 h .., 16 bytes in the first
// plane and 8 in the second), reads them back through the map as the kernel's lanes do, and restates the matrix instruction by its
// definition: operand lane l = row l & 15, K block l >> 4 of a K = 128 step; result lane (j, kg), register r = D[4 kg + r][j].
// Prints one JSON object of failure counts (all zero when the map is right) and of what was covered.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../eacham_amd/csrc/match_screen.hpp"

using namespace eacham;

constexpr int ROWS = 32, DIM = 256, KSTEPS = 4, TILE_BYTES = KSTEPS * screen::STEP_BYTES;

// the stored image of one tile from codes[row][k]
static std::vector<unsigned char> store_tile(const std::vector<unsigned char>& codes) {
    std::vector<unsigned char> img(TILE_BYTES, 0);
    for (int ks = 0; ks < KSTEPS; ++ks)
        for (int h = 0; h < 2; ++h)
            for (int row = 0; row < ROWS; ++row) {
                uint32_t w[6];
                screen::pack32(&codes[(size_t)row * DIM + 64 * ks + 32 * h], w);
                const int lane = 32 * h + row;
                std::memcpy(&img[ks * screen::STEP_BYTES + 16 * lane], w, 16);
                std::memcpy(&img[ks * screen::STEP_BYTES + 1024 + 8 * lane], w + 4, 8);
            }
    return img;
}
// the 32 codes a lane holds after its two reads at the map's offsets
static void read_frag(const std::vector<unsigned char>& img, screen::FragSrc src, int out[32]) {
    uint32_t w[6];
    std::memcpy(w, &img[screen::frag_lo_offset(src)], 16);
    std::memcpy(w + 4, &img[screen::frag_hi_offset(src)], 8);
    for (int e = 0; e < 32; ++e) out[e] = screen::unpack32(w, e);
}
// D = C + A B of v_mfma_*_16x16x128 on integers: a[l][e], b[l][e] = element e of operand lane l, c / d[l][r] = register r of lane l
static void mfma16(const int a[64][32], const int b[64][32], const long long c[64][4], long long d[64][4]) {
    for (int lo = 0; lo < 64; ++lo)
        for (int r = 0; r < 4; ++r) {
            const int i = 4 * (lo >> 4) + r, j = lo & 15;
            long long sum = c[lo][r];
            for (int kb = 0; kb < 4; ++kb)
                for (int e = 0; e < 32; ++e) sum += (long long)a[i + 16 * kb][e] * b[j + 16 * kb][e];
            d[lo][r] = sum;
        }
}

int main() {
    long bad_row = 0, bad_block = 0, bad_step = 0, bad_cover = 0, bad_query = 0, bad_group = 0, bad_product = 0, bad_bounds = 0;
    // 1. identifiers: code plane p of position (row, k) = bits 6 p .. 6 p + 5 of id = 256 row + k (13 bits: three planes)
    std::vector<unsigned char> img[3];
    for (int p = 0; p < 3; ++p) {
        std::vector<unsigned char> codes((size_t)ROWS * DIM);
        for (int row = 0; row < ROWS; ++row)
            for (int k = 0; k < DIM; ++k) codes[(size_t)row * DIM + k] = (unsigned char)(((256 * row + k) >> (6 * p)) & 63);
        img[p] = store_tile(codes);
    }
    int cover[ROWS][8] = {};
    for (int u = 0; u < 2; ++u)
        for (int S = 0; S < 2; ++S)
            for (int lane = 0; lane < 64; ++lane) {
                const screen::FragSrc src = screen::frag16_src(u, S, lane);
                if (screen::frag_lo_offset(src) < 0 || screen::frag_lo_offset(src) + 16 > TILE_BYTES || screen::frag_hi_offset(src) < 0 ||
                    screen::frag_hi_offset(src) + 8 > TILE_BYTES || src.row < 0 || src.row >= ROWS) {
                    ++bad_bounds;
                    continue;
                }
                int c[3][32];
                for (int p = 0; p < 3; ++p) read_frag(img[p], src, c[p]);
                const int kb = screen::frag_kblock(src);
                for (int e = 0; e < 32; ++e) {
                    const int id = c[0][e] | (c[1][e] << 6) | (c[2][e] << 12), row = id >> 8, k = id & 255;
                    if (row != 16 * u + (lane & 15) || row != src.row) ++bad_row;
                    if (k != 32 * kb + e) ++bad_block;      // one K block, its codes ascending
                }
                if ((kb >> 2) != S) ++bad_step;             // a block of the K = 128 step S
                ++cover[src.row][kb];
                // the query side names the same K block for the same lane, whichever sub-tile
                for (int s4 = 0; s4 < 4; ++s4) {
                    const screen::FragSrc q = screen::query16_src(s4, S, lane);
                    if (screen::frag_kblock(q) != kb || q.row != 16 * (s4 & 1) + (lane & 15) || screen::query16_tile(s4) != (s4 >> 1)) ++bad_query;
                }
                for (int r = 0; r < 4; ++r) {
                    const int row = screen::acc16_row(u, lane, r);
                    if ((row >> 2) != 4 * u + (lane >> 4) || (row & 3) != r) ++bad_group;
                }
            }
    for (int row = 0; row < ROWS; ++row)
        for (int kb = 0; kb < 8; ++kb)
            if (cover[row][kb] != 1) ++bad_cover;

    // 2. a 64 x 32 x 256 product in the kernel's order against the integer |M_a - M_b|^2 of screen::decode
    std::mt19937 rng(16128);
    long products = 0;
    for (int round = 0; round < 3; ++round) {
        std::vector<unsigned char> tc((size_t)ROWS * DIM), qc[2];
        for (auto& v : tc) v = (unsigned char)(rng() & 63);
        for (int t = 0; t < 2; ++t) {
            qc[t].resize((size_t)ROWS * DIM);
            for (auto& v : qc[t]) v = (unsigned char)(rng() & 63);
        }
        if (round == 1)   // padded dimensions carry code 0 on both sides
            for (int row = 0; row < ROWS; ++row)
                for (int k = 129; k < DIM; ++k) tc[(size_t)row * DIM + k] = qc[0][(size_t)row * DIM + k] = qc[1][(size_t)row * DIM + k] = 0;
        const std::vector<unsigned char> timg = store_tile(tc), qimg[2] = {store_tile(qc[0]), store_tile(qc[1])};
        long long m2b[ROWS], m2a[64];
        for (int row = 0; row < ROWS; ++row) {
            m2b[row] = 0;
            for (int k = 0; k < DIM; ++k) m2b[row] += (long long)screen::decode(tc[(size_t)row * DIM + k]) * screen::decode(tc[(size_t)row * DIM + k]);
        }
        for (int j = 0; j < 64; ++j) {
            m2a[j] = 0;
            for (int k = 0; k < DIM; ++k) {
                const int m = screen::decode(qc[j >> 5][(size_t)(j & 31) * DIM + k]);
                m2a[j] += (long long)m * m;
            }
        }
        for (int u = 0; u < 2; ++u)
            for (int s4 = 0; s4 < 4; ++s4) {
                // everything doubled to stay in integers: C-init |M_b|^2, products -2 M_a M_b (the query's sign flipped)
                long long acc[64][4], next[64][4];
                for (int lane = 0; lane < 64; ++lane)
                    for (int r = 0; r < 4; ++r) acc[lane][r] = m2b[screen::acc16_row(u, lane, r)];
                for (int S = 0; S < 2; ++S) {
                    int a[64][32], b[64][32];
                    for (int lane = 0; lane < 64; ++lane) {
                        int c[32];
                        read_frag(timg, screen::frag16_src(u, S, lane), c);
                        for (int e = 0; e < 32; ++e) a[lane][e] = screen::decode(c[e]);
                        read_frag(qimg[screen::query16_tile(s4)], screen::query16_src(s4, S, lane), c);
                        for (int e = 0; e < 32; ++e) b[lane][e] = -2 * screen::decode(c[e]);
                    }
                    mfma16(a, b, acc, next);
                    std::memcpy(acc, next, sizeof(acc));
                }
                for (int lane = 0; lane < 64; ++lane)
                    for (int r = 0; r < 4; ++r) {
                        const int trow = screen::acc16_row(u, lane, r), j = 16 * s4 + (lane & 15);
                        long long n = 0;
                        for (int k = 0; k < DIM; ++k) {
                            const int d = screen::decode(qc[j >> 5][(size_t)(j & 31) * DIM + k]) - screen::decode(tc[(size_t)trow * DIM + k]);
                            n += (long long)d * d;
                        }
                        if (acc[lane][r] + m2a[j] != n) ++bad_product;
                        ++products;
                    }
            }
    }
    std::printf("{\"bad_bounds\": %ld, \"bad_row\": %ld, \"bad_block\": %ld, \"bad_step\": %ld, \"bad_cover\": %ld, \"bad_query\": %ld, \"bad_group\": %ld, "
                "\"bad_product\": %ld, \"fragments\": %d, \"products\": %ld}\n",
                bad_bounds, bad_row, bad_block, bad_step, bad_cover, bad_query, bad_group, bad_product, 2 * 2 * 64, products);
    return 0;
}
