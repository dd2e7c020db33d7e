// CPU driver of the query-side map of the screen sweep with 128 rows per wave (eacham_amd/csrc/match_screen.hpp: query16_tile,
// query16_src, query16_block, query16_wave_row over QUERY_SUBTILES = 8 sub-tiles), judged by tests/test_screen_rows128_host.py. It
// builds the wave's four stored query tiles and a train tile the way quantize_screen_kernel does, reads them back through the map as
// the kernel's lanes do, and runs the sweep of one train tile in the kernel's order: ONE set of accumulators, four steps (u, S) =
// (0,0) (1,0) (0,1) (1,1) of eight MFMAs, the chains of row half 0 consumed behind step 2 and those of half 1 behind step 3, then
// the tail per wave-block of 64 rows with one row per lane. Prints one JSON object of failure counts (all zero when the map is
// right) and of what was covered.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../eacham_amd/csrc/match_screen.hpp"

using namespace eacham;

constexpr int ROWS = 32, DIM = 256, KSTEPS = 4, TILE_BYTES = KSTEPS * screen::STEP_BYTES;
constexpr int NQ = screen::QUERY_SUBTILES, WAVE_TILES = NQ / 2, WAVE_ROWS = ROWS * WAVE_TILES;

// the stored image of one tile from codes[row][k]
static std::vector<unsigned char> store_tile(const unsigned char* codes) {
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
    long bad_bounds = 0, bad_row = 0, bad_block = 0, bad_cover = 0, bad_wave_block = 0, bad_owner = 0, bad_product = 0, bad_minimum = 0;
    // 1. identifiers: code plane p of position (wave row, k) = bits 6 p .. 6 p + 5 of id = 256 row + k (15 bits: three planes)
    std::vector<unsigned char> img[3][WAVE_TILES];
    for (int p = 0; p < 3; ++p)
        for (int t = 0; t < WAVE_TILES; ++t) {
            std::vector<unsigned char> codes((size_t)ROWS * DIM);
            for (int row = 0; row < ROWS; ++row)
                for (int k = 0; k < DIM; ++k) codes[(size_t)row * DIM + k] = (unsigned char)(((256 * (ROWS * t + row) + k) >> (6 * p)) & 63);
            img[p][t] = store_tile(codes.data());
        }
    static int cover[WAVE_ROWS][8];
    for (int s8 = 0; s8 < NQ; ++s8)
        for (int S = 0; S < 2; ++S)
            for (int lane = 0; lane < 64; ++lane) {
                const screen::FragSrc src = screen::query16_src(s8, S, lane);
                const int tile = screen::query16_tile(s8);
                if (tile < 0 || tile >= WAVE_TILES || screen::frag_lo_offset(src) < 0 || screen::frag_lo_offset(src) + 16 > TILE_BYTES ||
                    screen::frag_hi_offset(src) < 0 || screen::frag_hi_offset(src) + 8 > TILE_BYTES || src.row < 0 || src.row >= ROWS) {
                    ++bad_bounds;
                    continue;
                }
                int c[3][32];
                for (int p = 0; p < 3; ++p) read_frag(img[p][tile], src, c[p]);
                // the K block is the one the train side gives this lane in step S
                const int kb = screen::frag_kblock(src);
                if (kb != screen::frag_kblock(screen::frag16_src(0, S, lane)) || kb != screen::frag_kblock(screen::frag16_src(1, S, lane))) ++bad_block;
                for (int e = 0; e < 32; ++e) {
                    const int id = c[0][e] | (c[1][e] << 6) | (c[2][e] << 12), row = id >> 8, k = id & 255;
                    if (row != 16 * s8 + (lane & 15) || row != screen::query16_wave_row(s8, lane)) ++bad_row;   // the wave's rows 16 s8 ..
                    if (k != 32 * kb + e) ++bad_block;
                }
                ++cover[screen::query16_wave_row(s8, lane)][kb];
                // wave-block of the sub-tile: its rows lie in that block of 64, its tile is one of the block's two
                if (screen::query16_block(s8) != screen::query16_wave_row(s8, lane) / 64 || tile / 2 != screen::query16_block(s8) ||
                    screen::query16_tile(s8 & 3) != tile % 2)
                    ++bad_wave_block;
            }
    for (int row = 0; row < WAVE_ROWS; ++row)
        for (int kb = 0; kb < 8; ++kb)
            if (cover[row][kb] != 1) ++bad_cover;
    // the tail: in wave-block H lane t keeps the pair of sub-tile 4 H + (t >> 4) and owns row t of the block — that sub-tile's column t & 15
    for (int H = 0; H < 2; ++H)
        for (int t = 0; t < 64; ++t) {
            const int s8 = 4 * H + (t >> 4);
            if (screen::query16_block(s8) != H || screen::query16_wave_row(s8, t) != 64 * H + t || screen::query16_tile(s8) != 2 * H + (t >> 5)) ++bad_owner;
        }

    // 2. 128 query rows x 32 train rows x 256 codes in the kernel's order against the integer |M_a - M_b|^2 of screen::decode
    std::mt19937 rng(128128);
    long products = 0, minima = 0;
    for (int round = 0; round < 2; ++round) {
        std::vector<unsigned char> tc((size_t)ROWS * DIM), qc((size_t)WAVE_ROWS * DIM);
        for (auto& v : tc) v = (unsigned char)(rng() & 63);
        for (auto& v : qc) v = (unsigned char)(rng() & 63);
        if (round == 1) {   // padded dimensions carry code 0 on both sides
            for (int row = 0; row < ROWS; ++row)
                for (int k = 129; k < DIM; ++k) tc[(size_t)row * DIM + k] = 0;
            for (int row = 0; row < WAVE_ROWS; ++row)
                for (int k = 129; k < DIM; ++k) qc[(size_t)row * DIM + k] = 0;
        }
        const std::vector<unsigned char> timg = store_tile(tc.data());
        std::vector<unsigned char> qimg[WAVE_TILES];
        for (int t = 0; t < WAVE_TILES; ++t) qimg[t] = store_tile(&qc[(size_t)ROWS * t * DIM]);
        long long m2b[ROWS], m2a[WAVE_ROWS];
        for (int row = 0; row < ROWS; ++row) {
            m2b[row] = 0;
            for (int k = 0; k < DIM; ++k) m2b[row] += (long long)screen::decode(tc[(size_t)row * DIM + k]) * screen::decode(tc[(size_t)row * DIM + k]);
        }
        for (int j = 0; j < WAVE_ROWS; ++j) {
            m2a[j] = 0;
            for (int k = 0; k < DIM; ++k) m2a[j] += (long long)screen::decode(qc[(size_t)j * DIM + k]) * screen::decode(qc[(size_t)j * DIM + k]);
        }
        // the direct distances and, per query row, the minimum over each group of four train rows (a tile's eight subsets)
        static long long n[WAVE_ROWS][ROWS];
        for (int j = 0; j < WAVE_ROWS; ++j)
            for (int trow = 0; trow < ROWS; ++trow) {
                long long s = 0;
                for (int k = 0; k < DIM; ++k) {
                    const int d = screen::decode(qc[(size_t)j * DIM + k]) - screen::decode(tc[(size_t)trow * DIM + k]);
                    s += (long long)d * d;
                }
                n[j][trow] = s;
            }
        // one set of accumulators acc[u][s8]; everything doubled to stay in integers: C-init |M_b|^2, products -2 M_a M_b
        static long long acc[2][NQ][64][4], xm[NQ][2][64];
        auto consume = [&](int u) {
            for (int s8 = 0; s8 < NQ; ++s8)
                for (int lane = 0; lane < 64; ++lane) {
                    long long m = acc[u][s8][lane][0];
                    for (int r = 1; r < 4; ++r) m = acc[u][s8][lane][r] < m ? acc[u][s8][lane][r] : m;
                    xm[s8][u][lane] = m;
                }
        };
        for (int step = 0; step < 4; ++step) {
            const int u = step % 2, S = step / 2;
            int a[64][32];
            for (int lane = 0; lane < 64; ++lane) {
                int c[32];
                read_frag(timg, screen::frag16_src(u, S, lane), c);
                for (int e = 0; e < 32; ++e) a[lane][e] = screen::decode(c[e]);
            }
            for (int s8 = 0; s8 < NQ; ++s8) {
                int b[64][32];
                for (int lane = 0; lane < 64; ++lane) {
                    int c[32];
                    read_frag(qimg[screen::query16_tile(s8)], screen::query16_src(s8, S, lane), c);
                    for (int e = 0; e < 32; ++e) b[lane][e] = -2 * screen::decode(c[e]);
                }
                long long cin[64][4], next[64][4];
                for (int lane = 0; lane < 64; ++lane)
                    for (int r = 0; r < 4; ++r) cin[lane][r] = S ? acc[u][s8][lane][r] : m2b[screen::acc16_row(u, lane, r)];
                mfma16(a, b, cin, next);
                std::memcpy(acc[u][s8], next, sizeof(next));
            }
            if (step == 2) {   // the chains of row half 0 have ended: checked, then consumed (under step 3 in the kernel)
                for (int s8 = 0; s8 < NQ; ++s8)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int r = 0; r < 4; ++r, ++products)
                            if (acc[0][s8][lane][r] + m2a[screen::query16_wave_row(s8, lane)] != n[screen::query16_wave_row(s8, lane)][screen::acc16_row(0, lane, r)]) ++bad_product;
                consume(0);
            }
        }
        for (int s8 = 0; s8 < NQ; ++s8)
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 4; ++r, ++products)
                    if (acc[1][s8][lane][r] + m2a[screen::query16_wave_row(s8, lane)] != n[screen::query16_wave_row(s8, lane)][screen::acc16_row(1, lane, r)]) ++bad_product;
        consume(1);   // (under step 0 of the next tile, or by last())
        // the tail of wave-block H: lane t's row 64 H + t, the minimum over the row's column (lanes t & 15 + 16 kg of its sub-tile) and both halves
        for (int H = 0; H < 2; ++H)
            for (int t = 0; t < 64; ++t, ++minima) {
                const int s8 = 4 * H + (t >> 4), row = 64 * H + t;
                long long got = xm[s8][0][t & 15], want = n[row][0];
                for (int u = 0; u < 2; ++u)
                    for (int kg = 0; kg < 4; ++kg) got = xm[s8][u][(t & 15) + 16 * kg] < got ? xm[s8][u][(t & 15) + 16 * kg] : got;
                for (int trow = 1; trow < ROWS; ++trow) want = n[row][trow] < want ? n[row][trow] : want;
                if (got + m2a[row] != want) ++bad_minimum;
            }
    }
    std::printf("{\"bad_bounds\": %ld, \"bad_row\": %ld, \"bad_block\": %ld, \"bad_cover\": %ld, \"bad_wave_block\": %ld, \"bad_owner\": %ld, "
                "\"bad_product\": %ld, \"bad_minimum\": %ld, \"fragments\": %d, \"products\": %ld, \"minima\": %ld}\n",
                bad_bounds, bad_row, bad_block, bad_cover, bad_wave_block, bad_owner, bad_product, bad_minimum, NQ * 2 * 64, products, minima);
    return 0;
}
