// Host self-test of csrc/gt_window.h, the b = 3, 4 garbled-table kernels' reading of the labels OT's tile-major
// matrix: for every nw in 1 .. 17 and 42 (Npad = 64 nw, two groups, so a window's tail lies in the next bit's or
// group's OTs, or past the matrix), every window, and every lane (q, rg) of a wave,
//   - the window's start word o / 32 is even and maps to (tile, word) = (o / 512, o % 512 / 32),
//   - a lane past the plane row takes the row's last word, a live lane its own, and every column a lane reads
//     lies inside its bit's own OTs (so inside m),
//   - gt_window_fold + transpose32 gives word rg of S = e_0 ^ sigma(e_1) ^ .. for the lane's 32 tests, with S
//     from the per-label Horner rule S = 2 S ^ e_k in GF(2^128) (x^128 = x^7 + x^2 + x + 1).
#include <cstdio>
#include <random>
#include <vector>

#include "../../fuzzyheavyhitters_amd/csrc/bitslice.h"
#include "../../fuzzyheavyhitters_amd/csrc/gt_window.h"

static void ref_dbl(uint32_t (&x)[4]) {
    const uint32_t carry = x[3] >> 31;
    x[3] = (x[3] << 1) | (x[2] >> 31);
    x[2] = (x[2] << 1) | (x[1] >> 31);
    x[1] = (x[1] << 1) | (x[0] >> 31);
    x[0] = (x[0] << 1) ^ (carry ? 0x87u : 0u);
}

// the 128-bit label of OT o: bit r = bit o % 32 of word o % 512 / 32 of row r of tile o / 512
static void label_of(const std::vector<uint32_t>& M, uint64_t o, uint32_t (&e)[4]) {
    for (int c = 0; c < 4; c++) e[c] = 0;
    for (int r = 0; r < 128; r++) {
        const uint32_t wd = M[(o / 512) * fhh::kGtTileWords + (uint64_t)r * 16 + (o % 512) / 32];
        e[r / 32] |= ((wd >> (o % 32)) & 1u) << (r % 32);
    }
}

template <int B>
static int run(uint32_t nw, std::mt19937& rng) {
    const uint64_t G = 2, Npad = 64ull * nw, m = G * B * Npad, mp = (m + 8191) / 8192 * 8192;
    const uint32_t nw2 = 2 * nw, windows = (nw + 7) / 8;
    std::vector<uint32_t> M(mp * 4);
    for (auto& v : M) v = rng();
    for (uint64_t g = 0; g < G; g++)
        for (uint32_t iw = 0; iw < windows; iw++) {
            for (uint32_t k = 0; k < (uint32_t)B; k++) {   // the window's start word -> (tile, word)
                const uint64_t o = (g * B + k) * Npad + 512ull * iw, col = fhh::gt_window_col(g, B, k, nw2, 16 * iw);
                if (col != o / 32 || col % 2 || fhh::gt_col_offset(col) != (o / 512) * fhh::kGtTileWords + (o % 512) / 32) {
                    std::printf("FAIL start b %d nw %u g %llu iw %u k %u\n", B, nw, (unsigned long long)g, iw, k);
                    return 1;
                }
            }
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t q = lane >> 2, rg = lane & 3, w0 = 16 * iw + q, w = fhh::gt_window_word(w0, nw2);
                if ((w0 < nw2 && w != w0) || (w0 >= nw2 && w != nw2 - 1)) {
                    std::printf("FAIL live word b %d nw %u w0 %u\n", B, nw, w0);
                    return 1;
                }
                for (uint32_t k = 0; k < (uint32_t)B; k++) {   // every column read lies in bit k's own OTs
                    const uint64_t col = fhh::gt_window_col(g, B, k, nw2, w);
                    if (col * 32 < (g * B + k) * Npad || (col + 1) * 32 > (g * B + k + 1) * Npad || (col + 1) * 32 > m) {
                        std::printf("FAIL bounds b %d nw %u g %llu iw %u lane %u k %u\n", B, nw, (unsigned long long)g, iw, lane, k);
                        return 1;
                    }
                }
                uint32_t x[32];
                fhh::gt_window_fold<B>(M.data(), g, nw2, w, rg, x);
                fhh::transpose32(x);   // x[t] = word rg of S for test 32 w + t
                for (uint32_t t = 0; t < 32; t++) {
                    uint32_t S[4] = {0, 0, 0, 0};
                    for (int k = B - 1; k >= 0; k--) {
                        uint32_t e[4];
                        label_of(M, (g * B + k) * Npad + 32ull * w + t, e);
                        ref_dbl(S);
                        for (int c = 0; c < 4; c++) S[c] ^= e[c];
                    }
                    if (x[t] != S[rg]) {
                        std::printf("FAIL fold b %d nw %u g %llu iw %u lane %u test %u: %08x != %08x\n", B, nw,
                                    (unsigned long long)g, iw, lane, t, x[t], S[rg]);
                        return 1;
                    }
                }
            }
        }
    return 0;
}

int main() {
    std::mt19937 rng(11);
    for (uint32_t nw = 1; nw <= 42; nw = nw == 17 ? 42 : nw + 1)
        if (run<3>(nw, rng) || run<4>(nw, rng)) return 1;
    std::printf("OK\n");
    return 0;
}
