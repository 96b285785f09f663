// Host self-test of csrc/bincode_span.h, the span arithmetic of an appended add_keys batch: for an edge list
// and random (c0, m), over the words bc_span_words gives,
//   - every destination client in [c0, c0 + m) is taken exactly once, by the lane (c mod 64) of the word
//     (c / 64), from the source record c - c0,
//   - no lane before c0 and no lane of another word is touched,
//   - the tail-zero mask is exactly the lanes after the batch in its last word, and empty in every other word,
//   - an empty batch (m = 0) inside a word is that word's lanes from c0 on as tail and nothing else; at a word
//     boundary it is no word at all.
// A sequence of batches is also replayed on a model layout: after every batch the lanes past the running count
// in the words written so far are zero, and the lanes below it hold their own client.
#include <cstdio>
#include <random>
#include <vector>

#include "../../fuzzyheavyhitters_amd/csrc/bincode_span.h"

static int check(uint64_t c0, uint64_t m) {
    const uint64_t nwb = fhh::bc_span_words(c0, m), w0 = fhh::bc_span_first_word(c0);
    if (m == 0) {
        if (nwb != ((c0 % 64) ? 1u : 0u)) return std::printf("FAIL words of the empty batch at %llu\n", (unsigned long long)c0);
    } else if (w0 != c0 / 64 || w0 + nwb - 1 != (c0 + m - 1) / 64) {
        return std::printf("FAIL words c0 %llu m %llu\n", (unsigned long long)c0, (unsigned long long)m);
    }
    std::vector<uint32_t> hits(m, 0);
    for (uint64_t j = 0; j < nwb; j++) {
        const fhh::BcWord s = fhh::bc_span_word(c0, m, j);
        const uint64_t base = (w0 + j) * 64;
        if (s.lanes & s.tail) return std::printf("FAIL lanes and tail overlap\n");
        for (uint32_t l = 0; l < 64; l++) {
            const uint64_t c = base + l;
            const bool in = (s.lanes >> l) & 1, tz = (s.tail >> l) & 1;
            if (in != (c >= c0 && c < c0 + m))
                return std::printf("FAIL lane c0 %llu m %llu word %llu lane %u\n", (unsigned long long)c0,
                                   (unsigned long long)m, (unsigned long long)j, l);
            if (in) {
                const int64_t src = s.src0 + (int64_t)l;
                if (src < 0 || (uint64_t)src >= m || (uint64_t)src != c - c0) return std::printf("FAIL source record\n");
                hits[(size_t)src]++;
            }
            // the lanes after the batch's end, in its last word only
            if (tz != (j + 1 == nwb && c >= c0 + m))
                return std::printf("FAIL tail c0 %llu m %llu word %llu lane %u\n", (unsigned long long)c0,
                                   (unsigned long long)m, (unsigned long long)j, l);
            if (c < c0 && (in || tz)) return std::printf("FAIL a lane before c0 is touched\n");
        }
    }
    for (uint64_t i = 0; i < m; i++)
        if (hits[(size_t)i] != 1) return std::printf("FAIL record %llu taken %u times\n", (unsigned long long)i, hits[(size_t)i]);
    return 0;
}

// batches replayed on a model: cell = client index + 1 (0 = zero lane), -1 = never written
static int replay(const std::vector<uint64_t>& batches) {
    uint64_t total = 0;
    for (uint64_t b : batches) total += b;
    std::vector<int64_t> cell((total / 64 + 2) * 64, -1);
    uint64_t n = 0;
    for (uint64_t m : batches) {
        const uint64_t nwb = fhh::bc_span_words(n, m), w0 = fhh::bc_span_first_word(n);
        for (uint64_t j = 0; j < nwb; j++) {
            const fhh::BcWord s = fhh::bc_span_word(n, m, j);
            for (uint32_t l = 0; l < 64; l++) {
                int64_t& x = cell[(size_t)((w0 + j) * 64 + l)];
                if ((s.lanes >> l) & 1) x = (int64_t)(n + (uint64_t)(s.src0 + (int64_t)l)) + 1;
                else if ((s.tail >> l) & 1) x = 0;
            }
        }
        n += m;
        const uint64_t used = (n + 63) / 64 * 64;
        for (uint64_t c = 0; c < used; c++)
            if (cell[(size_t)c] != (c < n ? (int64_t)c + 1 : 0))
                return std::printf("FAIL replay: client %llu after %llu clients\n", (unsigned long long)c, (unsigned long long)n);
    }
    return 0;
}

int main() {
    const uint64_t c0s[] = {0, 1, 30, 62, 63, 64, 65, 127, 128, 129, 133, 199, (1ull << 31) - 1, (1ull << 31) + 63, (1ull << 40) + 5};
    const uint64_t ms[] = {0, 1, 2, 5, 25, 62, 63, 64, 65, 67, 100, 127, 128, 129, 200, 1000};
    for (uint64_t c0 : c0s)
        for (uint64_t m : ms)
            if (check(c0, m)) return 1;
    std::mt19937_64 rng(20240611);
    for (int it = 0; it < 20000; it++) {
        const uint64_t c0 = rng() % 5000, m = rng() % 700;
        if (check(c0, m)) return 1;
    }
    if (replay({1, 62, 1, 64, 5, 67}) || replay({100, 30}) || replay({64}) || replay({64, 1}) || replay({30, 25, 15}))
        return 1;
    for (int it = 0; it < 200; it++) {
        std::vector<uint64_t> b;
        for (int k = 0; k < 12; k++) b.push_back(1 + rng() % 150);
        if (replay(b)) return 1;
    }
    std::printf("OK\n");
    return 0;
}
