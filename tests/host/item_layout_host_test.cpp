// Host check of the k_expand work decomposition (fhh_internal.h item_layout) and of the
// item -> (entry range, word range) decode k_expand runs (fhh_internal.h item_range, the same
// function the kernel calls; the job search restates k_expand's loop): for random job sizes,
// every (job, entry, word) is covered exactly once, no item is empty or reaches past n_live or
// nw, and a multi-word layout still gives every wave at least kMwItemsPerWave items.
// Built with hipcc (host code only) by tests/test_host_aes.py; prints "OK" on success.
#include "../../fuzzyheavyhitters_amd/csrc/fhh_internal.h"
#include <cstdio>
#include <random>
#include <vector>

int main() {
    std::mt19937_64 rng(7);
    int fails = 0;
    for (int it = 0; it < 3000; it++) {
        const uint32_t njobs = 1 + rng() % fhh::kMaxJobs;
        const uint32_t unit = 1 + rng() % 64;
        const uint32_t max_group = 1 + rng() % 16;
        const uint64_t waves = 1 + rng() % 512;
        const uint32_t max_wpi = (rng() & 1) ? 1u : 1u + (uint32_t)(rng() % 16);
        uint32_t n_live[fhh::kMaxJobs] = {};
        for (uint32_t k = 0; k < njobs; k++) n_live[k] = (it % 7 == 0) ? (uint32_t)(rng() % 3) : (uint32_t)(rng() % 700);
        fhh::ItemLayout L;
        fhh::item_layout(n_live, njobs, unit, max_group, waves, L, max_wpi);
        std::vector<std::vector<uint8_t>> seen(njobs);
        for (uint32_t k = 0; k < njobs; k++) seen[k].assign((size_t)n_live[k] * unit, 0);
        if (L.g < 1 || L.g > max_group) fails++;
        if (L.wpi < 1 || L.wpi > max_wpi) fails++;
        if (L.wpi > 1 && L.total < fhh::kMwItemsPerWave * waves) fails++;
        for (uint64_t item = 0; item < L.total; item++) {
            uint32_t ji = 0;
            while (ji + 1 < njobs && item >= L.begin[ji + 1]) ji++;
            const fhh::ItemRange r = fhh::item_range(item - L.begin[ji], n_live[ji], unit, L.g, L.wpi);
            if (r.e0 >= r.e1 || r.e1 > n_live[ji]) { fails++; continue; }   // an item with no work
            if (r.w0 >= r.w1 || r.w1 > unit) { fails++; continue; }
            for (uint32_t e = r.e0; e < r.e1; e++)
                for (uint32_t w = r.w0; w < r.w1; w++) seen[ji][(size_t)e * unit + w]++;
        }
        for (uint32_t k = 0; k < njobs; k++)
            for (uint8_t v : seen[k])
                if (v != 1) { fails++; break; }
    }
    // the narrow / wide cases of DESIGN.md §5 at 1M clients (nw 15 625, 4 096 waves)
    {
        const uint32_t narrow[4] = {1, 1, 1, 1};   // configs[3]: ~1 entry per (server, dim)
        fhh::ItemLayout L;
        fhh::item_layout(narrow, 4, 15625, 16, 4096, L, 16);
        if (L.wpi != 3 || L.total != 4 * 5209) fails++;   // lowered until 4 items per wave
        const uint32_t wide[2] = {200, 200};                // a deep d = 1 level
        fhh::item_layout(wide, 2, 15625, 16, 4096, L, 16);
        if (L.g != 16) fails++;
        if (L.wpi != 1) fails++;
    }
    if (fails) { std::printf("FAIL %d\n", fails); return 1; }
    std::printf("OK\n");
    return 0;
}
