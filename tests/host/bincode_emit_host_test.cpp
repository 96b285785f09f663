// Host self-test of csrc/bincode_emit.h, the span arithmetic of serialized add_keys requests. For an edge list
// and random (first, count, batch, d, L, n) the writers of k_bincode_emit_cw / k_bincode_emit_headers are
// replayed on a model of the output, owner by owner, exactly as the kernels cut them: per request its u64 m (by
// the thread of its first client), per client its u64 d, per key its 25 header bytes, per (source word, key,
// level block) tile and in-range lane one CW segment as head bytes, aligned interior dwords and tail bytes.
//   - every byte of [0, len) has exactly one writer, and len = 8 ceil(count / B) + count R,
//   - nothing is written outside [0, len) (a write there fails at once),
//   - every interior dword is 4-byte aligned and lies inside its own segment (so it is shared with no other
//     writer), head and tail are at most 3 bytes,
//   - a slice [i0, i0 + m) cut at any client (a shard boundary) writes exactly [be_slice_begin, be_slice_end),
//     and the slices of a cut tile [0, len),
//   - a segment sits where the decoder reads it, and the offsets hold past 2^32 (the last client of 1M at
//     L = 512).
#include <cstdio>
#include <random>
#include <vector>

#include "../../fuzzyheavyhitters_amd/csrc/bincode_emit.h"

using namespace fhh;
typedef unsigned long long ull;

struct Model {
    std::vector<uint8_t> hits;
    uint64_t lo, hi;   // the bytes this run may write
    int put(uint64_t g, const char* who) {
        if (g < lo || g >= hi) return std::printf("FAIL %s writes byte %llu outside [%llu, %llu)\n", who, (ull)g, (ull)lo, (ull)hi);
        if (hits[(size_t)g]++) return std::printf("FAIL %s writes byte %llu a second time\n", who, (ull)g);
        return 0;
    }
};

// the writers of clients [src_first, src_first + m) = clients [i0, i0 + m) of the export, as the kernels run them
static int emit_slice(Model& M, uint64_t src_first, uint64_t m, uint64_t i0, uint64_t count, uint64_t B, uint32_t d,
                      uint32_t L) {
    const uint32_t K = 2 * d;
    const uint64_t R = be_record_bytes(d, L);
    // k_bincode_emit_headers
    for (uint64_t j = 0; j < m; j++)
        for (uint32_t kk = 0; kk < K; kk++) {
            const uint64_t i = i0 + j, key = be_key_off(i, kk, L, B, R);
            for (int b = 0; b < 25; b++)
                if (M.put(key + b, "key header")) return 1;
            if (kk == 0) {
                const uint64_t rec = be_client_off(i, B, R);
                for (int b = 0; b < 8; b++)
                    if (M.put(rec + b, "client d")) return 1;
                if (i % B == 0) {
                    const uint64_t mq = be_request_clients(i, count, B);
                    if (mq == 0 || mq > B || i + mq > count || (i + mq < count && mq != B)) return std::printf("FAIL request count\n");
                    for (int b = 0; b < 8; b++)
                        if (M.put(rec - 8 + b, "request m")) return 1;
                }
            }
        }
    // k_bincode_emit_cw: tiles over the source words
    const uint64_t w0 = src_first >> 6, w1 = (src_first + m - 1) >> 6;
    for (uint64_t w = w0; w <= w1; w++)
        for (uint32_t kk = 0; kk < K; kk++)
            for (uint32_t l0 = 0; l0 < L; l0 += kBeLevels) {
                const uint32_t nl = L - l0 < kBeLevels ? L - l0 : kBeLevels, bytes = 20 * nl;
                for (uint32_t ln = 0; ln < 64; ln++) {
                    const uint64_t c = w * 64 + ln;
                    if (c < src_first || c >= src_first + m) continue;
                    const uint64_t i = i0 + (c - src_first), g = be_seg_off(i, kk, l0, L, B, R);
                    // where the decoder looks for this CorWord (k_bincode_cw_tiles: 8 + c R + 8 + kk KB + 25 + 20 l)
                    const uint64_t q = i / B, inq = i % B;
                    if (g != 8 * q + q * B * R + 8 + inq * R + 8 + kk * be_key_bytes(L) + 25 + 20ull * l0)
                        return std::printf("FAIL segment offset\n");
                    const BeSeg s = be_seg_split(g, bytes);
                    if (s.head > 3 || s.tail > 3 || s.head + 4 * s.ndw + s.tail != bytes || s.ndw > 5 * kBeLevels)
                        return std::printf("FAIL split of %u bytes at %llu\n", bytes, (ull)g);
                    if (s.ndw && ((g + s.head) & 3)) return std::printf("FAIL interior unaligned at %llu\n", (ull)g);
                    for (uint32_t b = 0; b < s.head; b++)
                        if (M.put(g + b, "head")) return 1;
                    for (uint32_t k = 0; k < s.ndw; k++) {
                        const uint64_t a = g + s.head + 4ull * k;
                        if (a < g || a + 4 > g + bytes) return std::printf("FAIL interior dword leaves its segment\n");
                        // the row dwords v_alignbit reads: k and k + 1 (k + 1 only when head > 0), inside the 161-dword row
                        if (k + 1 > 5 * kBeLevels) return std::printf("FAIL row index\n");
                        for (int b = 0; b < 4; b++)
                            if (M.put(a + b, "interior")) return 1;
                    }
                    for (uint32_t b = 0; b < s.tail; b++) {
                        const uint32_t bi = s.head + 4 * s.ndw + b;
                        if (bi >= bytes) return std::printf("FAIL tail index\n");
                        if (M.put(g + bi, "tail")) return 1;
                    }
                }
            }
    return 0;
}

static int check(uint64_t n, uint64_t first, uint64_t count, uint64_t batch, uint32_t d, uint32_t L, std::mt19937_64& rng) {
    if (first + count > n) return std::printf("FAIL bad case\n");
    const uint64_t R = be_record_bytes(d, L), B = be_batch(count, batch);
    const uint64_t nreq = (count + B - 1) / B, len = be_total_bytes(count, B, R);
    if (R != 8 + 2ull * d * (25 + 20ull * L) || len != 8 * nreq + count * R) return std::printf("FAIL sizes\n");
    if (be_slice_begin(0, B, R) != 0 || be_slice_end(0, count, B, R) != len) return std::printf("FAIL whole slice\n");
    // one owner of the whole range
    {
        Model M{std::vector<uint8_t>((size_t)len, 0), 0, len};
        if (emit_slice(M, first, count, 0, count, B, d, L)) return 1;
        for (uint64_t g = 0; g < len; g++)
            if (M.hits[(size_t)g] != 1) return std::printf("FAIL byte %llu unwritten (first %llu count %llu batch %llu d %u L %u)\n",
                                                            (ull)g, (ull)first, (ull)count, (ull)batch, d, L);
    }
    // cut into up to three owners at arbitrary clients (shards cut at 64-client words of the population, which
    // are arbitrary clients of the export): each writes exactly its slice's bytes, and the slices tile [0, len)
    if (count >= 2) {
        uint64_t cut[4] = {0, 1 + rng() % (count - 1), 1 + rng() % (count - 1), count};
        if (cut[1] > cut[2]) std::swap(cut[1], cut[2]);
        Model M{std::vector<uint8_t>((size_t)len, 0), 0, 0};
        uint64_t prev_end = 0;
        for (int k = 0; k < 3; k++) {
            const uint64_t i0 = cut[k], m = cut[k + 1] - cut[k];
            if (!m) continue;
            M.lo = be_slice_begin(i0, B, R);
            M.hi = be_slice_end(i0, m, B, R);
            if (M.lo != prev_end) return std::printf("FAIL slices do not tile\n");
            prev_end = M.hi;
            if (emit_slice(M, first + i0, m, i0, count, B, d, L)) return 1;
        }
        if (prev_end != len) return std::printf("FAIL slices end at %llu of %llu\n", (ull)prev_end, (ull)len);
        for (uint64_t g = 0; g < len; g++)
            if (M.hits[(size_t)g] != 1) return std::printf("FAIL byte %llu unwritten by the slices\n", (ull)g);
    }
    return 0;
}

int main() {
    std::mt19937_64 rng(20240913);
    const uint32_t Ls[] = {1, 31, 32, 33, 512};
    // every lane as first % 64, every L of the list, every batch kind
    for (uint32_t lane = 0; lane < 64; lane++) {
        const uint32_t L = Ls[lane % 5], d = 1 + lane % 4;
        const uint64_t first = 64 * (rng() % 3) + lane, count = 1 + rng() % (L == 512 ? 70 : 150), n = first + count + rng() % 5;
        const uint64_t batches[] = {0, 1, count, count + 1, 1 + rng() % count};
        for (uint64_t b : batches)
            if (check(n, first, count, b, d, L, rng)) return 1;
    }
    for (uint32_t L : Ls)
        for (uint32_t d = 1; d <= 4; d++) {
            const uint64_t count = L == 512 ? 66 : 130;
            const uint64_t batches[] = {0, 1, count, count + 1, 7, 100};
            for (uint64_t b : batches)
                if (check(count + 3, 1, count, b, d, L, rng)) return 1;
        }
    for (int it = 0; it < 400; it++) {
        const uint32_t d = 1 + (uint32_t)(rng() % 4), L = (it % 8 == 0) ? Ls[rng() % 5] : 1 + (uint32_t)(rng() % 70);
        const uint64_t first = rng() % 200, count = 1 + rng() % 200, n = first + count + rng() % 100;
        const uint64_t pick[] = {0, 1, count, count + 1, 1 + rng() % (count + 5)};
        if (check(n, first, count, pick[rng() % 5], d, L, rng)) return 1;
    }
    // offsets past 2^32: one client's bytes of a 1M-client export at L = 512 (no model of 20 GB: the slice alone)
    {
        const uint32_t d = 1, L = 512;
        const uint64_t count = 1000000, B = 100, R = be_record_bytes(d, L), i0 = 999999;
        Model M{std::vector<uint8_t>(), be_slice_begin(i0, B, R), be_slice_end(i0, 1, B, R)};
        if (M.hi != be_total_bytes(count, B, R) || M.hi != 20538080000ull) return std::printf("FAIL large sizes\n");
        // count the bytes instead of marking them
        uint64_t written = 0;
        for (uint32_t kk = 0; kk < 2; kk++) {
            const uint64_t key = be_key_off(i0, kk, L, B, R);
            if (key < M.lo || key + be_key_bytes(L) > M.hi) return std::printf("FAIL large key offset\n");
            written += 25;
            for (uint32_t l0 = 0; l0 < L; l0 += kBeLevels) {
                const uint64_t g = be_seg_off(i0, kk, l0, L, B, R);
                const BeSeg s = be_seg_split(g, 20 * kBeLevels);
                if (g != key + 25 + 20ull * l0 || ((g + s.head) & 3) || s.head + 4 * s.ndw + s.tail != 20 * kBeLevels)
                    return std::printf("FAIL large segment\n");
                written += 20 * kBeLevels;
            }
        }
        if (written + 8 != M.hi - M.lo) return std::printf("FAIL large slice size\n");
    }
    std::printf("OK\n");
    return 0;
}
