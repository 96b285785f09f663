// Span arithmetic of an appended add_keys batch (k_bincode_cw_tiles_at / k_keys_from_bincode_at in
// fhh_kernels.hip): a batch of m client records lands on the clients [c0, c0 + m) of the device layout, c0 any
// value, so its first and last 64-client words may be shared with clients that are already there. For word j
// of the batch this gives the lanes the batch owns, the source record of lane 0 and the lanes after the batch's
// end, which the batch's last word writes as zero (the layout's lanes past n hold zero seeds and zero plane
// bits; the next batch overwrites them). m = 0 at a c0 inside a word is the span of that word's lanes from c0
// on, all tail: what re-zeroes the word a refused batch shared. Host self-test
// tests/host/bincode_span_host_test.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fhh {

struct BcWord {
    uint64_t lanes;   // lanes of this word that take a record of the batch
    uint64_t tail;    // lanes after the batch's end (its last word only): written as zero
    int64_t src0;     // lane l takes record src0 + l (negative for the lanes before c0)
};

// bits [0, k) of a word, k <= 64
__host__ __device__ __forceinline__ uint64_t bc_bits_below(uint32_t k) { return k >= 64 ? ~0ull : (1ull << k) - 1; }

// first 64-client word the batch touches
__host__ __device__ __forceinline__ uint64_t bc_span_first_word(uint64_t c0) { return c0 >> 6; }

// number of words the batch touches (0: an empty batch at a word boundary)
__host__ __device__ __forceinline__ uint64_t bc_span_words(uint64_t c0, uint64_t m) {
    if (m == 0) return (c0 & 63) ? 1 : 0;
    return ((c0 + m - 1) >> 6) - (c0 >> 6) + 1;
}

// word j < bc_span_words(c0, m) of the batch: the layout's word bc_span_first_word(c0) + j
__host__ __device__ __forceinline__ BcWord bc_span_word(uint64_t c0, uint64_t m, uint64_t j) {
    const uint64_t base = ((c0 >> 6) + j) << 6, end = c0 + m;
    const uint32_t lo = c0 > base ? (uint32_t)(c0 - base) : 0u;
    const uint32_t hi = end < base + 64 ? (uint32_t)(end - base) : 64u;   // end > base, or end = c0 > base (m = 0)
    BcWord s;
    s.lanes = bc_bits_below(hi) & ~bc_bits_below(lo);
    s.tail = ~bc_bits_below(hi);   // hi < 64 only in the batch's last word
    s.src0 = (int64_t)base - (int64_t)c0;
    return s;
}

}  // namespace fhh
