// The b = 3, 4 garbled-table kernels' view of the labels OT's tile-major matrix (fhh_gc.hip gt_tile_rows): the
// word addressing of a 512-test window that starts at any even word of a tile, and the row-domain fold of a
// test's b labels into its Horner key. Host self-test tests/host/gt_window_host_test.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fhh {

constexpr uint32_t kGtTileWords = 128 * 16;   // one 512-OT tile of Q / T: 128 rows x 16 words

// word w (of 32 tests) of a group's plane row of nw2 = 2 nw words, or the row's last word where w lies beyond it
// (the tail of the group's last window): every load stays inside the bit's own OTs
__host__ __device__ __forceinline__ uint32_t gt_window_word(uint32_t w, uint32_t nw2) { return w < nw2 ? w : nw2 - 1; }

// 32-OT word column of the matrix that holds word w of bit k of group g (OT index (g b + k) 64 nw + 32 w)
__host__ __device__ __forceinline__ uint64_t gt_window_col(uint64_t g, uint32_t b, uint32_t k, uint32_t nw2, uint32_t w) {
    return (g * b + k) * nw2 + w;
}

// row 0's word of column col: word col % 16 of tile col / 16 (row r: + 16 r)
__host__ __device__ __forceinline__ uint64_t gt_col_offset(uint64_t col) { return (col >> 4) * kGtTileWords + (col & 15); }

// Rows 32 rg .. 32 rg + 31 of S = e_0 ^ sigma(e_1) ^ .. ^ sigma^(B-1)(e_(B-1)) for the 32 tests of word w of group
// g, into x (x[i] = row 32 rg + i; the caller transposes). Row r of sigma^k(e) is row r - k of e; the k rows
// shifted out, 128 - k + j (j < k), come back by x^128 = x^7 + x^2 + x + 1 into rows j, j + 1, j + 2, j + 7 —
// all within rows 0 .. 9, lane group rg = 0. No branch depends on the lane: a branch around the loads made the
// compiler keep x as one 32-register tuple and spill it whole.
template <int B>
__host__ __device__ __forceinline__ void gt_window_fold(const uint32_t* lab, uint64_t g, uint32_t nw2, uint32_t w,
                                                        uint32_t rg, uint32_t (&x)[32]) {
#pragma unroll
    for (int i = 0; i < 32; i++) x[i] = 0u;
#pragma unroll
    for (int k = 0; k < B; k++) {
        const uint32_t* tk = lab + gt_col_offset(gt_window_col(g, B, k, nw2, w));
#pragma unroll
        for (int i = 0; i < k; i++) {   // rg = 0: the wrapped rows 128 - k + i
            const uint32_t y = __builtin_nontemporal_load(tk + (rg ? 32 * rg + i - k : 128 - k + i) * 16);
            const uint32_t yr = rg ? 0u : y;
            x[i] ^= y;
            x[i + 1] ^= yr;
            x[i + 2] ^= yr;
            x[i + 7] ^= yr;
        }
#pragma unroll
        for (int i = k; i < 32; i++) {
            x[i] ^= __builtin_nontemporal_load(tk + (32 * rg + i - k) * 16);
#if defined(__HIP_DEVICE_COMPILE__)
            if (B == 4 && i == 15) __builtin_amdgcn_sched_barrier(0);
#endif
        }
#if defined(__HIP_DEVICE_COMPILE__)
        // b = 4: half a bit's words in flight beside x; with all four bits' loads issued first the kernels spilled
        if (B == 4 && k + 1 < B) __builtin_amdgcn_sched_barrier(0);
#endif
    }
}

}  // namespace fhh
