// fhh_retain_clients' two gather kernels: the survivors of a keep mask, in their old order, into
// buffers of the smaller collection's layout (fhh_internal.h: npad' = 64 nw', nw' = ceil(n' / 64)).
// Both read idx[c] = the old index of survivor c (fhh_retain_plan's src list, uploaded once) and,
// for a prefix table, rows[r] = the source row of destination row r (the live entries, made dense).
//
// Never in place: destination column c of a row is the source column of some c'' <= c of the same
// row, and once npad' < npad the destination rows overlap earlier source rows, so no launch order
// of one grid is safe. Every array is gathered into a new exact-size buffer that replaces the old
// one after the stream has drained (fhh_retain.cpp); the old one is then freed. Peak extra device
// memory: the survivors' collection itself, (n' / n) of what the ctx holds in keys and live entries.
#include "fhh_internal.h"

namespace fhh {

namespace {

constexpr int kRetainThreads = 256;     // one lane per destination column; a wave = one 64-client word
constexpr int kRetainRows = 4;          // rows in flight per lane (independent 16-B loads)
constexpr uint64_t kRetainBlocks = 2048;   // blocks of a launch: 8 resident per CU x 256 CUs; rows beyond are strided

typedef uint32_t rt_v4 __attribute__((ext_vector_type(4)));   // for the nontemporal builtins

// grid.y of a launch of `groups` row groups over `tiles` column tiles
unsigned retain_grid_y(uint64_t groups, uint64_t tiles) {
    uint64_t gy = kRetainBlocks / tiles;
    if (gy < 1) gy = 1;
    if (gy > groups) gy = groups;
    if (gy > 65535) gy = 65535;
    return (unsigned)gy;
}

}  // namespace

// 16-byte-per-client arrays (cw_seed, root_seed, a table's seed): dst[r][c] = src[rows ? rows[r] : r][idx[c]]
// for c < n2, zero for n2 <= c < npad2. The data is touched once: streaming (nontemporal) loads and stores, 1 - 3 %
// faster than plain ones over a dense mask and equal over a 50 % one (profiles/retain/). Over a dense mask idx[c]
// runs with c, so both sides are coalesced.
__global__ __launch_bounds__(kRetainThreads) void k_retain_cols(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                                const uint32_t* __restrict__ idx,
                                                                const uint32_t* __restrict__ rows, uint64_t n_rows,
                                                                uint64_t npad, uint64_t npad2, uint32_t n2) {
    const uint64_t c = (uint64_t)blockIdx.x * kRetainThreads + threadIdx.x;
    if (c >= npad2) return;
    const bool live = c < n2;
    const uint64_t sc = live ? idx[c] : 0;
    for (uint64_t r0 = (uint64_t)blockIdx.y * kRetainRows; r0 < n_rows; r0 += (uint64_t)gridDim.y * kRetainRows) {
        rt_v4 v[kRetainRows];
#pragma unroll
        for (int u = 0; u < kRetainRows; u++) {
            const uint64_t r = r0 + u;
            v[u] = rt_v4{0u, 0u, 0u, 0u};
            if (live && r < n_rows) {
                const uint64_t sr = rows ? rows[r] : r;
                v[u] = __builtin_nontemporal_load(reinterpret_cast<const rt_v4*>(src + sr * npad + sc));
            }
        }
#pragma unroll
        for (int u = 0; u < kRetainRows; u++) {
            const uint64_t r = r0 + u;
            if (r < n_rows) __builtin_nontemporal_store(v[u], reinterpret_cast<rt_v4*>(dst + r * npad2 + c));
        }
    }
}

// bit-plane arrays (cw_bits, key_idx, a table's t / y): bit c % 64 of dst[r][c / 64] = bit idx[c] % 64 of
// src[rows ? rows[r] : r][idx[c] / 64], lanes at or beyond n2 contribute 0. A wave is one destination word: each
// lane fetches its client's source word (neighbouring lanes share it) and the wave's ballot is the word.
__global__ __launch_bounds__(kRetainThreads) void k_retain_planes(const uint64_t* __restrict__ src,
                                                                  uint64_t* __restrict__ dst,
                                                                  const uint32_t* __restrict__ idx,
                                                                  const uint32_t* __restrict__ rows, uint64_t n_rows,
                                                                  uint64_t nw, uint64_t nw2, uint32_t n2) {
    const uint64_t c = (uint64_t)blockIdx.x * kRetainThreads + threadIdx.x;
    const uint64_t w = c >> 6;
    if (w >= nw2) return;   // whole waves
    const bool live = c < n2;
    const uint32_t sc = live ? idx[c] : 0;
    const uint64_t sw = sc >> 6;
    const uint32_t sb = sc & 63;
    for (uint64_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const uint64_t sr = rows ? rows[r] : r;
        const uint64_t x = live ? src[sr * nw + sw] : 0ull;
        const uint64_t m = __ballot(live && ((x >> sb) & 1));
        if ((threadIdx.x & 63) == 0) dst[r * nw2 + w] = m;
    }
}

hipError_t launch_retain_cols(const uint4* src, uint4* dst, const uint32_t* idx, const uint32_t* rows, uint64_t n_rows,
                              uint64_t npad, uint64_t npad2, uint32_t n2, hipStream_t stream) {
    if (n_rows == 0 || npad2 == 0) return hipSuccess;
    const uint64_t tiles = (npad2 + kRetainThreads - 1) / kRetainThreads;
    const uint64_t groups = (n_rows + kRetainRows - 1) / kRetainRows;
    hipLaunchKernelGGL(k_retain_cols, dim3((unsigned)tiles, retain_grid_y(groups, tiles)), dim3(kRetainThreads), 0,
                       stream, src, dst, idx, rows, n_rows, npad, npad2, n2);
    return hipGetLastError();
}

hipError_t launch_retain_planes(const uint64_t* src, uint64_t* dst, const uint32_t* idx, const uint32_t* rows,
                                uint64_t n_rows, uint64_t nw, uint64_t nw2, uint32_t n2, hipStream_t stream) {
    if (n_rows == 0 || nw2 == 0) return hipSuccess;
    const uint64_t tiles = (nw2 * 64 + kRetainThreads - 1) / kRetainThreads;
    hipLaunchKernelGGL(k_retain_planes, dim3((unsigned)tiles, retain_grid_y(n_rows, tiles)), dim3(kRetainThreads), 0,
                       stream, src, dst, idx, rows, n_rows, nw, nw2, n2);
    return hipGetLastError();
}

}  // namespace fhh
