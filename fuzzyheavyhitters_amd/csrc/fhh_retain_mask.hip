// fhh_retain_clients_device's survivor list: the idx list k_retain_cols / k_retain_planes consume (fhh_retain.hip),
// made on the GPU from a keep mask that is already there (the `ok` bytes of the sketch verification), so that
// neither the mask nor the list crosses to the host. Three kernels:
//   k_keep_words   a wave per 64-client word: each lane ANDs its client's byte of every row, the ballot is the
//                  keep word; the word and its popcount are stored, a byte other than 0/1 is recorded
//   k_keep_scan    one workgroup: the counts' exclusive prefix sum (in place) and the total
//   k_keep_emit    a wave per word: kept lane l writes idx[base[w] + popcount(word below l)] = 64 w + l
// The host reads the 16-byte record between the scan and the emit: it needs n' to size the destination and
// refuses before anything is allocated.
#include "fhh_internal.h"

namespace fhh {

namespace {

constexpr int kKeepThreads = 256;    // words / emit: 4 waves = 4 words per block
constexpr int kScanThreads = 1024;   // the one scan workgroup: 1024 words (65 536 clients) per step

}  // namespace

// keep[r * row_stride + i], r < n_rows, i < n: bytes 0/1. words[w] bit l = AND_r keep[r][64 w + l] (0 for lanes at or
// beyond n); cnt[w] = its popcount. A byte > 1 enters rec->bad by a 64-bit minimum of (i << 8 | byte), so the lowest
// client index wins whichever wave meets it first. Row r's 64 bytes of a wave are one coalesced segment.
__global__ __launch_bounds__(kKeepThreads) void k_keep_words(const uint8_t* __restrict__ keep, uint64_t n,
                                                             uint32_t n_rows, uint64_t row_stride, uint64_t nw,
                                                             uint64_t* __restrict__ words, uint32_t* __restrict__ cnt,
                                                             KeepRecord* __restrict__ rec) {
    const uint64_t i = (uint64_t)blockIdx.x * kKeepThreads + threadIdx.x;
    const uint64_t w = i >> 6;
    if (w >= nw) return;   // whole waves
    const bool in = i < n;
    uint32_t acc = 1;
    if (in) {
        for (uint32_t r = 0; r < n_rows; r++) {
            const uint32_t b = keep[(uint64_t)r * row_stride + i];
            if (b > 1) atomicMin(reinterpret_cast<unsigned long long*>(&rec->bad), (unsigned long long)(i << 8 | b));
            acc &= b;
        }
    }
    const uint64_t m = __ballot(in && acc == 1);
    if ((threadIdx.x & 63) == 0) {
        words[w] = m;
        cnt[w] = (uint32_t)__popcll(m);
    }
}

// base[w] = sum of cnt[0 .. w) in place (thread t of step s reads and then writes entry 1024 s + t only), and
// rec->n_kept = the total (< 2^32: a client index is a u32). One workgroup walks the words 1024 at a time with a
// running carry: a wave scans its 64 counts by shuffles, the 16 wave totals meet in LDS.
__global__ __launch_bounds__(kScanThreads) void k_keep_scan(uint32_t* __restrict__ base, uint64_t nw,
                                                            KeepRecord* __restrict__ rec) {
    __shared__ uint32_t wave_sum[kScanThreads / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    uint32_t carry = 0;
    for (uint64_t w0 = 0; w0 < nw; w0 += kScanThreads) {
        const uint64_t w = w0 + t;
        const uint32_t c = w < nw ? base[w] : 0;
        uint32_t inc = c;   // inclusive over the wave
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t up = __shfl_up(inc, s);
            if (lane >= (uint32_t)s) inc += up;
        }
        if (lane == 63) wave_sum[wv] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kScanThreads / 64; k++) {
            const uint32_t x = wave_sum[k];
            if ((uint32_t)k < wv) before += x;
            total += x;
        }
        if (w < nw) base[w] = carry + before + inc - c;
        carry += total;
        __syncthreads();   // wave_sum is rewritten by the next step
    }
    if (t == 0) rec->n_kept = carry;
}

// idx[base[w] + (kept lanes of word w below l)] = 64 w + l for every kept lane: increasing in k, the list
// fhh_retain_plan makes on the host. The words hold no lane at or beyond n, so every store is below n'.
__global__ __launch_bounds__(kKeepThreads) void k_keep_emit(const uint64_t* __restrict__ words,
                                                            const uint32_t* __restrict__ base, uint64_t nw,
                                                            uint32_t* __restrict__ idx) {
    const uint64_t i = (uint64_t)blockIdx.x * kKeepThreads + threadIdx.x;
    const uint64_t w = i >> 6;
    if (w >= nw) return;
    const uint64_t m = words[w];
    if (!((m >> (threadIdx.x & 63)) & 1)) return;
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    idx[base[w] + below] = (uint32_t)i;
}

hipError_t launch_keep_scan(const uint8_t* keep, uint64_t n, uint32_t n_rows, uint64_t row_stride, uint64_t* words,
                            uint32_t* base, KeepRecord* rec, hipStream_t stream) {
    const uint64_t nw = (n + 63) / 64;
    if (nw == 0 || (n >> 32)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(rec, 0xFF, sizeof(KeepRecord), stream);   // bad = none; n_kept is the scan's
    if (e != hipSuccess) return e;
    const uint64_t blocks = (nw * 64 + kKeepThreads - 1) / kKeepThreads;
    hipLaunchKernelGGL(k_keep_words, dim3((unsigned)blocks), dim3(kKeepThreads), 0, stream, keep, n, n_rows, row_stride,
                       nw, words, base, rec);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_keep_scan, dim3(1), dim3(kScanThreads), 0, stream, base, nw, rec);
    return hipGetLastError();
}

hipError_t launch_keep_emit(const uint64_t* words, const uint32_t* base, uint64_t nw, uint32_t* idx,
                            hipStream_t stream) {
    if (nw == 0) return hipSuccess;
    const uint64_t blocks = (nw * 64 + kKeepThreads - 1) / kKeepThreads;
    hipLaunchKernelGGL(k_keep_emit, dim3((unsigned)blocks), dim3(kKeepThreads), 0, stream, words, base, nw, idx);
    return hipGetLastError();
}

}  // namespace fhh
