// Device keys -> AddKeysRequest.keys payloads (fhh_export_keys_bincode, row f5): the inverse of the decoders
// k_bincode_cw_tiles / k_keys_from_bincode in fhh_kernels.hip. Clients [src_first, src_first + m) of one ctx's
// SoA layout leave as the bytes of clients [i0, i0 + m) of an export of `count` clients in requests of B
// (bincode_emit.h has the offsets), written into a staging buffer whose byte 0 is byte `org` of the export
// (org a multiple of 4, so a dword-aligned export offset is a dword-aligned address).
//
//   k_bincode_emit_cw       the CorWords: 99.8 % of the bytes, HBM-bound (16.1 B read, 20 B written per
//                           (client, key, level))
//   k_bincode_emit_headers  key_idx bool, root seed and u64 L of every key, u64 d of every client, u64 m of
//                           every request whose first client is in the slice; byte stores only
//
// The two rules every store here obeys:
//   Ownership. Every byte of the export has exactly one writer: the header kernel's thread of that (client,
//     key), or the CW tile of that (client, key, level block). A CW segment starts at an arbitrary byte
//     offset (a key is 25 + 20 L bytes and a request count may precede any record), so the dword at either of its
//     ends may hold bytes of another owner — the next level block of the key, the key's 25-byte header, the
//     next record's u64 d, the next request's u64 m. Such a dword is never read-modify-written and never
//     stored whole: each owner writes its own bytes of it with byte stores. Only dwords that lie entirely
//     inside one segment are stored as dwords. Hence no atomics and no ordering between workgroups or between
//     the two kernels.
//   Bounds. A writer's bytes lie in [be_slice_begin(i0), be_slice_end(i0, m)) of the export, which the host
//     sizes the staging buffer for; nothing is written outside it. All offsets are 64-bit (1M clients at
//     L = 512 are 20.5 GB).
#include "fhh_internal.h"
#include "bincode_emit.h"

namespace fhh {

constexpr int kBeRow = 5 * (int)kBeLevels + 1;   // dwords of a client's LDS row (odd pitch: conflict-free)

// The slice and the layout's strides. The key buffers (cw_seed [L][K][npad], cw_bits [L][K][4][nw], root_seed
// [K][npad], key_idx [K][nw]) and stg are __restrict__ kernel parameters of their own: read-only inputs that do
// not alias the output, so the wave-uniform plane words compile to scalar loads.
struct EmitArgs {
    uint64_t org;               // byte g of the export is stg[g - org]
    uint64_t src_first, m;      // clients of this ctx's layout
    uint64_t i0, count, B;      // their place in the export
    uint32_t d, L, npad, nw;
};

// A tile is one source 64-client word x one key x kBeLevels levels. Wave wv reads the seed rows of levels
// wv + 4 t (whole 1 KiB lines, lane = client) and their four bit-plane words (wave-uniform), all loads of the
// tile issued before the first LDS write; a lane composes its client's 5 dwords per level (seed, then the four
// bools as bytes 0 / 1) into its LDS row. Then wave wv writes the segments of clients wv + 4 i, each store
// instruction within one client's segment: the 20 nl bytes are contiguous in the export, the interior leaves as aligned dwords assembled with
// v_alignbit from two neighbouring row dwords (64 lanes = 256 contiguous bytes per store), the <= 3 head and
// <= 3 tail bytes as byte stores. Lanes (clients) outside [src_first, src_first + m) are loaded (the layout
// is padded to whole words) and never written out.
__global__ __launch_bounds__(256) void k_bincode_emit_cw(const uint4* __restrict__ cw_seed,
                                                         const uint64_t* __restrict__ cw_bits,
                                                         uint8_t* __restrict__ stg, const EmitArgs a) {
    __shared__ uint32_t st[64 * kBeRow];
    const uint32_t K = 2 * a.d, L = a.L;
    const uint64_t R = be_record_bytes(a.d, L);
    const uint32_t nlb = (L + kBeLevels - 1) / kBeLevels;
    const uint64_t w0 = a.src_first >> 6, nwb = ((a.src_first + a.m - 1) >> 6) - w0 + 1;
    const uint64_t tiles = nwb * K * nlb;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t tq = tile / nwb;   // < K nlb
        const uint64_t w = w0 + (tile - tq * nwb);
        const uint32_t kk = (uint32_t)tq % K;
        const uint32_t l0 = (uint32_t)tq / K * kBeLevels;
        const uint32_t nl = min(kBeLevels, L - l0);
        uint4 v[8];
        uint64_t pl[8][4];
#pragma unroll
        for (int t = 0; t < 8; t++) {
            // a level past a partial block's end is clamped to its last level: loaded, not kept (no branch)
            const uint32_t li = min(wv + 4 * t, nl - 1);
            const size_t row = (size_t)(l0 + li) * K + kk;
            v[t] = cw_seed[row * a.npad + w * 64 + lane];
#pragma unroll
            for (int b = 0; b < 4; b++) pl[t][b] = cw_bits[(row * 4 + b) * a.nw + w];
        }
        // lane = client: where its segment goes (one 64-bit division per lane and tile, under the loads' latency)
        const uint64_t cl = w * 64 + lane;
        const bool in = cl >= a.src_first && cl < a.src_first + a.m;
        const uint64_t gl = in ? be_seg_off(a.i0 + (cl - a.src_first), kk, l0, L, a.B, R) - a.org : 0;
        const uint64_t inmask = __ballot(in);
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const uint32_t li = wv + 4 * t;
            if (li < nl) {
                uint32_t* row = st + lane * kBeRow + 5 * li;
                uint32_t bools = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) bools |= (uint32_t)((pl[t][b] >> lane) & 1) << (8 * b);
                row[0] = v[t].x;
                row[1] = v[t].y;
                row[2] = v[t].z;
                row[3] = v[t].w;
                row[4] = bools;
            }
        }
        __syncthreads();
        // the segments of clients wv + 4 i, four at a time: all their LDS reads (unconditional, indices clamped
        // into the row) go out before the first store, so a wave pays one LDS latency per four clients
        const uint32_t bytes = 20 * nl;
        const uint32_t q2 = min(lane + 128, 5 * kBeLevels - 1);
        for (uint32_t ib = 0; ib < 16; ib += 4) {
            uint32_t x[4][8];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t ln = wv + 4 * (ib + u);
                const uint32_t glo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)gl, (int)ln);
                const BeSeg s = be_seg_split(glo, bytes);   // the split needs the offset mod 4 only
                const uint32_t* row = st + ln * kBeRow;
                x[u][0] = row[lane];
                x[u][1] = row[lane + 1];
                x[u][2] = row[lane + 64];
                x[u][3] = row[lane + 65];
                x[u][4] = row[q2];
                x[u][5] = row[q2 + 1];   // <= row[5 kBeLevels] = row[kBeRow - 1]
                x[u][6] = row[0];
                x[u][7] = row[min((s.head + 4 * s.ndw + lane) >> 2, 5 * kBeLevels)];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t ln = wv + 4 * (ib + u);
                if (!((inmask >> ln) & 1)) continue;   // wave-uniform
                const uint64_t g = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)gl, (int)ln) |
                                   (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(gl >> 32), (int)ln) << 32;
                const BeSeg s = be_seg_split(g, bytes);
                uint8_t* dst = stg + g;
                if (lane < s.head) dst[lane] = (uint8_t)(x[u][6] >> (8 * lane));
                uint32_t* dw = reinterpret_cast<uint32_t*>(dst + s.head);   // (g + head) % 4 == 0: org % 4 == 0
                const uint32_t sh = 8 * s.head;
                if (lane < s.ndw) dw[lane] = __builtin_amdgcn_alignbit(x[u][1], x[u][0], sh);
                if (lane + 64 < s.ndw) dw[lane + 64] = __builtin_amdgcn_alignbit(x[u][3], x[u][2], sh);
                if (lane + 128 < s.ndw) dw[lane + 128] = __builtin_amdgcn_alignbit(x[u][5], x[u][4], sh);
                if (lane < s.tail) {
                    const uint32_t bi = s.head + 4 * s.ndw + lane;   // < bytes
                    dst[bi] = (uint8_t)(x[u][7] >> (8 * (bi & 3)));
                }
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void store_u64_bytes(uint8_t* p, uint64_t v) {
#pragma unroll
    for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i));
}

// one thread per (client, key) of the slice: the key's 25 header bytes; key 0's thread also writes the
// client's u64 d and, for a client that opens a request, that request's u64 m
__global__ void k_bincode_emit_headers(const uint4* __restrict__ root_seed, const uint64_t* __restrict__ key_idx,
                                       uint8_t* __restrict__ stg, const EmitArgs a) {
    const uint32_t K = 2 * a.d;
    const uint64_t R = be_record_bytes(a.d, a.L);
    const uint64_t items = a.m * K;
    for (uint64_t it = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items;
         it += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t j = it / K;
        const uint32_t kk = (uint32_t)(it % K);
        const uint64_t c = a.src_first + j, i = a.i0 + j;
        const uint4 root = root_seed[(size_t)kk * a.npad + c];
        const uint32_t ki = (uint32_t)((key_idx[(size_t)kk * a.nw + (c >> 6)] >> (c & 63)) & 1);
        uint8_t* key = stg + (be_key_off(i, kk, a.L, a.B, R) - a.org);
        key[0] = (uint8_t)ki;
        const uint32_t x[4] = {root.x, root.y, root.z, root.w};
#pragma unroll
        for (int k = 0; k < 16; k++) key[1 + k] = (uint8_t)(x[k >> 2] >> (8 * (k & 3)));
        store_u64_bytes(key + 17, a.L);
        if (kk == 0) {
            uint8_t* rec = stg + (be_client_off(i, a.B, R) - a.org);
            store_u64_bytes(rec, a.d);
            if (i % a.B == 0) store_u64_bytes(rec - 8, be_request_clients(i, a.count, a.B));
        }
    }
}

hipError_t launch_bincode_emit(const uint4* cw_seed, const uint64_t* cw_bits, const uint4* root_seed,
                               const uint64_t* key_idx, uint32_t d, uint32_t L, uint32_t npad, uint32_t nw,
                               uint64_t src_first, uint64_t m, uint64_t i0, uint64_t count, uint64_t B, uint8_t* stg,
                               uint64_t org, hipStream_t stream) {
    if (m == 0) return hipSuccess;
    // the caller's layout and export must hold the slice (the kernels trust these)
    if (src_first + m > (uint64_t)nw * 64 || (uint64_t)nw * 64 > npad || i0 + m > count || B == 0 || (org & 3) ||
        org > be_slice_begin(i0, B, be_record_bytes(d, L)))
        return hipErrorInvalidValue;
    EmitArgs a{org, src_first, m, i0, count, B, d, L, npad, nw};
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const uint64_t nwb = ((src_first + m - 1) >> 6) - (src_first >> 6) + 1;
    const uint64_t tiles = nwb * 2 * d * ((L + kBeLevels - 1) / kBeLevels);
    const uint64_t cap = (uint64_t)cus * 8;
    hipLaunchKernelGGL(k_bincode_emit_cw, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(256), 0, stream, cw_seed,
                       cw_bits, stg, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    uint64_t blocks = (m * 2 * d + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_bincode_emit_headers, dim3((unsigned)blocks), dim3(256), 0, stream, root_seed,
                       key_idx, stg, a);
    return hipGetLastError();
}

}  // namespace fhh
